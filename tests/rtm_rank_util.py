"""Shared by tests/test_rtm_rank_cpu.py and tests/test_gpu_rtm_rank.py: the review transformer over the whole catalogue
(``evaluate.rank_all_rtm``).

* ``assemble_chunk``: the candidate tensors ``ProductRanker.test`` reads, put together from an entries-only batch and the
  catalogue's ``[P, I]`` review matrix by the rule of the test collate (prod_search_dataloader.py:44-109): the user's
  reviews, then the candidate's, then padding.
* ``factorised_scores``: the split softmax and the linear key / value decomposition in ~40 lines of torch, the yardstick
  of what the re-association costs in fp32.
* ``make_case``: the data of the GPU cases.  ``oracle_scores``: ``oracle.rtm.rtm_test`` over chunks of them.
* ``CASES`` / ``YARDSTICK`` / ``bound``: the cases both files run, what fp32 on the host costs each of them against the
  float64 oracle, and the per-entry bound that follows from it.  ``plan_of``: ``ps_rtm_rank_plan`` for a case.
"""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from prodsearch_amd import default_args, rtm_data, synth

TOL = 1e-4            # the suite's eval bound (tests/test_gpu_parity.py LOSS_TOL, tests/test_gpu_saturated.py EVAL_TOL)


def leading(ids, pad):
    """Number of leading non-pad ids of every row."""
    ids = np.asarray(ids)
    ok = ids != pad
    return np.where(ok.all(-1), ids.shape[-1], (~ok).argmax(-1))


def assemble_chunk(qw, u_r, users, item_r, cands, review_u_p, user_pad, prod_pad, rev_pad, ids_from_reviews=False, limit=None):
    """``ProdSearchTestBatch`` tensors for candidates ``cands`` [B, C] (-1: a padded slot of a ragged list).  Per-position
    user / item ids as ``write_seq`` gives them: the entry's user and the review's item on the user's reviews, the review's
    author and the candidate on the item's.  ``ids_from_reviews``: both from ``review_u_p`` alone (synthetic data whose
    reviews do not belong to the entry's user / the candidate).  ``limit``: a sequence holds at most ``1 + limit`` positions —
    the user's reviews first, the item's after them, whatever is left over is cut (rr_entry_kernel / rr_pair_kernel)."""
    u_r, item_r, cands, up = (np.asarray(x) for x in (u_r, item_r, cands, review_u_p))
    B, C = cands.shape
    nu = leading(u_r, rev_pad)
    ni = leading(item_r, rev_pad)
    live = cands >= 0
    if limit is not None:
        nu = np.minimum(nu, limit)
    nc = ni[np.where(live, cands, 0)]                                     # [B, C] reviews of the candidate in this sequence
    if limit is not None:
        nc = np.minimum(nc, limit - nu[:, None])
    R = int(max(1, ((nu[:, None] + nc) * live).max()))
    ridx = np.full((B, C, R), rev_pad, dtype=np.int64)
    seg = np.full((B, C, R + 1), 3, dtype=np.int64)
    usr = np.full((B, C, R + 1), user_pad, dtype=np.int64)
    itm = np.full((B, C, R + 1), prod_pad, dtype=np.int64)
    for b in range(B):
        for c in range(C):
            i = int(cands[b, c])
            if i < 0:
                continue
            seg[b, c, 0] = 0
            a, n = int(nu[b]), int(nc[b, c])
            ridx[b, c, :a] = u_r[b, :a]
            ridx[b, c, a:a + n] = item_r[i, :n]
            seg[b, c, 1:1 + a] = 1
            seg[b, c, 1 + a:1 + a + n] = 2
            rs = ridx[b, c, :a + n]
            if up.size:
                usr[b, c, 1:1 + a + n] = up[rs, 0]
                itm[b, c, 1:1 + a + n] = up[rs, 1]
            if not ids_from_reviews:
                usr[b, c, 1:1 + a] = users[b]
                itm[b, c, 1 + a:1 + a + n] = i
    t = torch.from_numpy
    return rtm_data.ProdSearchTestBatch(list(range(B)), [int(u) for u in users], None, t(cands.astype(np.int64)), torch.as_tensor(qw),
                                        t(ridx), t(seg), t(usr), t(itm), to_tensor=False)


FAULTS = ('drop_last', 'pos_off', 'seg1_keys', 'no_cap', 'heads_merged')


def factorised_scores(P, a, qw, u_r, item_r, table, review_u_p, V, RC, T, fault=None, stats=None):
    """scores [B, n_items] by the factorisation the HIP path uses, in the dtype of ``table``.  T = longest sequence - 1.
    ``stats`` (a dict) receives ``wmax`` [B, n_items], the largest attention weight of every pair over heads and keys, and
    ``keys`` [B, n_items], the number of keys of the pair's softmax (1: the query token alone, whose weight is 1 by construction).
    ``fault`` (tests/test_rtm_rank_cpu.py's sensitivity test alone) computes what a kernel with one mistake would:
      'drop_last'    the last live key of an item is dropped where the item's count is no multiple of 4 (rr_step's group)
      'pos_off'      an item's reviews sit at positions n_u + j instead of 1 + n_u + j
      'seg1_keys'    an item's keys take the segment-1 (user's reviews) table
      'no_cap'       the cut at 1 + T positions is ignored
      'heads_merged' a logit is summed over 2 * (64 / H) lanes: heads 2k and 2k + 1 both get the sum of their logits
    and ``stats['acts']`` [B] says for which entries the mistake changes an operand at all."""
    from oracle.tem import ffn, no_dropout, positional_encoding, query_encode
    assert fault is None or fault in FAULTS
    d, H = a.embedding_size, a.heads
    dh, dt, pad = d // H, table.dtype, RC - 1
    te = 'transformer_encoder.'
    at = te + 'transformer_inter.0.self_attn.'
    lin = lambda x, n: F.linear(x, P[at + n + '.weight'], P[at + n + '.bias'])
    capped = fault != 'no_cap'
    T, T_cap = (T if capped else max(T, u_r.shape[1] + item_r.shape[1])), T
    merged = fault == 'heads_merged' and H >= 2
    mate = torch.arange(H) ^ 1
    pe = positional_encoding(5000, d).to(dt)[:T + 1] if a.use_pos_emb else torch.zeros(T + 1, d, dtype=dt)
    seg = P['seg_embeddings.weight'] if a.use_seg_emb else torch.zeros(4, d, dtype=dt)
    x0 = query_encode(P, a, qw, V - 1, no_dropout)[0] + seg[0] + pe[0]
    rev = table.clone()
    up = torch.as_tensor(np.asarray(review_u_p), dtype=torch.int64).reshape(-1, 2)
    if a.use_user_emb:
        rev[:len(up)] += P['user_emb.weight'][up[:, 0]]
        x0 = x0 + P['user_emb.weight'][-1]
    if a.use_item_emb:
        rev[:len(up)] += P['product_emb.weight'][up[:, 1]]
        x0 = x0 + P['product_emb.weight'][-1]
    KR, VR = F.linear(rev, P[at + 'linear_keys.weight']), F.linear(rev, P[at + 'linear_values.weight'])     # once per evaluation
    kt = [lin(seg[s] + pe, 'linear_keys') for s in (1, 2)]                                                  # [segment][position]
    vt = [lin(seg[s] + pe, 'linear_values') for s in (1, 2)]
    q, k0, v0 = lin(x0, 'linear_query') / math.sqrt(dh), lin(x0, 'linear_keys'), lin(x0, 'linear_values')   # once per entry
    nu_all, ni_all = leading(u_r, pad), leading(item_r, pad)
    nu = np.minimum(nu_all, T)                                                                              # the user's reviews first ...
    I = item_r.shape[1]
    out, wmax, keys, acts = [], [], [], []
    for e in range(qw.shape[0]):
        n = int(nu[e])
        ku = torch.cat([k0[e:e + 1], KR[u_r[e, :n]] + kt[0][1:1 + n]]).view(-1, H, dh)
        vu = torch.cat([v0[e:e + 1], VR[u_r[e, :n]] + vt[0][1:1 + n]]).view(-1, H, dh)
        lu = (ku * q[e].view(1, H, dh)).sum(-1)                                                             # [1 + n, H]
        if merged:
            lu = lu + lu[:, mate]
        mu = lu.max(0).values
        su, au = (lu - mu).exp().sum(0), ((lu - mu).exp()[:, :, None] * vu).sum(0)                         # the entry's partial
        cnt = np.minimum(ni_all, T - n)                                                                     # ... the item's in what is left
        cnt_true = np.minimum(ni_all, T_cap - min(int(nu_all[e]), T_cap))
        if fault == 'drop_last':
            cnt = np.where(cnt % 4 != 0, cnt - 1, cnt)
        acts.append({None: False, 'drop_last': bool((cnt_true % 4 != 0).any()),
                     'pos_off': bool(a.use_pos_emb) and bool((cnt_true > 0).any()),
                     'seg1_keys': bool(a.use_seg_emb) and bool((cnt_true > 0).any()),
                     'no_cap': int(nu_all[e]) > T_cap or bool((ni_all > cnt_true).any()), 'heads_merged': merged}[fault])
        pos = torch.arange(I)[None, :] + (n if fault == 'pos_off' else 1 + n)
        ok = (torch.arange(I)[None, :] < torch.from_numpy(cnt)[:, None])                                   # the loader's cut
        pos = pos.clamp(max=T)
        ki = (KR[item_r] + kt[0 if fault == 'seg1_keys' else 1][pos]).view(-1, I, H, dh)
        vi = (VR[item_r] + vt[1][pos]).view(-1, I, H, dh)
        li = (ki * q[e].view(1, 1, H, dh)).sum(-1)                                                          # [P, I, H]
        if merged:
            li = li + li[:, :, mate]
        li = li.masked_fill(~ok[:, :, None], -float('inf'))
        m = torch.maximum(mu[None], li.max(1).values)
        w = (li - m[:, None]).exp()
        s = su[None] * (mu[None] - m).exp() + w.sum(1)                                                     # merged like an online softmax
        acc = au[None] * (mu[None] - m).exp()[:, :, None] + (w[..., None] * vi).sum(1)
        wu = (lu - mu).exp().max(0).values[None] * (mu[None] - m).exp()                                     # [P, H]
        wmax.append((torch.maximum(wu, w.max(1).values) / s).max(1).values)
        keys.append(torch.from_numpy(1 + n + cnt))
        ctx = (acc / s[..., None]).reshape(-1, d)
        y1 = lin(ctx, 'final_linear') + x0[e]
        y2 = ffn(P, te + 'transformer_inter.0.feed_forward.', y1, no_dropout, 0)
        enc = F.layer_norm(y2, (d,), P[te + 'layer_norm.weight'], P[te + 'layer_norm.bias'], 1e-6)
        out.append(F.linear(enc, P[te + 'wo.weight'], P[te + 'wo.bias']).squeeze(-1))
    if stats is not None:
        stats.update(wmax=torch.stack(wmax), keys=torch.stack(keys), acts=np.array(acts))
    return torch.stack(out)


def make_args(d=128, ff=512, heads=8, encoder='pvc', U=4, I=6, WL=10, **kw):
    base = dict(model_name='review_transformer', review_encoder_name=encoder, embedding_size=d, heads=heads, ff_size=ff,
                inter_layers=1, dropout=0.0, corrupt_rate=0.0, review_word_limit=WL, uprev_review_limit=U, iprev_review_limit=I)
    base.update(kw)
    return default_args(**base)


def make_case(seed=5, P=37, I=6, U=4, B=5, V=300, RC=400, n_users=20, Q=5, **akw):
    """The GPU cases' data: entry 0 has no reviews and item 0 none (their pair is a softmax over the query key alone), entry 1
    has U and item 1 I reviews (a full sequence), items 2 and 3 share one review list, the last target is outside [0, P).
    Every other item has at least one review: items without any all score alike, which would fill the order with exact ties.
    ``review_u_p`` is random except that an entry's reviews carry the entry's user and an item's reviews the item."""
    a = make_args(U=U, I=I, **akw)
    rng = synth.rng_for(seed)
    pad = RC - 1
    WL = a.review_word_limit
    rw = rng.integers(0, V - 1, size=(RC, WL))
    rw[np.arange(WL)[None, :] >= rng.integers(1, WL + 1, size=RC)[:, None]] = V - 1
    rw[-1] = V - 1
    up = np.stack([rng.integers(0, n_users, size=pad), rng.integers(0, P, size=pad)], 1).astype(np.int64)
    pool = rng.permutation(pad)
    users = np.arange(1, B + 1) % n_users
    u_r = np.full((B, U), pad, dtype=np.int64)
    cur = 0
    for e in range(B):
        n = 0 if e == 0 else U if e == 1 else int(rng.integers(1, U + 1))
        u_r[e, :n] = pool[cur:cur + n]
        up[pool[cur:cur + n], 0] = users[e]
        cur += n
    item_r = np.full((P, I), pad, dtype=np.int64)
    for i in range(P):
        n = 0 if i == 0 else I if i == 1 else min(3, I) if i == 2 else int(rng.integers(1, I + 1))
        if i == 3:
            item_r[3] = item_r[2]
            continue
        item_r[i, :n] = rng.choice(pool[cur:], size=n, replace=False)
        up[item_r[i, :n], 1] = i
    qw = np.full((B, Q), V - 1, dtype=np.int64)
    for b in range(B):
        n = int(rng.integers(1, Q + 1))
        qw[b, :n] = rng.integers(0, V - 1, size=n)
    target = rng.integers(0, P, size=B).astype(np.int64)
    target[-1] = P + 5
    t = torch.from_numpy
    # T: the review positions of a sequence, which the model takes from its limits — not from the widths of the lists it is handed
    return types.SimpleNamespace(a=a, V=V, RC=RC, P=P, I=I, U=U, B=B, n_users=n_users, rw=t(rw), review_u_p=t(up), users=users,
                                 u_r=t(u_r), item_r=t(item_r), qw=t(qw), target=t(target),
                                 T=int(a.uprev_review_limit) + int(a.iprev_review_limit))


def build_model(c, device, seed=11, scale=1.0):
    """A ProductRanker (``fix_emb``: a PretrainedProductRanker) on ``device`` with synth.make_state_dict weights (drawn per parameter name) times ``scale`` on the
    tables; returns (model, CPU state dict for the oracle)."""
    from prodsearch_amd import PretrainedProductRanker, ProductRanker
    cls = PretrainedProductRanker if getattr(c.a, 'fix_emb', False) else ProductRanker     # (as trainer.create_model dispatches)
    state = torch.get_rng_state()
    try:
        m = cls(c.a, 'cpu', c.V, c.RC, c.P, c.n_users, c.rw, None, word_dists=None)
    finally:
        torch.set_rng_state(state)
    shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
    sd = synth.make_state_dict(shapes, seed, {})
    for k in sd:
        if 'emb' in k:
            sd[k] = sd[k] * scale
    m.load_state_dict(sd, strict=False)
    m = m.to(device)
    m.eval()
    return m, state_of(m)


def state_of(m):
    """The model's state dict on the host, for the oracle (fix_emb: without the model-level alias of the review table)."""
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sd.pop('review_embeddings', None)
    return sd


def rank_batch(c, device=None):
    b = rtm_data.ProdSearchRankBatch(list(range(c.B)), [int(u) for u in c.users], c.target, c.qw, c.u_r)
    return b if device is None else b.to(device)


def chunks(c, size):
    """The catalogue as candidate chunks of ``size`` for every entry: ProdSearchTestBatch objects and their item ids."""
    for lo in range(0, c.P, size):
        ids = np.arange(lo, min(c.P, lo + size))
        cands = np.tile(ids[None], (c.B, 1))
        yield ids, assemble_chunk(c.qw, c.u_r, c.users, c.item_r, cands, c.review_u_p, c.n_users, c.P, c.RC - 1, ids_from_reviews=True,
                                  limit=c.T)


def oracle_scores(c, sd, f64=False, chunk=16):
    """[B, P] scores of ``oracle.rtm.rtm_test`` (the reference's ``ProductRanker.test``) over chunks of the catalogue."""
    from oracle import rtm as ortm
    P = {k: (v.double() if f64 and v.dtype.is_floating_point else v) for k, v in sd.items()}
    rev = ortm.rtm_review_embeddings(P, c.a, c.rw, c.V)
    out = torch.empty(c.B, c.P, dtype=rev.dtype)
    for ids, b in chunks(c, chunk):
        out[:, ids] = ortm.rtm_test(P, c.a, b, rev, c.V, c.RC)
    return out, P, rev


def banded(ref, tol=TOL):
    """Per entry: the oracle's order (score desc, id asc) and which of its positions lie in a band — the gap to a neighbouring
    score is at most 2 * tol * max|score|, so an implementation within tol may swap them."""
    ref = ref.double().numpy()
    order = np.lexsort((np.arange(ref.shape[1])[None, :].repeat(ref.shape[0], 0), -ref), axis=1)
    rs = np.take_along_axis(ref, order, 1)
    close = np.abs(np.diff(rs, axis=1)) <= 2 * tol * np.abs(ref).max()
    band = np.zeros_like(rs, dtype=bool)
    band[:, :-1] |= close
    band[:, 1:] |= close
    return order, band


# ------------------------------------------------------------------------------------------------- the cases of both files
# make_case / make_args arguments, plus: 'items_per_pass' (rank_all_rtm), 'scale' (build_model).  `plan`: the fields of
# ps_rtm_rank_plan the case was written for — the branch it must take (csrc/rtm_rank.hip), asserted before anything is compared.
CASES = {'base': dict(),
         'd64': dict(d=64, ff=128),                                   # the unfused tail, one column per lane
         'd256': dict(d=256, ff=1024),                                # the unfused tail, four columns per lane
         'pv_user_item': dict(encoder='pv', use_user_emb=True, use_item_emb=True),   # the combined table T, pad rows at position 0
         'no_pos': dict(use_pos_emb=False),
         'no_seg': dict(use_seg_emb=False),
         'pretrained_fix_emb': dict(encoder='pv', fix_emb=True, use_user_emb=True),   # PretrainedProductRanker: the frozen pv table
         'passes': dict(B=33, items_per_pass=8),                      # five passes, a ragged last tile, more entries than waves
         'long': dict(U=20, I=30, P=70, B=3, RC=2500),                # the workload's own sequence length: 51 positions
         'd512': dict(d=512, ff=1024),                                # rr_entry_kernel<8> / rr_pair_kernel<8>
         'd512_lds80k': dict(d=512, ff=1024, I=20, P=12, B=3, RC=600),            # a tile above 64 KB: the raised LDS limit
         'lds_full': dict(d=256, ff=512, I=64, U=64, P=10, B=3, RC=3000),         # RR_LDS_MAX itself; a full ballot on both sides
         'heads1_d128': dict(heads=1, d=128), 'heads2_d512': dict(heads=2, d=512, ff=1024), 'heads4_d64': dict(heads=4, d=64, ff=128),
         'heads16_d128': dict(heads=16, d=128), 'heads32_d256': dict(heads=32, d=256, ff=1024), 'heads64_d64': dict(heads=64, d=64, ff=128),
         'cap': dict(U=4, I=6, uprev_review_limit=2, iprev_review_limit=3),       # lists wider than the limits: items cut
         # ... and a user list that alone fills the sequence: entry 1's six reviews are cut to five and no item's review is read
         # (seed: the first at which at most a quarter of the order is banded — entries that see one review per item nearly tie)
         'cap_user': dict(U=6, I=6, B=9, uprev_review_limit=2, iprev_review_limit=3, seed=36),
         'rev_fs': dict(encoder='fs'), 'rev_avg': dict(encoder='avg'), 'q_avg': dict(query_encoder_name='avg'),
         'ff256': dict(d=128, ff=256), 'ff1024': dict(d=128, ff=1024), 'ff384': dict(d=128, ff=384),   # the d = 128 tail, fused or not
         'big_table': dict(d=64, ff=128, RC=33000, WL=4, P=37),       # a review table tall enough for the bf16x3 GEMM
         'sharp': dict(scale=8)}                                      # attention weights near one-hot
PLAN = {'base': dict(epl=2, lph=8, items_per_workgroup=8, lds_bytes=49152, items_per_pass=37, passes=1, tail_fused=1, query_fs_fused=1),
        'd64': dict(epl=1, lph=8, items_per_workgroup=16, lds_bytes=49152, tail_fused=0, query_fs_fused=1),
        'd256': dict(epl=4, lph=8, items_per_workgroup=4, lds_bytes=49152, tail_fused=0, query_fs_fused=0),
        'pv_user_item': dict(epl=2, lph=8, tail_fused=1), 'no_pos': dict(epl=2, lph=8), 'no_seg': dict(epl=2, lph=8),
        'pretrained_fix_emb': dict(epl=2, lph=8, tail_fused=1),
        'passes': dict(items_per_pass=8, passes=5, items_per_workgroup=8, lds_bytes=49152),
        'long': dict(items_per_workgroup=1, lds_bytes=30720, items_per_pass=70, passes=1),
        'd512': dict(epl=8, lph=8, items_per_workgroup=2, lds_bytes=49152, tail_fused=0, query_fs_fused=0),
        'd512_lds80k': dict(epl=8, items_per_workgroup=1, lds_bytes=81920),
        'lds_full': dict(epl=4, items_per_workgroup=1, lds_bytes=131072),
        'heads1_d128': dict(lph=64, epl=2), 'heads2_d512': dict(lph=32, epl=8), 'heads4_d64': dict(lph=16, epl=1),
        'heads16_d128': dict(lph=4, epl=2), 'heads32_d256': dict(lph=2, epl=4), 'heads64_d64': dict(lph=1, epl=1),
        'cap': dict(epl=2, lph=8), 'cap_user': dict(epl=2, lph=8),
        'rev_fs': dict(tail_fused=1, query_fs_fused=1), 'rev_avg': dict(tail_fused=1, query_fs_fused=1), 'q_avg': dict(query_fs_fused=0),
        'ff256': dict(tail_fused=1, epl=2), 'ff1024': dict(tail_fused=1, epl=2), 'ff384': dict(tail_fused=0, epl=2),
        'big_table': dict(epl=1, items_per_workgroup=16, lds_bytes=49152, tail_fused=0),
        'sharp': dict(epl=2, lph=8, tail_fused=1)}
PLAN_FIELDS = ('epl', 'lph', 'items_per_workgroup', 'lds_bytes', 'items_per_pass', 'passes', 'tail_fused', 'query_fs_fused')

# What fp32 on the host costs each case against the float64 oracle, per entry (`entry_err`), the worst entry: the larger of
# the fp32 oracle's and the fp32 factorisation's error.  Measured on the CPU (tests/test_rtm_rank_cpu.py re-measures them and
# allows a tenth on top for another host's summation order; these are the largest over 1, 4 and 8 BLAS threads, which moved
# four of them by 8 to 17 %).  The GPU's per-entry bound is 8 x this, at most TOL.
YARDSTICK = {'base': 1.21e-6, 'd64': 3.53e-7, 'd256': 1.16e-6, 'pv_user_item': 9.70e-7, 'no_pos': 2.14e-6, 'no_seg': 1.13e-6,
             'pretrained_fix_emb': 1.21e-6, 'passes': 1.54e-6, 'long': 1.81e-6, 'd512': 4.40e-6, 'd512_lds80k': 2.14e-6,
             'lds_full': 5.34e-7, 'heads1_d128': 1.47e-6, 'heads2_d512': 2.60e-6, 'heads4_d64': 3.35e-7, 'heads16_d128': 1.34e-6,
             'heads32_d256': 1.08e-6, 'heads64_d64': 3.91e-7, 'cap': 1.74e-6, 'cap_user': 1.62e-6, 'rev_fs': 7.44e-7,
             'rev_avg': 1.21e-6, 'q_avg': 7.46e-7, 'ff256': 4.33e-7, 'ff1024': 2.89e-6, 'ff384': 8.11e-7, 'big_table': 3.38e-7,
             'sharp': 3.92e-6}
YARD_FACTOR = 8


def bound(name):
    return min(YARD_FACTOR * YARDSTICK[name], TOL)


def entry_err(got, ref64):
    """Per entry: max_i |got[e, i] - ref64[e, i]| / max_i |ref64[e, i]|."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref64).double()
    return ((got - ref).abs().amax(1) / ref.abs().amax(1)).numpy()


def case_of(name):
    """(case data, items_per_pass, build_model's scale) of a named case."""
    kw = dict(CASES[name])
    ipp, scale = kw.pop('items_per_pass', None), kw.pop('scale', 1.0)
    return make_case(**kw), ipp, scale


@functools.lru_cache(maxsize=None)
def host_case(name):
    """One case on the host, computed once and shared: the float64 and fp32 oracles and both factorisations."""
    c, ipp, scale = case_of(name)
    m, sd = build_model(c, 'cpu', scale=scale)
    ref64, P64, rev64 = oracle_scores(c, sd, f64=True)
    ref32, P32, rev32 = oracle_scores(c, sd, f64=False)
    st = {}
    f64 = factorised_scores(P64, c.a, c.qw, c.u_r, c.item_r, rev64, c.review_u_p, c.V, c.RC, c.T, stats=st)
    f32 = factorised_scores(P32, c.a, c.qw, c.u_r, c.item_r, rev32, c.review_u_p, c.V, c.RC, c.T)
    return types.SimpleNamespace(c=c, m=m, sd=sd, ipp=ipp, scale=scale, ref64=ref64, ref32=ref32, f64=f64, f32=f32, P64=P64, rev64=rev64,
                                 wmax=st['wmax'], keys=st['keys'], yard=float(max(entry_err(ref32, ref64).max(), entry_err(f32, ref64).max())))


def faulty_scores(h, fault):
    """(float64 scores of the factorisation with ``fault``, the entries it acts on) for a ``host_case``."""
    c, st = h.c, {}
    s = factorised_scores(h.P64, c.a, c.qw, c.u_r, c.item_r, h.rev64, c.review_u_p, c.V, c.RC, c.T, fault=fault, stats=st)
    return s, st['acts']


def plan_of(lib, m, c, k, ipp=None):
    """``ps_rtm_rank_plan`` for the call ``evaluate.rank_all_rtm(m, index, rank_batch(c), k, items_per_pass=ipp)`` makes."""
    from prodsearch_amd import _lib
    desc, sh = m._rank_all_desc(c.B, c.qw.shape[1], c.U, (c.P, c.RC - 1 if (c.a.use_user_emb or c.a.use_item_emb) else 0, c.I))
    nbytes = lib.ps_rtm_rank_scratch_bytes(desc, sh, k, int(ipp or 0))
    assert nbytes > 0, lib.ps_last_error()
    plan = _lib.PsRtmRankPlan()
    _lib.check(lib.ps_rtm_rank_plan(desc, sh, k, nbytes, plan), 'ps_rtm_rank_plan')
    return {f: int(getattr(plan, f)) for f in PLAN_FIELDS}
