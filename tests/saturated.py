"""Inputs and float64 references for the step at weights no other oracle comparison reaches (tests/test_saturated_cpu.py,
tests/test_gpu_saturated.py).  synth.make_state_dict draws tables at 0.5 N(0, 1) and matrices at 1 / sqrt(fan_in): softmax
rows near uniform, item logits below 9, tanh / GELU / BCE in their linear range.  Two regimes scale that state dict to where
a model is after a few thousand Adam steps, and past it:

  peaked     some softmax rows one-hot, some still spread, in the same batch (and so in the same wave): the max over the
             valid keys, exp(v - m) far from 0, and the P (dP - sum P dP) cancellation of the backward are all live;
  saturated  softmax one-hot, item logits of 30 and more, the FS projection's tanh at +-1, GELU inputs beyond +-6.

The scale factors are constants, chosen on the CPU; ``check_regime`` states what each regime has to show on the float64 oracle
and tests/test_saturated_cpu.py asserts it for every case, together with the yardstick: the fp32 oracle's own error against the
float64 oracle stays at or below 1e-4, which is what lets the GPU tests keep the suite's bounds against float64.

A softmax row here is one (sequence, head) of the last layer's consumed position, over the positives' and the negatives'
encodes; rows with a single valid key are left out of the shares (their only weight is 1 at any scale)."""
import functools
import types

import torch

import enc_paths

# name -> factors of scaled_state_dict.  The attention's logits grow with tables x kq^2 at the FS query (|tanh| <= 1) and with
# (tables x kq)^2 at an item query; fp32's own error in a softmax row with two nearly tied keys grows with them too (about
# 1e-6 of the logits' spread), which is what caps the saturated regime: at 8 / 6 / 6 the fp32 oracle is off by up to 4e-4.
REGIMES = {
    # the query projection's heads run from a quarter of to 32 times the benign scale: every sequence has spread and one-hot
    # heads side by side, at any S and with as few as two sequences
    'peaked': dict(tables=4.0, kq=1.0, w1=3.0, q_heads=(0.25, 32.0)),
    'saturated': dict(tables=8.0, kq=4.5, w1=6.0, fs=3.0),
}
_L1 = 'transformer_encoder__transformer_inter__1__self_attn__linear_'
# cases whose yardstick or whose conditions the regime's factors miss (measured on the CPU, float64 and fp32 oracle only):
CASE_SCALES = {
    # d = 256, wave form: at the regime's factors fp32's own error is 9.4e-5 here, and 1.0e-4 at kq = 6 on another host's CPU;
    # at tables 6 (fs keeps tables x fs = 24) it is 2.6e-5 with 94 % of the rows one-hot
    ('saturated', 'w_d256'): dict(tables=6.0, fs=4.0),
    # layer 0 attends from every position, items included, at (tables x kq)^2: one-hot in both layers puts the fp32 oracle
    # off by 1e-3 at any tables >= 3 with kq >= 4.5.  The last layer's input is LayerNorm'd, so its logits follow kq alone: its
    # keys and queries carry the regime (kq 8), layer 0 stays at tables 4, kq 2; fs keeps tables x fs = 24.
    ('saturated', 'o_two_layers'): dict(tables=4.0, kq=2.0, fs=6.0, **{_L1 + 'keys__weight': 4.0, _L1 + 'query__weight': 4.0}),
}
RTM_REGIMES = {
    # the module's own tables are N(0, 1), not 0.5 N(0, 1); its logits are wo . LayerNorm(..), bounded unless wo grows
    'saturated': dict(tables=3.0, kq=4.0, w1=6.0, fs=5.0, transformer_encoder__wo__weight=24.0),
}


def regime_scales(name, regime):
    return dict(REGIMES[regime], **CASE_SCALES.get((regime, name), {}))


# one enc_paths row per attention form and per fused / unfused tail, at its smallest shape
TEM_ROWS = ('e_2_5_20', 's24', 's25', 'e_7_2_12', 's64', 'e_6_4_40_nodrop', 'e_5_33_7', 'e_130_3_12', 'w_d256', 'd256_s25',
            'd512_drop', 'o_two_layers', 'o_item_pos', 'o_avg', 'mf1029')
QEM_CALL = dict(B=50, K=20, L=9, Q=4, model_name='QEM')            # test_gpu_tem_options.CASES['qem']
CASE_NAMES = TEM_ROWS + ('qem',)

MBM = 32                 # replica rows per workgroup of the fused forward (csrc/mlp_fused.hip)
FOLD_LIMIT = 524288.0    # a workgroup's loss partial at or past this poisons the folded hand-off


def row_of(name):
    return next(r for r in enc_paths.ALL_ROWS if r['name'] == name)


def call_of(name):
    """check_against_oracle-style arguments of a case."""
    return dict(QEM_CALL) if name == 'qem' else enc_paths.oracle_call(row_of(name))


def scaled_state_dict(sd, tables=1.0, kq=1.0, w1=1.0, fs=1.0, q_heads=None, heads=8, **named):
    """A copy of a synth.make_state_dict result with groups multiplied: ``tables`` every embedding table, ``kq`` the key and
    query projections' weights, ``w1`` the FFN's first weight, ``fs`` the FS projection's weight; ``q_heads`` = (lo, hi): on
    top of ``kq``, the query projection's rows of head h of ``heads`` are multiplied by lo (hi / lo)^(h / (heads - 1)), so
    that the heads of one sequence run from spread to one-hot; ``named``: factor per exact parameter name with '.' written
    '__' (product_emb__weight=...), applied on top.  Zero (pad) rows stay zero."""
    out = {}
    for k, v in sd.items():
        f = 1.0
        if k.endswith('f_W.weight'):
            f *= fs
        if q_heads is not None and k.endswith('linear_query.weight'):
            lo, hi = q_heads
            hf = torch.tensor([lo * (hi / lo) ** (h / max(1, heads - 1)) for h in range(heads)], dtype=v.dtype)
            v = v * hf.repeat_interleave(v.shape[0] // heads)[:, None]
        if 'emb' in k and k.endswith('.weight') and v.dim() == 2:
            f *= tables
        if k.endswith('linear_keys.weight') or k.endswith('linear_query.weight'):
            f *= kq
        if k.endswith('w_1.weight'):
            f *= w1
        f *= named.get(k.replace('.', '__'), 1.0)
        out[k] = (v * f) if v.dtype.is_floating_point else v.clone()
    unknown = [n for n in named if n.replace('__', '.') not in sd]
    assert not unknown, unknown
    return out


def oracle_f64(fn):
    """Run ``fn()`` — an oracle call on float64 parameters — under a float64 default dtype (the oracle's own constants:
    masks, targets, the positional table's container) and put the default back."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------- item transformer / QEM
def problem(B, K, L, Q, W=1, zero_hist=0.2, P_=700, V=900, edit=None, **over):
    """The inputs of test_gpu_tem_options.check_against_oracle for the same arguments, without a device.  ``edit(p)`` changes
    the finished problem in place (tests/tem_table_rows.py: refilled queries, a heavy item, a pretrained word table)."""
    from prodsearch_amd import default_args, synth
    kw = dict(model_name='item_transformer', embedding_size=128, heads=8, ff_size=256, inter_layers=1, neg_per_pos=K,
              dropout=0.1, uprev_review_limit=L, pv_window_size=W)
    kw.update(over)
    a = default_args(**kw)
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 7, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    batch = synth.make_tem_batch(11, B, P_, V, Q=Q, L=L, W=W, C=9, word_dists=wd, zero_hist_frac=zero_hist)
    ni, nw = synth.sample_negatives(12, B, K, W, P_, wd)
    p = types.SimpleNamespace(a=a, wd=wd, sd=sd, batch=batch, ni=ni, nw=nw, B=B, K=K, L=L, W=W, P_=P_, V=V,
                              qem=a.model_name == 'QEM')
    if edit is not None:
        edit(p)
    return p


OCC_KEYS = ('query_word_emb', 'target_emb', 'neg_emb', 'target_bias', 'neg_bias', 'pos_seq', 'neg_seq',
            'pv_prod', 'pv_wpos', 'pv_wneg', 'pv_bpos', 'pv_bneg')


def oracle_step(p, sd, f64, step=1, seed=666, want_eval=True, want_occ=False):
    """One training step (and the eval scores) of oracle.tem on ``sd`` in float64 or float32, replicated with the product's
    Philox masks of training step ``step``: loss, the [B, K + 1] logits, every gradient, eval scores, and ``keep``.
    ``want_occ``: also ``occ``, d loss / d of every tensor the oracle gathers from a table (OCC_KEYS, those the model has):
    one row of it is one occurrence's contribution to its table row (tests/tem_table_rows.py)."""
    from oracle import tem as otem, philox
    a = p.a

    def run():
        Pm = {k: (v.double() if f64 else v.clone()).requires_grad_(True) for k, v in sd.items()}
        drop = None
        if a.dropout > 0:
            drop = philox.PhiloxDropout(a.dropout, seed, step, p.B, p.K, a.heads, p.L + 1, a.inter_layers,
                                        p.L if a.use_item_pos else 0)
        keep = {}
        if p.qem:
            loss, _, _ = otem.qem_forward(Pm, a, p.batch, p.ni, p.nw, p.V, p.P_, training=True, drop=drop, keep=keep)
        else:
            loss, _, _ = otem.tem_forward(Pm, a, p.batch, p.ni, p.nw, p.V, p.P_, training=True, replicate=drop is not None,
                                          drop=drop, keep=keep)
        occ = None
        if want_occ:
            names = [k for k in OCC_KEYS if k in keep]
            occ = dict(zip(names, torch.autograd.grad(loss, [keep[k] for k in names], retain_graph=True)))
        grads = otem.grads_of(loss, Pm, otem.tem_pad_rows(a, p.V, p.P_))
        out = dict(loss=loss.detach(), grads=grads, keep=keep, occ=occ,
                   logits=torch.cat([keep['pos_scores'].detach()[:, None], keep['neg_scores'].detach()], 1))
        if want_eval:
            with torch.no_grad():
                Pe = {k: v.detach() for k, v in Pm.items()}
                out['eval'] = otem.qem_test(Pe, a, p.batch, p.V, p.P_) if p.qem else otem.tem_test(Pe, a, p.batch, p.V, p.P_)
        return out
    return oracle_f64(run) if f64 else run()


@functools.lru_cache(maxsize=None)
def case(name, regime):
    """(problem, scaled state dict, float64 oracle step, float32 oracle step) of a case in a regime; computed once per
    process and shared — nobody writes to it."""
    p = problem(**call_of(name))
    sd = scaled_state_dict(p.sd, heads=p.a.heads, **regime_scales(name, regime))
    return p, sd, oracle_step(p, sd, True), oracle_step(p, sd, False)


def _rows_at(keep, a, qpos):
    """(softmax rows [n, S], valid-key counts [n]) of the last layer's consumed position, and its GELU inputs."""
    lay = 'layer%d' % (a.inter_layers - 1)
    if 'seq_mask' in keep:                                   # oracle.tem: the negatives' encodes repeat the positives' mask
        pairs = [(keep, keep['seq_mask'])]
        if keep.get('neg'):
            n_neg = keep['neg'][lay]['attn'].shape[0]
            pairs.append((keep['neg'], keep['seq_mask'].repeat_interleave(n_neg // keep['seq_mask'].shape[0], 0)))
    else:                                                    # oracle.rtm
        pairs = [(keep, keep['pos_mask']), (keep['neg'], keep['neg_mask'].reshape(-1, keep['neg_mask'].shape[-1]))]
    att, a1, nv = [], [], []
    for kp, mask in pairs:
        at = kp[lay]['attn'].detach()                     # [N, H, Sq, S]
        N, H, _, S = at.shape
        att.append(at[:, :, qpos, :].reshape(N * H, S))
        nv.append(mask.sum(1).repeat_interleave(H))
        a1.append(kp[lay]['a1'].detach()[:, qpos, :].reshape(-1))
    return torch.cat(att), torch.cat(nv), torch.cat(a1)


def regime_stats(keep, a=None):
    """Where the float64 oracle's step sits: shares of softmax rows (two or more valid keys) whose largest weight is above 0.9 /
    below 2 / S_valid, max |item logit|, share of FS pre-activations beyond +-6, shares of GELU inputs below -6 / above +6.
    Entries a model does not have (QEM: no attention, no FFN; the AVG encoder: no FS projection) are None."""
    logit = torch.cat([keep['pos_scores'].detach().reshape(-1), keep['neg_scores'].detach().reshape(-1)]) \
        if 'pos_scores' in keep else keep['scores'].detach().reshape(-1)
    st = dict(rows=0, peaked=None, spread=None, max_logit=float(logit.abs().max()), fs_sat=None, gelu_lo=None, gelu_hi=None)
    if 'fs_pre' in keep:
        st['fs_sat'] = float((keep['fs_pre'].detach().abs() > 6).double().mean())
    if a is not None and any(k.startswith('layer') for k in keep):
        att, nv, a1 = _rows_at(keep, a, -1 if getattr(a, 'use_item_pos', False) else 0)
        live = nv >= 2
        top = att[live].max(1).values
        st.update(rows=int(live.sum()), peaked=float((top > 0.9).double().mean()),
                  spread=float((top < 2.0 / nv[live].double()).double().mean()),
                  gelu_lo=float((a1 < -6).double().mean()), gelu_hi=float((a1 > 6).double().mean()))
    return st


def check_regime(regime, st):
    """The conditions a regime has to meet on the float64 oracle (stated, not measured; where an entry is None the model has
    no such stage).  Returns the list of the ones that fail."""
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)
    if regime == 'peaked':
        if st['peaked'] is not None:
            need(0.25 <= st['peaked'] <= 0.75, 'softmax rows above 0.9: %.3f not in [0.25, 0.75]' % st['peaked'])
            need(st['spread'] >= 0.05, 'softmax rows below 2 / S_valid: %.3f < 0.05' % st['spread'])
    else:
        if st['peaked'] is not None:
            need(st['peaked'] >= 0.90, 'softmax rows above 0.9: %.3f < 0.90' % st['peaked'])
            need(st['gelu_lo'] >= 0.05 and st['gelu_hi'] >= 0.05, 'GELU inputs beyond -6 / +6: %.3f / %.3f < 0.05'
                 % (st['gelu_lo'], st['gelu_hi']))
        need(st['max_logit'] >= 30, 'max |item logit| %.1f < 30' % st['max_logit'])
        if st['fs_sat'] is not None:
            need(st['fs_sat'] >= 0.20, 'FS pre-activations beyond 6: %.3f < 0.20' % st['fs_sat'])
    return bad


def fmt_stats(st):
    f = lambda v: ' n/a ' if v is None else '%.3f' % v
    return 'rows %d peaked %s spread %s max|logit| %.1f fs>6 %s gelu<-6 %s gelu>6 %s' % (
        st['rows'], f(st['peaked']), f(st['spread']), st['max_logit'], f(st['fs_sat']), f(st['gelu_lo']), f(st['gelu_hi']))


def errors(got, ref, skip=('linear_keys.bias',)):
    """max |got - ref| / max |ref| of the loss, the logits and every gradient ``ref`` has (``got`` / ``ref``: oracle_step
    results or dicts of the same keys); linear_keys.bias is left out as everywhere: its true gradient is 0."""
    from golden_util import rel_err
    out = {'loss': rel_err(got['loss'], ref['loss']), 'logits': rel_err(got['logits'], ref['logits'])}
    for n, g in ref['grads'].items():
        if g is None or n.endswith(skip) or float(g.abs().max()) == 0.0 or got['grads'].get(n) is None:
            continue
        out[n] = rel_err(got['grads'][n], g)
    return out


def worst(errs, keys=None):
    k = max((k for k in errs if keys is None or k in keys), key=lambda k: errs[k])
    return errs[k], k


# ------------------------------------------------------------------------------------------------- review transformer
# tests/test_gpu_rtm_shapes.py's harness (dropout 0, corrupt 0, train_pv False) at its d = 128 pvc and its d = 256 pvc shape
RTM_SHAPES = {'rtm_d128': dict(d=128, heads=8, B=9, K=4, u_lim=9, i_lim=4, WL=128, encoder='pvc'),
              'rtm_d256': dict(d=256, heads=8, B=6, K=2, u_lim=5, i_lim=6, WL=40, encoder='pvc')}
RTM_SEQS_PER_WG = 4      # rtm_score_kernel: a wave per sequence, four per workgroup
RTM_FOLD_TOTAL = 134217728.0   # 2^27: a workgroup's partial times the grid stays below it


def rtm_problem(d, heads, B, K, u_lim, i_lim, WL, encoder, V=1500, RC=900, words=None, train_pv=False, edit=None):
    """The harness's inputs, with the state dict of the module's own initialisation under torch.manual_seed(0) (built on the
    CPU: the initialisation draws there whatever the device).  The global generator is put back.
    tests/rtm_word_rows.py's cases bring their own vocabulary and review count, their own review-word table (``words(rng, V,
    RC, WL)`` -> int64 [RC, WL], review lengths cut with the pad word; the pad review is written here), the PV loss
    (``train_pv``: its sampled words are drawn here, ``neg_words``) and ``edit(batch, rw)``, which changes the finished
    batch in place."""
    from prodsearch_amd import ProductRanker, default_args, synth, rtm_data
    a = default_args(model_name='review_transformer', review_encoder_name=encoder, embedding_size=d, heads=heads,
                     ff_size=2 * d, inter_layers=1, neg_per_pos=K, dropout=0.0, corrupt_rate=0.0, lr=0.0005,
                     review_word_limit=WL, uprev_review_limit=u_lim, iprev_review_limit=i_lim)
    wd = synth.make_word_dists(V)
    rng = synth.rng_for(3)
    if words is None:
        rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
        lens = torch.from_numpy(rng.integers(1, WL + 1, size=RC))
        rw[torch.arange(WL)[None, :] >= lens[:, None]] = V - 1
    else:
        rw = words(rng, V, RC, WL)
    rw[-1] = V - 1
    state = torch.get_rng_state()
    try:
        torch.manual_seed(0)
        m = ProductRanker(a, 'cpu', V, RC, 50, 60, rw, None, word_dists=wd)
    finally:
        torch.set_rng_state(state)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    batch = rtm_data.make_rtm_batch(21, B, K, RC, V, rw, Q=5, u_lim=u_lim, i_lim=i_lim, W=1, train_pv=train_pv,
                                    encoder=encoder, word_dists=wd)
    neg_words = None
    if train_pv:         # the PV loss's sampled words, [B R, W K] with W = 1 (PV.py:57 draws them from word_dists; pad excluded)
        neg_words = torch.from_numpy(synth.rng_for(22).integers(0, V - 1, size=(B * (u_lim + i_lim), K)))
    if edit is not None:
        edit(batch, rw)
    return types.SimpleNamespace(a=a, wd=wd, rw=rw, sd=sd, batch=batch, V=V, RC=RC, B=B, K=K, train_pv=train_pv,
                                 neg_words=neg_words)


def rtm_oracle_step(p, sd, f64):
    """Loss, the [B, K + 1] logits and every gradient of oracle.rtm on ``sd`` in float64 or float32, and ``keep``.  With a
    word-mean review encoder also ``slot_grads``: d loss / d word mean of the positives' [B R, d] and the negatives'
    [B K R, d] review slots."""
    from oracle import rtm as ortm

    def run():
        P = {}
        for k, v in sd.items():
            v = v.double() if (f64 and v.dtype.is_floating_point) else v.clone()
            P[k] = v.requires_grad_(True) if (v.dtype.is_floating_point and not k.endswith('pos_emb.pe')) else v
        keep = {}
        tpv = bool(getattr(p, 'train_pv', False))
        loss, _, _ = ortm.rtm_forward(P, p.a, p.batch, getattr(p, 'neg_words', None), p.V, p.RC, training=True, train_pv=tpv,
                                      keep=keep)
        names = [k for k, v in P.items() if torch.is_tensor(v) and v.requires_grad]
        slots = [keep[k] for k in ('mean_pos', 'mean_neg') if k in keep]
        gs = torch.autograd.grad(loss, [P[k] for k in names] + slots, allow_unused=True)
        out = dict(loss=loss.detach(), logits=keep['scores'].detach(), grads=dict(zip(names, gs)), keep=keep)
        if slots:
            out['slot_grads'] = tuple(gs[len(names):])
        return out
    return oracle_f64(run) if f64 else run()


@functools.lru_cache(maxsize=None)
def rtm_case(name, regime):
    p = rtm_problem(**RTM_SHAPES[name])
    sd = scaled_state_dict(p.sd, heads=p.a.heads, **RTM_REGIMES[regime])
    return p, sd, rtm_oracle_step(p, sd, True), rtm_oracle_step(p, sd, False)


def rtm_wo_factor(p, lo, hi):
    """A factor for transformer_encoder.wo.weight whose largest workgroup partial (four sequences n = b (K + 1) + j) on the
    float64 oracle lies in [lo, hi] x 2^27 / grid (``hi`` None: at least lo x).  The encoder's output does not depend on wo, so
    the logits are f (enc . wo) + bias."""
    r = rtm_oracle_step(p, p.sd, True)
    bias = p.sd['transformer_encoder.wo.bias'].double()
    base, w = r['logits'] - bias, r['keep']['weight'].double()
    grid = (base.numel() + RTM_SEQS_PER_WG - 1) // RTM_SEQS_PER_WG
    limit = RTM_FOLD_TOTAL / grid
    top = lambda f: float(workgroup_partials(w * bce_terms(base * f + bias), RTM_SEQS_PER_WG).max())
    b = 64.0
    while top(b) < (lo if hi is None else hi) * limit:
        b *= 2.0
    if hi is None:
        return b, limit
    a, target = 1.0, 0.5 * (lo + hi) * limit
    for _ in range(60):
        m = 0.5 * (a + b)
        a, b = (m, b) if top(m) < target else (a, m)
    return b, limit


# ------------------------------------------------------------------------------------------------- the loss hand-off
def bce_terms(logits, pos_weight=1.0):
    """The [B, K + 1] loss terms of bce_rank_loss on float64 logits: column 0 is the positive."""
    t = torch.nn.functional.softplus(logits.double())
    t[:, 0] = pos_weight * torch.nn.functional.softplus(-logits[:, 0].double())
    return t


def workgroup_partials(terms, rows_per_wg=MBM):
    """Sums of the loss terms over replica rows 32 w .. 32 w + 31, with m = b (K + 1) + j."""
    flat = terms.reshape(-1)
    n = (flat.numel() + rows_per_wg - 1) // rows_per_wg
    pad = torch.zeros(n * rows_per_wg, dtype=flat.dtype)
    pad[:flat.numel()] = flat
    return pad.view(n, rows_per_wg).sum(1)


def product_factor(base, lo, hi, limit=FOLD_LIMIT, rows_per_wg=MBM, start=64.0):
    """A factor for product_emb.weight (sep_prod_emb: the encoder's inputs do not move; no product bias) whose largest
    workgroup partial lies in [lo, hi] x limit (``hi`` None: at least lo x), from ``base``: the float64 oracle's logits at
    factor 1.  The logits are linear in the factor — enc . (f item) — so a bisection on them finds it; the caller asserts the
    condition on a full oracle step."""
    top = lambda f: float(workgroup_partials(bce_terms(base * f), rows_per_wg).max())
    if hi is None:
        f = start
        while top(f) < lo * limit:
            f *= 2.0
        return f
    a, b = 1.0, start
    while top(b) < hi * limit:
        b *= 2.0
    target = 0.5 * (lo + hi) * limit
    for _ in range(60):
        m = 0.5 * (a + b)
        if top(m) < target:
            a = m
        else:
            b = m
    return b
