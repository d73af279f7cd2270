#!/usr/bin/env python3
"""The review transformer over the whole catalogue: ``evaluate.rank_all_rtm`` against the chunked path it replaces, same process,
alternating (profiles/rtm_rank_all.md).

At the C4 shape (BASELINE configs[3]: d = 128, 8 heads, ff 512, one layer, 20 + 30 reviews, pvc, 296 k reviews), P = 10,000
products and B = 24 entries, two forms of one evaluation batch are timed:

    one_pass   rank_all_rtm: entry side once, then passes of pair kernel -> per-pair tail -> head, selection on the device
    chunked    what Trainer._scores_candidates does: 20 model.test() calls of 500 candidates + the torch ranking chain

and, once, the per-evaluation projection (``model.catalogue_index``).  Boxes of one pool differ by several per cent, so only
figures of one process are compared; the two forms alternate.  Per-stage times of the one-pass form come from the kernel
timer's bound event pairs (``ps_ktimer_arm``: the pair kernel and the fused tail, a run each).  One JSON line per form and
round, then the medians.

    python tools/bench_rtm_rank.py [--steps 5] [--warmup 2] [--rounds 5] [--products 10000] [--entries 24] [--only one_pass]

``--only one_pass --rounds 1`` under ``rocprofv3 --kernel-trace --stats`` (a run of its own) lists the form's launches.

In a job script every GPU step gets its own ``timeout`` and the steps are chained with ``&&``.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from prodsearch_amd import ProductRanker, _lib, default_args, evaluate, rtm_data, synth

U, I, WL, d, H, V, RC, CHUNK = 20, 30, 100, 128, 8, 32387, 296000, 500


def build(P, B, with_chunks=True):
    a = default_args(model_name='review_transformer', review_encoder_name='pvc', embedding_size=d, heads=H, ff_size=512,
                     inter_layers=1, dropout=0.1, corrupt_rate=0.9, review_word_limit=WL, uprev_review_limit=U,
                     iprev_review_limit=I, candi_batch_size=CHUNK)
    rng = synth.rng_for(5)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
    lens = torch.from_numpy(rng.integers(WL // 4, WL + 1, size=RC))
    rw[torch.arange(WL)[None, :] >= lens[:, None]] = V - 1
    rw[-1] = V - 1
    torch.manual_seed(1234)
    m = ProductRanker(a, 'cuda', V, RC, P, 1000, rw, None, word_dists=None)
    m.eval()
    pad = RC - 1

    def lists(n, width, lo):
        ids = torch.from_numpy(rng.integers(0, pad, size=(n, width)))
        cnt = torch.from_numpy(rng.integers(lo, width + 1, size=n))
        ids[torch.arange(width)[None, :] >= cnt[:, None]] = pad
        return ids, cnt
    item_r, ni = lists(P, I, 1)
    u_r, nu = lists(B, U, 0)
    qw = torch.from_numpy(rng.integers(0, V - 1, size=(B, 8)))
    target = torch.from_numpy(rng.integers(0, P, size=B))
    rb = rtm_data.ProdSearchRankBatch(list(range(B)), list(range(B)), target, qw, u_r).to('cuda')
    # the chunked path's batches: [user's reviews | item's reviews | pad] per (entry, candidate), as the test collate builds them
    R = U + I
    pos = torch.arange(R)[None, None, :]
    chunks = []
    for lo in range(0, P if with_chunks else 0, CHUNK):      # (tools/bench_rtm_cand.py assembles its own chunk)
        ids = torch.arange(lo, min(P, lo + CHUNK))
        from_u = pos < nu[:, None, None]
        j = (pos - nu[:, None, None]).clamp(0, I - 1).expand(B, len(ids), R)
        it = torch.gather(item_r[ids][None].expand(B, -1, -1), 2, j)
        from_i = ~from_u & (pos - nu[:, None, None] < ni[ids][None, :, None])
        ridx = torch.where(from_u, u_r[:, None, :].expand(-1, len(ids), -1).gather(2, pos.clamp(max=U - 1).expand(B, len(ids), R)),
                           torch.where(from_i, it, torch.full_like(it, pad)))
        seg = torch.full((B, len(ids), R + 1), 3, dtype=torch.int64)
        seg[:, :, 0] = 0
        seg[:, :, 1:] = torch.where(from_u, 1, torch.where(from_i, 2, 3))
        chunks.append((ids.cuda(), rtm_data.ProdSearchTestBatch(rb.query_idxs, rb.user_idxs, target, ids[None].expand(B, -1), qw,
                                                                ridx.contiguous(), seg, to_tensor=False).to('cuda')))
    return m, item_r.cuda(), rb, chunks


def chunked(m, rb, chunks, P, topk):
    """Trainer._scores_candidates over all products: model.test per chunk, then its ranking chain."""
    with torch.no_grad():
        sc = torch.cat([m.test(b) for _, b in chunks], 1)
        ids = torch.arange(P, device=sc.device)[None, :].expand(sc.shape[0], -1)
        hit = ids == rb.target_prod_idxs[:, None]
        pos = hit.float().argmax(1)
        st = sc.gather(1, pos[:, None])
        col = torch.arange(P, device=sc.device)[None, :]
        ahead = (sc > st) | ((sc == st) & (col < pos[:, None]))
        rank = torch.where(hit.any(1), ahead.sum(1) + 1, torch.zeros_like(pos))
        ts, ti = sc.topk(topk, dim=1)
    return ti, ts, rank, sc


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def stage_us(tag, fn):
    lib = _lib.load()
    _lib.check(lib.ps_ktimer_arm(tag.encode(), 256), 'ps_ktimer_arm')
    fn()
    avg, mn, n = C.c_double(0), C.c_double(0), C.c_int32(0)
    _lib.check(lib.ps_ktimer_read(C.byref(avg), C.byref(mn), C.byref(n)), 'ps_ktimer_read')
    return avg.value, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--products', type=int, default=10000)
    ap.add_argument('--entries', type=int, default=24)
    ap.add_argument('--topk', type=int, default=100)
    ap.add_argument('--only', default='one_pass,chunked')
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rtm_rank: no GPU (a timing needs one)")
    P, B = o.products, o.entries
    m, item_r, rb, chunks = build(P, B)
    m.get_review_embeddings()
    torch.cuda.synchronize()

    def project():
        m.__dict__.pop('_cat_index', None)
        return m.catalogue_index(item_r)
    index = project()
    forms = {'one_pass': lambda: evaluate.rank_all_rtm(m, index, rb, o.topk),
             'chunked': lambda: chunked(m, rb, chunks, P, o.topk)}
    forms = {n: forms[n] for n in o.only.split(',')}
    if len(forms) == 2:      # the two forms agree (the suite's eval bound) before anything is timed
        s1 = evaluate.rank_all_rtm(m, index, rb, o.topk, return_scores=True)[3]
        s0 = chunked(m, rb, chunks, P, o.topk)[3]
        err = float((s1 - s0).abs().max() / s0.abs().max())
        print(json.dumps(dict(check='one_pass vs chunked scores', rel_err=err)), flush=True)
        assert err < 1e-4, err
    for f in forms.values():
        timed(f, o.warmup)
    res = {n: [] for n in forms}
    names = list(forms)
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            ms = timed(forms[n], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(form=n, round=r, ms_per_batch=round(ms, 4))), flush=True)
    if len(forms) < 2:       # (a run for a kernel trace: one form alone, no stage timer)
        for n in names:
            print('%-9s %9.3f ms/batch' % (n, statistics.median(res[n])))
        return
    proj = [timed(project, 1) for _ in range(3)]
    pair_us, n_pair = stage_us('rtm_rank_pair', forms['one_pass'])
    tail_us, n_tail = stage_us('mlp_fwd', forms['one_pass'])
    one, chk = statistics.median(res['one_pass']), statistics.median(res['chunked'])
    print('# median of %d rounds, %d batches each: P=%d B=%d R=%d+%d d=%d H=%d ff=512 pvc, %d reviews, top-%d'
          % (o.rounds, o.steps, P, B, U, I, d, H, RC, o.topk))
    print('one_pass  %9.3f ms/batch (min %.3f, max %.3f)' % (one, min(res['one_pass']), max(res['one_pass'])))
    print('chunked   %9.3f ms/batch (min %.3f, max %.3f)   ratio %.2fx' % (chk, min(res['chunked']), max(res['chunked']), chk / one))
    print('projection (once per evaluation) %.3f ms (min of 3: %.3f)' % (statistics.median(proj), min(proj)))
    print('per pass: pair kernel %.1f us x %d, fused tail %.1f us x %d -> tail share of the two %.1f %%'
          % (pair_us, n_pair, tail_us, n_tail, 100.0 * tail_us * n_tail / max(1e-9, tail_us * n_tail + pair_us * n_pair)))
    print(json.dumps(dict(one_pass_ms=one, chunked_ms=chk, ratio=chk / one, projection_ms=statistics.median(proj),
                          pair_us=pair_us, tail_us=tail_us, passes=n_pair)))


if __name__ == '__main__':
    main()
