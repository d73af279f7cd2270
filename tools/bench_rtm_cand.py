#!/usr/bin/env python3
"""The review transformer over per-entry candidate lists: ``evaluate.rank_candidates_rtm`` against the chunked path it replaces,
same process, alternating (profiles/rtm_rank_candidates.md).

The shape is validation's: C4 (d = 128, 8 heads, ff 512, one layer, 20 + 30 reviews, pvc, 296 k reviews), P = 10,000 products,
B = 24 entries, C = 500 candidates per entry — 499 drawn without replacement from a Zipf-like product distribution plus the
target, as ``ProdSearchDataset`` draws them for ``--valid_candi_size 500``.  Two forms of one validation batch are timed:

    one_pass   rank_candidates_rtm: entry side once, rr_slot_kernel -> per-pair tail -> head, selection on the device
    chunked    what Trainer._scores_candidates does: one model.test() call on the assembled chunk + its torch ranking chain

Boxes of one pool differ by several per cent, so only figures of one process are compared; the two forms alternate.  The
slot kernel's (stage ``rtm_rank_cand``) and the fused tail's durations come from the kernel timer's bound event pairs (``ps_ktimer_arm``), a run
each.  One JSON line per form and round, then the medians.

    python tools/bench_rtm_cand.py [--steps 20] [--warmup 3] [--rounds 5] [--products 10000] [--entries 24] [--cands 500]

``--only one_pass --rounds 1`` under ``rocprofv3 --kernel-trace --stats`` (a run of its own) lists the form's launches.

In a job script every GPU step gets its own ``timeout`` and the steps are chained with ``&&``.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bench_rtm_rank as R
from prodsearch_amd import evaluate, rtm_data, synth

U, I, d = R.U, R.I, R.d


def lists_and_chunk(P, B, Cw, item_r, rb):
    """[B, Cw] candidate lists and the ProdSearchTestBatch the chunked path reads for them (host tensors)."""
    rng = synth.rng_for(9)
    p = 1.0 / np.arange(1, P + 1)
    p /= p.sum()
    target = rb.target_prod_idxs.cpu()
    cands = np.stack([np.append(rng.choice(P, size=Cw - 1, replace=False, p=p), int(target[b])) for b in range(B)]).astype(np.int64)
    cands = torch.from_numpy(cands)
    pad = R.RC - 1
    item_r, u_r, qw = item_r.cpu(), rb.u_ridxs.cpu(), rb.query_word_idxs.cpu()
    lead = lambda ids: torch.where((ids != pad).all(1), torch.full((ids.shape[0],), ids.shape[1]), (ids == pad).int().argmax(1))
    nu, ni = lead(u_r), lead(item_r)
    Rr = U + I
    pos = torch.arange(Rr)[None, None, :]
    from_u = (pos < nu[:, None, None]).expand(B, Cw, Rr)
    j = (pos - nu[:, None, None]).clamp(0, I - 1).expand(B, Cw, Rr)
    it = torch.gather(item_r[cands], 2, j)
    from_i = ~from_u & (pos - nu[:, None, None] < ni[cands][:, :, None])
    ur = u_r[:, None, :].expand(-1, Cw, -1).gather(2, pos.clamp(max=U - 1).expand(B, Cw, Rr))
    ridx = torch.where(from_u, ur, torch.where(from_i, it, torch.full_like(it, pad)))
    seg = torch.full((B, Cw, Rr + 1), 3, dtype=torch.int64)
    seg[:, :, 0] = 0
    seg[:, :, 1:] = torch.where(from_u, 1, torch.where(from_i, 2, 3))
    chunk = rtm_data.ProdSearchTestBatch(rb.query_idxs, rb.user_idxs, target, cands, qw, ridx.contiguous(), seg, to_tensor=False)
    listed = rtm_data.ProdSearchRankBatch(rb.query_idxs, rb.user_idxs, target, qw, u_r, cands)
    # review rows a batch reads: K and V, d floats each, per live review of every listed item
    rows = int(torch.minimum(ni[cands], (Rr - nu)[:, None]).sum())
    return listed, chunk, rows


def chunked(m, chunk, cands, target, topk):
    """Trainer._scores_candidates for one batch whose lists fit one chunk: model.test, then its ranking chain."""
    with torch.no_grad():
        sc = m.test(chunk)
        sc = sc.masked_fill(cands < 0, float('-inf'))
        hit = cands == target[:, None]
        found = hit.any(1)
        pos = hit.float().argmax(1)
        st = sc.gather(1, pos[:, None])
        col = torch.arange(sc.shape[1], device=sc.device)[None, :]
        ahead = (sc > st) | ((sc == st) & (col < pos[:, None]))
        rank = torch.where(found, ahead.sum(1) + 1, torch.zeros_like(pos))
        ts, ti = sc.topk(min(topk, sc.shape[1]), dim=1)
    return cands.gather(1, ti), ts, rank, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--products', type=int, default=10000)
    ap.add_argument('--entries', type=int, default=24)
    ap.add_argument('--cands', type=int, default=500)
    ap.add_argument('--topk', type=int, default=100)
    ap.add_argument('--only', default='one_pass,chunked')
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rtm_cand: no GPU (a timing needs one)")
    P, B, Cw = o.products, o.entries, o.cands
    m, item_r, rb, _ = R.build(P, B, with_chunks=False)
    listed, chunk, rows = lists_and_chunk(P, B, Cw, item_r, rb)
    listed, chunk = listed.to('cuda'), chunk.to('cuda')
    m.get_review_embeddings()
    index = m.catalogue_index(item_r)
    torch.cuda.synchronize()
    cands, target = listed.candi_prod_idxs, listed.target_prod_idxs
    forms = {'one_pass': lambda: evaluate.rank_candidates_rtm(m, index, listed, o.topk),
             'chunked': lambda: chunked(m, chunk, cands, target, o.topk)}
    forms = {n: forms[n] for n in o.only.split(',')}
    if len(forms) == 2:      # the two forms agree (the suite's eval bound; equal ranks) before anything is timed
        t1 = evaluate.rank_candidates_rtm(m, index, listed, o.topk, return_scores=True)
        t0 = chunked(m, chunk, cands, target, o.topk)
        err = float((t1[3] - t0[3]).abs().max() / t0[3].abs().max())
        same_rank = int((t1[2].long() == t0[2]).sum())
        print(json.dumps(dict(check='one_pass vs chunked scores', rel_err=err, equal_ranks='%d of %d' % (same_rank, B))), flush=True)
        assert err < 1e-4, err
    for f in forms.values():
        R.timed(f, o.warmup)
    res = {n: [] for n in forms}
    names = list(forms)
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            ms = R.timed(forms[n], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(form=n, round=r, ms_per_batch=round(ms, 4))), flush=True)
    if len(forms) < 2:       # (a run for a kernel trace: one form alone, no stage timer)
        for n in names:
            print('%-9s %9.3f ms/batch' % (n, statistics.median(res[n])))
        return
    many = lambda: [forms['one_pass']() for _ in range(o.steps)]          # (one launch per batch: a sample per batch)
    cand_us, n_cand = R.stage_us('rtm_rank_cand', many)
    tail_us, n_tail = R.stage_us('mlp_fwd', many)
    n_cand, n_tail = n_cand // o.steps, n_tail // o.steps
    one, chk = statistics.median(res['one_pass']), statistics.median(res['chunked'])
    pairs = B * Cw
    row_bytes = rows * 2 * d * 4
    print('# median of %d rounds, %d batches each: P=%d B=%d C=%d R=%d+%d d=%d H=%d ff=512 pvc, %d reviews, top-%d'
          % (o.rounds, o.steps, P, B, Cw, U, I, d, R.H, R.RC, o.topk))
    print('one_pass  %9.3f ms/batch (min %.3f, max %.3f)' % (one, min(res['one_pass']), max(res['one_pass'])))
    print('chunked   %9.3f ms/batch (min %.3f, max %.3f)   ratio %.2fx' % (chk, min(res['chunked']), max(res['chunked']), chk / one))
    print('rr_slot_kernel (static lists) %.1f us x %d: %.2f ns per pair over %d pairs (rr_pair_kernel: 76 us per 32,760 pairs = 2.32 ns); '
          '%d review rows, %.1f MB of K / V rows -> %.2f TB/s'
          % (cand_us, n_cand, 1e3 * cand_us / pairs, pairs, rows, row_bytes / 1e6, row_bytes / max(1e-9, cand_us) / 1e6))
    print('fused tail %.1f us x %d -> tail share of the two %.1f %%, of the batch %.1f %%'
          % (tail_us, n_tail, 100.0 * tail_us * n_tail / max(1e-9, tail_us * n_tail + cand_us * n_cand),
             100.0 * tail_us * n_tail / (1e3 * one)))
    print(json.dumps(dict(one_pass_ms=one, chunked_ms=chk, ratio=chk / one, cand_us=cand_us, tail_us=tail_us, passes=n_cand, pairs=pairs,
                          review_rows=rows, row_bytes=row_bytes)))


if __name__ == '__main__':
    main()
