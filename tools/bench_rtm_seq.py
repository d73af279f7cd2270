#!/usr/bin/env python3
"""The review transformer's one-pass evaluation in the time-ordered setting: ``evaluate.rank_seq_rtm`` against the chunked path
it replaces, same process, alternating (profiles/rtm_rank_seq.md).

The shape is tools/bench_rtm_cand.py's: C4 (d = 128, 8 heads, ff 512, one layer, 20 + 30 reviews, pvc, 296 k reviews),
P = 10,000 products, B = 24 entries, C = 500 candidates per entry — and the catalogue form (all P products) too.  The
timeline: item i has about N / (H_P (i + 1)) reviews (the bench's Zipf-like popularity: the most popular item ~30,000, the
median item 6), times uniform in [0, 100000), sorted per item; the entries' stamps are drawn from the middle half.  Four forms
of one batch are timed:

    seq_list      rank_seq_rtm over the entries' lists        chunked_list   model.test() on the assembled chunk + ranking chain
    seq_cat       rank_seq_rtm over the catalogue             chunked_cat    20 model.test() calls of 500 + ranking chain

Boxes of one pool differ by several per cent, so only figures of one process are compared; the forms alternate.  The cost of
the search and the window: ``rr_slot_kernel<EPL, true>`` with every stamp at INT64_MAX reads exactly the rows its static form
(``<EPL, false>``) reads from the static catalogue of every item's last 30 reviews, so the two kernels' times (the kernel timer's bound event pairs, a run
each) differ by the lookup alone.  One JSON line per form and round, then the medians.

    python tools/bench_rtm_seq.py [--steps 20] [--warmup 3] [--rounds 5] [--products 10000] [--entries 24] [--cands 500]

``--only seq_list,seq_cat --rounds 1`` under ``rocprofv3 --kernel-trace --stats`` (a run of its own) lists the launches.

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

import bench_rtm_cand as K
import bench_rtm_rank as R
from prodsearch_amd import evaluate, rtm_data, synth

U, I, d = R.U, R.I, R.d
T_SPAN = 100000


def timeline(P, B):
    """(ptr, rids, times, stamps) on the host."""
    rng = synth.rng_for(17)
    w = 1.0 / np.arange(1, P + 1)
    lens = np.maximum(1, np.round(R.RC * w / w.sum())).astype(np.int64)
    ptr = np.zeros(P + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lens)
    N = int(ptr[-1])
    rids = rng.integers(0, R.RC - 1, size=N).astype(np.int64)
    item = np.repeat(np.arange(P, dtype=np.int64), lens)
    t = rng.integers(0, T_SPAN, size=N).astype(np.int64)
    times = t[np.lexsort((t, item))]                                        # sorted inside every item
    stamps = rng.integers(T_SPAN // 4, 3 * T_SPAN // 4, size=B).astype(np.int64)
    return ptr, rids, times, stamps


def windows(ptr, rids, times, stamps):
    """[B, P, I] the review ids every (entry, item) pair reads, then the pad id — numpy's searchsorted on (item, time) keys."""
    P = len(ptr) - 1
    item = np.repeat(np.arange(P, dtype=np.int64), np.diff(ptr))
    big = np.int64(4) * T_SPAN
    keys = item * big + np.clip(times, 0, big - 1)
    out = np.full((len(stamps), P, I), R.RC - 1, dtype=np.int64)
    j = np.arange(I)[None, :]
    for b, s in enumerate(stamps.tolist()):
        cut = np.searchsorted(keys, np.arange(P, dtype=np.int64) * big + min(max(s, -1), big - 1), side='right') - ptr[:-1]
        n = np.minimum(cut, I)
        src = (ptr[:-1] + cut - n)[:, None] + j
        ok = j < n[:, None]
        out[b][ok] = rids[np.where(ok, src, 0)][ok]
    return torch.from_numpy(out)


def chunk_of(win, cands, rb):
    """The ProdSearchTestBatch of items ``cands`` [B, Cw] (host), every entry's rows from its own windows ``win`` [B, P, I]."""
    pad = R.RC - 1
    B, Cw = cands.shape
    u_r, qw = rb.u_ridxs.cpu(), rb.query_word_idxs.cpu()
    rows = win[torch.arange(B)[:, None], cands]                             # [B, Cw, I]
    lead = lambda ids: torch.where((ids != pad).all(-1), torch.full(ids.shape[:-1], ids.shape[-1]), (ids == pad).int().argmax(-1))
    nu, ni = lead(u_r), lead(rows)
    Rr = U + I
    pos = torch.arange(Rr)[None, None, :]
    from_u = (pos < nu[:, None, None]).expand(B, Cw, Rr)
    j = (pos - nu[:, None, None]).clamp(0, I - 1).expand(B, Cw, Rr)
    it = torch.gather(rows, 2, j)
    from_i = ~from_u & (pos - nu[:, None, None] < ni[:, :, None])
    ur = u_r[:, None, :].expand(-1, Cw, -1).gather(2, pos.clamp(max=U - 1).expand(B, Cw, Rr))
    ridx = torch.where(from_u, ur, torch.where(from_i, it, torch.full_like(it, pad)))
    seg = torch.full((B, Cw, Rr + 1), 3, dtype=torch.int64)
    seg[:, :, 0] = 0
    seg[:, :, 1:] = torch.where(from_u, 1, torch.where(from_i, 2, 3))
    n_rows = int(torch.minimum(ni, (Rr - nu)[:, None]).sum())
    return rtm_data.ProdSearchTestBatch(rb.query_idxs, rb.user_idxs, rb.target_prod_idxs.cpu(), cands, qw, ridx.contiguous(), seg,
                                        to_tensor=False), n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--products', type=int, default=10000)
    ap.add_argument('--entries', type=int, default=24)
    ap.add_argument('--cands', type=int, default=500)
    ap.add_argument('--topk', type=int, default=100)
    ap.add_argument('--only', default='seq_list,chunked_list,seq_cat,chunked_cat')
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rtm_seq: no GPU (a timing needs one)")
    P, B, Cw = o.products, o.entries, o.cands
    m, item_r, rb, _ = R.build(P, B, with_chunks=False)
    ptr, rids, times, stamps = timeline(P, B)
    print(json.dumps(dict(timeline_reviews=int(ptr[-1]), longest_item=int(np.diff(ptr).max()), median_item=int(np.median(np.diff(ptr))))),
          flush=True)
    listed, _, _ = K.lists_and_chunk(P, B, Cw, item_r, rb)                  # (the lists alone: the chunk is cut per entry below)
    cands = listed.candi_prod_idxs
    only = o.only.split(',')
    need_chunks = any(n.startswith('chunked') for n in only)
    chunk_list = chunks_cat = None
    rows_list = 0
    if need_chunks:
        win = windows(ptr, rids, times, stamps)
        chunk_list, rows_list = chunk_of(win, cands, rb)
        chunk_list = chunk_list.to('cuda')
        chunks_cat = []
        for lo in range(0, P, R.CHUNK):
            ids = torch.arange(lo, min(P, lo + R.CHUNK))
            chunks_cat.append((ids.cuda(), chunk_of(win, ids[None].expand(B, -1).contiguous(), rb)[0].to('cuda')))
        del win
    t_dev = lambda x: torch.from_numpy(x).cuda()
    mk = lambda lists, st: rtm_data.ProdSearchRankBatch(rb.query_idxs, rb.user_idxs, rb.target_prod_idxs, rb.query_word_idxs, rb.u_ridxs,
                                                        lists, t_dev(st)).to('cuda')
    b_list, b_cat = mk(cands, stamps), mk(None, stamps)
    b_list_max = mk(cands, np.full(B, np.iinfo(np.int64).max, dtype=np.int64))
    m.get_review_embeddings()
    index = m.timeline_index(t_dev(ptr), t_dev(rids), t_dev(times))
    # the static catalogue an INT64_MAX stamp sees: the last I reviews of every item
    last = np.full((P, I), R.RC - 1, dtype=np.int64)
    for p in range(P):
        s = rids[ptr[p]:ptr[p + 1]][-I:]
        last[p, :len(s)] = s
    st_index = m.catalogue_index(t_dev(last))
    st_listed = listed.to('cuda')
    torch.cuda.synchronize()
    cd, tg = b_list.candi_prod_idxs, b_list.target_prod_idxs
    forms = {'seq_list': lambda: evaluate.rank_seq_rtm(m, index, b_list, o.topk),
             'chunked_list': lambda: K.chunked(m, chunk_list, cd, tg, o.topk),
             'seq_cat': lambda: evaluate.rank_seq_rtm(m, index, b_cat, o.topk),
             'chunked_cat': lambda: R.chunked(m, rb, chunks_cat, P, o.topk)}
    forms = {n: forms[n] for n in only}
    if need_chunks:          # the forms agree (the suite's eval bound) before anything is timed
        for a, b in (('seq_list', 'chunked_list'), ('seq_cat', 'chunked_cat')):
            if a in forms and b in forms:
                kw = dict(return_scores=True)
                s1 = evaluate.rank_seq_rtm(m, index, b_list if a == 'seq_list' else b_cat, o.topk, **kw)
                s0 = forms[b]()
                err = float((s1[3] - s0[3]).abs().max() / s0[3].abs().max())
                print(json.dumps(dict(check='%s vs %s scores' % (a, b), rel_err=err,
                                      equal_ranks='%d of %d' % (int((s1[2].long() == s0[2]).sum()), B))), flush=True)
                assert err < 1e-4, err
    # ... and with every stamp at INT64_MAX the time-ordered kernel gives the static kernel's bits
    s_max = evaluate.rank_seq_rtm(m, index, b_list_max, o.topk, return_scores=True)[3]
    s_st = evaluate.rank_candidates_rtm(m, st_index, st_listed, o.topk, return_scores=True)[3]
    print(json.dumps(dict(check='rr_slot_kernel: time-ordered at INT64_MAX vs static', equal_bits=bool(torch.equal(s_max, s_st)))), flush=True)
    assert torch.equal(s_max, s_st)
    for f in forms.values():
        R.timed(f, o.warmup)
    res = {n: [] for n in forms}
    names = list(forms)
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            ms = R.timed(forms[n], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(form=n, round=r, ms_per_batch=round(ms, 4))), flush=True)
    med = {n: statistics.median(v) for n, v in res.items()}
    if not need_chunks:      # (a run for a kernel trace: the one-pass forms alone, no stage timer)
        for n in names:
            print('%-12s %9.3f ms/batch' % (n, med[n]))
        return
    many = lambda f: (lambda: [f() for _ in range(o.steps)])
    seq_us, _ = R.stage_us('rtm_rank_seq', many(forms['seq_list']))
    seq_max_us, _ = R.stage_us('rtm_rank_seq', many(lambda: evaluate.rank_seq_rtm(m, index, b_list_max, o.topk)))
    cand_us, _ = R.stage_us('rtm_rank_cand', many(lambda: evaluate.rank_candidates_rtm(m, st_index, st_listed, o.topk)))
    cat_us, n_cat = R.stage_us('rtm_rank_seq', many(forms['seq_cat']))
    pairs = B * Cw
    print('# median of %d rounds, %d batches each: P=%d B=%d C=%d R=%d+%d d=%d H=%d ff=512 pvc, %d reviews in the timeline, top-%d'
          % (o.rounds, o.steps, P, B, Cw, U, I, d, R.H, int(ptr[-1]), o.topk))
    out = dict(pairs=pairs, review_rows_list=rows_list)
    for a, b in (('seq_list', 'chunked_list'), ('seq_cat', 'chunked_cat')):
        if a in med and b in med:
            print('%-12s %9.3f ms/batch (min %.3f, max %.3f)' % (a, med[a], min(res[a]), max(res[a])))
            print('%-12s %9.3f ms/batch (min %.3f, max %.3f)   ratio %.2fx' % (b, med[b], min(res[b]), max(res[b]), med[b] / med[a]))
            assert min(res[b]) > max(res[a]), "the one-pass form must be faster by more than the spread of the rounds"
            out.update({a + '_ms': med[a], b + '_ms': med[b], a + '_ratio': med[b] / med[a]})
    print('rr_slot_kernel (time-ordered) %.1f us per %d pairs = %.2f ns per pair (the entries\' own stamps, %d review rows)'
          % (seq_us, pairs, 1e3 * seq_us / pairs, rows_list))
    print('same rows: time-ordered at INT64_MAX %.1f us = %.2f ns per pair, the static form on the static catalogue %.1f us = %.2f ns '
          'per pair -> the search and the window cost %.1f us, %.2f ns per pair'
          % (seq_max_us, 1e3 * seq_max_us / pairs, cand_us, 1e3 * cand_us / pairs, seq_max_us - cand_us, 1e3 * (seq_max_us - cand_us) / pairs))
    n_cat //= o.steps
    print('catalogue form: rr_slot_kernel (time-ordered) %.1f us x %d passes = %.2f ns per pair over %d pairs'
          % (cat_us, n_cat, 1e3 * cat_us * n_cat / (B * P), B * P))
    out.update(seq_us=seq_us, seq_max_us=seq_max_us, cand_us=cand_us, cat_us=cat_us, cat_passes=n_cat)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
