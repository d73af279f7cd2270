"""Shared by tests/test_rtm_seq_cpu.py and tests/test_gpu_rtm_seq.py: the review transformer's one-pass evaluation in the
time-ordered setting (``evaluate.rank_seq_rtm``).  The entries, the models and the host oracles are those of
tests/rtm_rank_util.py (``make_case`` / ``build_model`` / ``factorised_scores``); this file adds the timeline, the stamps, the
lists and what is stated about them.

* ``make_timeline``: every item's time-ordered review sequence (a CSR with times) and the entries' stamps, with the special
  items and stamps the GPU file checks one by one.
* ``cat_of``: the static ``[P, W]`` catalogue ONE entry sees, by ``np.searchsorted(side='right')`` — a second, independent
  statement of the rule the kernel's wave-wide search implements.  ``fault``: what a search with one mistake would see.
* ``make_lists``: the entries' candidate lists.  ``oracle_seq`` / ``factorised_seq``: ``oracle.rtm.rtm_test`` and the §8b.1
  factorisation, entry by entry on ``cat_of``.
* ``CASES`` / ``PLAN`` / ``YARDSTICK`` / ``bound``: the cases of both files, the fields of ``ps_rtm_rank_seq_plan`` each was
  written for, what fp32 on the host costs each of them, and the per-entry bound that follows.
"""
import copy
import functools
import types

import numpy as np
import torch

import rtm_cand_util as K
import rtm_rank_util as U
from prodsearch_amd import rtm_data, synth

TOL = U.TOL
YARD_FACTOR = U.YARD_FACTOR
BAND_CAP = K.BAND_CAP
I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
T_MAX = 60               # times are drawn from [0, T_MAX): small integers, so that runs of equal times exist
# items 0 .. 6: none; exactly W (the window); 70 (two search rounds, a window that is not at the front); 4,100; 64 and 65 (the
# one-round / two-round boundary on either side); 4,200.  The search drops the probed element from the range it keeps, so two
# rounds reach 64 * 65 = 4,160 reviews: item 3 is searched in two rounds and item 6 is the one that takes three.
LONG_ITEMS = {2: 70, 3: 4100, 4: 64, 5: 65, 6: 4200}
PAD_ITEM = 5             # the item with the pad id inside its last window: the second-to-last of its reviews
FAULTS = ('cut_left', 'first_I', 'no_stamp')


def window_of(c):
    """The window width of a case: ``iprev_review_limit`` (``shape->I``), not the width of the static case's lists."""
    return int(c.a.iprev_review_limit)


def make_timeline(c, seed=201):
    """-> namespace(ptr [P + 1], rids [N], times [N], stamps [B], tie_time).  Review ids are drawn from the whole table and
    may repeat across items (the oracle runs with ``ids_from_reviews=True``: a review's author and item come from
    ``review_u_p``).  Stamps: entry 0 INT64_MIN (no item has a review yet), entry 1 INT64_MAX (every review), entry 2 exactly a
    time that occurs in a run of equal times of item 2 (``bisect_right`` takes the whole run), the rest mid-range."""
    rng = synth.rng_for(seed)
    W, pad = window_of(c), c.RC - 1
    assert c.P > 7 and c.B >= 4
    lens = [0, W] + [LONG_ITEMS[i] for i in range(2, 7)] + [int(rng.integers(1, 3 * W + 1)) for _ in range(7, c.P)]
    ptr = np.zeros(c.P + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lens)
    N = int(ptr[-1])
    rids = rng.integers(0, pad, size=N).astype(np.int64)
    times = np.concatenate([np.sort(rng.integers(0, T_MAX, size=n)) for n in lens]).astype(np.int64)
    rids[ptr[PAD_ITEM + 1] - 2] = pad
    t2 = times[ptr[2]:ptr[3]]
    vals, counts = np.unique(t2, return_counts=True)
    runs = vals[(counts >= 2) & (vals > T_MAX // 4) & (vals < 3 * T_MAX // 4)]
    tie = int(runs[len(runs) // 2])
    stamps = np.empty(c.B, dtype=np.int64)
    stamps[:3] = (I64_MIN, I64_MAX, tie)
    stamps[3:] = rng.integers(T_MAX // 4, 3 * T_MAX // 4, size=c.B - 3)
    return types.SimpleNamespace(ptr=ptr, rids=rids, times=times, stamps=stamps, tie_time=tie, N=N)


def cat_of(tl, stamp, W, pad, fault=None):
    """[P, W] review ids, then the pad id: per item the last ``W`` of its reviews whose time is <= ``stamp``
    (prod_search_dataloader.py:73-77, 138-147: ``i_r_seq[item][:bisect_right(times, stamp)][-W:]``).
    ``fault`` (the sensitivity test alone): 'cut_left' ``bisect_left`` (differs only where the stamp equals a time);
    'first_I' the first ``W`` of the prefix, not the last; 'no_stamp' the static last ``W`` of the whole sequence."""
    assert fault is None or fault in FAULTS
    P = len(tl.ptr) - 1
    out = np.full((P, W), pad, dtype=np.int64)
    for p in range(P):
        lo, hi = int(tl.ptr[p]), int(tl.ptr[p + 1])
        cut = int(np.searchsorted(tl.times[lo:hi], stamp, side='left' if fault == 'cut_left' else 'right'))
        seq = tl.rids[lo:hi] if fault == 'no_stamp' else tl.rids[lo:lo + cut]
        s = seq[:W] if fault == 'first_I' else seq[len(seq) - min(W, len(seq)):]
        out[p, :len(s)] = s
    return out


def make_lists(c, C=12, seed=101):
    """[B, C] item ids, -1 padding a ragged list.  Entry 0 (INT64_MIN: every item scores alike, so its whole list is one exact
    tie) lists the four items 0..3 only; entry 1 (INT64_MAX) lists the long items, the pad-window item, its target at columns 2
    AND 7, an id past the catalogue at column 4 and a -1 at column 5; entry 2 (the tie stamp) opens with items 2..6; the rest
    are plain draws of 6..C items.  The last entry's target is outside [0, P) already (``make_case``)."""
    rng = synth.rng_for(seed)
    out = np.full((c.B, C), -1, np.int64)
    out[0, :4] = (0, 1, 2, 3)
    t1 = int(c.target[1])
    assert C >= 12
    out[1, :12] = (3, 5, t1, 6, c.P + 3, -1, 2, t1, 4, 1, 0, int(rng.integers(7, c.P)))
    rest = rng.permutation(np.arange(7, c.P))
    out[2, :5] = (2, 3, 4, 5, 6)
    out[2, 5:] = rest[:C - 5]
    for b in range(3, c.B):
        n = int(rng.integers(6, C + 1))
        out[b, :n] = rng.choice(c.P, size=n, replace=False)
    return out


def entry_chunk(c, e, item_r, cols, ids_from_reviews=True):
    """The ``ProdSearchTestBatch`` of ONE entry over the items ``cols`` (-1: a padded slot) of its own catalogue ``item_r``."""
    cols = np.asarray(cols, dtype=np.int64)[None]
    return U.assemble_chunk(c.qw[e:e + 1], c.u_r[e:e + 1], c.users[e:e + 1], item_r, cols, c.review_u_p, c.n_users, c.P, c.RC - 1,
                            ids_from_reviews=ids_from_reviews, limit=c.T)


def oracle_seq(c, sd, tl, f64=False, fault=None):
    """[B, P] scores of ``oracle.rtm.rtm_test``: entry by entry over the whole catalogue as that entry's stamp cuts it."""
    from oracle import rtm as ortm
    P = {k: (v.double() if f64 and v.dtype.is_floating_point else v) for k, v in sd.items()}
    rev = ortm.rtm_review_embeddings(P, c.a, c.rw, c.V)
    out = torch.empty(c.B, c.P, dtype=rev.dtype)
    for e in range(c.B):
        item_r = cat_of(tl, int(tl.stamps[e]), window_of(c), c.RC - 1, fault)
        out[e] = ortm.rtm_test(P, c.a, entry_chunk(c, e, item_r, np.arange(c.P)), rev, c.V, c.RC)[0]
    return out, P, rev


def factorised_seq(c, P, rev, tl, fault=None):
    """[B, P] scores of the §8b.1 factorisation (``rtm_rank_util.factorised_scores``), entry by entry on ``cat_of``; and per
    entry whether ``fault`` changes the catalogue the entry sees at all."""
    out, acts = [], []
    for e in range(c.B):
        true = cat_of(tl, int(tl.stamps[e]), window_of(c), c.RC - 1)
        item_r = cat_of(tl, int(tl.stamps[e]), window_of(c), c.RC - 1, fault)
        acts.append(not np.array_equal(true, item_r))
        out.append(U.factorised_scores(P, c.a, c.qw[e:e + 1], c.u_r[e:e + 1], torch.from_numpy(item_r), rev, c.review_u_p, c.V, c.RC,
                                       c.T)[0])
    return torch.stack(out), np.array(acts)


# ------------------------------------------------------------------------------------------------- the cases of both files
# data: the rtm_rank_util case whose entries, table and model the timeline is drawn for; seed: make_timeline; lseed: make_lists;
# spp_list / spp_cat: slots_per_pass of the list-form / catalogue-form call.  Every case runs both forms.
# Seeds: 201 / 101, the first tried, everywhere: tests/test_rtm_seq_cpu.py asserts the band cap of every case on the oracle.
CASES = {'base': dict(data='base'),
         'd64': dict(data='d64'), 'd256': dict(data='d256'), 'd512': dict(data='d512'),            # the four EPL
         'heads1_d128': dict(data='heads1_d128'), 'heads64_d64': dict(data='heads64_d64'),          # lph 64 and 1
         'pv_user_item': dict(data='pv_user_item'),                                                 # the combined table, pad rows
         'cap': dict(data='cap'),                                                                   # the cut at T1: W = 3, T = 5, 4 user reviews
         'rev_fs': dict(data='rev_fs'),                                                             # pad row tanh(b)
         'ff384': dict(data='ff384'),                                                               # the unfused d = 128 tail
         'sharp': dict(data='sharp'),                                                               # near one-hot attention weights
         'passes': dict(data='base', spp_list=5, spp_cat=8)}                                        # 5 + 5 + 2 columns; 8 x 4 + 5 rows
PLAN = {'base': dict(epl=2, lph=8, tail_fused=1, query_fs_fused=1), 'd64': dict(epl=1, lph=8, tail_fused=0),
        'd256': dict(epl=4, lph=8, tail_fused=0), 'd512': dict(epl=8, lph=8, tail_fused=0),
        'heads1_d128': dict(epl=2, lph=64, tail_fused=1), 'heads64_d64': dict(epl=1, lph=1, tail_fused=0),
        'pv_user_item': dict(epl=2, lph=8, tail_fused=1), 'cap': dict(epl=2, lph=8, tail_fused=1),
        'rev_fs': dict(epl=2, lph=8, tail_fused=1), 'ff384': dict(epl=2, lph=8, tail_fused=0),
        'sharp': dict(epl=2, lph=8, tail_fused=1), 'passes': dict(epl=2, lph=8, tail_fused=1)}
PLAN_FIELDS = ('slots_per_pass', 'passes', 'epl', 'lph', 'tail_fused', 'query_fs_fused')
C_LIST = 12


def plan_passes(name, c):
    """(slots_per_pass, passes) the case's two calls must take: {'list': .., 'cat': ..}."""
    kw = CASES[name]
    sl, sc = kw.get('spp_list') or C_LIST, kw.get('spp_cat') or c.P
    return {'list': (sl, -(-C_LIST // sl)), 'cat': (sc, -(-c.P // sc))}


# What fp32 on the host costs each case against the float64 oracle, per entry, the worst entry: the larger of the fp32 oracle's
# and the fp32 factorisation's error — §8b.1's rule.  (cat, list): over the whole catalogue (`rtm_rank_util.entry_err`) and over
# the listed live pairs with the list's normaliser (`rtm_cand_util.list_err`).  Measured on the CPU, the largest over 1, 4 and
# 8 BLAS threads; tests/test_rtm_seq_cpu.py re-measures them and allows a tenth on top.  The GPU's per-entry bound is 8 x this,
# at most TOL.
# Where entry 0 is the worst (base, heads1_d128, cap, passes) it is because its row — the query key alone for every item — is
# one small score, so the same absolute error weighs more; d256 moved by a third between thread counts, ff384 by a sixth.
YARDSTICK = {'base': (7.73e-6, 6.62e-6), 'd64': (4.36e-7, 4.41e-7), 'd256': (2.41e-6, 2.26e-6), 'd512': (4.00e-6, 4.01e-6),
             'heads1_d128': (7.73e-6, 6.62e-6), 'heads64_d64': (4.67e-7, 3.11e-7), 'pv_user_item': (1.24e-6, 1.28e-6),
             'cap': (7.73e-6, 6.62e-6), 'rev_fs': (5.59e-7, 5.97e-7), 'ff384': (9.47e-7, 6.67e-7), 'sharp': (2.51e-6, 4.94e-6),
             'passes': (7.73e-6, 6.62e-6)}


def bound(name, form):
    return min(YARD_FACTOR * YARDSTICK[name][0 if form == 'cat' else 1], TOL)


def case_of(name):
    """(case data with the time-ordered mode's flags set, the static twin's args, build_model's scale)."""
    kw = dict(U.CASES[CASES[name]['data']])
    kw.pop('items_per_pass', None)
    scale = kw.pop('scale', 1.0)
    c = U.make_case(**kw)
    static_a = c.a
    c.a = copy.copy(static_a)
    c.a.do_seq_review_test, c.a.train_review_only = True, False
    return c, static_a, scale


@functools.lru_cache(maxsize=None)
def host_case(name):
    """One case on the host, computed once and shared: the timeline, the lists, the float64 and fp32 oracles, both
    factorisations, and the two yardsticks."""
    kw = CASES[name]
    c, static_a, scale = case_of(name)
    tl = make_timeline(c, kw.get('seed', 201))
    lists = make_lists(c, C_LIST, kw.get('lseed', 101))
    m, sd = U.build_model(c, 'cpu', scale=scale)
    ref64, P64, rev64 = oracle_seq(c, sd, tl, f64=True)
    ref32, P32, rev32 = oracle_seq(c, sd, tl, f64=False)
    f64, _ = factorised_seq(c, P64, rev64, tl)
    f32, _ = factorised_seq(c, P32, rev32, tl)
    yard_cat = float(max(U.entry_err(ref32, ref64).max(), U.entry_err(f32, ref64).max()))
    l64, l32, lf32 = (K.take(x, lists, c.P) for x in (ref64, ref32, f32))
    yard_list = float(max(K.list_err(l32, l64, lists, c.P).max(), K.list_err(lf32, l64, lists, c.P).max()))
    return types.SimpleNamespace(c=c, static_a=static_a, scale=scale, tl=tl, lists=lists, m=m, sd=sd, ref64=ref64, ref32=ref32,
                                 f64=f64, f32=f32, P64=P64, rev64=rev64, yard=(yard_cat, yard_list),
                                 spp_list=kw.get('spp_list'), spp_cat=kw.get('spp_cat'))


def rank_batch(c, tl, lists=None, device=None, target=None):
    b = rtm_data.ProdSearchRankBatch(list(range(c.B)), [int(u) for u in c.users], c.target if target is None else target, c.qw, c.u_r,
                                     None if lists is None else torch.from_numpy(lists), torch.from_numpy(tl.stamps))
    return b if device is None else b.to(device)


def plan_of(lib, m, c, C, k, spp=None):
    """``ps_rtm_rank_seq_plan`` for the call ``evaluate.rank_seq_rtm(m, index, batch, k, slots_per_pass=spp)`` makes; ``C`` None:
    the catalogue form."""
    from prodsearch_amd import _lib
    desc, sh = m._rank_all_desc(c.B, c.qw.shape[1], c.U, (c.P, c.RC - 1 if (c.a.use_user_emb or c.a.use_item_emb) else 0, window_of(c)))
    C = _lib.PS_RTM_SEQ_NO_LIST if C is None else C
    nbytes = lib.ps_rtm_rank_seq_scratch_bytes(desc, sh, C, k, int(spp or 0))
    assert nbytes > 0, lib.ps_last_error()
    plan = _lib.PsRtmRankSeqPlan()
    _lib.check(lib.ps_rtm_rank_seq_plan(desc, sh, C, k, nbytes, plan), 'ps_rtm_rank_seq_plan')
    return {f: int(getattr(plan, f)) for f in PLAN_FIELDS}


def cat_bands(ref, skip=(0,)):
    """``rtm_rank_util.banded`` and the banded share of the positions of the entries not in ``skip``: entry 0 (INT64_MIN) sees
    no review of any item, so its row is one exact tie by construction — the GPU's row is bit-equal too and ties go to the
    lower id, which the tests assert directly."""
    order, band = U.banded(ref)
    rows = [e for e in range(band.shape[0]) if e not in skip]
    return order, band, float(band[rows].mean())
