"""Shared by tests/test_rtm_cand_cpu.py and tests/test_gpu_rtm_cand.py: the review transformer over per-entry candidate lists
(``evaluate.rank_candidates_rtm``).  The data, the models and the host oracles are those of
tests/rtm_rank_util.py (``make_case`` / ``host_case``); this file adds the lists and what is stated about them.

* ``make_cands``: the lists of a case, with the special slots the GPU file checks one by one.
* ``semantics``: the rank / top-k rule of ``Trainer._scores_candidates`` in numpy, slot by slot.
* ``CASES`` / ``PLAN`` / ``YARDSTICK`` / ``bound``: the cases of both files, the fields of ``ps_rtm_rank_cand_plan`` each was
  written for, what fp32 on the host costs each of them on its LISTED pairs, and the per-entry bound that follows.
* ``list_bands``: the oracle's order of every list and which of its positions lie in a band.
"""
import functools
import types

import numpy as np
import torch

import rtm_rank_util as U
from prodsearch_amd import rtm_data, synth

TOL = U.TOL
YARD_FACTOR = U.YARD_FACTOR
BAND_CAP = 0.25          # the project's cap: at most a quarter of the positions may lie in a band (tests/test_gpu_rtm_rank.py)


def make_cands(c, C=12, seed=101):
    """[B, C] item ids, -1 padding a ragged list.  The plain draw, then the special slots:
    entry 0, columns 0..3: items 0 (no reviews; entry 0 has none either — a softmax over the query key alone), 1 (a full list),
    2 and 3 (one shared list: bit-equal scores, ordered by column); entry 1: its target at columns 2 AND 7, an id past the
    catalogue (P + 3) at column 4, a -1 at column 5 — a dead slot in the middle.  The last entry's target is outside [0, P)
    already (``make_case``)."""
    rng = synth.rng_for(seed)
    out = np.full((c.B, C), -1, np.int64)
    for b in range(c.B):
        n = C if b < 2 else int(rng.integers(1, C + 1))
        out[b, :n] = rng.choice(c.P, size=n, replace=False)
    out[0, :4] = (0, 1, 2, 3)
    t1 = int(c.target[1])
    out[1, 2] = out[1, 7] = t1
    out[1, 4] = c.P + 3
    out[1, 5] = -1
    return out


def live_of(cands, P):
    cands = np.asarray(cands)
    return (cands >= 0) & (cands < P)


def semantics(scores, cands, target, P, k):
    """(top_idx [B,k] int64, top_score [B,k] fp32, rank [B]) of a dense [B, C] score matrix, stated slot by slot:
    a slot is live when its id lies in [0, P); the live slots are ordered by (score desc, column asc); ``top_idx`` holds their
    ITEM ids, -1 / -inf where there are fewer than k; ``rank`` is 1 + the number of live slots ahead of the FIRST live column
    that holds the target, 0 when there is none.  Duplicate ids are slots of their own."""
    s = np.asarray(scores, dtype=np.float32)
    cands, target = np.asarray(cands), np.asarray(target)
    B, C = cands.shape
    top_idx = np.full((B, k), -1, np.int64)
    top_score = np.full((B, k), -np.inf, np.float32)
    rank = np.zeros(B, np.int64)
    for b in range(B):
        slots = [col for col in range(C) if 0 <= cands[b, col] < P]
        slots.sort(key=lambda col: (-float(s[b, col]), col))
        for j, col in enumerate(slots[:k]):
            top_idx[b, j], top_score[b, j] = cands[b, col], s[b, col]
        hits = [col for col in range(C) if 0 <= cands[b, col] < P and cands[b, col] == target[b]]
        if hits:
            rank[b] = 1 + slots.index(hits[0])
    return top_idx, top_score, rank


def list_bands(ref, cands, P, tol=TOL):
    """Per entry: the oracle's order of its live slots (columns, by score desc, column asc) and which positions of that order
    lie in a band — the gap to a neighbouring score is at most 2 * tol * max|score| (the largest live listed score of the
    batch), so an implementation within tol may swap them.  -> (orders, bands: lists of arrays, the banded share of all
    positions)."""
    ref = np.asarray(torch.as_tensor(ref).double())
    live = live_of(cands, P)
    top = np.abs(ref[live]).max()
    orders, bands = [], []
    for b in range(ref.shape[0]):
        cols = np.flatnonzero(live[b])
        cols = cols[np.lexsort((cols, -ref[b, cols]))]
        rs = ref[b, cols]
        close = np.abs(np.diff(rs)) <= 2 * tol * top
        band = np.zeros(len(cols), dtype=bool)
        band[:-1] |= close
        band[1:] |= close
        orders.append(cols)
        bands.append(band)
    n = sum(len(x) for x in bands)
    return orders, bands, float(sum(int(x.sum()) for x in bands)) / max(n, 1)


# ------------------------------------------------------------------------------------------------- the cases of both files
# data: the name of the rtm_rank_util case whose entries, catalogue and model the lists are drawn over; C, seed: make_cands;
# cpp: cands_per_pass of the call.  Seeds: the first from 101 on at which at most a quarter of the listed positions lie in a
# band (tests/test_rtm_cand_cpu.py asserts the cap for every case) — 101 everywhere but:
# `cap_user`: 101 leaves 0.26 banded (entries that see one review per item nearly tie), 102 has 0.21.
# `lds_full` has P = 10 products: lists of 12 cannot be drawn without replacement, and the four fixed columns of entry 0 repeat
# ids drawn elsewhere in a list that wide (exact ties).  Its lists are 8 wide — the special columns end at 7 — and 114 is the
# first seed at the cap (0.25).  Entry 0 lists item 1 (64 reviews: rr_leading's full ballot), entry 1 has 64 of its own.
CASES = {'base': dict(data='base'),
         'd64': dict(data='d64'), 'd256': dict(data='d256'), 'd512': dict(data='d512'),           # the four EPL
         'heads1_d128': dict(data='heads1_d128'), 'heads64_d64': dict(data='heads64_d64'),         # lph 64 and 1
         'pv_user_item': dict(data='pv_user_item'),                                                # the combined table, pad rows
         'long': dict(data='long', C=20),                                                          # 51 positions
         'cap': dict(data='cap'), 'cap_user': dict(data='cap_user', seed=102),                     # the cut at T1
         'lds_full': dict(data='lds_full', C=8, seed=114),                                         # 64 live ids on both sides
         'rev_fs': dict(data='rev_fs'),                                                            # pad row tanh(b)
         'ff384': dict(data='ff384'),                                                              # the unfused d = 128 tail
         'sharp': dict(data='sharp'),                                                              # near one-hot attention weights
         'passes': dict(data='base', cpp=5)}                                                       # 5 + 5 + 2 columns of 12
PLAN = {'base': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=1, query_fs_fused=1),
        'd64': dict(cands_per_pass=12, passes=1, epl=1, lph=8, tail_fused=0),
        'd256': dict(cands_per_pass=12, passes=1, epl=4, lph=8, tail_fused=0),
        'd512': dict(cands_per_pass=12, passes=1, epl=8, lph=8, tail_fused=0),
        'heads1_d128': dict(cands_per_pass=12, passes=1, epl=2, lph=64, tail_fused=1),
        'heads64_d64': dict(cands_per_pass=12, passes=1, epl=1, lph=1, tail_fused=0),
        'pv_user_item': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=1),
        'long': dict(cands_per_pass=20, passes=1, epl=2, lph=8, tail_fused=1),
        'cap': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=1),
        'cap_user': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=1),
        'lds_full': dict(cands_per_pass=8, passes=1, epl=4, lph=8, tail_fused=0),
        'rev_fs': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=1),
        'ff384': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=0),
        'sharp': dict(cands_per_pass=12, passes=1, epl=2, lph=8, tail_fused=1),
        'passes': dict(cands_per_pass=5, passes=3, epl=2, lph=8, tail_fused=1)}
PLAN_FIELDS = ('cands_per_pass', 'passes', 'epl', 'lph', 'tail_fused', 'query_fs_fused')

# What fp32 on the host costs each case on its LISTED live pairs against the float64 oracle, per entry (`list_err`), the worst
# entry: the larger of the fp32 oracle's and the fp32 factorisation's error.  The rule of rtm_rank_util.YARDSTICK with the
# list's normaliser — the largest |float64 score| among the entry's live slots, not among the whole catalogue — hence other
# numbers.  Measured on the CPU; the largest over 1, 4 and 8 BLAS threads (tests/test_rtm_cand_cpu.py re-measures them and
# allows a tenth on top).  The GPU's per-entry bound is 8 x this, at most TOL.
YARDSTICK = {'base': 1.29e-6, 'd64': 3.30e-7, 'd256': 9.73e-7, 'd512': 3.10e-6, 'heads1_d128': 1.22e-6, 'heads64_d64': 2.94e-7,
             'pv_user_item': 1.28e-6, 'long': 1.80e-6, 'cap': 1.29e-6, 'cap_user': 1.90e-6, 'lds_full': 5.47e-7, 'rev_fs': 7.49e-7,
             'ff384': 4.74e-7, 'sharp': 2.61e-6, 'passes': 1.29e-6}      # (d512: 3.10e-6 / 2.60e-6 / 2.35e-6 at 1 / 4 / 8 threads)


def bound(name):
    return min(YARD_FACTOR * YARDSTICK[name], TOL)


def list_err(got, ref64, cands, P):
    """Per entry: max over its live slots of |got - ref64|, over the largest |ref64| among them.  got, ref64: [B, C]."""
    got, ref = np.asarray(torch.as_tensor(got).double()), np.asarray(torch.as_tensor(ref64).double())
    live = live_of(cands, P)
    out = np.zeros(got.shape[0])
    for b in range(got.shape[0]):
        if live[b].any():
            out[b] = np.abs(got[b, live[b]] - ref[b, live[b]]).max() / np.abs(ref[b, live[b]]).max()
    return out


def take(full, cands, P):
    """[B, C] from a [B, P] score matrix: the listed items' columns, -inf at dead slots."""
    full = torch.as_tensor(full)
    c = torch.as_tensor(np.asarray(cands))
    live = torch.as_tensor(live_of(cands, P))
    out = full.gather(1, c.clamp(0, P - 1))
    return out.masked_fill(~live, float('-inf'))


@functools.lru_cache(maxsize=None)
def host_case(name):
    """One case on the host: ``rtm_rank_util.host_case`` of its data (computed once per data name, shared with the catalogue
    tests), its lists, and the float64 / fp32 oracles and the fp32 factorisation at the listed pairs."""
    kw = CASES[name]
    h = U.host_case(kw['data'])
    c = h.c
    cands = make_cands(c, kw.get('C', 12), kw.get('seed', 101))
    ref64, ref32, f32 = (take(x, cands, c.P) for x in (h.ref64, h.ref32, h.f32))
    yard = float(max(list_err(ref32, ref64, cands, c.P).max(), list_err(f32, ref64, cands, c.P).max()))
    return types.SimpleNamespace(h=h, c=c, m=h.m, sd=h.sd, scale=h.scale, cands=cands, C=cands.shape[1], cpp=kw.get('cpp'),
                                 ref64=ref64, ref32=ref32, f32=f32, yard=yard)


def rank_batch(c, cands, device=None):
    b = rtm_data.ProdSearchRankBatch(list(range(c.B)), [int(u) for u in c.users], c.target, c.qw, c.u_r, torch.from_numpy(cands))
    return b if device is None else b.to(device)


def chunk_of(c, cands):
    """The lists as one ``ProdSearchTestBatch`` of ``ProductRanker.test``: a slot outside [0, P) is a padded one."""
    cands = np.where(live_of(cands, c.P), cands, -1)
    return U.assemble_chunk(c.qw, c.u_r, c.users, c.item_r, cands, c.review_u_p, c.n_users, c.P, c.RC - 1, ids_from_reviews=True,
                            limit=c.T)


def plan_of(lib, m, c, C, k, cpp=None):
    """``ps_rtm_rank_cand_plan`` for the call ``evaluate.rank_candidates_rtm(m, index, batch, k, cands_per_pass=cpp)`` makes."""
    from prodsearch_amd import _lib
    desc, sh = m._rank_all_desc(c.B, c.qw.shape[1], c.U, (c.P, c.RC - 1 if (c.a.use_user_emb or c.a.use_item_emb) else 0, c.I))
    nbytes = lib.ps_rtm_rank_cand_scratch_bytes(desc, sh, C, k, int(cpp or 0))
    assert nbytes > 0, lib.ps_last_error()
    plan = _lib.PsRtmRankCandPlan()
    _lib.check(lib.ps_rtm_rank_cand_plan(desc, sh, C, k, nbytes, plan), 'ps_rtm_rank_cand_plan')
    return {f: int(getattr(plan, f)) for f in PLAN_FIELDS}
