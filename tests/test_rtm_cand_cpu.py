"""Host-side checks of the review transformer over per-entry candidate lists (``evaluate.rank_candidates_rtm``, DESIGN.md
§8b.2; the GPU side is tests/test_gpu_rtm_cand.py): the ABI of include/prodsearch_rtm_cand.h, ``ps_rtm_rank_cand_plan`` per
case, the refusals, ``ProdSearchDataLoader.candidate_batches``, the rank / top-k semantics against
``Trainer._scores_candidates``' own chain, and the yardstick of every case on its listed pairs."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import rtm_cand_util as K
import rtm_rank_util as U
from prodsearch_amd import _lib, build as pbuild, default_args, synth
from prodsearch_amd.corpus import GlobalProdSearchData, ProdSearchData, ProdSearchDataset
from prodsearch_amd.rtm_loader import ProdSearchDataLoader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_FIELDS = ('query_word_idxs', 'candi_prod_ridxs', 'candi_seg_idxs', 'candi_seq_user_idxs', 'candi_seq_item_idxs')
NEW = ('ps_rtm_rank_cand_scratch_bytes', 'ps_rtm_rank_cand_plan', 'ps_rtm_rank_candidates')


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------- 1. ABI, plan, refusals
def test_candidate_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, 'include', 'prodsearch_rtm_cand.h')).read()
    declared = set(re.findall(r'\b(ps_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW) == set(_lib.RANK_CAND_SYMBOLS)
    for name in NEW:
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.PsRtmRankCandPlan) == 32
    body = re.search(r'typedef struct PsRtmRankCandPlan \{(.*?)\} PsRtmRankCandPlan;', hdr, re.S).group(1)
    assert tuple(re.findall(r'int(?:32|64)_t\s+(\w+);', body)) == tuple(n for n, _ in _lib.PsRtmRankCandPlan._fields_) == \
        ('cands_per_pass', 'passes', 'epl', 'lph', 'tail_fused', 'query_fs_fused')
    # the prototypes: the argument counts of the header and of the ctypes table
    for name in NEW:
        proto = re.search(r'\b%s\s*\((.*?)\);' % name, hdr, re.S).group(1)
        assert len(proto.split(',')) == len(_lib.RANK_CAND_SYMBOLS[name][1]), name
    assert _lib.RANK_CAND_SYMBOLS['ps_rtm_rank_cand_scratch_bytes'][0] is C.c_int64
    args = _lib.RANK_CAND_SYMBOLS['ps_rtm_rank_candidates'][1]
    assert args[8] is C.c_int64 and args[10] is C.c_int32 and args[-2] is C.c_int64      # C, topk, scratch_bytes


def test_case_tables_cover_the_same_names():
    assert set(K.CASES) == set(K.PLAN) == set(K.YARDSTICK)
    assert all(set(p) <= set(K.PLAN_FIELDS) for p in K.PLAN.values())
    assert all(0 < K.bound(n) <= K.TOL for n in K.CASES)
    assert all(kw['data'] in U.CASES for kw in K.CASES.values())


@pytest.mark.parametrize('name', sorted(K.CASES))
def test_plan_of_every_case(lib, name):
    """``ps_rtm_rank_cand_plan`` (host only) for the call the GPU case makes: the fields each case was written for (``K.PLAN``)
    and those that follow from the shape alone."""
    h = K.host_case(name)
    c = h.c
    plan = K.plan_of(lib, h.m, c, h.C, 10, h.cpp)
    print(name, plan)
    for f, v in K.PLAN[name].items():
        assert plan[f] == v, (name, f, plan[f], v)
    assert plan['epl'] * 64 == c.a.embedding_size and plan['lph'] * c.a.heads == 64
    assert plan['cands_per_pass'] == (h.cpp or h.C) and plan['passes'] == -(-h.C // plan['cands_per_pass'])


def _desc_shape(c, **edit):
    m, _ = U.build_model(c, 'cpu')
    d, sh = m._rank_all_desc(c.B, c.qw.shape[1], c.U, (c.P, c.RC - 1, c.I))
    for k, v in edit.items():
        setattr(d if hasattr(d, k) else sh, k, v)
    return m, d, sh


def test_plan_follows_the_scratch_ragged_passes_included(lib):
    """Passes are sized from the scratch: C = 12 cut into 3 passes of 5 (the last ragged: 2 columns), the most that fit one byte
    below a size, and the refusals of too small a scratch, topk, C and the pair count."""
    c = U.make_case()
    _, d, sh = _desc_shape(c)
    plan = _lib.PsRtmRankCandPlan()
    sizes = {n: lib.ps_rtm_rank_cand_scratch_bytes(d, sh, 12, 10, n) for n in (1, 5, 0, 40)}
    assert 0 < sizes[1] < sizes[5] < sizes[0] == sizes[40]                 # more per pass than the list holds: the list
    for n, want in ((1, 1), (5, 5), (0, 12)):
        assert lib.ps_rtm_rank_cand_plan(d, sh, 12, 10, sizes[n], plan) == 0
        assert (plan.cands_per_pass, plan.passes) == (want, -(-12 // want))
    assert (12 % 5, -(-12 // 5)) == (2, 3)                                  # three passes, the last ragged
    assert lib.ps_rtm_rank_cand_plan(d, sh, 12, 10, sizes[5] - 1, plan) == 0 and plan.cands_per_pass == 4   # the most that fit
    assert lib.ps_rtm_rank_cand_plan(d, sh, 12, 10, sizes[1] - 1, plan) != 0 and 'scratch' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_cand_plan(d, sh, 12, 257, sizes[0], plan) != 0 and 'topk' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_cand_plan(d, sh, 0, 10, sizes[0], plan) != 0 and 'candidates per entry' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_cand_plan(d, sh, 12, 10, sizes[0], None) != 0
    assert lib.ps_rtm_rank_cand_scratch_bytes(d, sh, 0, 10, 0) == -1 and 'candidates per entry' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_cand_scratch_bytes(d, sh, 12, 257, 0) == -1
    # B * cands_per_pass < 2^30
    big = 1 << 28
    assert c.B * big >= 1 << 30
    assert lib.ps_rtm_rank_cand_scratch_bytes(d, sh, big, 10, big) == -1 and 'per pass' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_cand_scratch_bytes(d, sh, big, 10, 7) > 0       # ... the list may be that long, a pass may not


@pytest.mark.parametrize('edit,flag', [(dict(n_layers=2), 'inter_layers'), (dict(seq_review_test=1), 'do_seq_review_test'),
                                       (dict(fix_emb=1, review_encoder=_lib.PS_RENC_FS), 'fix_emb'),
                                       (dict(fix_emb=1, review_encoder=_lib.PS_RENC_AVG), 'fix_emb')])
def test_c_entries_refuse_with_the_messages_of_rank_all(lib, edit, flag):
    c = U.make_case()
    _, d, sh = _desc_shape(c, **edit)
    assert lib.ps_rtm_rank_scratch_bytes(d, sh, 10, 0) == -1
    want = lib.ps_last_error().decode()
    assert flag in want
    assert lib.ps_rtm_rank_cand_scratch_bytes(d, sh, 12, 10, 0) == -1 and lib.ps_last_error().decode() == want
    plan = _lib.PsRtmRankCandPlan()
    assert lib.ps_rtm_rank_cand_plan(d, sh, 12, 10, 1 << 24, plan) != 0 and lib.ps_last_error().decode() == want
    dummy = C.c_void_p(256)                       # never read: the refusal comes before any argument is touched
    ps = _lib.PsRtmTensors()
    assert lib.ps_rtm_rank_candidates(d, sh, ps, dummy, dummy, dummy, dummy, dummy, 12, dummy, 10, dummy, dummy, dummy, None, dummy,
                                      1 << 20, None) != 0 and lib.ps_last_error().decode() == want


def test_python_refuses_up_front():
    from prodsearch_amd import evaluate
    c = U.make_case()
    cands = K.make_cands(c)
    for over, flag in ((dict(inter_layers=2), 'inter_layers'),
                       (dict(do_seq_review_test=True, train_review_only=False), 'do_seq_review_test')):
        c.a = U.make_args(**over)
        m, _ = U.build_model(c, 'cpu')
        with pytest.raises(NotImplementedError, match=flag):
            evaluate.rank_candidates_rtm(m, None, K.rank_batch(c, cands), 10)
    # a batch without lists: the constructor stays compatible, and the entry says what is missing
    c.a = U.make_args()
    m, _ = U.build_model(c, 'cpu')
    rb = U.rank_batch(c)
    assert rb.candi_prod_idxs is None and rb.to('cpu') is rb
    idx = types.SimpleNamespace(model=m, stale=lambda: False)
    with pytest.raises(RuntimeError, match='candi_prod_idxs'):
        evaluate.rank_candidates_rtm(m, idx, rb, 10)
    idx.stale = lambda: True
    with pytest.raises(RuntimeError, match='stale'):
        evaluate.rank_candidates_rtm(m, idx, K.rank_batch(c, cands), 10)
    moved = K.rank_batch(c, cands).to('meta')                             # .to() carries the lists along
    assert moved.candi_prod_idxs.shape == cands.shape and moved.candi_prod_idxs.device.type == 'meta'


# ------------------------------------------------------------------------------------------------- 2. the loader
def _loader(tmp_path, **over):
    kw = dict(model_name='review_transformer', uprev_review_limit=3, iprev_review_limit=4, review_word_limit=12,
              candi_batch_size=3, valid_candi_size=7, test_candi_size=-1)
    kw.update(over)
    args = default_args(**kw)
    data_path, inp = synth.write_corpus(str(tmp_path), 41, n_users=30, n_products=50, n_words=120)
    gd = GlobalProdSearchData(args, data_path, inp)
    pd = ProdSearchData(args, inp, 'valid', gd)
    ds = ProdSearchDataset(args, gd, pd)
    return args, gd, ds, ProdSearchDataLoader(args, ds, batch_size=4, shuffle=False)


def test_candidate_batches_reassemble_the_test_collate(tmp_path):
    """``valid_candi_size = 7`` in chunks of ``candi_batch_size = 3``: three dataset rows per entry, the last ragged (one
    candidate).  ``candidate_batches()`` gives the entries of those rows and their chunks concatenated in dataset order, and
    ``assemble_chunk`` of the lists reproduces the tensors of ``test_batch_from_ids`` over the same rows."""
    args, gd, ds, dl = _loader(tmp_path)
    seg = 3
    ent = dl.rank_entries()
    assert len(ent) * seg == len(ds) and np.array_equal(ent, np.arange(0, len(ds), seg))
    cat = dl.catalogue_reviews().numpy()
    pad = gd.review_count - 1
    up = np.asarray(gd.review_u_p, dtype=np.int64).reshape(-1, 2)
    batches = list(dl.candidate_batches())
    assert sum(len(b.user_idxs) for b in batches) == len(ent)
    assert len(batches) == -(-len(ent) // 4)
    lo = 0
    for rb in batches:
        ids = ent[lo:lo + len(rb.user_idxs)]
        lo += len(ids)
        cand = rb.candi_prod_idxs.numpy()
        assert cand.shape == (len(ids), 7) and (cand >= 0).all()          # 499 + 1 of the reference, here 6 + 1: no ragged list
        ref = dl.rank_batch_from_ids(ids)
        for f in ('query_word_idxs', 'u_ridxs', 'target_prod_idxs'):
            assert torch.equal(getattr(rb, f), getattr(ref, f)), f
        assert list(rb.user_idxs) == list(ref.user_idxs) and list(rb.query_idxs) == list(ref.query_idxs)
        assert (cand == rb.target_prod_idxs.numpy()[:, None]).any(1).all()     # the target is among its candidates
        widths = []
        for j in range(seg):
            tb = dl.test_batch_from_ids(ids + j)
            chunk = np.asarray(tb.candi_prod_idxs)
            widths.append(chunk.shape[1])
            mine_ids = cand[:, 3 * j:3 * j + chunk.shape[1]]
            assert np.array_equal(mine_ids, chunk), (lo, j)
            assert list(tb.user_idxs) == list(rb.user_idxs) and list(tb.query_idxs) == list(rb.query_idxs)
            assert np.array_equal(np.asarray(tb.target_prod_idxs), rb.target_prod_idxs.numpy())
            mine = U.assemble_chunk(rb.query_word_idxs, rb.u_ridxs, rb.user_idxs, cat, mine_ids, up, gd.user_size, gd.product_size,
                                    pad)
            for f in TEST_FIELDS:
                got, want = getattr(mine, f).numpy(), getattr(tb, f).numpy()
                assert got.shape == want.shape and np.array_equal(got, want), (lo, j, f)
        assert widths == [3, 3, 1]
    assert lo == len(ent)


def test_ragged_lists_are_padded_to_the_widest_of_the_batch(tmp_path):
    _, _, _, dl = _loader(tmp_path)
    first = dl.rank_entries()
    # cut the last chunk off every other entry's rows: lists of 7 and of 6 in one batch
    keep = np.ones(len(dl.entry_quad), dtype=bool)
    keep[first[1::2] + 2] = False
    lens = np.diff(dl.candi_ptr)
    items = [dl.candi_items[dl.candi_ptr[i]:dl.candi_ptr[i + 1]] for i in np.flatnonzero(keep)]
    dl.entry_quad = dl.entry_quad[keep]
    dl.candi_ptr = np.concatenate([[0], np.cumsum(lens[keep])])
    dl.candi_items = np.concatenate(items)
    b = next(dl.candidate_batches())
    cand = b.candi_prod_idxs.numpy()
    assert cand.shape == (4, 7)
    assert (cand[0::2] >= 0).all() and (cand[1::2, :6] >= 0).all() and (cand[1::2, 6] == -1).all()


def test_loader_refuses_entry_dependent_item_lists(tmp_path):
    _, _, _, dl = _loader(tmp_path, do_seq_review_test=True, train_review_only=False)
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        next(dl.candidate_batches())


# ------------------------------------------------------------------------------------------------- 3. the semantics
class _Chunked(object):
    """A loader and a model that hand ``Trainer._scores_candidates`` a given [B, C] score matrix in the dataset's form: an
    entry's list in consecutive rows of ``cbs`` candidates each, ``bs`` rows per batch."""

    def __init__(self, scores, cands, target, cbs, bs):
        B, Cw = cands.shape
        seg = (Cw - 1) // cbs + 1
        padw = seg * cbs - Cw
        s = np.pad(scores, ((0, 0), (0, padw)), constant_values=0.0).reshape(B * seg, cbs)
        c = np.pad(cands, ((0, 0), (0, padw)), constant_values=-1).reshape(B * seg, cbs)
        self.rows = [(s[r], c[r], int(target[r // seg]), r // seg) for r in range(B * seg)]
        self.bs = bs

    def loader(self, args, dataset, **kw):
        out = []
        for lo in range(0, len(self.rows), self.bs):
            rows = self.rows[lo:lo + self.bs]
            out.append(types.SimpleNamespace(scores=torch.from_numpy(np.stack([r[0] for r in rows])),
                                             candi_prod_idxs=np.stack([r[1] for r in rows]),
                                             target_prod_idxs=np.array([r[2] for r in rows]),
                                             user_idxs=[r[3] for r in rows], query_idxs=[r[3] for r in rows]))
        return out

    eval = get_review_embeddings = clear_review_embbeddings = lambda self: None

    def test(self, b):
        return b.scores


def _random_lists(seed, B=9, Cw=11, P=40):
    """Scores on a coarse grid (exact ties), ids drawn with replacement (duplicates), dead slots, absent targets, and a row
    with two live slots only."""
    rng = synth.rng_for(seed)
    scores = (rng.integers(-6, 7, size=(B, Cw)) / 4.0).astype(np.float32)
    cands = rng.integers(0, P, size=(B, Cw)).astype(np.int64)
    cands[rng.random((B, Cw)) < 0.2] = -1
    cands[2, 2:] = -1                                                      # fewer live slots than k
    target = cands[np.arange(B), rng.integers(0, Cw, size=B)].copy()
    target[target < 0] = P + 1
    target[3] = P + 2                                                      # absent
    cands[4, 1] = cands[4, 8] = target[4] = 7                              # the target twice
    scores[4, 1] = scores[4, 8] = scores[4, 3]
    return scores, cands, target, P


@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_numpy_semantics_agree_with_the_trainers_chain(seed):
    """``K.semantics`` against the chain of ``Trainer._scores_candidates`` itself, fed through a stand-in loader and model.
    ``torch.topk`` leaves the order inside a group of equal scores open, so the ids are compared where a score is unique in
    its list and as a group where it is not; scores and ranks exactly."""
    from prodsearch_amd import trainer
    scores, cands, target, P = _random_lists(seed)
    k, cbs = 6, 4
    fake = _Chunked(scores, cands, target, cbs, bs=5)
    args = default_args(model_name='review_transformer', candi_batch_size=cbs, valid_batch_size=5)
    tr = trainer.Trainer(args, None, None)
    tr.model, tr.ExpDataloader = fake, fake.loader
    rank, ids, ts, users, queries = tr._scores_candidates(args, None, cands.shape[1], topk=k)
    ti_np, ts_np, rank_np = K.semantics(scores, cands, target, P, k)
    assert users == list(range(len(target))) == queries
    assert np.array_equal(rank.numpy(), rank_np)
    assert np.array_equal(ts.numpy(), ts_np)
    ids = ids.numpy()
    live = K.live_of(cands, P)
    assert (live.sum(1) < k).any() and (rank_np == 0).any() and (rank_np > 1).any()
    n_tied = 0
    for b in range(len(target)):
        for j in range(k):
            same = np.flatnonzero(live[b] & (scores[b] == ts_np[b, j]))
            if len(same) <= 1:
                assert ids[b, j] == ti_np[b, j], (b, j)
            else:
                n_tied += 1
                assert ids[b, j] in cands[b, same], (b, j)
        assert (ids[b] == -1).sum() == (ti_np[b] == -1).sum()
    assert n_tied > 0
    # the first column decides a duplicated target's rank
    assert rank_np[4] == 1 + int((live[4] & ((scores[4] > scores[4, 1]) | ((scores[4] == scores[4, 1]) & (np.arange(11) < 1)))).sum())


# ------------------------------------------------------------------------------------------------- 4. the cases on the host
@pytest.mark.parametrize('name', sorted(K.CASES))
def test_lists_hold_their_special_slots_and_stay_under_the_band_cap(name):
    h = K.host_case(name)
    c, cands = h.c, h.cands
    assert cands.shape == (c.B, h.C) and c.B <= 9 and h.C <= 20
    assert list(cands[0, :4]) == [0, 1, 2, 3]
    pad = c.RC - 1
    ni = U.leading(c.item_r.numpy(), pad)
    assert ni[0] == 0 and U.leading(c.u_r.numpy(), pad)[0] == 0 and ni[1] == c.I and torch.equal(c.item_r[2], c.item_r[3])
    t1 = int(c.target[1])
    assert cands[1, 2] == t1 == cands[1, 7] and cands[1, 4] == c.P + 3 and cands[1, 5] == -1
    assert not 0 <= int(c.target[-1]) < c.P
    _, _, frac = K.list_bands(h.ref32, cands, c.P)
    print('%s: %.3f of the listed positions in a band' % (name, frac))
    assert frac <= K.BAND_CAP
    if name == 'lds_full':
        assert ni[1] == 64 and U.leading(c.u_r.numpy(), pad)[1] == 64


@pytest.mark.parametrize('name', sorted(K.CASES))
def test_recorded_yardstick_still_holds(name):
    """``K.YARDSTICK[name]``: the worst entry's error of fp32 on the host (the fp32 oracle, the fp32 factorisation) against the
    float64 oracle on the LISTED live pairs, normalised by the entry's largest listed |score|; re-measured, a tenth on top for
    this host's summation order.  The GPU's per-entry bound is 8 x the record."""
    h = K.host_case(name)
    print('%s: yardstick measured %.3g, recorded %.3g, bound %.3g' % (name, h.yard, K.YARDSTICK[name], K.bound(name)))
    assert 0 < h.yard <= 1.1 * K.YARDSTICK[name]
