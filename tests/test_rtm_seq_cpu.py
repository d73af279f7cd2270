"""Host-side checks of the review transformer's one-pass evaluation in the time-ordered setting (``evaluate.rank_seq_rtm``,
DESIGN.md §8b.3; the GPU side is tests/test_gpu_rtm_seq.py): the ABI of include/prodsearch_rtm_seq.h, ``ps_rtm_rank_seq_plan``
per case, the refusals (and that the static rankers still refuse the mode), ``timeline_index``'s check, the loader's
``timeline`` / ``seq_rank_batches`` / ``seq_candidate_batches`` against the test collate, the factorisation on ``cat_of`` in
float64, its sensitivity to three mistakes of the window rule, and the yardstick and band cap of every case."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import rtm_cand_util as K
import rtm_rank_util as U
import rtm_seq_util as S
from prodsearch_amd import _lib, build as pbuild, default_args, synth
from prodsearch_amd.corpus import GlobalProdSearchData, ProdSearchData, ProdSearchDataset
from prodsearch_amd.rtm_loader import ProdSearchDataLoader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_FIELDS = ('query_word_idxs', 'candi_prod_ridxs', 'candi_seg_idxs', 'candi_seq_user_idxs', 'candi_seq_item_idxs')
NEW = ('ps_rtm_rank_seq_scratch_bytes', 'ps_rtm_rank_seq_plan', 'ps_rtm_rank_seq')


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------- 1. ABI, plan, refusals
def test_seq_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, 'include', 'prodsearch_rtm_seq.h')).read()
    declared = set(re.findall(r'\b(ps_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW) == set(_lib.RANK_SEQ_SYMBOLS)
    for name in NEW:
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.PsRtmRankSeqPlan) == 32 and C.sizeof(_lib.PsRtmSeqTimeline) == 32 and C.sizeof(_lib.PsRtmRankShape) == 32
    body = re.search(r'typedef struct PsRtmRankSeqPlan \{(.*?)\} PsRtmRankSeqPlan;', hdr, re.S).group(1)
    assert tuple(re.findall(r'int(?:32|64)_t\s+(\w+);', body)) == tuple(n for n, _ in _lib.PsRtmRankSeqPlan._fields_) == S.PLAN_FIELDS
    body = re.search(r'typedef struct PsRtmSeqTimeline \{(.*?)\} PsRtmSeqTimeline;', hdr, re.S).group(1)
    assert tuple(re.findall(r'int64_t\*?\s+(\w+);', body)) == tuple(n for n, _ in _lib.PsRtmSeqTimeline._fields_) == \
        ('ptr', 'rids', 'times', 'n')
    assert int(re.search(r'#define PS_RTM_SEQ_NO_LIST \((-?\d+)\)', hdr).group(1)) == _lib.PS_RTM_SEQ_NO_LIST
    for name in NEW:
        proto = re.search(r'\b%s\s*\((.*?)\);' % name, hdr, re.S).group(1)
        assert len(proto.split(',')) == len(_lib.RANK_SEQ_SYMBOLS[name][1]), name
    args = _lib.RANK_SEQ_SYMBOLS['ps_rtm_rank_seq'][1]
    assert args[9] is C.c_int64 and args[11] is C.c_int32 and args[-2] is C.c_int64        # C, topk, scratch_bytes
    # the two older headers gained no declaration
    for h, n in (('prodsearch_hip.h', 5), ('prodsearch_rtm_cand.h', 3)):
        text = open(os.path.join(REPO, 'include', h)).read()
        assert len(set(re.findall(r'\b(ps_rtm_rank_[a-z0-9_]+)\s*\(', text))) == n and 'rank_seq' not in text


def test_case_tables_cover_the_same_names():
    assert set(S.CASES) == set(S.PLAN) == set(S.YARDSTICK)
    assert all(set(p) <= set(S.PLAN_FIELDS) for p in S.PLAN.values())
    assert all(0 < S.bound(n, f) <= S.TOL for n in S.CASES for f in ('cat', 'list'))
    assert all(kw['data'] in U.CASES for kw in S.CASES.values())


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_plan_of_every_case(lib, name):
    """``ps_rtm_rank_seq_plan`` (host only) for the two calls the GPU case makes."""
    h = S.host_case(name)
    c = h.c
    want = S.plan_passes(name, c)
    for form, Cw, spp in (('list', S.C_LIST, h.spp_list), ('cat', None, h.spp_cat)):
        plan = S.plan_of(lib, h.m, c, Cw, 10, spp)
        print(name, form, plan)
        for f, v in S.PLAN[name].items():
            assert plan[f] == v, (name, form, f, plan[f], v)
        assert plan['epl'] * 64 == c.a.embedding_size and plan['lph'] * c.a.heads == 64
        assert (plan['slots_per_pass'], plan['passes']) == want[form]


def _desc_shape(c, **edit):
    m, _ = U.build_model(c, 'cpu')
    d, sh = m._rank_all_desc(c.B, c.qw.shape[1], c.U, (c.P, c.RC - 1, c.I))
    for k, v in edit.items():
        setattr(d if hasattr(d, k) else sh, k, v)
    return m, d, sh


def test_plan_follows_the_scratch_in_both_forms_and_the_refusals(lib):
    c = U.make_case()
    _, d, sh = _desc_shape(c)
    plan = _lib.PsRtmRankSeqPlan()
    NO = _lib.PS_RTM_SEQ_NO_LIST
    sizes = {n: lib.ps_rtm_rank_seq_scratch_bytes(d, sh, 12, 10, n) for n in (1, 5, 0, 40)}
    assert 0 < sizes[1] < sizes[5] < sizes[0] == sizes[40]                 # the bytes grow with the pass, up to the list
    for n, want in ((1, 1), (5, 5), (0, 12)):
        assert lib.ps_rtm_rank_seq_plan(d, sh, 12, 10, sizes[n], plan) == 0
        assert (plan.slots_per_pass, plan.passes) == (want, -(-12 // want))
    assert lib.ps_rtm_rank_seq_plan(d, sh, 12, 10, sizes[5] - 1, plan) == 0 and plan.slots_per_pass == 4    # the most that fit
    cat = {n: lib.ps_rtm_rank_seq_scratch_bytes(d, sh, NO, 10, n) for n in (1, 8, 0, 100)}
    assert 0 < cat[1] < cat[8] < cat[0] == cat[100]                         # no list: the columns are the P = 37 rows
    for n, want in ((1, 1), (8, 8), (0, 37)):
        assert lib.ps_rtm_rank_seq_plan(d, sh, NO, 10, cat[n], plan) == 0
        assert (plan.slots_per_pass, plan.passes) == (want, -(-37 // want))
    assert (37 % 8, -(-37 // 8)) == (5, 5)
    # the field says what the run is; these entries serve both values of it — and size both alike
    sh.seq_review_test = 1
    assert lib.ps_rtm_rank_seq_scratch_bytes(d, sh, 12, 10, 5) == sizes[5]
    assert lib.ps_rtm_rank_seq_plan(d, sh, NO, 10, cat[8], plan) == 0 and plan.slots_per_pass == 8
    assert lib.ps_rtm_rank_cand_scratch_bytes(d, sh, 12, 10, 5) == -1 and 'do_seq_review_test' in lib.ps_last_error().decode()
    sh.seq_review_test = 0
    # refusals
    assert lib.ps_rtm_rank_seq_plan(d, sh, 12, 10, sizes[1] - 1, plan) != 0 and 'scratch' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_seq_plan(d, sh, 12, 257, sizes[0], plan) != 0 and 'topk' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_seq_scratch_bytes(d, sh, 12, 257, 0) == -1 and 'topk' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_seq_plan(d, sh, 0, 10, sizes[0], plan) != 0 and 'candidates per entry' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_seq_scratch_bytes(d, sh, 0, 10, 0) == -1 and 'candidates per entry' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_seq_plan(d, sh, 12, 10, sizes[0], None) != 0
    big = 1 << 28
    assert c.B * big >= 1 << 30
    assert lib.ps_rtm_rank_seq_scratch_bytes(d, sh, big, 10, big) == -1 and 'per pass' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_seq_scratch_bytes(d, sh, big, 10, 7) > 0
    # a null timeline (and a timeline with a null array): before anything is launched
    dummy = C.c_void_p(256)
    ps = _lib.PsRtmTensors()
    call = lambda tl: lib.ps_rtm_rank_seq(d, sh, ps, dummy, tl, dummy, dummy, dummy, dummy, 12, dummy, 10, dummy, dummy, dummy, None,
                                          dummy, 1 << 24, None)
    assert call(None) != 0 and 'null timeline' in lib.ps_last_error().decode()
    assert call(_lib.PsRtmSeqTimeline(256, None, 256, 4)) != 0 and 'null timeline' in lib.ps_last_error().decode()
    assert call(_lib.PsRtmSeqTimeline(256, 256, 256, 0)) != 0 and 'at least 1' in lib.ps_last_error().decode()


@pytest.mark.parametrize('edit,flag', [(dict(n_layers=2), 'inter_layers'),
                                       (dict(fix_emb=1, review_encoder=_lib.PS_RENC_FS), 'fix_emb'),
                                       (dict(fix_emb=1, review_encoder=_lib.PS_RENC_AVG), 'fix_emb'), (dict(d=96), 'embedding_size')])
def test_c_entries_refuse_with_the_messages_of_rank_all(lib, edit, flag):
    c = U.make_case()
    _, d, sh = _desc_shape(c, **edit)
    assert lib.ps_rtm_rank_scratch_bytes(d, sh, 10, 0) == -1
    want = lib.ps_last_error().decode()
    assert flag in want
    for seq in (0, 1):
        sh.seq_review_test = seq
        assert lib.ps_rtm_rank_seq_scratch_bytes(d, sh, 12, 10, 0) == -1 and lib.ps_last_error().decode() == want
        plan = _lib.PsRtmRankSeqPlan()
        assert lib.ps_rtm_rank_seq_plan(d, sh, 12, 10, 1 << 24, plan) != 0 and lib.ps_last_error().decode() == want
        dummy = C.c_void_p(256)                   # never read: the refusal comes before any argument is touched
        tl = _lib.PsRtmSeqTimeline(256, 256, 256, 4)
        assert lib.ps_rtm_rank_seq(d, sh, _lib.PsRtmTensors(), dummy, tl, dummy, dummy, dummy, dummy, 12, dummy, 10, dummy, dummy, dummy,
                                   None, dummy, 1 << 20, None) != 0 and lib.ps_last_error().decode() == want


def test_static_rankers_still_refuse_the_mode_and_the_new_entry_refuses_the_rest():
    from prodsearch_amd import evaluate
    c = U.make_case()
    cands = K.make_cands(c)
    c.a = U.make_args(do_seq_review_test=True, train_review_only=False)
    m, _ = U.build_model(c, 'cpu')
    assert 'do_seq_review_test' in m._rank_all_refusal() and m._rank_all_refusal(time_ordered=True) is None
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        m.catalogue_index(c.item_r)
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        evaluate.rank_all_rtm(m, None, U.rank_batch(c), 10)
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        evaluate.rank_candidates_rtm(m, None, K.rank_batch(c, cands), 10)
    assert m._rank_all_desc(1, 1, 1, (c.P, 0, c.I))[1].seq_review_test == 1
    # the new entry: the other refusals of _rank_all_refusal, then "another model" / "stale" / a batch without stamps
    tl = S.make_timeline(c)
    c.a = U.make_args(inter_layers=2, do_seq_review_test=True, train_review_only=False)
    m2, _ = U.build_model(c, 'cpu')
    with pytest.raises(NotImplementedError, match='inter_layers'):
        evaluate.rank_seq_rtm(m2, None, S.rank_batch(c, tl), 10)
    with pytest.raises(NotImplementedError, match='inter_layers'):
        m2.timeline_index(None, None, None)
    idx = types.SimpleNamespace(model=m2, stale=lambda: False)
    with pytest.raises(RuntimeError, match='another model'):
        evaluate.rank_seq_rtm(m, idx, S.rank_batch(c, tl), 10)
    idx.model, idx.stale = m, (lambda: True)
    with pytest.raises(RuntimeError, match='stale'):
        evaluate.rank_seq_rtm(m, idx, S.rank_batch(c, tl), 10)
    idx.stale = lambda: False
    with pytest.raises(RuntimeError, match='time_stamps'):
        evaluate.rank_seq_rtm(m, idx, U.rank_batch(c), 10)
    # the batch: the constructor stays positionally compatible, .to() carries the stamps along
    rb = K.rank_batch(c, cands)
    assert rb.time_stamps is None and rb.candi_prod_idxs is not None
    moved = S.rank_batch(c, tl, cands).to('meta')
    assert moved.time_stamps.shape == (c.B,) and moved.time_stamps.device.type == 'meta' and moved.candi_prod_idxs.shape == cands.shape


def test_timeline_check_names_the_item():
    from prodsearch_amd import ProductRanker
    c = U.make_case()
    tl = S.make_timeline(c)
    t = torch.from_numpy
    ProductRanker._timeline_check(t(tl.ptr), t(tl.rids), t(tl.times))       # sorted: passes (equal times and empty items included)
    times = tl.times.copy()
    at = int(tl.ptr[9]) + 1                                                 # inside item 9 ...
    assert tl.ptr[10] - tl.ptr[9] >= 2
    times[at - 1], times[at] = S.T_MAX + 5, S.T_MAX + 4
    with pytest.raises(RuntimeError, match='item 9 '):
        ProductRanker._timeline_check(t(tl.ptr), t(tl.rids), t(times))
    # ... while a fall from one item's last time to the next item's first is none
    times = tl.times.copy()
    times[int(tl.ptr[9]):int(tl.ptr[10])] += 1000
    ProductRanker._timeline_check(t(tl.ptr), t(tl.rids), t(times))
    for edit, msg in ((lambda p: p.__setitem__(0, 1), 'rise from 0'), (lambda p: p.__setitem__(-1, tl.N - 1), 'rise from 0'),
                      (lambda p: p.__setitem__(5, int(p[4]) - 1), 'falls after item 4')):
        ptr = tl.ptr.copy()
        edit(ptr)
        with pytest.raises(RuntimeError, match=msg):
            ProductRanker._timeline_check(t(ptr), t(tl.rids), t(tl.times))


# ------------------------------------------------------------------------------------------------- 2. the loader
def _loader(tmp_path, set_name='valid', **over):
    kw = dict(model_name='review_transformer', uprev_review_limit=3, iprev_review_limit=4, review_word_limit=12,
              candi_batch_size=3, valid_candi_size=7, test_candi_size=-1, do_seq_review_test=True, train_review_only=False)
    kw.update(over)
    args = default_args(**kw)
    data_path, inp = synth.write_corpus(str(tmp_path), 41, n_users=30, n_products=50, n_words=120)
    gd = GlobalProdSearchData(args, data_path, inp)
    pd = ProdSearchData(args, inp, set_name, gd)
    if set_name == 'train':
        pd.initialize_epoch()
    ds = ProdSearchDataset(args, gd, pd)
    return args, gd, ds, ProdSearchDataLoader(args, ds, batch_size=4, shuffle=False)


def _same_but_padding(got, want, fill, what):
    """``got`` [1, C, r] of one entry against its row of the batch's tensor ``want`` [1, C, R >= r], the rest padding."""
    r = got.shape[-1]
    assert want.shape[-1] >= r and np.array_equal(want[..., :r], got), what
    assert (want[..., r:] == fill).all(), what


def test_seq_batches_reassemble_the_test_collate(tmp_path):
    """The time-ordered mode on a synthetic corpus: ``timeline()`` is sorted; ``seq_candidate_batches()`` gives the entries of
    the dataset's rows with their chunks concatenated, the user's reviews by the time-ordered rule and the stamps; and
    ``assemble_chunk`` over ``cat_of`` PER ENTRY reproduces every tensor of ``test_batch_from_ids`` over the same rows, bit for
    bit.  At every live position the per-position user / item ids are the review's own author and item (``ids_from_reviews``
    changes nothing): the projection adds exactly those rows."""
    from prodsearch_amd import ProductRanker
    args, gd, ds, dl = _loader(tmp_path)
    seg, W = 3, int(args.iprev_review_limit)
    ptr, rids, times = (x.numpy() for x in dl.timeline())
    ProductRanker._timeline_check(*dl.timeline())
    assert len(ptr) == gd.product_size + 1 and ptr[-1] == len(rids) == len(times)
    assert all((np.diff(times[ptr[p]:ptr[p + 1]]) >= 0).all() for p in range(gd.product_size))
    lt = np.asarray(gd.review_loc_time, dtype=np.int64).reshape(-1, 3)
    assert np.array_equal(times, lt[rids, 2])
    tl = types.SimpleNamespace(ptr=ptr, rids=rids, times=times)
    ent = dl.rank_entries()
    pad = gd.review_count - 1
    up = np.asarray(gd.review_u_p, dtype=np.int64).reshape(-1, 2)
    fills = dict(candi_prod_ridxs=pad, candi_seg_idxs=3, candi_seq_user_idxs=gd.user_size, candi_seq_item_idxs=gd.product_size)
    batches, plain = list(dl.seq_candidate_batches()), list(dl.seq_rank_batches())
    assert len(batches) == len(plain) == -(-len(ent) // 4) and sum(len(b.user_idxs) for b in batches) == len(ent)
    lo, n_cut, n_prefix = 0, 0, 0
    for rb, pb in zip(batches, plain):
        ids = ent[lo:lo + len(rb.user_idxs)]
        lo += len(ids)
        assert pb.candi_prod_idxs is None
        for f in ('query_word_idxs', 'u_ridxs', 'target_prod_idxs', 'time_stamps'):
            assert torch.equal(getattr(rb, f), getattr(pb, f)), f
        assert list(rb.user_idxs) == list(pb.user_idxs) and list(rb.query_idxs) == list(pb.query_idxs)
        quad = dl.entry_quad[ids]
        assert np.array_equal(rb.time_stamps.numpy(), lt[quad[:, 3], 2])
        cand = rb.candi_prod_idxs.numpy()
        assert cand.shape == (len(ids), 7) and (cand >= 0).all()
        cats = [S.cat_of(tl, int(s), W, pad) for s in rb.time_stamps.tolist()]
        static = [S.cat_of(tl, int(s), W, pad, 'no_stamp') for s in rb.time_stamps.tolist()]
        n_cut += sum(not np.array_equal(a, b) for a, b in zip(cats, static))
        n_prefix += int((U.leading(rb.u_ridxs.numpy(), pad) > 0).sum())
        for j in range(seg):
            tb = dl.test_batch_from_ids(ids + j)
            chunk = np.asarray(tb.candi_prod_idxs)
            mine_ids = cand[:, 3 * j:3 * j + chunk.shape[1]]
            assert np.array_equal(mine_ids, chunk), (lo, j)
            assert list(tb.user_idxs) == list(rb.user_idxs) and list(tb.query_idxs) == list(rb.query_idxs)
            assert np.array_equal(np.asarray(tb.target_prod_idxs), rb.target_prod_idxs.numpy())
            assert torch.equal(tb.query_word_idxs, rb.query_word_idxs)
            for b in range(len(ids)):
                for from_reviews in (False, True):
                    mine = U.assemble_chunk(rb.query_word_idxs[b:b + 1], rb.u_ridxs[b:b + 1], rb.user_idxs[b:b + 1], cats[b],
                                            mine_ids[b:b + 1], up, gd.user_size, gd.product_size, pad, ids_from_reviews=from_reviews)
                    for f in TEST_FIELDS[1:]:
                        _same_but_padding(getattr(mine, f).numpy(), getattr(tb, f).numpy()[b:b + 1], fills[f], (lo, j, b, f))
    assert lo == len(ent)
    print('%d of %d entries see a catalogue the static rule would not give; %d have previous reviews of their user'
          % (n_cut, len(ent), n_prefix))
    assert n_cut > len(ent) // 2 and n_prefix > 0


def test_loader_serves_the_time_ordered_mode_alone(tmp_path):
    _, _, _, dl = _loader(tmp_path, do_seq_review_test=False)
    for call in (dl.timeline, lambda: next(dl.seq_rank_batches()), lambda: next(dl.seq_candidate_batches())):
        with pytest.raises(NotImplementedError, match='do_seq_review_test'):
            call()
    _, _, _, dl = _loader(tmp_path, train_review_only=True)
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        dl.timeline()
    next(dl.candidate_batches())                                            # ... which is the static rule's mode
    _, _, _, dl = _loader(tmp_path)
    for call in (dl.catalogue_reviews, lambda: next(dl.rank_batches()), lambda: next(dl.candidate_batches())):
        with pytest.raises(NotImplementedError, match='do_seq_review_test'):
            call()
    _, _, _, dl = _loader(tmp_path, set_name='train')
    for call in (dl.timeline, lambda: next(dl.seq_rank_batches()), lambda: next(dl.seq_candidate_batches())):
        with pytest.raises(RuntimeError, match='evaluation loader'):
            call()


# ------------------------------------------------------------------------------------------------- 3. the cases on the host
@pytest.mark.parametrize('name', sorted(S.CASES))
def test_timeline_holds_its_special_items_and_stamps(name):
    h = S.host_case(name)
    c, tl, W, pad = h.c, h.tl, S.window_of(h.c), h.c.RC - 1
    lens = np.diff(tl.ptr)
    assert list(lens[:7]) == [0, W, 70, 4100, 64, 65, 4200] and (lens[7:] >= 1).all() and (lens[7:] <= 3 * W).all()
    assert tl.N == lens.sum() and (tl.rids[np.arange(tl.N) != tl.ptr[6] - 2] != pad).all() and tl.rids[tl.ptr[6] - 2] == pad
    assert list(tl.stamps[:2]) == [S.I64_MIN, S.I64_MAX] and tl.stamps[2] == tl.tie_time
    assert all((np.diff(tl.times[tl.ptr[p]:tl.ptr[p + 1]]) >= 0).all() for p in range(c.P))
    # the tie: a run of at least two equal times in item 2, all of it inside the prefix
    t2 = tl.times[tl.ptr[2]:tl.ptr[3]]
    run = np.flatnonzero(t2 == tl.tie_time)
    assert len(run) >= 2
    right, left = S.cat_of(tl, tl.tie_time, W, pad), S.cat_of(tl, tl.tie_time, W, pad, 'cut_left')
    assert right[2, -1] == tl.rids[tl.ptr[2] + run[-1]] and left[2, -1] == tl.rids[tl.ptr[2] + run[0] - 1]
    # entry 0 sees nothing, entry 1 the last W of everything — the pad id ends item 5's window in its middle
    assert (S.cat_of(tl, S.I64_MIN, W, pad) == pad).all()
    last = S.cat_of(tl, S.I64_MAX, W, pad)
    assert np.array_equal(last, S.cat_of(tl, 0, W, pad, 'no_stamp'))
    assert 0 < U.leading(last, pad)[S.PAD_ITEM] == W - 2 and (U.leading(np.delete(last, [0, S.PAD_ITEM], 0), pad) >= 1).all()
    # the long items' windows of the mid-range entries are not at the front of their sequences
    for e in range(2, c.B):
        for i in (2, 3, 6):
            cut = int(np.searchsorted(tl.times[tl.ptr[i]:tl.ptr[i + 1]], tl.stamps[e], side='right'))
            assert W < cut < lens[i], (e, i, cut)
            assert np.array_equal(S.cat_of(tl, int(tl.stamps[e]), W, pad)[i], tl.rids[tl.ptr[i] + cut - W:tl.ptr[i] + cut])
    # the lists
    lists = h.lists
    assert lists.shape == (c.B, S.C_LIST) and list(lists[0]) == [0, 1, 2, 3] + [-1] * 8
    t1 = int(c.target[1])
    assert lists[1, 2] == t1 == lists[1, 7] and lists[1, 4] == c.P + 3 and lists[1, 5] == -1 and {3, 5, 6} <= set(lists[1].tolist())
    assert list(lists[2, :5]) == [2, 3, 4, 5, 6] and not 0 <= int(c.target[-1]) < c.P


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_factorisation_on_the_entrys_own_catalogue_in_float64(name):
    """``factorised_scores`` per entry on ``cat_of`` against ``oracle.rtm.rtm_test`` on the assembled chunk: nothing in the
    §8b.1 factorisation depends on the catalogue being the same for every entry."""
    h = S.host_case(name)
    e = U.entry_err(h.f64, h.ref64)
    print('%s: factorisation vs rtm_test in float64, worst entry %.3g' % (name, e.max()))
    assert e.max() < 1e-10
    assert float((h.ref64[0].max() - h.ref64[0].min()).abs()) <= 1e-12 * float(h.ref64[0].abs().max())   # INT64_MIN: all alike


@pytest.mark.parametrize('fault', S.FAULTS)
@pytest.mark.parametrize('name', sorted(n for n in S.CASES if n != 'passes'))
def test_bound_catches_a_wrong_window(name, fault):
    """In float64, a search with one mistake — ``bisect_left``, the first W of the prefix, no stamp at all — moves every entry it
    acts on by at least twice the case's bound; where it cannot act the bits are the same."""
    h = S.host_case(name)
    c = h.c
    got, acts = S.factorised_seq(c, h.P64, h.rev64, h.tl, fault)
    e = U.entry_err(got, h.f64)
    b = S.bound(name, 'cat')
    print('%s / %s: acts on entries %s, moves them by %s (bound %.3g)' % (name, fault, np.flatnonzero(acts).tolist(),
                                                                          ['%.3g' % x for x in e[acts]], b))
    want = {'cut_left': [False, False, True], 'first_I': [False, True, True], 'no_stamp': [True, False, True]}[fault]
    assert list(acts[:3]) == want and acts[3:].all()
    assert (e[acts] >= 2 * b).all()
    assert all(torch.equal(got[i], h.f64[i]) for i in np.flatnonzero(~acts))


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_recorded_yardstick_still_holds_and_the_oracle_stays_under_the_band_cap(name):
    """``S.YARDSTICK[name]`` re-measured (a tenth on top for this host's summation order), over the catalogue and over the
    lists; and on the fp32 oracle alone at most a quarter of the listed positions lie in a 2 * tol band — of the catalogue
    form's positions too, entry 0 apart, whose row is one exact tie by construction."""
    h = S.host_case(name)
    c = h.c
    print('%s: yardstick measured (%.3g, %.3g), recorded %s, bounds (%.3g, %.3g)'
          % ((name,) + h.yard + (S.YARDSTICK[name], S.bound(name, 'cat'), S.bound(name, 'list'))))
    assert all(0 < y <= 1.1 * r for y, r in zip(h.yard, S.YARDSTICK[name]))
    _, _, frac = K.list_bands(K.take(h.ref32, h.lists, c.P), h.lists, c.P)
    _, _, frac_cat = S.cat_bands(h.ref32)
    print('%s: %.3f of the listed positions in a band; %.3f of the catalogue form\'s, entry 0 apart' % (name, frac, frac_cat))
    assert frac <= S.BAND_CAP and frac_cat <= S.BAND_CAP
