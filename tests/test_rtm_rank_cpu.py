"""The review transformer over the whole catalogue (``evaluate.rank_all_rtm``), the parts that need no GPU:
the entries-only loader against the test collate, the factorisation itself against ``oracle.rtm.rtm_test``, the C ABI
and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rtm_rank_util as U
from golden_util import rel_err
from prodsearch_amd import _lib, build as pbuild, default_args, synth
from prodsearch_amd.corpus import GlobalProdSearchData, ProdSearchData, ProdSearchDataset
from prodsearch_amd.rtm_loader import ProdSearchDataLoader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_FIELDS = ('query_word_idxs', 'candi_prod_ridxs', 'candi_seg_idxs', 'candi_seq_user_idxs', 'candi_seq_item_idxs')


# ------------------------------------------------------------------------------------------------- 1. the loader
def _loader(tmp_path, **over):
    args = default_args(model_name='review_transformer', uprev_review_limit=3, iprev_review_limit=4, review_word_limit=12,
                        candi_batch_size=16, test_candi_size=-1, **over)
    data_path, inp = synth.write_corpus(str(tmp_path), 41, n_users=30, n_products=50, n_words=120)
    gd = GlobalProdSearchData(args, data_path, inp)
    pd = ProdSearchData(args, inp, 'test', gd)
    # a user without any train review: the corpus writer gives every user one, so one user's are taken out of the train set
    info = np.asarray(gd.train_review_info, dtype=np.int64).reshape(-1, 4)
    bare = int(np.asarray(pd.review_info, dtype=np.int64).reshape(-1, 4)[0, 1])
    gd.train_review_info = [tuple(int(x) for x in r) for r in info[info[:, 1] != bare]]
    ds = ProdSearchDataset(args, gd, pd)
    return args, gd, ds, ProdSearchDataLoader(args, ds, batch_size=7, shuffle=False), bare


def test_entries_only_batches_reassemble_the_test_collate(tmp_path):
    args, gd, ds, dl, bare = _loader(tmp_path)
    cat = dl.catalogue_reviews().numpy()
    pad = gd.review_count - 1
    assert cat.shape == (gd.product_size, 4)
    n_item = U.leading(cat, pad)
    assert (n_item == 0).any() and (n_item == 4).any()                     # an item with no reviews, one with a full list
    ent = dl.rank_entries()
    seg = (gd.product_size - 1) // args.candi_batch_size + 1
    assert len(ent) * seg == len(ds) and np.array_equal(ent, np.arange(0, len(ds), seg))
    up = np.asarray(gd.review_u_p, dtype=np.int64).reshape(-1, 2)
    saw_bare = False
    for lo in range(0, len(ent), 7):
        ids = ent[lo:lo + 7]
        rb = dl.rank_batch_from_ids(ids)
        n_user = U.leading(rb.u_ridxs.numpy(), pad)
        saw_bare |= bool(((np.asarray(rb.user_idxs) == bare) & (n_user == 0)).any())
        for j in range(seg):                                               # every chunk of these entries, the ragged last one too
            tb = dl.test_batch_from_ids(ids + j)
            mine = U.assemble_chunk(rb.query_word_idxs, rb.u_ridxs, rb.user_idxs, cat, np.asarray(tb.candi_prod_idxs), up,
                                    gd.user_size, gd.product_size, pad)
            for f in TEST_FIELDS:
                got, ref = getattr(mine, f).numpy(), getattr(tb, f).numpy()
                assert got.shape == ref.shape and np.array_equal(got, ref), (lo, j, f)
            assert np.array_equal(rb.target_prod_idxs.numpy(), np.asarray(tb.target_prod_idxs))
            assert list(rb.user_idxs) == list(tb.user_idxs) and list(rb.query_idxs) == list(tb.query_idxs)
            # what the projection relies on: at every live review position the ids are the review's own author and item
            r = tb.candi_prod_ridxs.numpy()
            live = r != pad
            assert np.array_equal(tb.candi_seq_user_idxs.numpy()[:, :, 1:][live], up[r[live], 0])
            assert np.array_equal(tb.candi_seq_item_idxs.numpy()[:, :, 1:][live], up[r[live], 1])
    assert saw_bare                                                        # the user with no reviews was among the entries


def test_loader_refuses_entry_dependent_item_lists(tmp_path):
    _, _, _, dl, _ = _loader(tmp_path, do_seq_review_test=True, train_review_only=False)
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        dl.catalogue_reviews()
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        dl.rank_batch_from_ids([0])


# ------------------------------------------------------------------------------------------------- 2. the factorisation
CASES = U.CASES          # every case the GPU file runs (tests/rtm_rank_util.py), computed once per name (U.host_case)


def test_case_tables_cover_the_same_names():
    assert set(U.CASES) == set(U.PLAN) == set(U.YARDSTICK)
    assert all(set(p) <= set(U.PLAN_FIELDS) for p in U.PLAN.values())
    assert all(0 < U.bound(n) <= U.TOL for n in U.CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_factorisation_is_exact_in_float64(name):
    """The split softmax + linear key / value decomposition against ``rtm_test``: 1e-10 in float64; in fp32 the figure is what
    the re-association alone costs — the yardstick beside the GPU's 1e-4 bound (profiles/rtm_rank_all.md: it stays two orders
    below it).  Also: at synth.make_state_dict's scale at most a quarter of the oracle's order lies in a 2 * tol band.
    The two sides cut a sequence independently (``assemble_chunk(limit=)`` feeds the oracle, ``factorised_scores`` cuts by the
    kernel's counts), so the ``cap`` cases pin the rule itself."""
    h = U.host_case(name)
    e64 = rel_err(h.f64, h.ref64)
    e32, o32 = rel_err(h.f32, h.ref64), rel_err(h.ref32, h.ref64)
    _, band = U.banded(h.ref32)
    print('%s: factorised f64 %.3g, factorised fp32 vs f64 %.3g, rtm_test fp32 vs f64 %.3g, banded %.3f'
          % (name, e64, e32, o32, band.mean()))
    assert e64 < 1e-10
    assert U.entry_err(h.f64, h.ref64).max() < 1e-10
    assert e32 < U.TOL
    assert band.mean() <= 0.25


@pytest.mark.parametrize('name', sorted(CASES))
def test_recorded_yardstick_still_holds(name):
    """``U.YARDSTICK[name]``: the worst entry's error of fp32 on the host (the fp32 oracle, the fp32 factorisation) against the
    float64 oracle, re-measured; a tenth on top for this host's summation order.  The GPU's per-entry bound is 8 x the record."""
    h = U.host_case(name)
    print('%s: yardstick measured %.3g, recorded %.3g, bound %.3g' % (name, h.yard, U.YARDSTICK[name], U.bound(name)))
    assert h.yard <= 1.1 * U.YARDSTICK[name]


def test_the_cases_hold_what_they_were_written_for():
    pad = lambda c: c.RC - 1
    c = U.host_case('lds_full').c                                          # a full ballot on both sides: 64 live ids
    assert U.leading(c.u_r.numpy(), pad(c))[1] == 64 and U.leading(c.item_r.numpy(), pad(c))[1] == 64
    c = U.host_case('cap').c                                               # T = 5 review positions under lists of 4 and 6
    nu, ni = U.leading(c.u_r.numpy(), pad(c)), U.leading(c.item_r.numpy(), pad(c))
    assert c.T == 5 and nu[1] == 4 and ((nu >= 2) & (nu <= 4)).sum() >= 2  # the full user list leaves every item one review
    assert (ni[None, :] > c.T - nu[:, None]).any(1).all()                   # every entry has items that are cut
    c = U.host_case('cap_user').c
    nu, ni = U.leading(c.u_r.numpy(), pad(c)), U.leading(c.item_r.numpy(), pad(c))
    assert c.T == 5 and nu[1] == 6                                          # cut to 5: the user's list alone fills the sequence
    assert ((nu >= 2) & (nu < 5)).any() and (ni > 3).any()
    h = U.host_case('cap_user')
    assert (h.keys[1] == 6).all()                                           # n = 0 for every item: one score for the whole catalogue
    assert float((h.ref64[1] - h.ref64[1, 0]).abs().max()) < 1e-12 * float(h.ref64[1].abs().max())
    # sharp: on the float64 side some pair's softmax over at least four keys puts more than 0.99 on one of them; base does not
    hs, hb = U.host_case('sharp'), U.host_case('base')
    assert float(hs.wmax[hs.keys >= 4].max()) > 0.99 and float(hb.wmax[hb.keys >= 4].max()) < 0.9


@pytest.mark.parametrize('name', sorted(CASES))
def test_one_mistake_in_the_kernel_would_exceed_the_bound(name):
    """What the per-entry bound (8 x yardstick) still catches, in float64: ``factorised_scores(fault=...)`` makes one mistake
    of the kind the kernels could make, and every entry it acts on must move its error by at least twice the bound; where a
    mistake cannot act by construction (no positions / no segments / nothing to cut / one head) the scores are the same bits."""
    h = U.host_case(name)
    base = U.entry_err(h.f64, h.ref64)
    a = h.c.a
    for fault in U.FAULTS:
        s, acts = U.faulty_scores(h, fault)
        moved = np.abs(U.entry_err(s, h.ref64) - base)
        print('%s %-12s acts on %d of %d entries, moves them by %.3g .. %.3g (bound %.3g)'
              % (name, fault, acts.sum(), len(acts), moved[acts].min() if acts.any() else 0, moved[acts].max() if acts.any() else 0,
                 U.bound(name)))
        assert (moved[acts] >= 2 * U.bound(name)).all(), (name, fault, moved)
        assert torch.equal(s[~acts], h.f64[~acts]), (name, fault)
        expect_none = (fault == 'pos_off' and not a.use_pos_emb) or (fault == 'seg1_keys' and not a.use_seg_emb) or \
                      (fault == 'no_cap' and not name.startswith('cap')) or (fault == 'heads_merged' and a.heads == 1)
        assert acts.any() != expect_none, (name, fault)
        if fault in ('no_cap', 'heads_merged') and not expect_none:
            assert acts.all(), (name, fault)
    if name == 'base':                                                      # orientation: the full item (6 reviews), its last key dropped
        s, _ = U.faulty_scores(h, 'drop_last')
        pair = ((s[:, 1] - h.ref64[:, 1]).abs() / h.ref64.abs().amax(1)).numpy()
        print('base: item 1 without its last key moves its pairs by %.3g .. %.3g' % (pair.min(), pair.max()))
        assert (pair >= 2 * U.bound(name)).all()


# ------------------------------------------------------------------------------------------------- 3. ABI and refusals
@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


NEW = ('ps_rtm_rank_index_floats', 'ps_rtm_rank_index', 'ps_rtm_rank_scratch_bytes', 'ps_rtm_rank_all', 'ps_rtm_rank_plan')


def test_rank_all_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, 'include', 'prodsearch_hip.h')).read()
    declared = set(re.findall(r'\b(ps_rtm_rank_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW)
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_lib.PsRtmRankShape) == 32
    assert C.sizeof(_lib.PsRtmRankPlan) == 40
    body = re.search(r'typedef struct PsRtmRankPlan \{(.*?)\} PsRtmRankPlan;', hdr, re.S).group(1)
    assert tuple(re.findall(r'int(?:32|64)_t\s+(\w+);', body)) == tuple(n for n, _ in _lib.PsRtmRankPlan._fields_)


@pytest.mark.parametrize('name', sorted(U.CASES))
def test_plan_of_every_case(lib, name):
    """``ps_rtm_rank_plan`` (host only) for the call the GPU case makes: the branch each case was written for (``U.PLAN``), and
    the fields that follow from the shape alone."""
    h = U.host_case(name)
    c = h.c
    plan = U.plan_of(lib, h.m, c, 10, h.ipp)
    print(name, plan)
    for f, v in U.PLAN[name].items():
        assert plan[f] == v, (name, f, plan[f], v)
    assert plan['epl'] * 64 == c.a.embedding_size and plan['lph'] * c.a.heads == 64
    assert plan['lds_bytes'] == plan['items_per_workgroup'] * c.I * 2 * c.a.embedding_size * 4 <= 128 * 1024
    assert plan['passes'] == -(-c.P // plan['items_per_pass']) and plan['items_per_pass'] == (h.ipp or c.P)


def test_plan_follows_the_scratch_and_refuses_as_the_launcher_does(lib):
    c = U.make_case()
    m, d, sh = _desc_shape(c)
    plan = _lib.PsRtmRankPlan()
    sizes = {n: lib.ps_rtm_rank_scratch_bytes(d, sh, 10, n) for n in (1, 8, 0)}
    for n, want in ((1, 1), (8, 8), (0, c.P)):
        assert lib.ps_rtm_rank_plan(d, sh, 10, sizes[n], plan) == 0
        assert (plan.items_per_pass, plan.passes) == (want, -(-c.P // want))
        assert plan.items_per_workgroup == min(8, want)                     # never more items than the pass holds
    assert lib.ps_rtm_rank_plan(d, sh, 10, sizes[8] - 1, plan) == 0 and plan.items_per_pass == 7   # the most that fit
    assert lib.ps_rtm_rank_plan(d, sh, 10, sizes[1] - 1, plan) != 0 and 'scratch' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_plan(d, sh, 257, sizes[0], plan) != 0
    _, d2, sh2 = _desc_shape(c, n_layers=2)
    assert lib.ps_rtm_rank_plan(d2, sh2, 10, sizes[0], plan) != 0 and 'inter_layers' in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_plan(d, sh, 10, sizes[0], None) != 0


def _desc_shape(c, **edit):
    m, _ = U.build_model(c, 'cpu')
    d, sh = m._rank_all_desc(c.B, c.qw.shape[1], c.U, (c.P, c.RC - 1, c.I))
    for k, v in edit.items():
        setattr(d if hasattr(d, k) else sh, k, v)
    return m, d, sh


@pytest.mark.parametrize('edit,flag', [(dict(n_layers=2), 'inter_layers'), (dict(seq_review_test=1), 'do_seq_review_test'),
                                       (dict(fix_emb=1, review_encoder=_lib.PS_RENC_FS), 'fix_emb'),
                                       (dict(fix_emb=1, review_encoder=_lib.PS_RENC_AVG), 'fix_emb')])
def test_c_entries_refuse(lib, edit, flag):
    c = U.make_case()
    _, d, sh = _desc_shape(c, **edit)
    assert lib.ps_rtm_rank_index_floats(d, sh) == -1 and flag in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_scratch_bytes(d, sh, 10, 0) == -1 and flag in lib.ps_last_error().decode()
    dummy = C.c_void_p(256)                       # never read: the refusal comes before any argument is touched
    ps = _lib.PsRtmTensors()
    assert lib.ps_rtm_rank_index(d, sh, ps, dummy, dummy, dummy, None) != 0 and flag in lib.ps_last_error().decode()
    assert lib.ps_rtm_rank_all(d, sh, ps, dummy, dummy, dummy, dummy, dummy, 10, dummy, dummy, dummy, None, dummy, 1 << 20,
                               None) != 0 and flag in lib.ps_last_error().decode()


def test_sizes_are_reported(lib):
    c = U.make_case()
    _, d, sh = _desc_shape(c)
    assert lib.ps_rtm_rank_index_floats(d, sh) > 2 * c.RC * 128
    one, eight, all_ = (lib.ps_rtm_rank_scratch_bytes(d, sh, 10, n) for n in (1, 8, 0))
    assert 0 < one < eight < all_                  # the pass size sets the workspace
    assert lib.ps_rtm_rank_scratch_bytes(d, sh, 257, 0) == -1


def test_python_refuses_up_front():
    from prodsearch_amd import evaluate
    c = U.make_case()
    for over, flag in ((dict(inter_layers=2), 'inter_layers'),
                       (dict(do_seq_review_test=True, train_review_only=False), 'do_seq_review_test')):
        c.a = U.make_args(**over)
        m, _ = U.build_model(c, 'cpu')
        with pytest.raises(NotImplementedError, match=flag):
            m.catalogue_index(c.item_r)
        with pytest.raises(NotImplementedError, match=flag):
            evaluate.rank_all_rtm(m, None, U.rank_batch(c), 10)
    # fs / avg with fix_emb: no ranker can be constructed so (next test); the branch itself, on a model put into that state
    c.a = U.make_args()
    m, _ = U.build_model(c, 'cpu')
    m.fix_emb, m.review_encoder_name = True, 'fs'
    with pytest.raises(NotImplementedError, match='fix_emb'):
        m.catalogue_index(c.item_r)
    # do_seq_review_test with train_review_only keeps the item lists entry-independent: not refused
    c.a = U.make_args(do_seq_review_test=True, train_review_only=True)
    m, _ = U.build_model(c, 'cpu')
    assert m._rank_all_refusal() is None


def test_pretrained_ranker_with_fs_and_fix_emb_is_refused_at_construction():
    """fs / avg review encoders together with fix_emb never reach rank_all_rtm: the ranker that owns fix_emb refuses them."""
    from prodsearch_amd.rtm_pretrained import PretrainedProductRanker
    c = U.make_case()
    for enc in ('fs', 'avg'):
        a = U.make_args(encoder=enc, fix_emb=True)
        with pytest.raises(NotImplementedError):
            PretrainedProductRanker(a, 'cpu', c.V, c.RC, c.P, c.n_users, c.rw, None, word_dists=None)
