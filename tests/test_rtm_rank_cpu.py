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
CASES = {'base': dict(),
         'pv_user_item': dict(encoder='pv', use_user_emb=True, use_item_emb=True),
         'no_pos': dict(use_pos_emb=False),
         'no_seg': dict(use_seg_emb=False),
         'long': dict(U=20, I=30, P=70, B=3, RC=2500)}


@pytest.mark.parametrize('name', sorted(CASES))
def test_factorisation_is_exact_in_float64(name):
    """The split softmax + linear key / value decomposition against ``rtm_test``: 1e-10 in float64; in fp32 the figure is what
    the re-association alone costs — the yardstick beside the GPU's 1e-4 bound (profiles/rtm_rank_all.md: it stays two orders
    below it).  Also: at synth.make_state_dict's scale at most a quarter of the oracle's order lies in a 2 * tol band."""
    c = U.make_case(**CASES[name])
    _, sd = U.build_model(c, 'cpu')
    T = c.U + c.I
    ref64, P64, rev64 = U.oracle_scores(c, sd, f64=True)
    got64 = U.factorised_scores(P64, c.a, c.qw, c.u_r, c.item_r, rev64, c.review_u_p, c.V, c.RC, T)
    e64 = rel_err(got64, ref64)
    ref32, P32, rev32 = U.oracle_scores(c, sd, f64=False)
    got32 = U.factorised_scores(P32, c.a, c.qw, c.u_r, c.item_r, rev32, c.review_u_p, c.V, c.RC, T)
    e32, o32 = rel_err(got32, ref64), rel_err(ref32, ref64)
    _, band = U.banded(ref32)
    print('%s: factorised f64 %.3g, factorised fp32 vs f64 %.3g, rtm_test fp32 vs f64 %.3g, banded %.3f'
          % (name, e64, e32, o32, band.mean()))
    assert e64 < 1e-10
    assert e32 < U.TOL
    assert band.mean() <= 0.25


# ------------------------------------------------------------------------------------------------- 3. ABI and refusals
@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


NEW = ('ps_rtm_rank_index_floats', 'ps_rtm_rank_index', 'ps_rtm_rank_scratch_bytes', 'ps_rtm_rank_all')


def test_rank_all_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, 'include', 'prodsearch_hip.h')).read()
    declared = set(re.findall(r'\b(ps_rtm_rank_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW)
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(_lib.PsRtmRankShape) == 32


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
