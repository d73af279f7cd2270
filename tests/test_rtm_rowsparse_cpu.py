"""CPU-only checks of the review transformer's row-sparse optimizer path (``args.row_sparse_adam``): which tables a
configuration puts on their touched-row lists (``ProductRanker._sparse_paths``), where they sit in the flat gradient buffer,
what ``ps_coalesce_tables`` refuses before it launches anything, and the data-parallel refusal.  No GPU compute here."""
import ctypes as C

import pytest
import torch

import pretrain_rtm_util
import pretrain_util
from prodsearch_amd import PretrainedProductRanker, ProductRanker, _lib, default_args, dist as pdist, hot_module, synth
from prodsearch_amd import build as pbuild
from prodsearch_amd.item_transformer import ItemTransformerRanker

V, RC, D = 60, 40, 32
REVIEW, USER, ITEM, WORD = ('review_emb',), ('user_emb',), ('product_emb',), ('word_emb',)


def _args(**kw):
    base = dict(model_name='review_transformer', embedding_size=D, heads=4, ff_size=64, inter_layers=1, neg_per_pos=2,
                review_word_limit=8, do_subsample_mask=True, row_sparse_adam=True)
    base.update(kw)
    return default_args(**base)


def _model(a, cls=ProductRanker):
    torch.manual_seed(0)
    rng = synth.rng_for(3)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, 8)))
    rw[-1] = V - 1
    return cls(a, 'cpu', V, RC, 50, 30, rw, pretrain_util.vocab_words(V))


# ------------------------------------------------------------------------------------------------------- _sparse_paths
@pytest.mark.parametrize('enc,user,item,want', [
    ('pv', False, False, {REVIEW, WORD}),
    ('pv', True, False, {REVIEW, USER, WORD}),
    ('pv', True, True, {REVIEW, USER, ITEM, WORD}),
    ('pvc', False, False, set()),                      # the word table of a word-mean encoder stays in the dense plan
    ('pvc', False, True, {ITEM}),
    ('pvc', True, True, {USER, ITEM}),
    ('fs', False, False, set()),
    ('fs', True, True, {USER, ITEM}),
])
def test_sparse_paths_per_configuration(enc, user, item, want):
    m = _model(_args(review_encoder_name=enc, use_user_emb=user, use_item_emb=item))
    assert m._row_sparse()
    assert set(m._sparse_paths()) == want
    # the flat gradient buffer: every sparse table behind everything dense
    paths = [r[0] for r in m._grad_layout()[0]]
    n = len(want)
    assert set(paths[len(paths) - n:]) == want and not (set(paths[:len(paths) - n]) & want)
    # the same model without the flag: nothing sparse, the parent's order (by size alone)
    d = _model(_args(review_encoder_name=enc, use_user_emb=user, use_item_emb=item, row_sparse_adam=False))
    assert not d._row_sparse() and d._sparse_paths() == ()
    numel = {path: p.numel() for path, p in d._named_hot_params()}
    dp = [r[0] for r in d._grad_layout()[0]]
    assert dp == sorted(dp, key=lambda path: numel[path]) and set(dp) == set(paths)


def test_lazy_exact_adam_keeps_the_model_dense():
    m = _model(_args(review_encoder_name='pv', use_user_emb=True, use_item_emb=True, lazy_exact_adam=True))
    assert not m._row_sparse() and m._sparse_paths() == ()
    m = _model(_args(review_encoder_name='pv', row_sparse_adam=False, lazy_exact_adam=True))
    assert not m._row_sparse() and m._sparse_paths() == ()


def test_a_frozen_table_is_not_sparse(tmp_path):
    m = _model(_args(review_encoder_name='pv', use_user_emb=True, use_item_emb=True))
    m.user_emb.weight.requires_grad_(False)
    assert set(m._sparse_paths()) == {REVIEW, ITEM, WORD}
    m.review_encoder.review_embeddings.weight.requires_grad_(False)
    m.word_embeddings.weight.requires_grad_(False)
    assert set(m._sparse_paths()) == {ITEM}
    # pretrained: the review and word tables come frozen from the files, the user / item tables too until thawed
    emb = pretrain_rtm_util.write_dir(str(tmp_path / 'emb'), pretrain_util.vocab_words(V), RC, D, seed=7)
    up = pretrain_rtm_util.write_up_dir(str(tmp_path / 'up'), 30, 50, D, seed=9)
    p = _model(_args(review_encoder_name='pv', pretrain_emb_dir=emb, pretrain_up_emb_dir=up, use_user_emb=True,
                     use_item_emb=True), PretrainedProductRanker)
    assert p._row_sparse() and p._sparse_paths() == ()
    p.user_emb.weight.requires_grad_(True)
    assert p._sparse_paths() == (USER,)
    assert [r[0] for r in p._grad_layout()[0]][-1] == USER


def test_the_host_plumbing_is_the_base_class_own():
    for name in ('_coalesce_touched', '_rows_view', 'touched_rows', '_zero_for_backward', '_refuse_dirty_accumulation'):
        assert getattr(ProductRanker, name) is getattr(ItemTransformerRanker, name) is getattr(hot_module.HotPathModule, name)
    assert ProductRanker.check_index_errors is hot_module.HotPathModule.check_index_errors
    m = _model(_args(review_encoder_name='pvc', row_sparse_adam=False))
    assert m.check_index_errors() is None            # nothing to read without the flag (and no device needed)


# --------------------------------------------------------------------------------------------------- ps_coalesce_tables
@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


def _tab(t, n_lists=1, n=4, idx=0x1000, n_rows=100, cap=4, ws=None):
    for i in range(n_lists):
        t.lists[i].idx, t.lists[i].n = idx, n
    t.n_lists, t.n_rows, t.pad_row = n_lists, n_rows, n_rows - 1
    t.rows_out_dev, t.cap, t.count_out_dev = 0x3000, cap, 0x4000
    if ws is not None:
        t.ws_dev = ws


def test_coalesce_tables_struct_matches_the_header():
    assert C.sizeof(_lib.PsIdxList) == 16
    assert C.sizeof(_lib.PsCoalesceTable) == 8 * 16 + 8 + 6 * 8
    assert _lib.PsCoalesceTable.n_rows.offset == 136 and _lib.PsCoalesceTable.count_out_dev.offset == 176


def test_coalesce_tables_refuses_before_launching(lib):
    """Every refusal is an error code and a message; none of them touches the (made-up) device addresses."""
    def refused(tabs, n, match):
        rc = lib.ps_coalesce_tables(tabs, n, None)
        assert rc != 0
        msg = lib.ps_last_error().decode()
        assert 'coalesce_tables' in msg and match in msg, msg
    tabs = (_lib.PsCoalesceTable * 5)()
    for i, t in enumerate(tabs):
        _tab(t, ws=0x2000 + 0x1000 * i)
    refused(tabs, 0, '1..4 tables')
    refused(tabs, 5, '1..4 tables')
    refused(tabs, -1, '1..4 tables')
    refused(None, 1, '1..4 tables')
    _tab(tabs[1], idx=None)                                     # a null list with n > 0
    refused(tabs, 2, 'table 1: list 0 null')
    _tab(tabs[1])
    _tab(tabs[2], n_lists=2, n=4, cap=7)                         # cap below min(total, n_rows) = 8
    refused(tabs, 3, 'table 2: rows_out capacity 7 < 8')
    _tab(tabs[2], n_lists=2, n=400, n_rows=100, cap=99)          # ... = n_rows
    refused(tabs, 3, 'table 2: rows_out capacity 99 < 100')
    _tab(tabs[2])
    tabs[0].n_lists = 0
    refused(tabs, 1, 'table 0: 1..8 index lists')
    tabs[0].n_lists = 9
    refused(tabs, 1, 'table 0: 1..8 index lists')
    _tab(tabs[0], n_rows=0)
    refused(tabs, 1, 'table 0: bad argument')
    _tab(tabs[0])
    tabs[3].ws_dev = tabs[0].ws_dev                              # two tables on one bitmap
    refused(tabs, 4, 'tables 0 and 3 share a workspace')


# ------------------------------------------------------------------------------------------------------- data parallel
def test_data_parallel_wrappers_refuse_the_row_sparse_review_transformer():
    m = _model(_args(review_encoder_name='pv', use_user_emb=True))
    for call in (lambda: pdist.make_exchange(m), lambda: pdist.flatten_parameters(m),
                 lambda: pdist.SparseGradExchange(m, None, None)):
        with pytest.raises(NotImplementedError, match='data-parallel.*row_sparse_adam'):
            call()
    # with lazy_exact_adam the model is dense and passes this check (flatten_parameters then asks for the device)
    d = _model(_args(review_encoder_name='pv', use_user_emb=True, lazy_exact_adam=True))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pdist.flatten_parameters(d)
