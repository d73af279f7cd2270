"""CPU-only checks of the one-message row exchange (``dist.TablesGradExchange``, ``make_exchange(mode='tables')``): the wire
layout (``ps_row_msg_layout``), what ``ps_pack_tables`` / ``ps_union_tables`` / ``ps_merge_tables`` refuse before they launch
anything, the routing and refusals of ``make_exchange``, and the review transformer's message bound
(``ProductRanker._index_cap_bound``).  No GPU compute here."""
import ctypes as C
import types

import pytest
import torch

import pretrain_util
from prodsearch_amd import ProductRanker, _lib, default_args, dist as pdist, rtm_data, synth
from prodsearch_amd import build as pbuild

V, RC, D, U_SIZE, P_SIZE = 60, 40, 32, 30, 50
REVIEW, USER, ITEM, WORD = ('review_emb',), ('user_emb',), ('product_emb',), ('word_emb',)


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


def _args(**kw):
    base = dict(model_name='review_transformer', embedding_size=D, heads=4, ff_size=64, inter_layers=1, neg_per_pos=2,
                review_word_limit=8, do_subsample_mask=True, row_sparse_adam=True, review_encoder_name='pv',
                use_user_emb=True, use_item_emb=True)
    base.update(kw)
    return default_args(**base)


def _review_words():
    rng = synth.rng_for(3)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, 8)))
    rw[-1] = V - 1
    return rw


def _model(a):
    torch.manual_seed(0)
    return ProductRanker(a, 'cpu', V, RC, P_SIZE, U_SIZE, _review_words(), pretrain_util.vocab_words(V))


# ---------------------------------------------------------------------------------------------------------- the layout
def test_layout_of_the_hand_computed_case(lib):
    """caps (5, 64, 1, 130), widths (128, 8, 128, 4).  Id sections: 40 B -> 48, 512, 8 -> 16, 1040; value sections:
    5*128*4 = 2560, 64*8*4 = 2048, 512, 130*4*4 = 2080."""
    ids, vals, total = pdist.row_msg_layout([5, 64, 1, 130], [128, 8, 128, 4])
    assert ids == [0, 48, 560, 576]
    assert vals == [1616, 4176, 6224, 6736]
    assert total == 8816 and total % 16 == 0


@pytest.mark.parametrize('caps,ds', [([1], [4]), ([7], [12]), ([3, 3], [4, 8]), ([5, 64, 1, 130], [128, 8, 128, 4]),
                                     ([1, 1, 1, 1], [4, 4, 4, 4]), ([1000001, 2], [256, 128])])
def test_layout_sections_are_aligned_and_disjoint(lib, caps, ds):
    ids, vals, total = pdist.row_msg_layout(caps, ds)
    spans = [(o, o + 8 * c) for o, c in zip(ids, caps)] + [(o, o + 4 * c * d) for o, c, d in zip(vals, caps, ds)]
    assert all(lo % 16 == 0 for lo, _ in spans) and total % 16 == 0
    assert spans == sorted(spans)                                          # ids of every table first, then the values
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi <= lo < hi + 16                                          # no overlap, no gap beyond the rounding
    assert spans[0][0] == 0 and spans[-1][1] == total


def test_layout_refuses_bad_arguments(lib):
    def refused(caps, ds, n, match):
        ca = None if caps is None else (C.c_int64 * 8)(*caps)
        da = None if ds is None else (C.c_int32 * 8)(*ds)
        assert lib.ps_row_msg_layout(ca, da, n, None, None) == -1
        msg = lib.ps_last_error().decode()
        assert 'row_msg_layout' in msg and match in msg, msg
    refused(None, [4], 1, 'null argument')
    refused([4], None, 1, 'null argument')
    refused([4], [4], 0, '1..4 tables (0 given)')
    refused([4] * 5, [4] * 5, 5, '1..4 tables (5 given)')
    refused([4, 0], [4, 4], 2, 'table 1: capacity 0')
    refused([4, 1 << 31], [4, 4], 2, 'table 1: capacity 2147483648')
    refused([4, 4, 4], [4, 4, 6], 3, 'table 2: width 6')
    refused([4], [0], 1, 'table 0: width 0')
    with pytest.raises(RuntimeError, match='row_msg_layout'):
        pdist.row_msg_layout([0], [4])


# ------------------------------------------------------------------------------------------ refusals of the three entries
def _tabs(n=4, caps=(5, 64, 1, 130), ds=(128, 8, 128, 4)):
    """Well-formed tables over made-up device addresses: every call below fails one check and launches nothing."""
    tabs = (_lib.PsRowMsgTable * 5)()
    for i in range(5):
        t = tabs[i]
        t.cap, t.d, t.n_rows = caps[i % 4], ds[i % 4], 5000
        t.grad_dev, t.rows_dev, t.count_dev, t.list_cap = 0x10000 * (i + 1), 0x20000 * (i + 1), 0x30000 * (i + 1), caps[i % 4]
        t.ws_dev, t.union_rows_dev, t.union_cap, t.union_count_dev = 0x40000 * (i + 1), 0x50000 * (i + 1), 8, 0x60000 * (i + 1)
    _, _, nbytes = pdist.row_msg_layout(list(caps[:n]), list(ds[:n]))
    return tabs, nbytes


def test_row_msg_struct_matches_the_header():
    assert C.sizeof(_lib.PsRowMsgTable) == 11 * 8
    assert _lib.PsRowMsgTable.n_rows.offset == 16 and _lib.PsRowMsgTable.union_count_dev.offset == 80


def _calls(lib):
    return {'pack_tables': lambda tabs, n, buf, nbytes, world: lib.ps_pack_tables(tabs, n, buf, nbytes, None),
            'union_tables': lambda tabs, n, buf, nbytes, world: lib.ps_union_tables(tabs, n, buf, nbytes, world, None),
            'merge_tables': lambda tabs, n, buf, nbytes, world: lib.ps_merge_tables(tabs, n, buf, nbytes, world, None)}


@pytest.mark.parametrize('who', ['pack_tables', 'union_tables', 'merge_tables'])
def test_the_shared_checks_of_the_three_entries(lib, who):
    call = _calls(lib)[who]

    def refused(tabs, n, buf, nbytes, match, world=2):
        assert call(tabs, n, buf, nbytes, world) != 0
        msg = lib.ps_last_error().decode()
        assert msg.startswith(who + ':') and match in msg, msg
    tabs, nbytes = _tabs()
    refused(None, 4, 0x1000, nbytes, '1..4 tables')
    refused(tabs, 0, 0x1000, nbytes, '1..4 tables (0 given)')
    refused(tabs, 5, 0x1000, nbytes, '1..4 tables (5 given)')
    refused(tabs, 4, None, nbytes, 'null message buffer')
    refused(tabs, 4, 0x1008, nbytes, 'message buffer not 16-byte aligned')
    refused(tabs, 4, 0x1000, nbytes + 16, 'msg_bytes %d, the tables\' layout has %d' % (nbytes + 16, nbytes))
    refused(tabs, 3, 0x1000, nbytes, 'msg_bytes')                        # the layout of three tables is another one
    tabs[2].cap = 0
    refused(tabs, 4, 0x1000, nbytes, 'table 2: capacity 0')
    tabs[2].cap = 1 << 31
    refused(tabs, 4, 0x1000, nbytes, 'table 2: capacity 2147483648')
    tabs, nbytes = _tabs()
    tabs[1].d = 6
    refused(tabs, 4, 0x1000, nbytes, 'table 1: width 6')
    tabs[1].d = 0
    refused(tabs, 4, 0x1000, nbytes, 'table 1: width 0')
    if who != 'pack_tables':
        tabs, nbytes = _tabs()
        for world in (0, -1, 33):
            refused(tabs, 4, 0x1000, nbytes, 'world %d (1..32)' % world, world=world)


def test_pack_tables_refuses_before_launching(lib):
    def refused(tabs, match, n=4):
        assert lib.ps_pack_tables(tabs, n, 0x1000, nbytes, None) != 0
        msg = lib.ps_last_error().decode()
        assert msg.startswith('pack_tables:') and match in msg, msg
    for field in ('grad_dev', 'rows_dev', 'count_dev'):
        tabs, nbytes = _tabs()
        setattr(tabs[3], field, None)
        refused(tabs, 'table 3: null pointer')
    tabs, nbytes = _tabs()
    tabs[1].grad_dev = 0x10008
    refused(tabs, 'table 1: gradient not 16-byte aligned')
    tabs, nbytes = _tabs()
    tabs[0].n_rows = 0
    refused(tabs, 'table 0: n_rows 0')
    tabs, nbytes = _tabs()
    tabs[2].list_cap = 0
    refused(tabs, 'table 2: list capacity 0, message capacity 1')
    tabs[2].list_cap = 2                                                 # a touched list longer than the message
    refused(tabs, 'table 2: list capacity 2, message capacity 1')


def test_union_tables_refuses_before_launching(lib):
    def refused(tabs, match, n=4, world=2, nb=None):
        assert lib.ps_union_tables(tabs, n, 0x1000, nbytes if nb is None else nb, world, None) != 0
        msg = lib.ps_last_error().decode()
        assert msg.startswith('union_tables:') and match in msg, msg
    for field in ('ws_dev', 'union_rows_dev', 'union_count_dev'):
        tabs, nbytes = _tabs()
        setattr(tabs[2], field, None)
        refused(tabs, 'table 2: null pointer')
    tabs, nbytes = _tabs()
    tabs[1].n_rows = 0
    refused(tabs, 'table 1: n_rows 0')
    tabs[1].n_rows = 1 << 37
    refused(tabs, 'table 1: n_rows %d' % (1 << 37))
    tabs, nbytes = _tabs()
    tabs[3].union_cap = 0
    refused(tabs, 'table 3: union capacity 0')
    tabs, nbytes = _tabs()
    tabs[3].ws_dev = tabs[1].ws_dev                                      # two tables on one bitmap
    refused(tabs, 'tables 1 and 3 share a workspace')
    tabs, nb = _tabs(1, caps=(1 << 30, 64, 1, 130))                      # 2^30 slots a rank: world 2 is 2^31
    refused(tabs, 'table 0: too many id slots', n=1, world=2, nb=nb)


def test_merge_tables_refuses_before_launching(lib):
    def refused(tabs, match, n=4):
        assert lib.ps_merge_tables(tabs, n, 0x1000, nbytes, 2, None) != 0
        msg = lib.ps_last_error().decode()
        assert msg.startswith('merge_tables:') and match in msg, msg
    for field in ('grad_dev', 'union_rows_dev', 'union_count_dev'):
        tabs, nbytes = _tabs()
        setattr(tabs[0], field, None)
        refused(tabs, 'table 0: null pointer')
    tabs, nbytes = _tabs()
    tabs[2].grad_dev = 0x30004
    refused(tabs, 'table 2: gradient not 16-byte aligned')
    tabs, nbytes = _tabs()
    tabs[1].union_cap = -3
    refused(tabs, 'table 1: union capacity -3')
    tabs[1].union_cap = 1 << 40
    refused(tabs, 'grid too large')


# ------------------------------------------------------------------------------------------------------------- routing
def test_tables_mode_refuses_a_model_that_is_not_row_sparse(monkeypatch):
    m = _model(_args(row_sparse_adam=False))
    with pytest.raises(NotImplementedError, match='not row-sparse'):
        pdist.make_exchange(m, None, None, mode='tables')
    monkeypatch.setenv('PS_DP_EXCHANGE', 'tables')                       # the environment's spelling of the same request
    with pytest.raises(NotImplementedError, match='not row-sparse'):
        pdist.make_exchange(m)
    with pytest.raises(NotImplementedError, match='not row-sparse'):
        pdist.TablesGradExchange(m)


def test_tables_mode_refuses_lazy_exact_adam_and_shard_tables():
    with pytest.raises(NotImplementedError, match="mode='tables'.*lazy_exact_adam"):
        pdist.make_exchange(_model(_args(lazy_exact_adam=True)), None, None, mode='tables')
    with pytest.raises(NotImplementedError, match="mode='tables'.*shard_tables"):
        pdist.make_exchange(_model(_args(shard_tables=True)), None, None, mode='tables')


@pytest.mark.parametrize('name', ['word_emb', 'review_emb', 'user_emb', 'product_emb'])
def test_tables_mode_refuses_a_frozen_table(name):
    m = _model(_args())
    m._hot_tables()[name].requires_grad_(False)
    with pytest.raises(NotImplementedError, match='data-parallel training with a frozen'):
        pdist.make_exchange(m, None, None, mode='tables')


def test_tables_mode_builds_for_the_row_sparse_review_transformer_and_the_default_still_refuses_it():
    m = _model(_args())
    x = pdist.make_exchange(m, None, None, mode='tables')
    assert isinstance(x, pdist.TablesGradExchange) and x.world == 1 and x() is None      # one process: nothing to exchange
    opt = types.SimpleNamespace(grad_scale=None)
    pdist.TablesGradExchange(m, opt)
    assert opt.grad_scale == 1.0
    for call in (lambda: pdist.make_exchange(m), lambda: pdist.make_exchange(m, None, None, mode='sharded'),
                 lambda: pdist.flatten_parameters(m), lambda: pdist.SparseGradExchange(m, None, None)):
        with pytest.raises(NotImplementedError, match="data-parallel.*row_sparse_adam.*mode='tables'"):
            call()


def test_a_step_beyond_the_agreed_capacity_raises_before_any_collective():
    """No process group exists here: entering a collective would fail in torch.distributed, with another error."""
    m = _model(_args())
    x = pdist.TablesGradExchange(m)
    p = m.user_emb.weight
    p._ps_rows = dict(cap=9)
    m.__dict__['_sparse_tabs'] = [(USER, p, None)]
    x.world, x._caps = 2, [8]
    with pytest.raises(RuntimeError, match='addresses up to 9 rows of user_emb but the ranks agreed on messages of 8 rows'):
        x()


# ---------------------------------------------------------------------------------------------------- _index_cap_bound
def _lists_plan(m, batch, train_pv, K):
    """What ``_run_forward`` leaves for ``_index_lists``: the batch's index tensors by name (the PV draws are one per
    window word and negative)."""
    lists = {k: getattr(batch, k) for k in ('query_word_idxs', 'pos_prod_ridxs', 'neg_prod_ridxs', 'pos_prod_rword_idxs',
                                            'pos_user_idxs', 'neg_user_idxs', 'pos_item_idxs', 'neg_item_idxs')}
    lists['neg_word_idxs'] = torch.empty(batch.pos_prod_rword_idxs.numel() * K, dtype=torch.int64) if train_pv else None
    return types.SimpleNamespace(lists=lists, desc=types.SimpleNamespace(train_pv=int(train_pv)))


@pytest.mark.parametrize('train_pv', [True, False])
def test_index_cap_bound_holds_and_is_tight(train_pv):
    B, K, UL, IL, W, Q = 6, 2, 3, 4, 2, 7
    a = _args(batch_size=B, neg_per_pos=K, uprev_review_limit=UL, iprev_review_limit=IL, pv_window_size=W, max_query_len=Q)
    m = _model(a)
    R = UL + IL
    assert m._index_cap_bound(REVIEW) == B * (1 + K) * R
    assert m._index_cap_bound(USER) == m._index_cap_bound(ITEM) == B * (1 + K) * (R + 1)
    assert m._index_cap_bound(WORD) == B * Q + B * R * W * (1 + K)
    rw = _review_words()
    for u_lim, i_lim, q, b in ((UL, IL, Q, B), (UL - 1, IL, Q, B), (UL, IL - 2, Q - 3, B), (1, 1, 2, B - 1)):
        batch = rtm_data.make_rtm_batch(5, b, K, RC, V, rw, Q=q, u_lim=u_lim, i_lim=i_lim, W=W, train_pv=train_pv,
                                        encoder='pv', user_size=U_SIZE, product_size=P_SIZE)
        plan = _lists_plan(m, batch, train_pv, K)
        full = (u_lim, i_lim, q, b) == (UL, IL, Q, B)
        for path in m._sparse_paths():
            lists, _ = m._index_lists(path, plan)
            total = sum(t.numel() for t in lists)
            bound = m._index_cap_bound(path)
            assert total <= bound, (path, total, bound)
            if full and (path != WORD or train_pv):                      # every width at its limit: the bound is met
                assert total == bound, (path, total, bound)
            if not full:
                assert total < bound
    assert set(m._sparse_paths()) == {REVIEW, USER, ITEM, WORD}


def test_index_cap_bound_without_a_query_length_is_the_word_table():
    m = _model(_args(batch_size=6))
    assert m.args.max_query_len is None
    assert m._index_cap_bound(WORD) == m.word_embeddings.weight.shape[0]
