"""Review transformer on pretrained / fixed paragraph vectors (``pretrain_emb_dir``, ``pretrain_up_emb_dir``, ``fix_emb``) on the
host: the loaders and table mappings against the reference's own fixtures (tests/golden/rtmpre_*.npz,
make_golden_rtm_pretrained.py), the model boundary (class dispatch, requires_grad, state_dict, optimizer parameter list,
refusals), the host-only backward plan (``ps_rtm_backward_plan``) against a table written out here, and the test-side oracle
with frozen leaves.  No GPU compute is called here."""
import gzip
import itertools
import os
import types

import numpy as np
import pytest
import torch

import pretrain_rtm_util
import pretrain_util
from golden_util import rel_err
from golden_util_rtmpre import PRODUCT_SIZE, REVIEW_TABLE, RTMPRE_CASES, USER_SIZE, RtmPreGolden
from oracle import optim as ooptim
from oracle import rtm as ortm
from prodsearch_amd import PretrainedProductRanker, ProductRanker, _lib, build_optim, default_args, pretrained, synth

V, RC, D = 60, 40, 32


def _args(**kw):
    base = dict(model_name='review_transformer', embedding_size=D, heads=4, ff_size=64, inter_layers=1, neg_per_pos=2,
                review_word_limit=8, do_subsample_mask=True)
    base.update(kw)
    return default_args(**base)


def _review_words():
    rng = synth.rng_for(3)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, 8)))
    rw[-1] = V - 1
    return rw


def _model(a, cls=PretrainedProductRanker, user=30, prod=50):
    torch.manual_seed(0)
    return cls(a, 'cpu', V, RC, prod, user, _review_words(), pretrain_util.vocab_words(V))


@pytest.fixture(scope='module')
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp('rtmpre_small')
    emb = pretrain_rtm_util.write_dir(str(root / 'emb'), pretrain_util.vocab_words(V), RC, D, seed=7)
    up = pretrain_rtm_util.write_up_dir(str(root / 'up'), 30, 50, D, seed=9)
    return emb, up


# ------------------------------------------------------------------------------------------------ fixtures of the reference
def test_fixture_set_is_complete():
    assert set(RTMPRE_CASES) == {'rtmpre_pvc', 'rtmpre_pvc_pv_drop', 'rtmpre_pv_drop', 'rtmpre_fs', 'rtmpre_fix_pvc',
                                 'rtmpre_fix_pv', 'rtmpre_ui'}
    largest = max(os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', f))
                  for f in os.listdir(os.path.join(os.path.dirname(__file__), 'golden')) if f.startswith('rtm_'))
    for c in RTMPRE_CASES:
        g = RtmPreGolden(c)
        assert g.args.embedding_size == 32 and g.V <= 200 and g.B <= 16
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', c + '.npz')) < min(largest, 1 << 20)


@pytest.mark.parametrize('case', RTMPRE_CASES)
def test_tables_keys_and_optimizer_are_the_references(case):
    g = RtmPreGolden(case)
    m = g.build()
    named = dict(m.named_parameters())
    assert list(m.state_dict().keys()) == g.meta['state_dict_keys']
    assert list(named) == g.meta['param_names']
    for n in g.meta['pretrained']:
        assert torch.equal(named[n].detach(), torch.from_numpy(g.z['table_' + n])), n       # bitwise
    assert [n for n, p in named.items() if not p.requires_grad] == g.meta['frozen']
    opt = build_optim(g.args, m, None)
    assert opt._names == g.meta['optim_params']
    assert not any(n in opt._names for n in g.meta['frozen'])
    assert m.review_encoder_name == g.meta['encoder']
    if g.args.fix_emb:
        # the table test() reads is the frozen parameter from construction on, and clearing is a no-op (ps_model.py:163-182)
        assert m.review_embeddings is m.review_encoder.review_embeddings.weight
        m.clear_review_embbeddings()
        assert m.review_embeddings is m.review_encoder.review_embeddings.weight
    else:
        assert m.review_embeddings is None
    if g.meta['encoder'] == 'pvc':
        assert m.review_encoder.context_embeddings is m.word_embeddings
    # initialize_parameters leaves pretrained tables alone and re-draws the others
    before = {n: p.detach().clone() for n, p in named.items()}
    m.initialize_parameters()
    for n in g.meta['pretrained']:
        assert torch.equal(named[n].detach(), before[n]), n
    if 'word_embeddings.weight' not in g.meta['pretrained']:
        assert not torch.equal(named['word_embeddings.weight'].detach(), before['word_embeddings.weight'])


# ------------------------------------------------------------------------------------------------ loaders
def test_word_file_follows_the_argument_and_the_mapping_rules(dirs):
    emb, _ = dirs
    words = pretrain_util.vocab_words(V)
    for enc, fname in (('pvc', 'context_emb.txt.gz'), ('pv', 'word_emb.txt.gz'), ('fs', 'word_emb.txt.gz'),
                       ('avg', 'word_emb.txt.gz')):
        m = _model(_args(review_encoder_name=enc, pretrain_emb_dir=emb))
        keys, rows = pretrained.load_pretrain_embeddings(os.path.join(emb, fname))
        tab = m.word_embeddings.weight.detach().numpy()
        assert not m.word_embeddings.weight.requires_grad
        assert np.array_equal(tab[0], rows[0])                                       # row 0 is file row 0
        for i in (1, 7, V - 2):
            assert np.array_equal(tab[i], rows[keys[words[i]]]), (enc, i)            # words 1.. by key
        assert np.array_equal(tab[V - 1], rows[len(words)]) and float(np.abs(tab[V - 1]).min()) > 1.0    # pad row: not zeroed
        assert np.array_equal(tab, pretrained.word_table(emb, words, V, D, fname))
        if enc in ('fs', 'avg'):
            assert all(p.requires_grad for n, p in m.named_parameters() if n != 'word_embeddings.weight')
    # fix_emb renames pvc -> pv AFTER the file was chosen on the argument: context_emb, and the review table from doc_emb
    m = _model(_args(review_encoder_name='pvc', pretrain_emb_dir=emb, fix_emb=True))
    assert m.review_encoder_name == 'pv'
    assert np.array_equal(m.word_embeddings.weight.detach().numpy(), pretrained.word_table(emb, words, V, D, 'context_emb.txt.gz'))
    assert np.array_equal(m.review_encoder.review_embeddings.weight.detach().numpy(), pretrained.review_table(emb, RC, D))


def test_review_and_user_item_tables(dirs):
    emb, up = dirs
    _, rows = pretrained.load_pretrain_embeddings(os.path.join(emb, 'doc_emb.txt.gz'))
    tab = pretrained.review_table(emb, RC, D)
    assert tab.dtype == np.float32 and tab.shape == (RC, D)
    assert np.array_equal(tab[:-1], rows) and not tab[-1].any()                      # file order + one zero row
    m = _model(_args(review_encoder_name='pv', pretrain_emb_dir=emb))
    w = m.review_encoder.review_embeddings.weight
    assert np.array_equal(w.detach().numpy(), tab) and not w.requires_grad           # frozen without fix_emb
    for fname, n in (('user_emb.txt', 30), ('product_emb.txt', 50)):
        with open(os.path.join(up, fname)) as f:
            f.readline(), f.readline()
            want = np.array([[float(x) for x in ln.split()] for ln in f], dtype=np.float64).astype(np.float32)
        got = pretrained.user_item_table(os.path.join(up, fname), n + 1, D)
        assert got.shape == (n + 1, D) and np.array_equal(got[:-1], want) and not got[-1].any()
    a = _args(review_encoder_name='pv', pretrain_up_emb_dir=up, use_user_emb=True, use_item_emb=True)
    m = _model(a)
    assert not m.user_emb.weight.requires_grad and not m.product_emb.weight.requires_grad
    assert m.user_emb.padding_idx == 30 and m.product_emb.padding_idx == 50
    assert m.word_embeddings.weight.requires_grad and m.review_encoder.review_embeddings.weight.requires_grad
    # read only when the switch is on
    m = _model(_args(review_encoder_name='pv', pretrain_up_emb_dir=up, use_user_emb=True))
    assert not hasattr(m, 'product_emb') and not m.user_emb.weight.requires_grad


def test_all_loaders_parse_through_double(dirs):
    """The files hold decimals just above a float32 rounding midpoint: double-then-float32 rounds them down."""
    from test_pretrained_cpu import _direct_f32
    emb, up = dirs
    with gzip.open(os.path.join(emb, 'doc_emb.txt.gz'), 'rt') as f:
        f.readline(), f.readline()
        lines = [ln.split('\t')[1].split() for ln in f.read().splitlines()]
    tab = pretrained.review_table(emb, RC, D)[:-1]
    direct = np.array([[_direct_f32(x) for x in ln] for ln in lines], dtype=np.float32)
    assert 0.05 < float((tab != direct).mean()) < 0.3
    with open(os.path.join(up, 'user_emb.txt')) as f:
        f.readline(), f.readline()
        lines = [ln.split() for ln in f.read().splitlines()]
    tab = pretrained.user_item_table(os.path.join(up, 'user_emb.txt'), 31, D)[:-1]
    direct = np.array([[_direct_f32(x) for x in ln] for ln in lines], dtype=np.float32)
    assert 0.05 < float((tab != direct).mean()) < 0.3


def test_error_paths(tmp_path):
    words = pretrain_util.vocab_words(V)
    d = str(tmp_path)
    # word table: wrong width, a short file, a missing word, no vocabulary
    pretrain_util.write_word_emb(os.path.join(d, 'context_emb.txt.gz'), words, D, width=D + 1)
    with pytest.raises(ValueError, match='wide'):
        pretrained.word_table(d, words, V, D, 'context_emb.txt.gz')
    pretrain_util.write_word_emb(os.path.join(d, 'context_emb.txt.gz'), words, D, n_rows=V - 5)
    with pytest.raises((KeyError, IndexError)):
        pretrained.word_table(d, words, V, D, 'context_emb.txt.gz')
    pretrain_util.write_word_emb(os.path.join(d, 'context_emb.txt.gz'), words[:-3], D, n_extra=40)
    with pytest.raises(KeyError, match='no row for the vocabulary word'):
        pretrained.word_table(d, words, V, D, 'context_emb.txt.gz')
    with pytest.raises(ValueError, match='vocab_words'):
        pretrained.word_table(d, None, V, D, 'context_emb.txt.gz')
    with pytest.raises(FileNotFoundError):
        pretrained.word_table(d, words, V, D)                                       # word_emb.txt.gz is not there
    # review table: wrong width, wrong row count (review_count must be rows + 1), both directions
    pretrain_rtm_util.write_doc_emb(os.path.join(d, 'doc_emb.txt.gz'), RC - 1, D, width=D - 1)
    with pytest.raises(ValueError, match='wide'):
        pretrained.review_table(d, RC, D)
    pretrain_rtm_util.write_doc_emb(os.path.join(d, 'doc_emb.txt.gz'), RC - 2, D)
    with pytest.raises(ValueError, match='review_count'):
        pretrained.review_table(d, RC, D)
    pretrain_rtm_util.write_doc_emb(os.path.join(d, 'doc_emb.txt.gz'), RC, D)
    with pytest.raises(ValueError, match='review_count'):
        pretrained.review_table(d, RC, D)
    with pytest.raises(ValueError, match='review_count'):
        pretrain_util.write_word_emb(os.path.join(d, 'word_emb.txt.gz'), words, D)
        _model(_args(review_encoder_name='pv', pretrain_emb_dir=d))
    # user / item tables: wrong width, short file, ragged row
    p = os.path.join(d, 'user_emb.txt')
    pretrain_rtm_util.write_user_item_emb(p, 30, D, width=D + 2)
    with pytest.raises(ValueError, match='wide'):
        pretrained.user_item_table(p, 31, D)
    pretrain_rtm_util.write_user_item_emb(p, 29, D)
    with pytest.raises(ValueError, match='rows'):
        pretrained.user_item_table(p, 31, D)
    with open(p, 'w') as f:
        f.write('2\n3\n0.1 0.2 0.3\n0.1 0.2\n')
    with pytest.raises(ValueError, match='values'):
        pretrained.user_item_table(p, 3, 3)
    with open(p, 'w') as f:
        f.write('0\n3\n')
    with pytest.raises(ValueError, match='no embedding rows'):
        pretrained.user_item_table(p, 1, 3)


# ------------------------------------------------------------------------------------------------ the model boundary
def test_missing_directories_are_ignored(tmp_path):
    a = _args(review_encoder_name='pv', pretrain_emb_dir=str(tmp_path / 'nope'), pretrain_up_emb_dir=str(tmp_path / 'nope2'),
              use_user_emb=True)
    m = _model(a)
    assert m.pretrain_emb_dir is None and m.pretrain_up_emb_dir is None
    assert all(p.requires_grad for p in m.parameters())
    assert m._frozen_mask() == 0


def _global_data():
    return types.SimpleNamespace(vocab_size=V, review_count=RC, product_size=50, user_size=30, review_words=_review_words(),
                                 words=pretrain_util.vocab_words(V))


def test_create_model_dispatches(dirs, tmp_path):
    from prodsearch_amd import trainer
    emb, up = dirs
    pd = types.SimpleNamespace(word_dists=None)
    for kw, cls in ((dict(), ProductRanker), (dict(pretrain_emb_dir=str(tmp_path / 'missing')), ProductRanker),
                    (dict(pretrain_emb_dir=emb), PretrainedProductRanker), (dict(fix_emb=True), PretrainedProductRanker),
                    (dict(pretrain_up_emb_dir=up, use_user_emb=True), PretrainedProductRanker)):
        a = _args(review_encoder_name='pv', **kw)
        a.device = 'cpu'
        model, optim = trainer.create_model(a, _global_data(), pd)
        assert type(model) is cls, kw
        assert optim._names == [n for n, p in model.named_parameters() if p.requires_grad]


def test_refusals(dirs):
    emb, up = dirs
    for kw in (dict(pretrain_emb_dir=emb), dict(pretrain_up_emb_dir=up), dict(fix_emb=True)):
        with pytest.raises(NotImplementedError, match='PretrainedProductRanker'):
            _model(_args(review_encoder_name='pv', **kw), cls=ProductRanker)
    for enc in ('fs', 'avg'):
        with pytest.raises(NotImplementedError, match='fix_emb'):
            _model(_args(review_encoder_name=enc, fix_emb=True))
        with pytest.raises(NotImplementedError, match='fix_emb'):
            _model(_args(review_encoder_name=enc, fix_emb=True, pretrain_emb_dir=emb))


def test_fix_emb_alone_freezes_the_review_table_only():
    m = _model(_args(review_encoder_name='pv', fix_emb=True))
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ['review_embeddings']
    assert m.word_embeddings.weight.requires_grad
    assert m._frozen_mask() == _lib.PS_RTM_FROZEN_REVIEW
    assert m._desc(2, 2, 3, False).no_pv_drop == 1 and m._desc(2, 2, 3, False).frozen_mask == _lib.PS_RTM_FROZEN_REVIEW
    # an argument of pvc: the pv encoder's keys
    m2 = _model(_args(review_encoder_name='pvc', fix_emb=True))
    assert list(m2.state_dict().keys()) == list(m.state_dict().keys())
    assert 'review_encoder.review_embeddings.weight' in m2.state_dict()


def test_frozen_mask_follows_requires_grad(dirs):
    emb, up = dirs
    m = _model(_args(review_encoder_name='pv', pretrain_emb_dir=emb, pretrain_up_emb_dir=up, use_user_emb=True, use_item_emb=True))
    assert m._frozen_mask() == 15
    m.user_emb.weight.requires_grad_(True)
    assert m._frozen_mask() == 15 - _lib.PS_RTM_FROZEN_USER
    assert m._has_grad(('user_emb',)) and not m._has_grad(('product_emb',)) and not m._has_grad(('word_emb',))
    m = _model(_args(review_encoder_name='pvc'), cls=ProductRanker)
    assert m._frozen_mask() == 0
    m.word_embeddings.weight.requires_grad_(False)                                  # a caller's own freeze counts too
    assert m._frozen_mask() == _lib.PS_RTM_FROZEN_WORD


def test_data_parallel_wrappers_refuse(dirs):
    from prodsearch_amd import dist
    emb, up = dirs
    for kw in (dict(review_encoder_name='pvc', pretrain_emb_dir=emb), dict(review_encoder_name='pv', fix_emb=True),
               dict(review_encoder_name='pv', pretrain_up_emb_dir=up, use_item_emb=True)):
        m = _model(_args(**kw))
        with pytest.raises(NotImplementedError, match='data-parallel'):
            dist.make_exchange(m)
        with pytest.raises(NotImplementedError, match='data-parallel'):
            dist.SparseGradExchange(m)
        with pytest.raises(NotImplementedError, match='data-parallel'):
            dist.flatten_parameters(m)


# ------------------------------------------------------------------------------------------------ the backward plan
FINAL_LN_BIAS = 'transformer_encoder.layer_norm.bias'
W_, R_, U_, I_ = _lib.PS_RTM_FROZEN_WORD, _lib.PS_RTM_FROZEN_REVIEW, _lib.PS_RTM_FROZEN_USER, _lib.PS_RTM_FROZEN_ITEM
NONE, HIST = _lib.PS_RTM_INDEX_NONE, _lib.PS_RTM_INDEX_HIST
GENERAL, PLAIN, FROZEN = _lib.PS_RTM_EB_GENERAL, _lib.PS_RTM_EB_PLAIN, _lib.PS_RTM_EB_FROZEN
PLAN_FIELDS = ('index', 'word_reduce', 'slot_rows', 'review_scatter', 'pv_bwd', 'pv_bwd_kernel', 'fs_draw', 'query_scatter',
               'embed_form', 'slot_waves', 'side_fork')
#            (encoder, frozen, train_pv, det): index wreduce slot_rows rev_scatter pv_bwd pv_kernel fs_draw q_scatter form waves fork
PLAN_TABLE = {
    ('pvc', 0, 0, 0): (HIST, 1, 1, 0, 0, 0, 0, 1, PLAIN, 1, 1),
    ('pvc', 0, 1, 0): (HIST, 1, 1, 0, 3, 1, 0, 1, GENERAL, 1, 1),
    ('pvc', 0, 0, 1): (HIST, 1, 1, 0, 0, 0, 0, 1, PLAIN, 1, 1),
    ('pvc', 0, 1, 1): (HIST, 1, 1, 0, 3, 1, 0, 1, GENERAL, 1, 1),
    ('pvc', W_, 0, 0): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pvc', W_, 1, 0): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pvc', W_, 0, 1): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pvc', W_, 1, 1): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('avg', 0, 0, 0): (HIST, 1, 1, 0, 0, 0, 0, 1, PLAIN, 1, 1),
    ('avg', 0, 0, 1): (HIST, 1, 1, 0, 0, 0, 0, 1, PLAIN, 1, 1),
    ('avg', W_, 0, 0): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('avg', W_, 0, 1): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('fs', 0, 0, 0): (HIST, 1, 1, 0, 0, 0, 1, 1, GENERAL, 1, 1),
    ('fs', 0, 0, 1): (HIST, 1, 1, 0, 0, 0, 1, 1, GENERAL, 1, 1),
    ('fs', W_, 0, 0): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('fs', W_, 0, 1): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pv', 0, 0, 0): (NONE, 0, 0, 1, 0, 0, 0, 1, GENERAL, 1, 0),
    ('pv', 0, 1, 0): (NONE, 0, 0, 1, 3, 1, 0, 1, GENERAL, 1, 0),
    ('pv', 0, 0, 1): (NONE, 0, 1, 1, 0, 0, 0, 1, GENERAL, 1, 0),
    ('pv', 0, 1, 1): (NONE, 0, 1, 1, 3, 1, 0, 1, GENERAL, 1, 0),
    ('pv', W_, 0, 0): (NONE, 0, 0, 1, 0, 0, 0, 0, GENERAL, 1, 0),
    ('pv', W_, 0, 1): (NONE, 0, 1, 1, 0, 0, 0, 0, GENERAL, 1, 0),          # deterministic + trainable reviews: rows parked
    ('pv', W_, 1, 0): (NONE, 0, 0, 1, 1, 1, 0, 0, GENERAL, 1, 0),          # d vec only
    ('pv', W_, 1, 1): (NONE, 0, 1, 1, 1, 1, 0, 0, GENERAL, 1, 0),
    ('pv', R_, 0, 0): (NONE, 0, 0, 0, 0, 0, 0, 1, FROZEN, 1, 0),
    ('pv', R_, 0, 1): (NONE, 0, 0, 0, 0, 0, 0, 1, FROZEN, 1, 0),
    ('pv', R_, 1, 0): (NONE, 0, 0, 0, 2, 1, 0, 1, FROZEN, 1, 0),           # word rows only
    ('pv', R_, 1, 1): (NONE, 0, 0, 0, 2, 0, 0, 1, FROZEN, 1, 0),           # ... deterministic: the keys + sole-owner scatter alone
    ('pv', W_ | R_, 0, 0): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pv', W_ | R_, 0, 1): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pv', W_ | R_, 1, 0): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
    ('pv', W_ | R_, 1, 1): (NONE, 0, 0, 0, 0, 0, 0, 0, FROZEN, 1, 0),
}
ENC_ID = dict(pv=_lib.PS_RENC_PV, pvc=_lib.PS_RENC_PVC, fs=_lib.PS_RENC_FS, avg=_lib.PS_RENC_AVG)


def _plan_desc(enc, frozen, train_pv, **over):
    d = _lib.PsRtmDesc()
    d.B, d.K, d.R, d.Q, d.W, d.WL, d.C = 8, 3, 7, 5, 2, 20, 0
    d.d, d.H, d.F, d.n_layers = 128, 8, 256, 1
    d.vocab_size, d.review_count = 1000, 500
    d.review_encoder, d.query_encoder = ENC_ID[enc], _lib.PS_QENC_FS
    d.use_pos_emb, d.use_seg_emb, d.train_pv, d.training = 1, 1, train_pv, 1
    d.dropout, d.corrupt_rate = 0.1, 0.9
    d.user_size, d.product_size = 30, 50
    d.frozen_mask = frozen
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _plan(d):
    import ctypes as C
    lib = _lib.load()
    out = _lib.PsRtmBwdPlan()
    _lib.check(lib.ps_rtm_backward_plan(C.byref(d), C.byref(out)), 'ps_rtm_backward_plan')
    return out


@pytest.fixture
def det_switch():
    lib = _lib.load()
    prev = lib.ps_set_deterministic(0)
    yield lib
    lib.ps_set_deterministic(prev)


def test_backward_plan_equals_the_table(det_switch):
    """Host only: no device is touched.  Every encoder x frozen mask x train_pv x deterministic cell that exists (fs / avg have
    no PV loss and no review table)."""
    cells = set()
    for enc, frozen, tpv, det in itertools.product(('pvc', 'avg', 'fs', 'pv'), (0, W_, R_, W_ | R_), (0, 1), (0, 1)):
        if enc != 'pv' and (frozen & R_):
            continue
        if enc in ('fs', 'avg') and tpv:
            continue
        key = (enc, frozen, tpv, det)
        assert key in PLAN_TABLE, "an existing cell has no row in PLAN_TABLE: %r" % (key,)
        cells.add(key)
        det_switch.ps_set_deterministic(det)
        got = _plan(_plan_desc(enc, frozen, tpv))
        assert tuple(getattr(got, f) for f in PLAN_FIELDS) == PLAN_TABLE[key], key
        assert got.user_scatter == 0 and got.item_scatter == 0
    assert cells == set(PLAN_TABLE)


def test_backward_plan_user_item_and_the_query_only_grid(det_switch):
    # user / item rows: scattered unless frozen; a trainable one turns the plain form into the general one
    p = _plan(_plan_desc('pvc', 0, 0, use_user_emb=1, use_item_emb=1))
    assert (p.user_scatter, p.item_scatter, p.embed_form) == (1, 1, GENERAL)
    p = _plan(_plan_desc('pvc', U_ | I_, 0, use_user_emb=1, use_item_emb=1))
    assert (p.user_scatter, p.item_scatter, p.embed_form) == (0, 0, PLAIN)
    p = _plan(_plan_desc('pvc', W_ | U_, 0, use_user_emb=1, use_item_emb=1))
    assert (p.user_scatter, p.item_scatter, p.embed_form, p.slot_waves) == (0, 1, FROZEN, 1)
    # frozen form, no segment embedding: review-slot waves only for trainable user / item rows ...
    p = _plan(_plan_desc('pvc', W_, 0, use_seg_emb=0))
    assert (p.embed_form, p.slot_waves) == (FROZEN, 0)
    p = _plan(_plan_desc('pvc', W_, 0, use_seg_emb=0, use_item_emb=1))
    assert (p.embed_form, p.slot_waves) == (FROZEN, 1)
    p = _plan(_plan_desc('pvc', W_ | I_, 0, use_seg_emb=0, use_item_emb=1))
    assert (p.embed_form, p.slot_waves) == (FROZEN, 0)
    p = _plan(_plan_desc('pv', R_, 1, use_seg_emb=0))
    assert (p.embed_form, p.slot_waves, p.pv_bwd) == (FROZEN, 0, _lib.PS_RTM_PV_WORDS)
    # ... which deterministic mode scatters beforehand through the sole-owner pass: no slot waves there either
    det_switch.ps_set_deterministic(1)
    p = _plan(_plan_desc('pvc', W_, 0, use_seg_emb=0, use_item_emb=1))
    assert (p.item_scatter, p.slot_waves) == (1, 0)
    # a trainable form always launches them
    p = _plan(_plan_desc('pvc', 0, 0, use_seg_emb=0))
    assert p.slot_waves == 1


def test_backward_plan_vocabulary_above_the_histogram_limit(det_switch):
    """Above RTM_HIST_MAXV (38000 words) trainable words fall back to the forward's counts; frozen words need no index at all."""
    p = _plan(_plan_desc('pvc', 0, 0, vocab_size=40000))
    assert (p.index, p.side_fork) == (_lib.PS_RTM_INDEX_FWD_COUNTS, 1)
    p = _plan(_plan_desc('pvc', 0, 0, vocab_size=40000, d=512, H=8))       # ... where the per-slot embed kernel cannot count: late
    assert (p.index, p.side_fork) == (_lib.PS_RTM_INDEX_LATE, 0)
    p = _plan(_plan_desc('pvc', W_, 0, vocab_size=40000))
    assert (p.index, p.word_reduce, p.side_fork) == (NONE, 0, 0)


def test_backward_plan_rejects_a_bad_descriptor():
    import ctypes as C
    lib = _lib.load()
    out = _lib.PsRtmBwdPlan()
    assert lib.ps_rtm_backward_plan(C.byref(_plan_desc('pvc', 0, 0, d=33)), C.byref(out)) != 0
    assert lib.ps_rtm_backward_plan(None, C.byref(out)) != 0


# ------------------------------------------------------------------------------------------------ the oracle, frozen leaves
def _oracle_forward(g, P, step):
    drop, tok = g.dropout(step)
    return ortm.rtm_forward(P, g.oracle_args(), g.batch(), g.neg_words(step), g.V, g.RC, training=True,
                            train_pv=g.steps_train_pv[step], drop=drop, tok_drop=tok)


@pytest.mark.parametrize('case', RTMPRE_CASES)
def test_oracle_with_frozen_leaves_matches_fixture(case):
    """oracle.rtm with ``requires_grad=False`` on the frozen tables (fix_emb: its pv branch with the 'rev_pv' drop the
    identity) against the reference: the three loss terms, which gradients are None, every gradient of steps 0 and 1, the
    pre-clip norm, the three clipped Adam steps.  Loss terms, gradients (relative to the tensor's largest entry), the norm and
    the eval scores below are held to the oracle suites' 2e-6 (test_oracle_golden.FP_TOL: same fp32 CPU ops, reassociation
    only); the stepped parameters by test_pretrained_cpu's rule.  Two named exceptions: ``linear_keys.bias`` (its gradient is
    rounding noise: softmax is shift-invariant) and the final LayerNorm's bias, whose gradient is the plain column sum of
    d enc over all n = B (1 + K) sequences with cancellation — recursive fp32 summation errs by up to (n - 1) 2^-24 of the
    summed magnitudes on each side (reference and oracle add the positive and the negative encoder call in different
    orders), so it is held to 2 (n - 1) 2^-24 (5.6e-6 at n = 48; measured 2.6e-6 at worst, rtmpre_fix_pv step 1)."""
    g = RtmPreGolden(case)
    a = g.args
    frozen = set(g.frozen())
    P = {k: v.clone().requires_grad_(k not in frozen) for k, v in g.params().items()}
    init = {k: v.detach().clone() for k, v in P.items()}
    opt = ooptim.ClipAdam(a.lr, a.max_grad_norm, a.beta1, a.beta2, 1e-9, a.l2_lambda, a.decay_method, a.warmup_steps)
    pad = {'word_embeddings.weight': g.V - 1, 'seg_embeddings.weight': 3, REVIEW_TABLE: g.RC - 1,
           'user_emb.weight': USER_SIZE, 'product_emb.weight': PRODUCT_SIZE}
    from oracle.tem import grads_of
    colsum_tol = 2 * (g.B * (1 + g.K) - 1) * 2.0 ** -24
    for step in range(g.steps):
        loss, ps, pv = _oracle_forward(g, P, step)
        for got, key in ((loss, 'loss_%d'), (ps, 'ps_loss_%d'), (pv if pv is not None else torch.zeros(()), 'pv_loss_%d')):
            ref = g.tensor(key % step)
            assert abs(float(got.detach()) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref))), (key % step, float(got.detach()), float(ref))
        grads = grads_of(loss, P, pad)
        assert not frozen & set(grads)
        if step in (0, 1):
            none = {g.oracle_name(n) for n in g.meta['none_grads_%d' % step]}
            assert {n for n in P if grads.get(n) is None} == none, step
            for n in g.meta['param_names']:
                on = g.oracle_name(n)
                if grads.get(on) is None or on.endswith('linear_keys.bias'):
                    continue
                assert rel_err(grads[on], g.tensor('grad%d_%s' % (step, n))) < (colsum_tol if on == FINAL_LN_BIAS else 2e-6), (step, n)
        with torch.no_grad():
            total = opt.step(P, grads)
        ref = float(g.tensor('gnorm_%d' % step))
        assert abs(float(total) - ref) < 2e-6 * ref, step
        if step == 0:
            assert float(total) > a.max_grad_norm                      # the clip is active
        if step in (0, g.steps - 1):
            for n in g.meta['optim_params']:
                on = g.oracle_name(n)
                ref = g.tensor('param%d_%s' % (step, n), base=init[on])
                diff = (P[on].detach() - ref).abs()
                if on.endswith('linear_keys.bias'):       # (its gradient is rounding noise: softmax is shift-invariant)
                    assert float(diff.max()) <= 2.01 * a.lr * (step + 1), (step, n)
                    continue
                bad = diff > 1e-4 * float(ref.abs().max())
                assert float(bad.float().mean()) <= 1e-3, (step, n)
    for n in frozen:
        assert torch.equal(P[n].detach(), init[n]), n


@pytest.mark.parametrize('case', RTMPRE_CASES)
def test_oracle_eval_scores(case):
    g = RtmPreGolden(case)
    P = g.params()
    a = g.oracle_args()
    with torch.no_grad():
        rev = ortm.rtm_review_embeddings(P, a, g.review_words, g.V)
        assert abs(float(rev.double().sum()) - float(g.z['test_review_embeddings_sum'])) < 1e-3
        s = ortm.rtm_test(P, a, g.test_batch(), rev, g.V, g.RC)
    assert rel_err(s, g.tensor('test_scores')) < 2e-6
