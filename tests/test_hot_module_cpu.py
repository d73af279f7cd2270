"""The host base class of the two HIP-backed rankers (prodsearch_amd/hot_module.py) on the CPU: the flat gradient buffer's
slice rule on hand-written cases, the layout both real models derive from it (order, absent paths, the re-plan key), the
per-layer field list, and what the module may import.  Nothing is launched."""
import ast
import inspect
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from prodsearch_amd import ItemTransformerRanker, ProductRanker, _lib, default_args, hot_module, ps_model
from prodsearch_amd.hot_module import encoder_layer_params, flat_layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_FIELDS = 'wk bk wv bv wq bq wo bo w1 b1 w2 b2 ff_ln_g ff_ln_b ln_g ln_b'.split()


# ------------------------------------------------------------------------------------------------------------- flat_layout
@pytest.mark.parametrize('pad_to', [4, 32])
@pytest.mark.parametrize('numels', [[1, 3, 4, 5, 37 * 8], [37 * 8, 5, 4, 3, 1], [4], [7, 7, 7], [1] * 9])
def test_flat_layout_slices(numels, pad_to):
    offs, total = flat_layout(numels, pad_to)
    assert len(offs) == len(numels) and offs[0] == 0
    assert all(o % 4 == 0 for o in offs)
    for (o, n), nxt in zip(zip(offs, numels), offs[1:]):           # the given order, no overlap, no gap wider than the alignment
        assert o + n <= nxt < o + n + 4
    assert total % pad_to == 0
    assert offs[-1] + (numels[-1] + 3) // 4 * 4 <= total < offs[-1] + (numels[-1] + 3) // 4 * 4 + pad_to


def test_flat_layout_by_hand():
    assert flat_layout([1, 3, 4, 5, 296], 4) == ([0, 4, 8, 12, 20], 316)
    assert flat_layout([1, 3, 4, 5, 296], 32) == ([0, 4, 8, 12, 20], 320)
    assert flat_layout([], 4) == ([], 0) and flat_layout([], 32) == ([], 0)
    assert flat_layout([32], 32) == ([0], 32) and flat_layout([33], 32) == ([0], 64)


# ------------------------------------------------------------------------------------------------------------- the models
def _tem(**over):
    a = default_args(**dict(dict(model_name='item_transformer', inter_layers=2, embedding_size=32, ff_size=64, heads=4), **over))
    return ItemTransformerRanker(a, 'cpu', 300, 200, None)


def _rtm(**over):
    a = default_args(**dict(dict(model_name='review_transformer', review_encoder_name='pv', embedding_size=32, heads=4,
                                 ff_size=64, inter_layers=2, use_user_emb=True, use_item_emb=True), **over))
    rw = torch.full((40, 5), 59, dtype=torch.int64)
    return ProductRanker(a, 'cpu', 60, 40, 50, 30, rw, None)


def _check_layout(m, key_of):
    """The layout is the stable sort of the graded hot parameters by ``key_of(path, numel)``, laid out by flat_layout."""
    numel = {path: p.numel() for path, p in m._named_hot_params()}
    graded = [path for path, _ in m._named_hot_params() if m._has_grad(path)]
    want = sorted(graded, key=lambda path: key_of(path, numel[path]))
    for pad in (4, 32):
        m.__dict__['_flat_pad_to'] = pad
        rows, total = m._grad_layout()
        assert [r[0] for r in rows] == want
        assert [r[2] for r in rows] == [numel[p] for p in want]
        assert ([r[1] for r in rows], total) == flat_layout([numel[p] for p in want], pad)
    m.__dict__.pop('_flat_pad_to')
    return [r[0] for r in m._grad_layout()[0]]


def test_item_model_layout_order_and_absent_paths():
    m = _tem()
    paths = _check_layout(m, lambda path, n: n)                      # no row-sparse table, no shard: by numel alone
    assert ('product_bias',) not in paths and ('word_emb',) in paths
    assert ('layer', 0, 'ln_g') not in paths and ('layer', 0, 'ln_b') not in paths
    assert ('layer', 1, 'ln_g') in paths and ('layer', 1, 'ln_b') in paths
    assert ('product_bias',) in _check_layout(_tem(sim_func='bias_product'), lambda path, n: n)
    m.word_embeddings.weight.requires_grad_(False)
    assert ('word_emb',) not in _check_layout(m, lambda path, n: n)
    # row-sparse mode: the tables go behind every dense tensor, whatever their size
    sp = _tem(row_sparse_adam=True, sep_prod_emb=True)
    tables = (('product_emb',), ('word_emb',), ('hist_product_emb',))
    paths = _check_layout(sp, lambda path, n: (path in tables, False, n))
    assert set(paths[-3:]) == set(tables)
    assert ItemTransformerRanker._grad_layout is hot_module.HotPathModule._grad_layout
    with pytest.raises(RuntimeError, match='no CPU fallback'):      # ... and it needed no device: _structs still does
        m._structs()


def test_review_model_layout_order_and_absent_paths():
    m = _rtm(use_seg_emb=True)
    paths = _check_layout(m, lambda path, n: n)
    assert ('seg_emb',) in paths
    assert ('layer', 0, 'ln_g') not in paths and ('layer', 1, 'ln_g') in paths
    assert ('seg_emb',) not in _check_layout(_rtm(use_seg_emb=False), lambda path, n: n)
    tabs = m._hot_tables()
    assert set(tabs) == {name for name, _ in ProductRanker._TABLE_BITS}
    for name, p in tabs.items():
        assert (name,) in _check_layout(m, lambda path, n: n)
        p.requires_grad_(False)
        assert (name,) not in _check_layout(m, lambda path, n: n)
        p.requires_grad_(True)


def test_grad_key_changes_exactly_with_what_the_layout_drops():
    m = _tem()
    k0 = m._grad_key()
    m.product_bias.requires_grad_(False)                             # not a path whose requires_grad the layout follows
    m.product_emb.weight.requires_grad_(False)
    assert m._grad_key() == k0
    m.word_embeddings.weight.requires_grad_(False)
    assert m._grad_key() != k0
    m.word_embeddings.weight.requires_grad_(True)
    assert m._grad_key() == k0

    r = _rtm()
    k0, seen = r._grad_key(), set()
    r.seg_embeddings.weight.requires_grad_(False)
    r.transformer_encoder.wo.weight.requires_grad_(False)
    assert r._grad_key() == k0
    for name, p in r._hot_tables().items():
        p.requires_grad_(False)
        k = r._grad_key()
        assert k != k0 and k not in seen, name
        seen.add(k)
        p.requires_grad_(True)
        assert r._grad_key() == k0
    for p in r._hot_tables().values():
        p.requires_grad_(False)
    assert r._grad_key() not in seen | {k0}                           # every combination is its own key
    assert r._grad_key() == sum(bit for _, bit in ProductRanker._TABLE_BITS)


# --------------------------------------------------------------------------------------------------- encoder_layer_params
@pytest.mark.parametrize('n_layers', [1, 2])
def test_encoder_layer_params(n_layers):
    te = _tem(inter_layers=n_layers).transformer_encoder
    got = encoder_layer_params(te)
    assert [path for path, _ in got] == [('layer', i, f) for i in range(n_layers) for f in LAYER_FIELDS]
    assert set(LAYER_FIELDS) <= {f for f, _ in _lib.PsLayerTensors._fields_}
    named = {id(p): n for n, p in te.named_parameters()}
    assert len({id(p) for _, p in got}) == 16 * n_layers and all(id(p) in named for _, p in got)
    l0 = te.transformer_inter[0]
    by_path = dict(got)
    assert by_path[('layer', 0, 'wk')] is l0.self_attn.linear_keys.weight
    assert by_path[('layer', 0, 'bo')] is l0.self_attn.final_linear.bias
    assert by_path[('layer', 0, 'w2')] is l0.feed_forward.w_2.weight
    assert by_path[('layer', 0, 'ff_ln_g')] is l0.feed_forward.layer_norm.weight
    assert by_path[('layer', 0, 'ln_b')] is l0.layer_norm.bias


# --------------------------------------------------------------------------------------------------------- import hygiene
def _imports(obj):
    """Every import statement in the source of ``obj`` (a module or a function), at any depth."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(obj)))
    return [ast.unparse(n) for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]


def test_hot_module_imports_neither_model():
    assert _imports(hot_module) == ['import torch', 'import torch.nn as nn', 'from . import _lib']
    # a child interpreter with the package's __init__ (which imports the models) replaced by a bare namespace
    code = ("import sys, types; "
            "pkg = types.ModuleType('prodsearch_amd'); pkg.__path__ = [%r]; sys.modules['prodsearch_amd'] = pkg; "
            "import prodsearch_amd.hot_module as h; "
            "assert h.HotPathModule and h.flat_layout([], 4) == ([], 0); "
            "bad = [m for m in sys.modules if m.endswith(('item_transformer', 'ps_model'))]; "
            "assert not bad, bad" % os.path.join(REPO, 'prodsearch_amd'))
    r = subprocess.run([sys.executable, '-c', code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_step_path_has_no_function_level_import():
    for fn in (ps_model.ProductRanker.forward, ItemTransformerRanker.forward, hot_module.HotPathModule._loss_forward,
               hot_module._RankLossFn.forward, hot_module._RankLossFn.backward, hot_module._LossTensor.backward):
        assert _imports(fn) == [], fn
    assert not hasattr(ps_model, '_RtmLossFn')
    assert ProductRanker._structs is ItemTransformerRanker._structs is hot_module.HotPathModule._structs
    assert ProductRanker._regrade is ItemTransformerRanker._regrade is hot_module.HotPathModule._regrade


def test_a_plan_reads_by_attribute_and_by_subscript():
    plan = hot_module._Plan()
    plan.desc, plan.dummy_items = 3, None
    assert plan.desc == plan['desc'] == 3 and plan['dummy_items'] is None      # callers that knew the review model's dicts
    with pytest.raises(AttributeError):
        plan.unknown = 1
