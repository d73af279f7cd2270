"""ZAM / AEM on the host (CPU only): the test-side oracle against the reference's own fixtures (tests/golden/attn_*.npz),
the AttentionEmbeddingRanker boundary (state_dict, initialisation, refusals) and the C ABI's workspace layout for the two
new model ids.  No GPU compute is called here."""
import pytest
import torch

from attn_oracle import ATTN_CASES, AttnGolden, attn_forward, attn_test
from golden_util import rel_err
from oracle import optim as ooptim
from oracle import tem as otem
from prodsearch_amd import AttentionEmbeddingRanker, ItemTransformerRanker, _lib, default_args, synth
from prodsearch_amd import build as pbuild


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


def _fwd(g, P, step):
    ni, nw = g.negs(step)
    drop = g.dropout(step) if g.args.dropout > 0 else None
    return attn_forward(P, g.args, g.batch(), ni, nw, g.V, g.P, training=True, drop=drop)


def test_fixture_set_is_complete():
    assert {'attn_zam', 'attn_aem', 'attn_zam_drop', 'attn_aem_drop', 'attn_aem_empty', 'attn_zam_opts'} <= set(ATTN_CASES)
    g = AttnGolden('attn_aem_empty')
    assert g.meta['empty_rows'] >= g.B // 4


@pytest.mark.parametrize('case', ATTN_CASES)
def test_oracle_loss_scores_and_gradients(case):
    g = AttnGolden(case)
    P = {k: v.clone().requires_grad_(True) for k, v in g.params().items()}
    keep = {}
    ni, nw = g.negs(0)
    drop = g.dropout(0) if g.args.dropout > 0 else None
    loss, ps, il = attn_forward(P, g.args, g.batch(), ni, nw, g.V, g.P, drop=drop, keep=keep)
    assert rel_err(loss, g.tensor('loss_0')) < 2e-6
    assert rel_err(ps, g.tensor('ps_loss_0')) < 2e-6
    assert rel_err(il, g.tensor('item_loss_0')) < 2e-6
    scores = torch.cat([keep['pos_scores'].unsqueeze(-1), keep['neg_scores']], -1)
    assert rel_err(scores, g.tensor('prod_scores')) < 1e-5
    grads = otem.grads_of(loss, P, otem.tem_pad_rows(g.args, g.V, g.P))
    assert sorted(n for n, v in grads.items() if v is None) == sorted(g.meta['none_grads'])
    for n, v in grads.items():
        if v is None:
            continue
        ref = g.tensor('grad_' + n)
        if n.endswith('linear_keys.bias'):       # exactly 0 in real arithmetic (softmax shift invariance): rounding noise
            scale = float(g.tensor('grad_' + n.replace('.bias', '.weight')).abs().max())
            assert float(v.abs().max()) < 1e-5 * scale and float(ref.abs().max()) < 1e-5 * scale, n
            continue
        assert rel_err(v, ref) < 2e-5, n
        if v.dim() == 2 and v.shape[0] > 256:
            assert torch.equal(v.ne(0).any(1), ref.ne(0).any(1)), n


@pytest.mark.parametrize('case', ATTN_CASES)
def test_oracle_two_adam_steps(case):
    g = AttnGolden(case)
    a = g.args
    P = {k: v.clone().requires_grad_(True) for k, v in g.params().items()}
    init = {k: v.detach().clone() for k, v in P.items()}
    opt = ooptim.ClipAdam(a.lr, a.max_grad_norm, a.beta1, a.beta2, 1e-9, a.l2_lambda, a.decay_method, a.warmup_steps)
    pad = otem.tem_pad_rows(a, g.V, g.P)
    for step in range(g.steps):
        loss, _, _ = _fwd(g, P, step)
        assert rel_err(loss, g.tensor('loss_%d' % step)) < 5e-6, step
        grads = otem.grads_of(loss, P, pad)
        with torch.no_grad():
            opt.step(P, grads)
        if step in (0, g.steps - 1):
            for n in P:
                ref = g.tensor('param%d_%s' % (step, n), base=init[n])
                diff = (P[n].detach() - ref).abs()
                if n.endswith('linear_keys.bias'):
                    assert float(diff.max()) <= 2.01 * a.lr * (step + 1), (step, n)
                    continue
                bad = diff > 5e-6 * float(ref.abs().max())
                assert float(bad.float().mean()) <= 2e-4 and (int(bad.sum()) == 0 or
                                                             float(diff[bad].max()) <= 2.01 * a.lr * (step + 1)), (step, n)


@pytest.mark.parametrize('case', ATTN_CASES)
def test_oracle_eval_scores(case):
    g = AttnGolden(case)
    with torch.no_grad():
        s = attn_test(g.params(), g.args, g.batch(), g.V, g.P)
    assert rel_err(s, g.tensor('test_scores')) < 1e-5


@pytest.mark.parametrize('case', ATTN_CASES)
def test_state_dict_matches_reference_keys(case):
    g = AttnGolden(case)
    m = AttentionEmbeddingRanker(g.args, 'cpu', g.V, g.P, None)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == g.meta['sd_keys']
    m.load_state_dict(g.params(), strict=True)


@pytest.mark.parametrize('name', ['ZAM', 'AEM'])
def test_initialisation_like_reference(name):
    a = default_args(model_name=name, embedding_size=64, heads=4)
    m = AttentionEmbeddingRanker(a, 'cpu', 300, 200, None)
    # attention_encoder keeps nn.Linear's default init (uniform, bound 1/sqrt(in)): the reference's initialize_parameters
    # does not touch it (item_transformer.py:576-586)
    bound = 1.0 / 64 ** 0.5
    for lin in (m.attention_encoder.linear_keys, m.attention_encoder.linear_values, m.attention_encoder.linear_query,
                m.attention_encoder.final_linear):
        assert float(lin.weight.abs().max()) <= bound and float(lin.weight.std()) > 0.4 * bound
        assert float(lin.bias.abs().max()) <= bound and float(lin.bias.abs().max()) > 0
    assert float(m.product_emb.weight[200].abs().max()) == 0.0
    assert abs(float(m.product_emb.weight[:200].std()) - 1.0) < 0.05          # nn.Embedding's N(0, 1)
    want = synth.tem_param_shapes(a, 300, 200)
    assert [k for k in m.state_dict()] == list(want)


def test_model_names_and_refusals():
    for name in ('ZAM', 'AEM'):
        with pytest.raises(NotImplementedError):
            ItemTransformerRanker(default_args(model_name=name), 'cpu', 300, 200, None)
        with pytest.raises(NotImplementedError, match='shard_tables'):
            AttentionEmbeddingRanker(default_args(model_name=name, shard_tables=True), 'cpu', 300, 200, None)
    for name in ('item_transformer', 'QEM', 'review_transformer'):
        with pytest.raises(NotImplementedError):
            AttentionEmbeddingRanker(default_args(model_name=name), 'cpu', 300, 200, None)
    m = AttentionEmbeddingRanker(default_args(model_name='ZAM'), 'cpu', 300, 200, None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m._dev()


def test_create_model_dispatches_attention_models():
    from prodsearch_amd import trainer
    import inspect
    src = inspect.getsource(trainer.create_model)
    assert 'AttentionEmbeddingRanker' in src


def _desc(model, L=20, dropout=0.1, C=0):
    d = _lib.PsTemDesc()
    d.B, d.K, d.L, d.Q, d.W, d.C = 384, 20, L, 8, 1, C
    d.d, d.H, d.F, d.n_layers = 128, 8, 512, 0
    d.product_size, d.vocab_size = 18357, 32387
    d.model, d.training, d.dropout = model, 1, dropout
    return d


def test_workspace_layout_attention_models(lib):
    lay = _lib.PsTemWsLayout()
    for model, S in ((_lib.PS_MODEL_ZAM, 21), (_lib.PS_MODEL_AEM, 20)):
        _lib.check(lib.ps_tem_workspace_layout(_desc(model), lay), 'layout')
        assert lay.R == 21 and lay.S == S and lay.total_floats > 0
        assert lay.enc > 0 and lay.kp > 0 and lay.vp > 0 and lay.ctx > 0 and lay.attn > 0
        _lib.check(lib.ps_tem_workspace_layout(_desc(model, dropout=0.0), lay), 'layout')
        assert lay.R == 1 and lay.S == S
        _lib.check(lib.ps_tem_workspace_layout(_desc(model, C=100), lay), 'layout')
        assert lay.R == 1
    # AEM needs a history column; ZAM runs on the zero column alone
    assert lib.ps_tem_workspace_layout(_desc(_lib.PS_MODEL_AEM, L=0), lay) != 0
    _lib.check(lib.ps_tem_workspace_layout(_desc(_lib.PS_MODEL_ZAM, L=0), lay), 'layout')
    assert lay.S == 1
    assert lib.ps_tem_workspace_layout(_desc(_lib.PS_MODEL_ZAM, L=64), lay) != 0        # S <= 64
    assert lib.ps_tem_workspace_layout(_desc(4), lay) != 0
