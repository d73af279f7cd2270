"""The item rows' gradient scatter inside the fused per-replica backward (mlp_fused.hip, MlpBwdArgs::g_product_emb; the score
backward then launches its word tasks only, ScoreArgs::items_elsewhere) against the golden gradients and the oracle.  Every case
runs with the form on and off (``ps_set_item_scatter_fused``); on, ``ps_item_scatter_fused_taken()`` must say that the last
backward really took it, so no case can pass through the score backward's own item workgroups.

The form exists where the fused backward does: d = 128 with replicas.  The golden cases with dropout at d = 32 run as well —
there the call must report that the form was NOT taken (d != 128 keeps the score backward's item workgroups).

Tolerances are the project's: GRAD_TOL = 5e-4 max-norm relative (fp32 atomics reassociate sums), touched rows bit-exact."""
import pytest
import torch

from golden_util import TEM_CASES, Golden, rel_err

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-4
DROP_CASES = [c for c in TEM_CASES if Golden(c).args.dropout > 0]


class _Forms(object):
    """Fused backward forced (ps_set_fuse_bwd_min(1)) and the item scatter set to ``on``; both restored on exit."""

    def __init__(self, on):
        from prodsearch_amd import _lib
        self.lib, self.on = _lib.load(), int(on)

    def __enter__(self):
        self.old_min = self.lib.ps_set_fuse_bwd_min(1)
        self.old_on = self.lib.ps_set_item_scatter_fused(self.on)
        return self.lib

    def __exit__(self, *exc):
        self.lib.ps_set_item_scatter_fused(self.old_on)
        self.lib.ps_set_fuse_bwd_min(self.old_min)
        return False


def _check_item_grads(m, ref_of, P_, with_bias):
    got = dict(m.named_parameters())['product_emb.weight'].grad.cpu()
    ref = ref_of('product_emb.weight')
    err = rel_err(got, ref)
    print('grad product_emb: rel_err %.3g' % err)
    assert err < GRAD_TOL
    assert torch.equal(got.ne(0).any(1), ref.ne(0).any(1))
    assert float(got[P_].abs().max()) == 0.0                      # the padding row's gradient stays exactly zero
    if with_bias:
        gb, rb = dict(m.named_parameters())['product_bias'].grad.cpu(), ref_of('product_bias')
        err = rel_err(gb, rb)
        print('grad product_bias: rel_err %.3g' % err)
        assert err < GRAD_TOL


@pytest.mark.parametrize('on', [1, 0])
@pytest.mark.parametrize('case', DROP_CASES)
def test_golden_item_gradients(case, on):
    from test_gpu_parity import _model
    g = Golden(case)
    served = g.args.embedding_size == 128 and g.args.ff_size in (256, 512, 1024)      # where the fused backward exists
    with _Forms(on) as lib:
        m = _model(g)
        ni, nw = g.negs(0)
        loss = m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        assert lib.ps_item_scatter_fused_taken() == (1 if on and served else 0)
    _check_item_grads(m, lambda n: g.tensor('grad_' + n), g.P, g.args.sim_func == 'bias_product')


def _edited_batch(B, K, P_, V, wd):
    """A synthetic batch whose item indices meet every special case of the scatter: a padding target, a padding negative, one
    item three times among one row's negatives and as another row's target."""
    from prodsearch_amd import synth
    batch = synth.make_tem_batch(3, B, P_, V, Q=8, L=20, W=1, word_dists=wd)
    ni, nw = synth.sample_negatives(4, B, K, 1, P_, wd)
    rep = 17
    tgt = batch.target_prod_idxs
    tgt[0] = P_
    ni[1, 0] = P_
    ni[2, :3] = rep
    tgt[3] = rep
    assert int(tgt[0]) == P_ and int((tgt == P_).sum()) == 1
    assert int((ni == P_).sum()) == 1 and int(ni[1, 0]) == P_
    assert int((ni[2] == rep).sum()) >= 3 and int(tgt[3]) == rep
    return batch, ni, nw, rep


SHAPES = [(32, 7, 'product'),          # 256 replica rows: a multiple of the kernel's 32-row tiles
          (37, 5, 'product'),          # 222 rows: a last workgroup with 30 valid rows
          (37, 5, 'bias_product')]


@pytest.mark.parametrize('on', [1, 0])
@pytest.mark.parametrize('B,K,sim', SHAPES)
def test_synthetic_item_gradients_match_oracle(B, K, sim, on):
    from oracle import tem as otem, philox
    from prodsearch_amd import ItemTransformerRanker, default_args, synth
    P_, V, d, F, L = 300, 500, 128, 512, 20
    a = default_args(model_name='item_transformer', embedding_size=d, ff_size=F, heads=8, inter_layers=1,
                     neg_per_pos=K, dropout=0.1, uprev_review_limit=L, sim_func=sim)
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 5, {'product_emb.weight': P_})
    batch, ni, nw, rep = _edited_batch(B, K, P_, V, wd)
    with _Forms(on) as lib:
        m = ItemTransformerRanker(a, 'cuda', V, P_, None, word_dists=wd)
        m.load_state_dict(sd, strict=False)
        m.train()
        loss = m(batch.to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        assert lib.ps_item_scatter_fused_taken() == on
    Pm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    drop = philox.PhiloxDropout(0.1, m._seed, m._fwd_step, B, K, 8, L + 1, 1, L if a.use_item_pos else 0)
    oloss, _, _ = otem.tem_forward(Pm, a, batch, ni, nw, V, P_, training=True, replicate=True, drop=drop)
    assert torch.isfinite(oloss)
    assert rel_err(loss.detach().cpu(), oloss.detach()) < 1e-4
    grads = otem.grads_of(oloss, Pm, otem.tem_pad_rows(a, V, P_))
    assert bool(grads['product_emb.weight'][rep].ne(0).any())
    _check_item_grads(m, lambda n: grads[n], P_, sim == 'bias_product')


def test_scaled_loss_gives_twice_the_gradients_with_the_form_taken():
    """(2 * loss).backward() goes through autograd with a device-side scale (MlpBwdArgs::scale_dev): twice the gradients of
    loss.backward(), the item rows' scatter inside the fused backward both times."""
    from test_gpu_parity import _model
    g = Golden('tem_c2s_drop')
    ni, nw = g.negs(0)
    grads = []
    with _Forms(1) as lib:
        for scale in (None, 2.0):
            m = _model(g)
            loss = m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
            m.zero_grad()
            (loss if scale is None else loss * scale).backward()
            torch.cuda.synchronize()
            assert lib.ps_item_scatter_fused_taken() == 1
            grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    for n in grads[0]:
        if n.endswith('linear_keys.bias'):
            continue
        assert rel_err(grads[1][n], 2.0 * grads[0][n]) < 1e-5, n
