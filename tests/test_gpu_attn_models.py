"""ZAM / AEM (AttentionEmbeddingRanker, csrc/attn_emb.hip) on an MI355X: against the reference's own fixtures
(tests/golden/attn_*.npz), against the oracle (tests/attn_oracle.py) with the product's Philox masks at the shipped shapes, and
through every mode the step offers: row-sparse / lazy-exact optimizers, deterministic mode, the graph-replayed step,
full-catalogue ranking, alternation with the item transformer in one process, and create_model + Trainer end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from attn_oracle import ATTN_CASES, AttnGolden, attn_encode, attn_forward, attn_test, philox_drop
from golden_util import rel_err

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)


def _model(a, V, P_, sd, wd=None):
    from prodsearch_amd import AttentionEmbeddingRanker
    m = AttentionEmbeddingRanker(a, 'cuda', V, P_, None, word_dists=wd)
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


# ------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize('case', ATTN_CASES)
def test_fixture_loss_grads_adam_and_eval(case):
    from prodsearch_amd import build_optim
    g = AttnGolden(case)
    a = g.args
    sd = g.params()
    m = _model(a, g.V, g.P, sd, g.word_dists)
    b = g.batch().to('cuda')
    m.eval()
    with torch.no_grad():
        s = m.test(b).cpu()
    assert rel_err(s, g.tensor('test_scores')) < 1e-4
    m.train()
    opt = build_optim(a, m, None)
    init = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for step in range(g.steps):
        ni, nw = g.negs(step)
        loss = m(b, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        assert rel_err(loss.detach().cpu(), g.tensor('loss_%d' % step)) < 1e-4, step
        if step == 0:
            for n, p in m.named_parameters():
                assert (p.grad is None) == (n in g.meta['none_grads']), n
                if p.grad is None or n.endswith('linear_keys.bias'):
                    continue
                ref = g.tensor('grad_' + n)
                got = p.grad.cpu()
                assert rel_err(got, ref) < 5e-4, (n, rel_err(got, ref))
                if ref.dim() == 2 and ref.shape[0] > 256:
                    assert torch.equal(got.ne(0).any(1), ref.ne(0).any(1)), n
        opt.step()
        if step in (0, g.steps - 1):
            for n, p in m.named_parameters():
                ref = g.tensor('param%d_%s' % (step, n), base=init[n])
                diff = (p.detach().cpu() - ref).abs()
                if n.endswith('linear_keys.bias'):
                    assert float(diff.max()) <= 2.01 * a.lr * (step + 1), (step, n)
                    continue
                # Adam(eps 1e-9) turns gradient elements of the order of eps into lr-sized steps either way: such elements
                # may differ by up to lr per step, everything else is pinned
                bad = diff > 1e-4 * float(ref.abs().max())
                assert float(bad.float().mean()) <= 1e-3 and (int(bad.sum()) == 0 or
                                                             float(diff[bad].max()) <= 2.01 * a.lr * (step + 1)), (step, n)


# ------------------------------------------------------------------------------------------------ oracle, shipped shapes
def check_against_oracle(B, K, L, Q, model_name='ZAM', W=1, zero_hist=0.2, P_=700, V=900, **over):
    """One training forward + backward through the module API and one eval call against attn_oracle (replicated negatives,
    the product's Philox masks).  ``over``: default_args overrides on top of d = 128, 8 heads, dropout 0.1."""
    from oracle import tem as otem
    from prodsearch_amd import default_args, synth
    kw = dict(model_name=model_name, embedding_size=128, heads=8, neg_per_pos=K, dropout=0.1, uprev_review_limit=L,
              pv_window_size=W)
    kw.update(over)
    a = default_args(**kw)
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 7, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    m = _model(a, V, P_, sd, wd)
    batch = synth.make_tem_batch(11, B, P_, V, Q=Q, L=L, W=W, C=9, word_dists=wd, zero_hist_frac=zero_hist)
    ni, nw = synth.sample_negatives(12, B, K, W, P_, wd)
    loss = m(batch.to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()

    Pm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    drop = philox_drop(a, m._seed, m._fwd_step, B, K, L) if a.dropout > 0 else None
    oloss, _, _ = attn_forward(Pm, a, batch, ni, nw, V, P_, training=True, drop=drop)
    assert rel_err(loss.detach().cpu(), oloss.detach()) < 1e-4
    grads = otem.grads_of(oloss, Pm, otem.tem_pad_rows(a, V, P_))
    for n, p in m.named_parameters():
        ref = grads.get(n)
        assert (p.grad is None) == (ref is None), n
        if ref is None or n.endswith('linear_keys.bias'):       # (rounding noise: softmax is shift-invariant)
            continue
        got = p.grad.cpu()
        assert rel_err(got, ref) < 5e-4, (n, rel_err(got, ref))
        if ref.dim() == 2 and ref.shape[0] > 256:
            assert torch.equal(got.ne(0).any(1), ref.ne(0).any(1)), n
    m.eval()
    with torch.no_grad():
        s = m.test(batch.to('cuda')).cpu()
    assert rel_err(s, attn_test(sd, a, batch, V, P_)) < 1e-4
    return m


C2S = dict(B=50, K=20, L=9, Q=4)
CASES = {
    'zam_fs': dict(C2S),
    'aem_fs': dict(C2S, model_name='AEM'),
    'zam_avg': dict(C2S, query_encoder_name='avg'),
    'aem_avg': dict(C2S, model_name='AEM', query_encoder_name='avg'),
    'zam_fs_l20': dict(B=50, K=20, L=20, Q=6),
    'aem_avg_l20': dict(B=50, K=20, L=20, Q=6, model_name='AEM', query_encoder_name='avg'),
    'zam_nodrop': dict(C2S, dropout=0.0),
    'aem_nodrop': dict(C2S, model_name='AEM', dropout=0.0),
    'aem_zero_hist': dict(C2S, model_name='AEM', zero_hist=0.5),
    'aem_zero_hist_nodrop': dict(C2S, model_name='AEM', zero_hist=0.5, dropout=0.0),
    'zam_opts': dict(C2S, W=3, sim_func='bias_product', pos_weight=True, sep_prod_emb=True),
    'aem_opts': dict(C2S, model_name='AEM', W=3, sim_func='bias_product', pos_weight=True, sep_prod_emb=True),
    'zam_d256': dict(B=70, K=20, L=20, Q=8, embedding_size=256),
    'aem_d256_avg': dict(B=70, K=20, L=20, Q=8, embedding_size=256, model_name='AEM', query_encoder_name='avg'),
    'zam_c2': dict(B=384, K=20, L=20, Q=8, P_=3000, V=4000),           # the C2 shape: 8,064 replica rows
    'aem_c2': dict(B=384, K=20, L=20, Q=8, P_=3000, V=4000, model_name='AEM'),
}


@pytest.mark.parametrize('case', list(CASES))
def test_matches_oracle(case):
    check_against_oracle(**CASES[case])


# ------------------------------------------------------------------------------------------------ modes
def _train(model_name, steps=3, **over):
    """A few module-API steps with the product's optimizer on one fixed batch; returns the final state_dict (CPU)."""
    from prodsearch_amd import build_optim, default_args, synth
    V, P_, B, K, L = 900, 700, 40, 6, 9
    a = default_args(model_name=model_name, embedding_size=128, heads=8, neg_per_pos=K, dropout=0.1, lr=0.002, **over)
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 9, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    m = _model(a, V, P_, sd, wd)
    opt = build_optim(a, m, None)
    batch = synth.make_tem_batch(21, B, P_, V, Q=5, L=L, W=1, word_dists=wd).to('cuda')
    for step in range(steps):
        ni, nw = synth.sample_negatives(30 + step, B, K, 1, P_, wd)
        loss = m(batch, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        opt.step()
    return m, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize('model_name', ['ZAM', 'AEM'])
def test_lazy_exact_adam_equals_dense(model_name):
    _, dense = _train(model_name)
    m, lazy = _train(model_name, lazy_exact_adam=True)
    for k in dense:
        if k.endswith('linear_keys.bias'):
            continue
        assert rel_err(lazy[k], dense[k]) < 1e-4, k


@pytest.mark.parametrize('model_name', ['ZAM', 'AEM'])
def test_row_sparse_adam_touches_the_history_rows(model_name):
    """Row-sparse Adam updates exactly the rows the step touched — the history rows included — with the dense step's first
    update (zero moments), and keeps every other row."""
    m, sparse = _train(model_name, steps=1, row_sparse_adam=True, sep_prod_emb=True)
    _, dense_sep = _train(model_name, steps=1, sep_prod_emb=True)
    for k in dense_sep:
        if k.endswith('linear_keys.bias'):
            continue
        assert rel_err(sparse[k], dense_sep[k]) < 1e-4, k
    from prodsearch_amd import synth
    batch = synth.make_tem_batch(21, 40, 700, 900, Q=5, L=9, W=1, word_dists=synth.make_word_dists(900))
    hist = torch.unique(batch.u_item_idxs)
    hist = hist[hist != 700]
    rows = m.touched_rows()['hist_product_emb.weight'].cpu()
    assert torch.equal(rows, hist)


def test_deterministic_mode_is_bitwise_run_to_run():
    from prodsearch_amd import _lib
    lib = _lib.load()
    old = lib.ps_set_deterministic(1)
    try:
        for name in ('ZAM', 'AEM'):
            _, s1 = _train(name)
            _, s2 = _train(name)
            for k in s1:
                assert torch.equal(s1[k], s2[k]), (name, k)
    finally:
        lib.ps_set_deterministic(old)


def test_graph_replayed_step_is_bitwise_the_eager_step():
    """PS_GRAPHS=1 (ps_tem_forward_step / ps_tem_backward_step, captured on the second call) against the eager step, both in
    deterministic mode so that table sums do not reassociate between the runs."""
    code = r"""
import sys, json, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_gpu_attn_models import _train
from prodsearch_amd import _lib
out = {}
for name in ('ZAM', 'AEM'):
    m, sd = _train(name, steps=4)
    out[name] = {k: v.double().sum().item() for k, v in sd.items()}
    out[name + '_bits'] = {k: v.view(torch.int32).long().sum().item() for k, v in sd.items()}
print(json.dumps({'graphs': int(_lib.load().ps_graph_replay_enabled()), 'r': out}))
""" % (REPO, TESTS)
    out = {}
    for flag in ('0', '1'):
        env = dict(os.environ, PS_GRAPHS=flag, PS_DETERMINISTIC='1')
        r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, 'PS_GRAPHS=%s: exit %d\n%s' % (flag, r.returncode, r.stderr[-3000:])
        out[flag] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['0']['graphs'] == 0 and out['1']['graphs'] == 1
    assert out['0']['r'] == out['1']['r']


@pytest.mark.parametrize('model_name', ['ZAM', 'AEM'])
def test_rank_all_matches_oracle(model_name):
    from prodsearch_amd import default_args, evaluate, synth
    V, P_, B = 900, 700, 33
    a = default_args(model_name=model_name, embedding_size=128, heads=8, dropout=0.1)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 5, {'product_emb.weight': P_})
    m = _model(a, V, P_, sd)
    batch = synth.make_tem_batch(3, B, P_, V, Q=5, L=12, W=1, C=4, zero_hist_frac=0.3)
    top_idx, top_score, rank = evaluate.rank_all(m, batch.to('cuda'), topk=20)
    with torch.no_grad():
        q = attn_encode(sd, a, batch, V, P_)
        full = q @ sd['product_emb.weight'][:P_].t()
    ref_top = full.topk(20, dim=1)
    assert rel_err(top_score.cpu(), ref_top.values) < 1e-4
    tgt = batch.target_prod_idxs
    ref_rank = 1 + (full > full.gather(1, tgt[:, None])).sum(1)
    assert (rank.cpu().long() - ref_rank).abs().max() <= 1      # ties within fp noise may move a rank by one


def test_alternating_item_transformer_and_zam_steps():
    """TEM, ZAM, TEM, AEM, TEM in one process: every step against its own oracle (per-call decisions of one model must never
    reach the next)."""
    sys.path.insert(0, TESTS)
    from test_gpu_tem_options import check_against_oracle as tem_check
    tem_case = dict(B=50, K=20, L=9, Q=4)
    tem_check(**tem_case)
    check_against_oracle(**CASES['zam_fs'])
    tem_check(**tem_case)
    check_against_oracle(**CASES['aem_avg'])
    tem_check(**dict(tem_case, query_encoder_name='avg'))


@pytest.mark.parametrize('model_name', ['ZAM', 'AEM'])
def test_create_model_and_trainer_end_to_end(tmp_path, model_name):
    from prodsearch_amd import AttentionEmbeddingRanker, default_args, synth, trainer
    data_path, inp = synth.write_corpus(str(tmp_path / 'corpus'), 21, n_users=60, n_products=80, n_words=200)
    save = str(tmp_path / 'run')
    args = default_args(model_name=model_name, embedding_size=32, heads=4, batch_size=32, neg_per_pos=5,
                        uprev_review_limit=5, subsampling_rate=1e-2, lr=0.01, max_train_epoch=2, steps_per_checkpoint=20,
                        has_valid=True, valid_candi_size=-1, valid_batch_size=24, data_dir=data_path, input_train_dir=inp,
                        save_dir=save, device='cuda', dropout=0.1)
    np.random.seed(5)
    mrr, p1 = trainer.train(args)
    assert 0.0 < mrr <= 1.0 and 0.0 <= p1 <= 1.0
    lines = open(os.path.join(save, args.rankfname)).read().splitlines()
    assert lines and all(len(ln.split(' ')) == 6 for ln in lines)
    from prodsearch_amd import corpus
    gd = corpus.GlobalProdSearchData(args, data_path, inp)
    model, _ = trainer.create_model(args, gd, corpus.ProdSearchData(args, inp, 'train', gd))
    assert isinstance(model, AttentionEmbeddingRanker)
