"""Pretrained, frozen word table (``pretrain_emb_dir``) on an MI355X: the item models (TEM, QEM, ZAM, AEM) against the
reference's own fixtures (tests/golden/frozen_*.npz), and at the C2 shape against the oracle with the product's Philox
masks through every mode of the step: dense / row-sparse / lazy-exact Adam, deterministic mode, graph replay, flipping
``requires_grad`` between steps, and create_model + Trainer end to end with a checkpoint reload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pretrain_util
from attn_oracle import attn_forward, philox_drop
from golden_util import rel_err
from test_pretrained_cpu import FROZEN_CASES, FrozenGolden, _cls

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
WORD = 'word_embeddings.weight'


# ------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize('case', FROZEN_CASES)
def test_fixture_loss_grads_and_three_clipped_steps(case):
    from prodsearch_amd import build_optim
    g = FrozenGolden(case)
    a = g.args
    torch.manual_seed(0)
    m = _cls(a)(a, 'cuda', g.V, g.P, g.words, word_dists=g.word_dists)
    sd = g.params()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('pos_emb.pe') for k in missing)
    table = m.word_embeddings.weight.detach().clone()
    assert torch.equal(table.cpu(), g.tensor('word_table'))
    m.train()
    opt = build_optim(a, m, None)
    assert not any(p is m.word_embeddings.weight for p in opt.params)
    b = g.batch().to('cuda')
    init = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for step in range(g.steps):
        ni, nw = g.negs(step)
        loss = m(b, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        assert m.word_embeddings.weight.grad is None
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
                bad = diff > 1e-4 * float(ref.abs().max())
                assert float(bad.float().mean()) <= 1e-3 and (int(bad.sum()) == 0 or
                                                             float(diff[bad].max()) <= 2.01 * a.lr * (step + 1)), (step, n)
    assert torch.equal(m.word_embeddings.weight.detach(), table)


# ------------------------------------------------------------------------------------------------ C2 shape, the oracle
C2 = dict(B=384, K=20, L=20, Q=8, P_=3000, V=4000)


def _setup(model_name, tmp, seed=7, **over):
    """A model at the C2 shape whose word table comes from a pretrained file written into ``tmp``."""
    from prodsearch_amd import default_args, synth
    kw = dict(model_name=model_name, embedding_size=128, heads=8, ff_size=512, inter_layers=1, neg_per_pos=C2['K'],
              dropout=0.1, uprev_review_limit=C2['L'], lr=0.002, max_grad_norm=1.0)
    kw.update(over)
    a = default_args(**kw)
    V, P_ = C2['V'], C2['P_']
    words = pretrain_util.vocab_words(V)
    emb = os.path.join(tmp, 'emb')
    if not os.path.exists(os.path.join(emb, 'word_emb.txt.gz')):
        os.makedirs(emb, exist_ok=True)
        pretrain_util.write_word_emb(os.path.join(emb, 'word_emb.txt.gz'), words, 128, seed=11, n_extra=50, tie_share=0.02)
    a.pretrain_emb_dir = emb
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), seed, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    del sd[WORD]
    m = _cls(a)(a, 'cuda', V, P_, words, word_dists=wd)
    m.load_state_dict(sd, strict=False)
    m.train()
    sd[WORD] = m.word_embeddings.weight.detach().cpu().clone()
    return a, m, sd, wd


def _batch(step, wd):
    from prodsearch_amd import synth
    b = synth.make_tem_batch(100 + step, C2['B'], C2['P_'], C2['V'], Q=C2['Q'], L=C2['L'], W=1, C=9, word_dists=wd,
                             zero_hist_frac=0.2)
    ni, nw = synth.sample_negatives(200 + step, C2['B'], C2['K'], 1, C2['P_'], wd)
    return b, ni, nw


def _oracle_grads(a, m, sd, batch, ni, nw, trainable_words=False):
    from oracle import philox
    from oracle import tem as otem
    V, P_, B, K, L = C2['V'], C2['P_'], C2['B'], C2['K'], C2['L']
    Pm = {k: v.clone().requires_grad_(trainable_words or k != WORD) for k, v in sd.items()}
    if a.model_name in ('ZAM', 'AEM'):
        drop = philox_drop(a, m._seed, m._fwd_step, B, K, L) if a.dropout > 0 else None
        loss = attn_forward(Pm, a, batch, ni, nw, V, P_, training=True, drop=drop)[0]
    else:
        drop = philox.PhiloxDropout(a.dropout, m._seed, m._fwd_step, B, K, a.heads, L + 1, a.inter_layers, 0) \
            if a.dropout > 0 else None
        loss = otem.tem_forward(Pm, a, batch, ni, nw, V, P_, training=True, replicate=True, drop=drop)[0]
    return loss, otem.grads_of(loss, Pm, otem.tem_pad_rows(a, V, P_))


def _check_step(a, m, sd, step, wd, trainable_words=False):
    """One training forward + backward through the module API against the oracle; returns nothing, asserts."""
    batch, ni, nw = _batch(step, wd)
    loss = m(batch.to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    oloss, grads = _oracle_grads(a, m, sd, batch, ni, nw, trainable_words)
    assert rel_err(loss.detach().cpu(), oloss.detach()) < 1e-4
    for n, p in m.named_parameters():
        ref = grads.get(n)
        assert (p.grad is None) == (ref is None), n
        if ref is None or n.endswith('linear_keys.bias'):
            continue
        got = p.grad.cpu()
        assert rel_err(got, ref) < 5e-4, (n, rel_err(got, ref))
        if ref.dim() == 2 and ref.shape[0] > 256:
            assert torch.equal(got.ne(0).any(1), ref.ne(0).any(1)), n


@pytest.mark.parametrize('model_name', ['item_transformer', 'ZAM'])
@pytest.mark.parametrize('qenc', ['fs', 'avg'])
def test_c2_gradients_match_oracle(model_name, qenc, tmp_path):
    a, m, sd, wd = _setup(model_name, str(tmp_path), query_encoder_name=qenc)
    _check_step(a, m, sd, 0, wd)
    assert m.word_embeddings.weight.grad is None


def _train(model_name, tmp, steps=3, **over):
    from prodsearch_amd import build_optim
    a, m, sd, wd = _setup(model_name, tmp, **over)
    table = m.word_embeddings.weight.detach().clone()
    opt = build_optim(a, m, None)
    for step in range(steps):
        batch, ni, nw = _batch(step, wd)
        loss = m(batch.to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        assert m.word_embeddings.weight.grad is None
        opt.step()
    assert torch.equal(m.word_embeddings.weight.detach(), table)
    return m, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize('model_name', ['item_transformer', 'ZAM'])
def test_c2_dense_adam_matches_oracle(model_name, tmp_path):
    from oracle import optim as ooptim
    from oracle import tem as otem
    _, got = _train(model_name, str(tmp_path), steps=2)
    a, m, sd, wd = _setup(model_name, str(tmp_path))
    P = {k: v.clone() for k, v in sd.items()}
    opt = ooptim.ClipAdam(a.lr, a.max_grad_norm, a.beta1, a.beta2, 1e-9, a.l2_lambda)
    for step in range(2):
        m._fwd_step = step + 1                       # the oracle's dropout masks follow the product's step counter
        batch, ni, nw = _batch(step, wd)
        _, grads = _oracle_grads(a, m, P, batch, ni, nw)
        assert WORD not in grads
        with torch.no_grad():
            total = opt.step(P, grads)
        assert float(total) > a.max_grad_norm                         # the clip is active
    for n, ref in P.items():
        if n.endswith('linear_keys.bias') or n not in got:
            continue
        diff = (got[n] - ref).abs()
        bad = diff > 1e-4 * float(ref.abs().max())
        assert float(bad.float().mean()) <= 1e-3 and (int(bad.sum()) == 0 or float(diff[bad].max()) <= 4.02 * a.lr), n
    assert torch.equal(got[WORD], sd[WORD])


@pytest.mark.parametrize('model_name', ['item_transformer', 'ZAM'])
def test_c2_row_sparse_and_lazy_exact(model_name, tmp_path):
    _, dense1 = _train(model_name, str(tmp_path), steps=1)
    m, sparse = _train(model_name, str(tmp_path), steps=1, row_sparse_adam=True)
    assert WORD not in m.touched_rows()
    for k in dense1:
        if not k.endswith('linear_keys.bias'):
            assert rel_err(sparse[k], dense1[k]) < 1e-4, k
    _, dense = _train(model_name, str(tmp_path))
    _, lazy = _train(model_name, str(tmp_path), lazy_exact_adam=True)
    for k in dense:
        if not k.endswith('linear_keys.bias'):
            assert rel_err(lazy[k], dense[k]) < 1e-4, k


def test_c2_deterministic_mode_is_bitwise_run_to_run(tmp_path):
    from prodsearch_amd import _lib
    lib = _lib.load()
    old = lib.ps_set_deterministic(1)
    try:
        for name in ('item_transformer', 'ZAM'):
            for qenc in ('fs', 'avg'):
                _, s1 = _train(name, str(tmp_path), query_encoder_name=qenc)
                _, s2 = _train(name, str(tmp_path), query_encoder_name=qenc)
                for k in s1:
                    assert torch.equal(s1[k], s2[k]), (name, qenc, k)
    finally:
        lib.ps_set_deterministic(old)


def test_c2_graph_replayed_step_equals_the_eager_step(tmp_path):
    """PS_GRAPHS=1 (capture on the second call, replays after) against the eager step, both deterministic.  ZAM: bitwise.
    TEM: the eager forward sums the loss in the fused forward's epilogue and the step API in its own launches (two
    association orders, test_gpu_parity.py::test_graph_replayed_step_is_bitwise_the_eager_step), so the parameters agree to
    the rounding of that sum."""
    code = r"""
import sys, json, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_gpu_pretrained import _train
from prodsearch_amd import _lib
out = {}
for name in ('item_transformer', 'ZAM'):
    m, sd = _train(name, %r, steps=4)
    out[name] = {k: v.view(torch.int32).long().sum().item() for k, v in sd.items()}
    out[name + '_sum'] = {k: v.double().sum().item() for k, v in sd.items()}
    out[name + '_abs'] = {k: v.double().abs().sum().item() for k, v in sd.items()}
print(json.dumps({'graphs': int(_lib.load().ps_graph_replay_enabled()), 'r': out}))
""" % (REPO, TESTS, str(tmp_path))
    out = {}
    for flag in ('0', '1'):
        env = dict(os.environ, PS_GRAPHS=flag, PS_DETERMINISTIC='1')
        r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, 'PS_GRAPHS=%s: exit %d\n%s' % (flag, r.returncode, r.stderr[-3000:])
        out[flag] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['0']['graphs'] == 0 and out['1']['graphs'] == 1
    r0, r1 = out['0']['r'], out['1']['r']
    assert r0['ZAM'] == r1['ZAM']
    assert r0['item_transformer'][WORD] == r1['item_transformer'][WORD]          # frozen: bitwise the file's table
    for k, v in r0['item_transformer_sum'].items():
        if not k.endswith('linear_keys.bias'):
            assert abs(v - r1['item_transformer_sum'][k]) <= 1e-6 * max(1.0, r0['item_transformer_abs'][k]), k


@pytest.mark.parametrize('model_name', ['item_transformer', 'ZAM'])
def test_c2_flipping_requires_grad_between_steps(model_name, tmp_path):
    """frozen -> trainable -> frozen: every step's gradients against the oracle in the matching mode; the optimizer
    re-plans (the table joins the update once it has a gradient, as torch.optim does for a parameter it holds)."""
    from prodsearch_amd import build_optim
    a, m, sd, wd = _setup(model_name, str(tmp_path))
    w = m.word_embeddings.weight
    opt = build_optim(a, m, None)
    _check_step(a, m, sd, 0, wd)
    assert w.grad is None
    opt.step()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    w.requires_grad_(True)
    _check_step(a, m, sd, 1, wd, trainable_words=True)
    assert w.grad is not None and float(w.grad.abs().sum()) > 0
    opt.step()                                   # (the optimizer was built without the table: it is not updated)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    w.requires_grad_(False)
    before = w.detach().clone()
    _check_step(a, m, sd, 2, wd)
    assert w.grad is None
    opt.step()
    assert torch.equal(w.detach(), before)


def test_trainer_end_to_end_with_checkpoint_reload(tmp_path):
    from prodsearch_amd import ItemTransformerRanker, AttentionEmbeddingRanker, corpus, default_args, synth, trainer
    from prodsearch_amd.pretrained import word_table
    data_path, inp = synth.write_corpus(str(tmp_path / 'corpus'), 21, n_users=60, n_products=80, n_words=200)
    for model_name in ('item_transformer', 'QEM', 'ZAM', 'AEM'):
        save = str(tmp_path / ('run_' + model_name))
        args = default_args(model_name=model_name, embedding_size=32, heads=4, ff_size=64, batch_size=32, neg_per_pos=5,
                            uprev_review_limit=5, subsampling_rate=1e-2, lr=0.01, max_train_epoch=2, steps_per_checkpoint=20,
                            has_valid=True, valid_candi_size=-1, valid_batch_size=24, data_dir=data_path, input_train_dir=inp,
                            save_dir=save, device='cuda', dropout=0.1)
        gd = corpus.GlobalProdSearchData(args, data_path, inp)
        emb = tmp_path / 'emb'
        if not emb.exists():
            emb.mkdir()
            pretrain_util.write_word_emb(str(emb / 'word_emb.txt.gz'), gd.words, 32, seed=4, n_extra=9)
        args.pretrain_emb_dir = str(emb)
        table = torch.from_numpy(word_table(str(emb), gd.words, gd.vocab_size, 32))
        np.random.seed(5)
        mrr, p1 = trainer.train(args)
        assert 0.0 < mrr <= 1.0 and 0.0 <= p1 <= 1.0
        ckpts = sorted(f for f in os.listdir(save) if f.endswith('.ckpt'))
        assert ckpts
        ck = torch.load(os.path.join(save, ckpts[-1]), map_location='cpu', weights_only=False)
        assert torch.equal(ck['model'][WORD], table)                   # never updated
        model, optim = trainer.create_model(args, gd, corpus.ProdSearchData(args, inp, 'train', gd),
                                            os.path.join(save, ckpts[-1]))
        assert isinstance(model, AttentionEmbeddingRanker if model_name in ('ZAM', 'AEM') else ItemTransformerRanker)
        assert not model.word_embeddings.weight.requires_grad
        assert list(model.state_dict()) == list(ck['model'])
        for k, v in model.state_dict().items():
            assert torch.equal(v.cpu(), ck['model'][k]), k
        assert not any(p is model.word_embeddings.weight for p in optim.params)
