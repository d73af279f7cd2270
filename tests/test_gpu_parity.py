"""GPU parity: the HIP path (through the C ABI) against the golden vectors of the
reference and, stage by stage, against the oracle.  Run on an MI355X with -m gpu.

Tolerances (north_star): index work bit-exact; fp32 scores / loss within 1e-4
relative.  Gradients and post-Adam parameters are compared in max-norm relative
to the tensor's largest entry (fp32 atomics reassociate sums).
"""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import CASES, Golden, rel_err

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
STAGE_TOL = 2e-4
GRAD_TOL = 5e-4


def _model(g, training=True):
    from prodsearch_amd import ItemTransformerRanker
    torch.manual_seed(0)
    m = ItemTransformerRanker(g.args, 'cuda', g.V, g.P, None, word_dists=g.word_dists)
    missing = m.load_state_dict(g.params(), strict=False)
    assert [k for k in missing.missing_keys if not k.endswith('pos_emb.pe')] == []
    m.train(training)
    return m


def _oracle_keep(g, step=0):
    from oracle import tem as otem
    P = g.params()
    ni, nw = g.negs(step)
    keep = {}
    with torch.no_grad():
        if g.args.model_name == 'QEM':
            out = otem.qem_forward(P, g.args, g.batch(), ni, nw, g.V, g.P, keep=keep)
        elif g.args.dropout > 0:
            out = otem.tem_forward(P, g.args, g.batch(), ni, nw, g.V, g.P, replicate=True,
                                   drop=g.dropout(step), keep=keep)
        else:
            out = otem.tem_forward(P, g.args, g.batch(), ni, nw, g.V, g.P, keep=keep)
    return out, keep


# ------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize('M,N,K', [(64, 64, 32), (70, 132, 96), (384, 128, 128), (8064, 512, 128),
                                   (33, 128, 512), (1, 32, 32), (132, 68, 100), (200, 260, 2048)])
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('x3', [-1, 0, 1, 2, 3])
def test_mfma_gemm_layouts(M, N, K, ta, tb, x3, x3_restore):
    """x3 = -1: the form the launch takes by itself (fp32 MFMA at these sizes); 0 / 1 / 2: the bf16x3 form (three-way exact bf16
    split, six bf16 MFMAs per product step) forced with 64x64 / 128x64 / 128x128 tiles, 3: its direct-to-LDS form (gemm_x3d_kernel, 128x128; shapes with a ragged reduction
    tail fall back to 128x64) — same tolerance against fp64."""
    from prodsearch_amd import _lib
    lib = _lib.load()
    lib.ps_gemm_x3_config(1, x3)
    if ta and M % 4:
        pytest.skip('ta needs M % 4 == 0')
    if tb and N % 4:
        pytest.skip('tb needs N % 4 == 0')
    if not ta and K % 4:
        pytest.skip('K % 4')
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K, generator=gen)          # asymmetric data catches transposed C writes
    Bm = torch.randn(K, N, generator=gen)
    bias = torch.randn(N, generator=gen)
    ref = (A.double() @ Bm.double() + bias.double()) * 0.5
    Ad = (A.t().contiguous() if ta else A.contiguous()).cuda()          # ta: stored [K][M]
    Bd = (Bm.contiguous() if tb else Bm.t().contiguous()).cuda()        # tb=0: stored [N][K]
    Cd = torch.zeros(M, N, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.ps_gemm_f32(Ad.data_ptr(), M if ta else K, ta, Bd.data_ptr(), N if tb else K, tb, Cd.data_ptr(), N,
                         M, N, K, bias.cuda().data_ptr(), 0.5, 0, st)
    _lib.check(rc, 'ps_gemm_f32')
    torch.cuda.synchronize()
    assert rel_err(Cd.cpu(), ref.float()) < 2e-6
    # atomic split-K accumulate into a pre-filled C (weight-gradient form)
    C2 = torch.ones(M, N, device='cuda')
    rc = lib.ps_gemm_f32(Ad.data_ptr(), M if ta else K, ta, Bd.data_ptr(), N if tb else K, tb, C2.data_ptr(), N,
                         M, N, K, None, 1.0, 2, st)
    _lib.check(rc, 'ps_gemm_f32')
    torch.cuda.synchronize()
    assert rel_err(C2.cpu(), (A.double() @ Bm.double() + 1).float()) < 2e-6


def test_wide_products_take_the_bf16x3_form_and_match_fp64(x3_restore):
    """The d = 256 shard's linears (21,504 rows) are picked up by the size rule: forward, dX and weight-gradient layouts
    against fp64, and against the fp32-MFMA form of the same launch (both within the same bound of the exact product)."""
    from prodsearch_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(5)
    for (M, N, K, ta, tb, acc) in [(21504, 256, 256, 0, 0, 0), (21504, 256, 1024, 0, 1, 0), (1024, 512, 8192, 1, 1, 2)]:
        A = torch.randn(M, K, generator=gen)
        Bm = torch.randn(K, N, generator=gen) * 0.1
        Ad = (A.t().contiguous() if ta else A.contiguous()).cuda()
        Bd = (Bm.contiguous() if tb else Bm.t().contiguous()).cuda()
        ref = (A.double() @ Bm.double())
        mag = (A.double().abs() @ Bm.double().abs())
        out = []
        for mode in (1, 0):
            lib.ps_gemm_x3_config(mode, -1)
            C = torch.zeros(M, N, device='cuda')
            _lib.check(lib.ps_gemm_f32(Ad.data_ptr(), M if ta else K, ta, Bd.data_ptr(), N if tb else K, tb, C.data_ptr(), N,
                                       M, N, K, None, 1.0, acc, st), 'ps_gemm_f32')
            torch.cuda.synchronize()
            out.append(C.cpu().double())
        e3, e1 = float(((out[0] - ref).abs() / mag).max()), float(((out[1] - ref).abs() / mag).max())
        assert e3 < 6e-7 and e1 < 6e-7, (M, N, K, e3, e1)          # |error| / sum |a b|: a few fp32 ulps, either form
        assert not torch.equal(out[0], out[1])                     # (the two forms really are different kernels)


# ---------------------------------------------------------------------- forward
@pytest.mark.parametrize('case', CASES)
def test_forward_loss_matches_reference(case):
    g = Golden(case)
    m = _model(g)
    ni, nw = g.negs(0)
    with torch.no_grad():
        loss = m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    assert rel_err(loss.cpu(), g.tensor('loss_0')) < LOSS_TOL
    assert abs(m.ps_loss - float(g.z['ps_loss_0'])) < LOSS_TOL * abs(float(g.z['ps_loss_0']))
    assert abs(m.item_loss - float(g.z['item_loss_0'])) < LOSS_TOL * abs(float(g.z['item_loss_0']))


@pytest.mark.parametrize('case', CASES)
def test_forward_stages_match_oracle(case):
    g = Golden(case)
    a = g.args
    m = _model(g)
    ni, nw = g.negs(0)
    with torch.no_grad():
        m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    plan = next(iter(m._plans.values()))
    _, keep = _oracle_keep(g)
    B, K, W, d = g.B, g.K, g.W, a.embedding_size
    R, S = plan.layout.R, plan.layout.S
    view = lambda n, *shape: m.workspace_view(plan, n, shape).cpu()
    assert R == (K + 1 if (a.dropout > 0 and a.model_name == 'item_transformer') else 1)
    assert rel_err(view('query_emb', B, d), g.tensor('query_emb')) < STAGE_TOL      # vs reference
    assert rel_err(view('query_emb', B, d), keep['query_emb']) < STAGE_TOL
    if a.model_name == 'item_transformer':
        assert rel_err(view('x', B, S, d), keep['x']) < STAGE_TOL
        lk = keep['layer%d' % (a.inter_layers - 1)]
        qpos = S - 1 if a.use_item_pos else 0
        if a.inter_layers == 1:
            # K / V exist for the valid key positions only (the query column and the non-pad history items): the
            # projection runs over the batch's row list and the attention kernels read masked positions as zeros
            live = torch.cat([torch.ones(B, 1, dtype=torch.bool), g.batch().u_item_idxs != g.P], 1)
            assert rel_err(view('kp', B, S, d)[live], lk['K'][live]) < STAGE_TOL
            assert rel_err(view('vp', B, S, d)[live], lk['V'][live]) < STAGE_TOL
            assert rel_err(view('qp', B, d), lk['Qs'][:, qpos]) < STAGE_TOL
            assert rel_err(view('attn', B, a.heads, S), lk['attn'][:, :, qpos]) < STAGE_TOL
        if R == 1:
            assert rel_err(view('ctx', B, d), lk['ctx'][:, qpos]) < STAGE_TOL
            assert rel_err(view('y1', B, d), lk['y1'][:, qpos]) < STAGE_TOL
            assert rel_err(view('ln1', B, d), lk['ln1'][:, qpos]) < STAGE_TOL
            assert rel_err(view('a1', B, a.ff_size), lk['a1'][:, qpos]) < STAGE_TOL
            assert rel_err(view('y2', B, d), lk['y2'][:, qpos]) < STAGE_TOL
        # replica j = 0 is the positive encode (the only one the oracle keeps per stage)
        enc = view('enc', B, R, d)[:, 0]
        assert rel_err(enc, keep['enc']) < STAGE_TOL
        if g.has('enc_full'):
            assert rel_err(enc, g.tensor('enc_full')[:, qpos]) < STAGE_TOL             # vs reference
    scores = view('item_scores', B, K + 1)
    assert rel_err(scores, g.tensor('prod_scores')) < LOSS_TOL                        # vs reference
    assert rel_err(view('word_scores', B, W, K + 1), g.tensor('word_scores')) < LOSS_TOL


# --------------------------------------------------------------------- backward
def _table_like(t):
    return t.dim() == 2 and t.shape[0] > 256


@pytest.mark.parametrize('case', CASES)
def test_gradients_match_reference(case):
    g = Golden(case)
    m = _model(g)
    ni, nw = g.negs(0)
    loss = m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    none = sorted(n for n, p in m.named_parameters() if p.grad is None)
    assert none == sorted(g.meta['none_grads'])
    for n, p in m.named_parameters():
        if p.grad is None:
            continue
        got, ref = p.grad.cpu(), g.tensor('grad_' + n)
        if n.endswith('linear_keys.bias'):      # exactly 0 in real arithmetic: rounding noise on both sides
            scale = float(g.tensor('grad_' + n.replace('.bias', '.weight')).abs().max())
            assert float(got.abs().max()) < 1e-4 * scale, n
            continue
        assert rel_err(got, ref) < GRAD_TOL, n
        if _table_like(ref):                    # bit-exact index work: the set of touched rows
            assert torch.equal(got.ne(0).any(1), ref.ne(0).any(1)), n


@pytest.mark.parametrize('case', [c for c in CASES if c.startswith('tem')])
def test_gradients_match_reference_fused_backward(case):
    """The fused per-replica backward kernel (mlp_fused.hip) normally starts at 1024 replica rows; forced on here so
    the golden cases (<= 672 rows) check it against the reference's gradients as well."""
    from prodsearch_amd import _lib
    old = _lib.load().ps_set_fuse_bwd_min(1)
    try:
        test_gradients_match_reference(case)
        test_train_steps_match_reference(case)
    finally:
        _lib.load().ps_set_fuse_bwd_min(old)


@pytest.mark.parametrize('case', CASES)
def test_train_steps_match_reference(case):
    """trainer.py:74-79 call order for every golden step: losses, lr and post-Adam parameters."""
    from prodsearch_amd import build_optim
    g = Golden(case)
    m = _model(g)
    init = {k: v.clone() for k, v in g.params().items()}
    optim = build_optim(g.args, m, None)
    b = g.batch().to('cuda')
    for step in range(g.steps):
        ni, nw = g.negs(step)
        loss = m(b, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        m.zero_grad()
        loss.backward()
        optim.step()
        assert rel_err(loss.detach().cpu(), g.tensor('loss_%d' % step)) < 2 * LOSS_TOL, step
        assert abs(optim.learning_rate - float(g.z['lr_%d' % step])) < 1e-9
        if step in (0, g.steps - 1):
            sd = m.state_dict()
            for n, _ in m.named_parameters():
                ref = g.tensor('param%d_%s' % (step, n), base=init[n])
                got = sd[n].cpu()
                if n.endswith('linear_keys.bias'):     # noise-driven +-lr steps (see test_oracle_golden)
                    assert float((got - ref).abs().max()) <= 2.01 * g.args.lr * (step + 1), (step, n)
                    continue
                if _table_like(ref):                   # rows Adam moved are exactly the touched rows
                    assert torch.equal((got != init[n]).any(1), (ref != init[n]).any(1)), (step, n)
                # Adam normalises: |delta| <= lr per step wherever a gradient is rounding noise
                assert float((got - ref).abs().max()) < 2e-3 * float(ref.abs().max()) + 0.02 * g.args.lr, (step, n)
                # a gradient element of the order of Adam's eps (1e-9) turns fp32 rounding noise into a few % of
                # lr (measured up to 5.4 % on one element of f_W); a wrong sign or a missing term gives >= 1
                # ... and ISOLATED elements whose gradient is itself of the order of eps after the clip (|g| ~ 3e-8: one element
                # of linear_keys.weight in tem_c2s_drop) up to ~0.2 lr — the reference against its own CPU restatement differs
                # by 0.1 lr there (tests/test_oracle_golden.py).  At most 2 in 10^4 elements, each bounded by lr per step.
                dd = ((got - init[n]) - (ref - init[n])).abs()
                bad = dd > 1e-1 * float((ref - init[n]).abs().max())
                assert float(bad.float().mean()) <= 2e-4 and (int(bad.sum()) == 0 or
                                                             float(dd[bad].max()) <= 1.01 * g.args.lr * (step + 1)), (step, n)


# ------------------------------------------------------------------------- eval
@pytest.mark.parametrize('case', CASES)
def test_eval_scores_and_ranklist(case):
    from oracle import tem as otem
    g = Golden(case)
    m = _model(g, training=False)
    b = g.batch()
    with torch.no_grad():
        s = m.test(b.to('cuda')).cpu()
    ref = g.tensor('test_scores')
    assert s.shape == ref.shape
    assert rel_err(s, ref) < LOSS_TOL
    order, mrr, p1 = otem.rank_metrics(s, b.candi_prod_idxs, b.target_prod_idxs)
    ref_order = g.z['test_ranklist']
    # ranklist: identical wherever the reference's adjacent score gap exceeds the fp tolerance
    rs = np.take_along_axis(ref.numpy(), ref_order, axis=1)
    gap_ok = np.abs(np.diff(rs, axis=1)) > 2 * LOSS_TOL * np.abs(rs).max()
    same = order == ref_order
    assert (same[:, :-1] | ~gap_ok).all() and (same[:, 1:] | ~gap_ok).all()
    assert abs(mrr - float(g.z['test_mrr'])) < 1e-6 and abs(p1 - float(g.z['test_p1'])) < 1e-6


# ------------------------------------------------------------- dropout replicas
def test_dropout_replicas_bitwise_reproducible():
    g = Golden('tem_c1_drop')
    losses = []
    for _ in range(2):
        m = _model(g)
        ni, nw = g.negs(0)
        with torch.no_grad():
            losses.append(float(m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())))
    assert losses[0] == losses[1]


def test_sampler_distribution_and_ranges():
    """Device sampler = stand-in for the two torch.multinomial draws: ranges bit-exact
    (items in [0,P), words never the pad), frequencies match word_dists."""
    g = Golden('tem_c2s')
    m = _model(g)
    plan = m._plan_for(g.batch().to('cuda'), eval_mode=False)
    counts = torch.zeros(g.V, dtype=torch.float64)
    n = 0
    for step in range(200):
        plan.desc.step = step + 1
        ni, nw = m.sample_negatives(plan)
        assert int(ni.min()) >= 0 and int(ni.max()) < g.P
        assert int(nw.min()) >= 0 and int(nw.max()) < g.V - 1
        counts += torch.bincount(nw.flatten().cpu(), minlength=g.V).double()
        n += nw.numel()
    freq = counts / n
    wd = torch.from_numpy(g.word_dists)
    assert float((freq - wd).abs().max()) < 5 * float((wd.max() / n) ** 0.5) + 1e-3


def test_scaled_loss_takes_the_autograd_path_and_matches_the_direct_one():
    """loss.backward() short-circuits the engine; (2*loss).backward() must go through autograd and give 2x the grads."""
    g = Golden('tem_c1')
    ni, nw = g.negs(0)
    grads = []
    for scale in (None, 2.0):
        m = _model(g)
        loss = m(g.batch().to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
        assert loss.requires_grad and loss.grad_fn is not None
        m.zero_grad()
        (loss if scale is None else loss * scale).backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    for n in grads[0]:
        if n.endswith('linear_keys.bias'):
            continue
        assert rel_err(grads[1][n], 2.0 * grads[0][n]) < 1e-5, n


def test_graph_replayed_step_is_bitwise_the_eager_step():
    """PS_GRAPHS=1 (ps_tem_forward_step / ps_tem_backward_step: capture on the second call, replay afterwards, inputs
    through the staging prologue) must reproduce the eager step exactly: same kernels, same order."""
    import subprocess, sys, os, json
    code = r"""
import sys, json, faulthandler, torch
faulthandler.enable()                      # a crash of the child names the Python line it happened under
sys.path.insert(0, %r); sys.path.insert(0, %r)
from golden_util import Golden
from prodsearch_amd import ItemTransformerRanker, build_optim, _lib
g = Golden('tem_c2s_drop')
m = ItemTransformerRanker(g.args, 'cuda', g.V, g.P, None, word_dists=g.word_dists)
m.load_state_dict(g.params(), strict=False); m.train()
opt = build_optim(g.args, m, None)
b = g.batch().to('cuda'); losses = []
for step in range(5):                      # eager, capture, then three replays (two with device-drawn negatives)
    if step < 3:
        ni, nw = g.negs(step %% g.steps)
        loss = m(b, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    else:
        loss = m(b)
    m.zero_grad(); loss.backward(); opt.step(); losses.append(float(loss))
sd = m.state_dict()
print(json.dumps({'graphs': int(_lib.load().ps_graph_replay_enabled()), 'losses': losses,
                  'sum': {k: float(v.double().sum()) for k, v in sd.items()},
                  'abs': {k: float(v.double().abs().sum()) for k, v in sd.items()}}))
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ('0', '1'):
        env = dict(os.environ, PS_GRAPHS=flag)
        r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, 'PS_GRAPHS=%s: exit %d\n%s\nstdout: %s' % (flag, r.returncode, r.stderr[-3000:], r.stdout[-500:])
        out[flag] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['0']['graphs'] == 0 and out['1']['graphs'] == 1
    # same parameters, same encoder kernels; the loss itself is summed by the fused forward's epilogue in the eager step and by the
    # stand-alone gather+score + loss launches in the step API (ps_tem_forward_step never folds): two association orders of the same
    # terms — equal to an fp32 ulp or two, and bitwise only by luck (it was, until round 4's GELU form moved the last bits)
    assert abs(out['0']['losses'][0] - out['1']['losses'][0]) <= 4e-7 * abs(out['0']['losses'][0])
    for a, b in zip(out['0']['losses'][:3], out['1']['losses'][:3]):  # later steps see atomically-summed table grads
        assert abs(a - b) <= 1e-5 * abs(a)
    for k in out['0']['sum']:
        if k.endswith('linear_keys.bias'):
            continue
        # atomics reassociate table sums run to run; everything else is bitwise
        assert abs(out['0']['sum'][k] - out['1']['sum'][k]) <= 1e-6 * max(1.0, out['0']['abs'][k]), k


def test_folded_sampling_draws_equal_the_standalone_sampler():
    """The negatives drawn inside the forward's first launch are the ones ps_sample_negatives draws for the same step."""
    from prodsearch_amd import _lib
    if _lib.load().ps_graph_replay_enabled():
        pytest.skip('PS_GRAPHS=1 draws the negatives in the staging prologue (covered by the graph-vs-eager test)')
    g = Golden('tem_c1')
    m = _model(g)
    loss = m(g.batch().to('cuda'))                          # no injected negatives: drawn in the embed launch
    plan = next(iter(m._plans.values()))
    got_i, got_w = plan.neg_items.clone(), plan.neg_words.clone()
    ref_i, ref_w = m.sample_negatives(plan)                 # same desc.step, standalone kernel
    torch.cuda.synchronize()
    assert torch.equal(got_i, ref_i) and torch.equal(got_w, ref_w)
    assert int(got_i.min()) >= 0 and int(got_i.max()) < g.P and int(got_w.max()) < g.V - 1
    m.zero_grad()
    loss.backward()                                         # and the backward reads them from the plan
    assert m.product_emb.weight.grad[got_i.flatten().unique()].abs().sum() > 0


def test_backward_of_a_superseded_forward_is_refused():
    """One workspace per batch shape: forward A, forward B, then A.backward() would silently differentiate B's
    activations and negatives — every backward path (the direct one, autograd with a scaled loss) must raise instead."""
    g = Golden('tem_c1')
    m = _model(g)
    b = g.batch().to('cuda')
    ni, nw = g.negs(0)
    loss_a = m(b, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    scaled_a = loss_a * 2.0
    loss_b = m(b, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    m.zero_grad()
    with pytest.raises(RuntimeError, match='no longer'):
        scaled_a.backward()                                  # autograd path (_RankLossFn.backward)
    with pytest.raises(RuntimeError, match='no longer'):
        loss_a.backward()                                    # direct path (_LossTensor.backward)
    loss_b.backward()                                        # the latest forward is fine
    torch.cuda.synchronize()
    assert m.word_embeddings.weight.grad is not None
