"""Review transformer on pretrained / fixed paragraph vectors on an MI355X, through the C ABI (``PsRtmDesc.frozen_mask`` /
``no_pv_drop``, NULL table gradients, the frozen forms of csrc/rtm_embed_bwd.hip and rtm_score.hip):

* every ``rtmpre_*`` fixture of the reference (tests/golden/make_golden_rtm_pretrained.py): loss terms, ``test()`` scores, every
  gradient, which are None, the frozen tables bitwise after three clipped Adam steps, the stepped parameters;
* oracle-driven shapes with the product's Philox masks (oracle.rtm with frozen leaves): the smallest shapes at which each frozen
  form can go wrong — long reviews, ragged four-review groups, all-padding sequences and groups, d = 64 / 128 / 256, one and two
  layers, the query-only grid, user / item rows frozen and trainable, pv with frozen reviews and trainable words, fs, and the
  smallest batch whose plan has the fused last-layer kernels and the side stream;
* the same batch and seed trainable against frozen; deterministic mode bitwise (a vocabulary above the histogram index's limit
  included); flipping ``requires_grad`` between steps; the trainer end to end with a pretrained directory and ``fix_emb``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pretrain_rtm_util
from golden_util import rel_err
from golden_util_rtmpre import REVIEW_TABLE, RTMPRE_CASES, RtmPreGolden

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-4, 5e-4
TABLES = ('word_embeddings.weight', REVIEW_TABLE, 'user_emb.weight', 'product_emb.weight')


# ------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize('case', RTMPRE_CASES)
def test_fixture_loss_grads_tables_and_three_clipped_steps(case):
    from prodsearch_amd import build_optim
    g = RtmPreGolden(case)
    a = g.args
    m = g.build('cuda')
    missing, unexpected = m.load_state_dict(g.generated(), strict=False)
    assert not unexpected
    named = dict(m.named_parameters())
    assert list(named) == g.meta['param_names'] and list(m.state_dict().keys()) == g.meta['state_dict_keys']
    frozen = {n: named[n].detach().clone() for n in g.meta['frozen']}
    for n in g.meta['pretrained']:
        assert torch.equal(frozen[n].cpu(), torch.from_numpy(g.z['table_' + n])), n
    # eval on the initial weights (trainer.py:193,201)
    m.eval()
    with torch.no_grad():
        m.get_review_embeddings()
        assert abs(float(m.review_embeddings.double().sum().cpu()) - float(g.z['test_review_embeddings_sum'])) < 1e-2
        s = m.test(g.test_batch().to('cuda')).cpu()
    m.clear_review_embbeddings()
    assert (m.review_embeddings is not None) == bool(a.fix_emb)
    assert rel_err(s, g.tensor('test_scores')) < LOSS_TOL
    m.train()
    opt = build_optim(a, m, None)
    assert opt._names == g.meta['optim_params']
    b = g.batch().to('cuda')
    init = {n: p.detach().cpu().clone() for n, p in named.items()}
    terms, run_forward = [], m._run_forward

    def tapped(*args):             # {loss, ps loss, pv loss}: the C ABI returns the three, the module API hands on the first
        plan, loss3 = run_forward(*args)
        terms.append(loss3)
        return plan, loss3
    m._run_forward = tapped
    for step in range(g.steps):
        tpv = g.steps_train_pv[step]
        nw = g.neg_words(step)
        loss = m(b, train_pv=tpv, neg_word_idxs=None if nw is None else nw.cuda())
        m.zero_grad()
        loss.backward()
        l3 = terms[-1].cpu()
        for n in frozen:
            assert named[n].grad is None, n
        ref = g.tensor('loss_%d' % step)
        assert rel_err(loss.detach().cpu(), ref) < LOSS_TOL, (step, float(loss), float(ref))
        print('%s step %d: loss %.6f ps %.6f pv %.6f (reference %.6f %.6f %.6f)'
              % (case, step, l3[0], l3[1], l3[2], ref, g.tensor('ps_loss_%d' % step), g.tensor('pv_loss_%d' % step)))
        assert rel_err(l3[1], g.tensor('ps_loss_%d' % step)) < LOSS_TOL, step
        if tpv:
            assert rel_err(l3[2], g.tensor('pv_loss_%d' % step)) < LOSS_TOL, step
        if step in (0, 1):
            for n, p in named.items():
                assert (p.grad is None) == (n in g.meta['none_grads_%d' % step]), (step, n)
                if p.grad is None or n.endswith('linear_keys.bias'):
                    continue
                want = g.tensor('grad%d_%s' % (step, n))
                if step == 1 and float(want.abs().max()) == 0.0:
                    continue
                got = p.grad.cpu()
                assert rel_err(got, want) < GRAD_TOL, (step, n, rel_err(got, want))
        opt.step()
        if step in (0, g.steps - 1):
            for n in g.meta['optim_params']:
                ref = g.tensor('param%d_%s' % (step, n), base=init[n])
                diff = (named[n].detach().cpu() - ref).abs()
                if n.endswith('linear_keys.bias'):
                    assert float(diff.max()) <= 2.01 * a.lr * (step + 1), (step, n)
                    continue
                bad = diff > 1e-4 * float(ref.abs().max())
                assert float(bad.float().mean()) <= 1e-3 and (int(bad.sum()) == 0 or
                                                             float(diff[bad].max()) <= 2.01 * a.lr * (step + 1)), (step, n)
    for n, t in frozen.items():
        assert torch.equal(named[n].detach(), t), n                                  # bitwise the loaded table


# ------------------------------------------------------------------------------------------------ oracle-driven shapes
V_, RC_ = 1500, 900


def _setup(encoder, d=128, heads=8, layers=1, K=3, WL=40, u_lim=3, i_lim=4, dropout=0.1, corrupt=0.5, seg=True, ui=False,
           frozen=('word_embeddings.weight',), fix_emb=False, V=V_, RC=RC_, ff=None, seed=7):
    """A ProductRanker whose ``frozen`` tables have ``requires_grad`` False (what from_pretrained / fix_emb leave behind; the
    file loaders are the fixture tests' matter), random weights, and its state dict on the host."""
    from prodsearch_amd import PretrainedProductRanker, default_args, synth
    a = default_args(model_name='review_transformer', review_encoder_name=encoder, embedding_size=d, heads=heads,
                     ff_size=ff or 2 * d, inter_layers=layers, neg_per_pos=K, dropout=dropout,
                     corrupt_rate=corrupt if encoder == 'pvc' else 0.0, lr=0.002, max_grad_norm=1.0, review_word_limit=WL,
                     uprev_review_limit=u_lim, iprev_review_limit=i_lim, use_seg_emb=seg, use_user_emb=ui, use_item_emb=ui,
                     pv_window_size=2, fix_emb=fix_emb, seed=seed)
    wd = synth.make_word_dists(V)
    rng = synth.rng_for(3)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
    lens = torch.from_numpy(rng.integers(1, WL + 1, size=RC))
    rw[torch.arange(WL)[None, :] >= lens[:, None]] = V - 1
    rw[-1] = V - 1
    torch.manual_seed(seed)
    m = PretrainedProductRanker(a, 'cuda', V, RC, 50, 60, rw, None, word_dists=wd)
    named = dict(m.named_parameters())
    for n in frozen:
        named['review_embeddings' if (fix_emb and n == REVIEW_TABLE) else n].requires_grad_(False)
    m.train()
    return a, m, rw, wd


def _state(m):
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sd.pop('review_embeddings', None)                    # (fix_emb: the model-level name of the review table)
    return sd


def _batch(a, rw, wd, seed, B, train_pv, V=V_, RC=RC_):
    from prodsearch_amd import rtm_data, synth
    enc = 'pv' if a.fix_emb else a.review_encoder_name
    K, R, W = a.neg_per_pos, a.uprev_review_limit + a.iprev_review_limit, a.pv_window_size
    bt = rtm_data.make_rtm_batch(seed, B, K, RC, V, rw, Q=5, u_lim=a.uprev_review_limit, i_lim=a.iprev_review_limit, W=W,
                                 train_pv=train_pv, encoder=enc, word_dists=wd, user_size=60 if a.use_user_emb else None,
                                 product_size=50 if a.use_item_emb else None)
    nw = torch.from_numpy(synth.rng_for(seed + 1).choice(V, size=(B * R, W * K), p=wd).astype(np.int64)) if train_pv else None
    return bt, nw


def _oracle(a, m, sd, frozen, bt, nw, train_pv, V=V_, RC=RC_):
    """Loss and gradients of oracle.rtm at ``sd`` with the masks of the step the model just ran (m._fwd_step)."""
    import copy
    from oracle import rtm as ortm
    from oracle.philox import RtmPhiloxDropout
    oa = copy.copy(a)
    if a.fix_emb and a.review_encoder_name == 'pvc':
        oa.review_encoder_name = 'pv'
    pvc = oa.review_encoder_name == 'pvc'
    B, R = bt.pos_prod_ridxs.shape
    drop = tok = None
    if a.dropout > 0 or (pvc and a.corrupt_rate > 0):
        gen = RtmPhiloxDropout(a.dropout, m._seed, m._fwd_step, B, a.neg_per_pos, a.heads, R + 1, a.inter_layers,
                               a.corrupt_rate if pvc else 0.0)
        if a.dropout > 0:
            drop = (lambda x, kind, call: x if kind == 'rev_pv' else gen(x, kind, call)) if a.fix_emb else gen
        tok = gen.tok if (pvc and a.corrupt_rate > 0) else None
    P = {k: (v.clone().requires_grad_(k not in frozen) if (v.dtype.is_floating_point and not k.endswith('pos_emb.pe')) else v)
         for k, v in sd.items()}
    loss, _, _ = ortm.rtm_forward(P, oa, bt, nw, V, RC, training=True, train_pv=train_pv, drop=drop, tok_drop=tok)
    names = [k for k, v in P.items() if torch.is_tensor(v) and v.requires_grad]
    gs = torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)
    pad = {'word_embeddings.weight': V - 1, 'seg_embeddings.weight': 3, REVIEW_TABLE: RC - 1, 'user_emb.weight': 60,
           'product_emb.weight': 50}
    grads = {}
    for k, gr in zip(names, gs):
        if gr is not None and k in pad:
            gr = gr.clone()
            gr[pad[k]] = 0
        grads[k] = gr
    return loss.detach(), grads


def _check_step(a, m, rw, wd, seed, B, train_pv, frozen, V=V_, RC=RC_, min_checked=12):
    """One training forward + backward through the module API against the oracle: loss, every gradient, None where frozen."""
    sd = _state(m)
    bt, nw = _batch(a, rw, wd, seed, B, train_pv, V, RC)
    loss = m(bt.to('cuda'), train_pv=train_pv, neg_word_idxs=None if nw is None else nw.cuda())
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    oloss, grads = _oracle(a, m, sd, set(frozen), bt, nw, train_pv, V, RC)
    assert rel_err(loss.detach().cpu(), oloss) < LOSS_TOL, (float(loss), float(oloss))
    got = {(REVIEW_TABLE if n == 'review_embeddings' else n): p for n, p in m.named_parameters()}
    checked = 0
    for n in TABLES:
        if n in got:
            assert (got[n].grad is None) == (n in frozen), n
    for k, gr in grads.items():
        if k not in got or k.endswith('linear_keys.bias'):
            continue
        if gr is None or float(gr.abs().max()) == 0.0:
            assert got[k].grad is None or float(got[k].grad.abs().max()) == 0.0, k
            continue
        assert got[k].grad is not None, k
        e = rel_err(got[k].grad.cpu(), gr)
        assert e < GRAD_TOL, (k, e)
        if gr.dim() == 2 and gr.shape[0] > 256:                       # tables: the same rows touched
            assert torch.equal(got[k].grad.cpu().ne(0).any(1), gr.ne(0).any(1)), k
        checked += 1
    assert checked >= min_checked, checked
    return bt


def _plan_of(m):
    from prodsearch_amd import _lib
    plan = [p for k, p in m._plans.items() if k[0] != 'eval'][-1]
    out = _lib.PsRtmBwdPlan()
    _lib.check(_lib.load().ps_rtm_backward_plan(C.byref(plan.desc), C.byref(out)), 'ps_rtm_backward_plan')
    return out


def test_pvc_frozen_long_reviews_ragged_groups_and_padding():
    """d = 128, B = 5, K = 3, R = 7, WL = 40: reviews of more than 32 words, B*R = 35 and B*K*R = 105 review rows (no multiple of
    a four-review group), negatives without any review (whole groups of padding), with and without the PV loss."""
    from prodsearch_amd import _lib
    frozen = ('word_embeddings.weight',)
    a, m, rw, wd = _setup('pvc', frozen=frozen)
    bt = _check_step(a, m, rw, wd, 21, 5, False, frozen)
    pad = bt.neg_prod_ridxs.eq(RC_ - 1)
    assert bool(pad.all(-1).any()) and bool(pad.reshape(-1)[:104].reshape(-1, 4).all(-1).any())
    assert int(bt.neg_prod_rword_idxs.ne(V_ - 1).sum(-1).max()) > 32
    p = _plan_of(m)
    assert (p.index, p.word_reduce, p.embed_form, p.slot_waves, p.query_scatter) == (0, 0, _lib.PS_RTM_EB_FROZEN, 1, 0)
    _check_step(a, m, rw, wd, 22, 5, True, frozen)                  # train_pv: the PV loss is in the loss, nothing takes its gradient
    assert _plan_of(m).pv_bwd == _lib.PS_RTM_PV_NONE


@pytest.mark.parametrize('d,heads,layers', [(64, 4, 1), (256, 8, 1), (128, 8, 2), (64, 4, 2)])
def test_pvc_frozen_widths_and_layers(d, heads, layers):
    frozen = ('word_embeddings.weight',)
    a, m, rw, wd = _setup('pvc', d=d, heads=heads, layers=layers, K=2, u_lim=2, i_lim=3, WL=24, frozen=frozen)
    _check_step(a, m, rw, wd, 23, 4, False, frozen, min_checked=12)


@pytest.mark.parametrize('encoder', ['pvc', 'avg'])
def test_query_only_grid(encoder):
    """No segment embedding, no user / item embedding, frozen words: the embed backward's grid is the query-position waves."""
    from prodsearch_amd import _lib
    frozen = ('word_embeddings.weight',)
    a, m, rw, wd = _setup(encoder, seg=False, frozen=frozen, K=2, u_lim=2, i_lim=3, WL=24)
    _check_step(a, m, rw, wd, 24, 4, False, frozen, min_checked=10)
    p = _plan_of(m)
    assert (p.embed_form, p.slot_waves) == (_lib.PS_RTM_EB_FROZEN, 0)
    assert m.seg_embeddings.weight.grad is None


@pytest.mark.parametrize('ui_frozen', [True, False])
@pytest.mark.parametrize('seg', [True, False])
def test_user_item_rows_frozen_and_trainable(ui_frozen, seg):
    from prodsearch_amd import _lib
    frozen = ('word_embeddings.weight',) + (('user_emb.weight', 'product_emb.weight') if ui_frozen else ())
    a, m, rw, wd = _setup('pvc', ui=True, seg=seg, frozen=frozen, K=2, u_lim=2, i_lim=3, WL=24)
    _check_step(a, m, rw, wd, 25, 6, False, frozen)
    p = _plan_of(m)
    assert (p.user_scatter, p.item_scatter) == ((0, 0) if ui_frozen else (1, 1))
    assert (p.embed_form, p.slot_waves) == (_lib.PS_RTM_EB_FROZEN, int(seg or not ui_frozen))
    if not ui_frozen:
        assert float(m.user_emb.weight.grad.abs().max()) > 0 and float(m.product_emb.weight.grad[50].abs().max()) == 0


def test_user_item_rows_frozen_beside_trainable_words():
    """Only the user / item tables frozen (pretrain_up_emb_dir alone): the trainable forms with NULL user / item gradients."""
    frozen = ('user_emb.weight', 'product_emb.weight')
    for enc, tpv in (('pvc', False), ('pv', True)):
        a, m, rw, wd = _setup(enc, ui=True, frozen=frozen, K=2, u_lim=2, i_lim=3, WL=24)
        _check_step(a, m, rw, wd, 26, 6, tpv, frozen)


@pytest.mark.parametrize('frozen,form,fix_emb', [
    ((REVIEW_TABLE,), 'WORDS', False), ((REVIEW_TABLE,), 'WORDS', True), (('word_embeddings.weight',), 'DVEC', False),
    (('word_embeddings.weight', REVIEW_TABLE), 'NONE', False), (('word_embeddings.weight', REVIEW_TABLE), 'NONE', True)])
def test_pv_partly_frozen_with_the_pv_loss(frozen, form, fix_emb):
    """pv with ``train_pv``: frozen reviews + trainable words (the PV backward's word rows only; fix_emb's shape, whose PV
    drop site is off), frozen words + trainable reviews (d vec only), both frozen (no PV backward).  Then a plain step."""
    from prodsearch_amd import _lib
    a, m, rw, wd = _setup('pv', frozen=frozen, fix_emb=fix_emb, K=2, u_lim=3, i_lim=4, dropout=0.2)
    _check_step(a, m, rw, wd, 27, 5, True, frozen)
    p = _plan_of(m)
    assert p.pv_bwd == getattr(_lib, 'PS_RTM_PV_' + form)
    assert p.embed_form == (_lib.PS_RTM_EB_FROZEN if REVIEW_TABLE in frozen else _lib.PS_RTM_EB_GENERAL)
    _check_step(a, m, rw, wd, 28, 5, False, frozen)


@pytest.mark.parametrize('d,heads', [(64, 4), (128, 8)])
def test_fs_frozen(d, heads):
    """fs: f_W trains straight from d x (rtm_fs_bwd_kernel + the weight gradient), the d raw product is gone."""
    from prodsearch_amd import _lib
    frozen = ('word_embeddings.weight',)
    a, m, rw, wd = _setup('fs', d=d, heads=heads, frozen=frozen, K=2, u_lim=2, i_lim=3, WL=36)
    _check_step(a, m, rw, wd, 29, 5, False, frozen)
    p = _plan_of(m)
    assert (p.fs_draw, p.embed_form) == (0, _lib.PS_RTM_EB_FROZEN)
    assert float(m.review_encoder.f_W.weight.grad.abs().max()) > 0


def _enc_plan(lib, nseq, R, a):
    from prodsearch_amd import _lib
    import enc_paths as ep
    t = _lib.PsTemDesc()
    t.B, t.K, t.L, t.Q, t.W, t.C = nseq, 0, R, 1, 0, 0
    t.d, t.H, t.F, t.n_layers = a.embedding_size, a.heads, a.ff_size, a.inter_layers
    t.product_size, t.vocab_size = 1, 2
    t.model, t.query_encoder = _lib.PS_MODEL_TEM, _lib.PS_QENC_AVG
    t.use_pos_emb, t.training, t.dropout, t.seed = int(a.use_pos_emb), 1, a.dropout, 666
    p = _lib.PsEncPath()
    _lib.check(lib.ps_tem_plan(t, None, 1, C.byref(p)), 'ps_tem_plan')
    return ep.path_dict(p)


def test_smallest_batch_with_the_fused_last_layer_and_the_side_stream():
    """The encoder plan (ps_tem_plan over the review transformer's B*(1+K) sequences) takes the fused last-layer backward from
    PS_FUSE_BWD_MIN = 1,024 rows (tests/enc_paths.py) with its K / V / Q weight gradients on the side stream: B = 256 at K = 3 is
    the smallest such batch, B = 255 is not.  The frozen backward forks no side stream of its own for an index; the encoder's
    still runs.  Asserted on what the step really launched (ps_enc_path_taken)."""
    import enc_paths as ep
    from prodsearch_amd import _lib
    lib = _lib.load()
    if not ep.default_switches():
        pytest.skip("the process runs under a plan switch")
    frozen = ('word_embeddings.weight',)
    a, m, rw, wd = _setup('pvc', frozen=frozen, K=3, u_lim=2, i_lim=3, WL=20, ff=256)
    R = 5
    small, big = _enc_plan(lib, 255 * 4, R, a), _enc_plan(lib, 256 * 4, R, a)
    assert (small['fwd_fuse_last'], small['bwd_fuse_last']) == (1, 0)
    assert (big['fwd_fuse_last'], big['bwd_fuse_last'], big['wg3_main']) == (1, 1, 0)
    _check_step(a, m, rw, wd, 30, 256, False, frozen)
    fwd, bwd = ep.taken(lib, _lib, 0), ep.taken(lib, _lib, 1)
    assert fwd['fwd_fuse_last'] == 1 and fwd['rowlist'] == big['rowlist']
    assert (bwd['bwd_fuse_last'], bwd['wg3_main'], bwd['listed']) == (1, 0, big['listed'])
    p = _plan_of(m)
    assert (p.index, p.side_fork, p.embed_form) == (0, 0, _lib.PS_RTM_EB_FROZEN)


# ------------------------------------------------------------------------------------------------ trainable against frozen
def _three_steps(encoder, frozen, train_pv, det=False, V=V_, d=64, heads=4, B=6, **kw):
    from prodsearch_amd import _lib, build_optim
    lib = _lib.load()
    old = lib.ps_set_deterministic(1 if det else 0)
    try:
        a, m, rw, wd = _setup(encoder, d=d, heads=heads, frozen=frozen, K=2, u_lim=2, i_lim=3, WL=24, V=V, **kw)
        init = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt = build_optim(a, m, None)
        g0 = None
        for s in range(3):
            bt, nw = _batch(a, rw, wd, 40 + s, B, train_pv, V=V)
            loss = m(bt.to('cuda'), train_pv=train_pv, neg_word_idxs=None if nw is None else nw.cuda())
            m.zero_grad()
            loss.backward()
            if s == 0:
                g0 = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
            opt.step()
        torch.cuda.synchronize()
        return init, g0, {n: p.detach().clone() for n, p in m.named_parameters()}
    finally:
        lib.ps_set_deterministic(old)


@pytest.mark.parametrize('encoder,table,train_pv', [('pvc', 'word_embeddings.weight', False), ('fs', 'word_embeddings.weight', False),
                                                    ('pv', REVIEW_TABLE, True)])
def test_same_batch_and_seed_trainable_against_frozen(encoder, table, train_pv):
    i0, gt, pt = _three_steps(encoder, (), train_pv)
    i1, gf, pf = _three_steps(encoder, (table,), train_pv)
    assert gf[table] is None and gt[table] is not None and float(gt[table].abs().max()) > 0
    for n in gt:
        assert torch.equal(i0[n], i1[n]), n
        if n == table or gt[n] is None or n.endswith('linear_keys.bias') or float(gt[n].abs().max()) == 0.0:
            continue
        assert gf[n] is not None and rel_err(gf[n], gt[n]) < GRAD_TOL, (n, rel_err(gf[n], gt[n]))
    assert torch.equal(pf[table], i1[table])                                   # frozen: bitwise unchanged after three steps
    assert not torch.equal(pt[table], i0[table])                               # trainable: it has moved
    assert int((pt[table] != i0[table]).any(1).sum()) > 10


# ------------------------------------------------------------------------------------------------ deterministic mode
@pytest.mark.parametrize('encoder,frozen,train_pv,kw', [
    ('pvc', ('word_embeddings.weight',), False, dict()),
    ('pvc', ('word_embeddings.weight',), False, dict(ui=True)),
    ('fs', ('word_embeddings.weight',), False, dict()),
    ('pv', (REVIEW_TABLE,), True, dict(ui=True)),
    ('pv', ('word_embeddings.weight',), True, dict())])
def test_deterministic_mode_two_frozen_runs_are_bitwise_equal(encoder, frozen, train_pv, kw):
    _, g1, p1 = _three_steps(encoder, frozen, train_pv, det=True, **kw)
    _, g2, p2 = _three_steps(encoder, frozen, train_pv, det=True, **kw)
    for n in p1:
        assert (g1[n] is None) == (g2[n] is None) and (g1[n] is None or torch.equal(g1[n], g2[n])), n
        assert torch.equal(p1[n], p2[n]), n
    _, g0, _ = _three_steps(encoder, frozen, train_pv, det=False, **kw)          # the default path: the same sums in another order
    for n in g1:
        if g1[n] is not None and not n.endswith('linear_keys.bias') and float(g0[n].abs().max()) > 0:
            assert rel_err(g1[n], g0[n]) < 1e-4, n


def test_deterministic_mode_vocabulary_above_the_histogram_limit():
    """40,000 words (RTM_HIST_MAXV = 38,000): trainable pvc has no deterministic word index and refuses; frozen words need none."""
    V = 40000
    _, g1, p1 = _three_steps('pvc', ('word_embeddings.weight',), False, det=True, V=V)
    _, g2, p2 = _three_steps('pvc', ('word_embeddings.weight',), False, det=True, V=V)
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n
    with pytest.raises(RuntimeError, match='deterministic mode needs the LDS-histogram word index'):
        _three_steps('pvc', (), False, det=True, V=V)


# ------------------------------------------------------------------------------------------------ requires_grad flips
@pytest.mark.parametrize('encoder,table,train_pv', [('pvc', 'word_embeddings.weight', False), ('pv', REVIEW_TABLE, True)])
def test_flipping_requires_grad_between_steps(encoder, table, train_pv):
    """frozen -> trainable -> frozen: each step's gradients against the oracle in the matching mode; the structs and the flat
    gradient buffer are rebuilt, the frozen table never moves."""
    from prodsearch_amd import build_optim
    a, m, rw, wd = _setup(encoder, d=64, heads=4, frozen=(table,), K=2, u_lim=2, i_lim=3, WL=24)
    w = dict(m.named_parameters())[table]
    opt = build_optim(a, m, None)
    _check_step(a, m, rw, wd, 50, 5, train_pv, (table,))
    assert w.grad is None and m._desc(1, 1, 1, False).frozen_mask != 0
    opt.step()
    w.requires_grad_(True)
    _check_step(a, m, rw, wd, 51, 5, train_pv, ())
    assert w.grad is not None and float(w.grad.abs().sum()) > 0 and m._desc(1, 1, 1, False).frozen_mask == 0
    opt.step()                                   # (the optimizer was built without the table: it is not updated)
    w.requires_grad_(False)
    before = w.detach().clone()
    _check_step(a, m, rw, wd, 52, 5, train_pv, (table,))
    assert w.grad is None
    opt.step()
    assert torch.equal(w.detach(), before)


def test_backward_refuses_gradient_pointers_that_disagree_with_the_mask():
    """The C entry point wants NULL exactly where the descriptor says frozen (host-side check, before any launch)."""
    from prodsearch_amd import _lib
    a, m, rw, wd = _setup('pvc', d=64, heads=4, frozen=('word_embeddings.weight',), K=2, u_lim=2, i_lim=3, WL=24)
    bt, _ = _batch(a, rw, wd, 60, 4, False)
    plan, loss3 = m._run_forward(bt.to('cuda'), False)
    ps, gs = m._structs()
    desc = plan.desc
    desc.frozen_mask = 0                                                         # ... but the word gradient is NULL
    rc = _lib.load().ps_rtm_backward(desc, ps, plan.batch, plan.ws.data_ptr(), gs, 1.0, None, m._stream())
    assert rc != 0 and b'frozen_mask' in _lib.load().ps_last_error()
    desc.frozen_mask = _lib.PS_RTM_FROZEN_WORD
    _lib.check(_lib.load().ps_rtm_backward(desc, ps, plan.batch, plan.ws.data_ptr(), gs, 1.0, None, m._stream()),
               'ps_rtm_backward')
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the trainer, end to end
def test_trainer_end_to_end_with_pretrained_directory_and_fix_emb(tmp_path):
    """create_model + Trainer on a tiny gz corpus with ``pretrain_emb_dir`` and ``fix_emb`` (argument pvc): a PV epoch and a plain
    one, validation, the ranklist, and the best checkpoint reloaded — frozen tables in ``model`` (equal to the files) and not in
    ``optim``."""
    from prodsearch_amd import PretrainedProductRanker, corpus, default_args, synth, trainer
    from prodsearch_amd import pretrained
    data_path, inp = synth.write_corpus(str(tmp_path / 'corpus'), 31, n_users=50, n_products=40, n_words=150)
    save = str(tmp_path / 'run')
    args = default_args(model_name='review_transformer', review_encoder_name='pvc', embedding_size=32, ff_size=64,
                        heads=4, inter_layers=1, batch_size=16, neg_per_pos=3, uprev_review_limit=3, iprev_review_limit=4,
                        review_word_limit=12, subsampling_rate=1e-2, lr=0.01, max_train_epoch=2, steps_per_checkpoint=5,
                        has_valid=True, valid_candi_size=8, candi_batch_size=8, test_candi_size=-1, valid_batch_size=6,
                        data_dir=data_path, input_train_dir=inp, save_dir=save, device='cuda', dropout=0.1, fix_emb=True,
                        train_pv_epoch=1, pv_window_size=4)
    gd = corpus.GlobalProdSearchData(args, data_path, inp)
    emb = pretrain_rtm_util.write_dir(str(tmp_path / 'emb'), gd.words, gd.review_count, 32, seed=4)
    args.pretrain_emb_dir = emb
    words = torch.from_numpy(pretrained.word_table(emb, gd.words, gd.vocab_size, 32, 'context_emb.txt.gz'))
    reviews = torch.from_numpy(pretrained.review_table(emb, gd.review_count, 32))
    np.random.seed(7)
    mrr, p1 = trainer.train(args)
    assert 0.0 < mrr <= 1.0 and 0.0 <= p1 <= 1.0
    lines = open(os.path.join(save, args.rankfname)).read().splitlines()
    assert lines and all(len(ln.split(' ')) == 6 for ln in lines)
    best = os.path.join(save, 'model_best.ckpt')
    ck = torch.load(best, map_location='cpu', weights_only=False)
    assert torch.equal(ck['model']['word_embeddings.weight'], words)             # never updated
    assert torch.equal(ck['model'][REVIEW_TABLE], reviews) and torch.equal(ck['model']['review_embeddings'], reviews)
    train_pd = corpus.ProdSearchData(args, inp, 'train', gd)
    model, optim = trainer.create_model(args, gd, train_pd, best)
    assert type(model) is PretrainedProductRanker and model.review_encoder_name == 'pv'
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen == ['review_embeddings', 'word_embeddings.weight']
    assert list(model.state_dict()) == list(ck['model'])
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), ck['model'][k]), k
    assert not any(n in optim._names for n in frozen)
    # the optimizer's checkpoint holds the trainable parameters only, no moment in a frozen table's shape
    n_trainable = sum(1 for p in model.parameters() if p.requires_grad)
    assert len(ck['optim']['param_groups'][0]['params']) == n_trainable and ck['optim']['state']
    trainable = [p for p in model.parameters() if p.requires_grad]
    for i, st in ck['optim']['state'].items():
        assert tuple(st['exp_avg'].shape) == tuple(trainable[i].shape), i
    test_pd = corpus.ProdSearchData(args, inp, 'test', gd)
    mrr2, p12 = trainer.Trainer(args, model, None).test(args, gd, test_pd, 'again.ranklist')
    assert mrr2 == mrr and p12 == p1
    assert open(os.path.join(save, 'again.ranklist')).read().splitlines() == lines
