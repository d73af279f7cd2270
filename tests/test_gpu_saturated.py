"""The training step at weights no other oracle comparison reaches, against a FLOAT64 oracle (tests/saturated.py; the GEMM
alone has tests/test_gpu_gemm_x3.py).  Every other case of the suite runs at synth.make_state_dict's scale, where each
softmax row is near uniform and tanh / GELU / BCE sit in their linear range.  Here:

  * one case per attention form and per fused / unfused tail (the rows of tests/enc_paths.py, path asserted), QEM, and two
    review-transformer shapes, in the ``peaked`` and the ``saturated`` regime: the softmax forward and backward with one-hot
    and spread rows in one wave, exp(v - m) far from 0, the hand-written tanh / GELU / sigmoid / softplus at their tails, the
    LayerNorm stages on large rows.  tests/test_saturated_cpu.py asserts on the CPU that each case is in its regime and that
    fp32 arithmetic's own error there stays below 1e-4 — so the suite's bounds hold against float64: loss and logits 1e-4,
    every gradient 5e-4 of its max, the query words' rows of word_embeddings on their own, eval scores 1e-4;
  * the 64-bit fixed-point loss hand-off of the folded scoring (csrc/mlp_fused.hip, csrc/rtm_score.hip) at and past its range: the
    largest workgroup partial just under the limit (at 1, 33 and 263 workgroups: 2^20 and 2^19 units), past it (the loss is
    +inf, never a finite number), a NaN operand — and after each of the last two a benign step through the same module, which
    must match the oracle again: the poison word and the arrival count are cleared per step.

Touched rows: a table row's gradient is zero where the oracle's is zero (a row outside the batch), and nonzero where the
oracle's row reaches 1e-6 of the tensor's largest entry.  Between the two a row may be either: a saturated term's
sigmoid(s) - target is 4e-44 at s = -100 in float64 and 0 in fp32, and sigmoid(s) - 1 is exactly 0 in fp32 — the reference's own
arithmetic included — once 1 - sigmoid(s) < 2^-24 = 6e-8, so rows that only such terms reach stay below 6e-8 of an unsaturated
row's entries.

No input here is illegal: every one is a finite or NaN value in a tensor of a shape other tests run."""
import functools

import pytest
import torch

import enc_paths
import saturated as S
from golden_util import rel_err

pytestmark = pytest.mark.gpu

LOSS_TOL, LOGIT_TOL, GRAD_TOL, EVAL_TOL = 1e-4, 1e-4, 5e-4, 1e-4
LIVE = 1e-6             # of the tensor's largest entry: above fp32's 2^-24 rounding of a saturated sigmoid against its target


def assert_same_rows_touched(got, ref, name):
    live = ref.abs().amax(1)
    touched = got.ne(0).any(1)
    assert bool(touched[live >= LIVE * float(live.max())].all()), (name, 'a row the oracle updates is left untouched')
    assert not bool(touched[live == 0].any()), (name, 'a row outside the batch is touched')


# ------------------------------------------------------------------------------------------------- item transformer / QEM
def new_module(p):
    from prodsearch_amd import ItemTransformerRanker
    return ItemTransformerRanker(p.a, 'cuda', p.V, p.P_, None, word_dists=p.wd)


def module_step(m, p, sd, expect=None, backward=True, want_eval=True):
    """Load ``sd`` and run one training forward (+ backward, + eval scores) through the module API."""
    m.load_state_dict(sd, strict=False)
    m.train()
    loss = m(p.batch.to('cuda'), neg_item_idxs=p.ni.cuda(), neg_word_idxs=p.nw.cuda())
    if expect:
        expect(0)
    out = dict(loss=loss.detach().cpu(), step=m._fwd_step)
    plan = next(pl for key, pl in m._plans.items() if key[-1])
    out['logits'] = m.workspace_view(plan, 'item_scores', (p.B, p.K + 1)).cpu()
    if backward:
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        if expect:
            expect(1)
        out['grads'] = {n: (None if q.grad is None else q.grad.cpu()) for n, q in m.named_parameters()}
    if want_eval:
        m.eval()
        with torch.no_grad():
            out['eval'] = m.test(p.batch.to('cuda')).cpu()
    return out


def assert_step_matches(got, r64, p, what):
    """The suite's measures and bounds (tests/test_gpu_tem_options.check_against_oracle), against the float64 oracle."""
    assert rel_err(got['loss'], r64['loss']) < LOSS_TOL, (what, 'loss', float(got['loss']), float(r64['loss']))
    assert rel_err(got['logits'], r64['logits']) < LOGIT_TOL, (what, 'logits', rel_err(got['logits'], r64['logits']))
    for n, g in got['grads'].items():
        ref = r64['grads'].get(n)
        assert (g is None) == (ref is None), (what, n)
        if ref is None or n.endswith('linear_keys.bias'):       # (its true gradient is 0: softmax is shift-invariant)
            continue
        assert bool(torch.isfinite(g).all()), (what, n)
        assert rel_err(g, ref) < GRAD_TOL, (what, n, rel_err(g, ref))
        if ref.dim() == 2 and ref.shape[0] > 256:
            assert_same_rows_touched(g, ref, (what, n))
    qrows = torch.unique(p.batch.query_word_idxs)
    qrows = qrows[qrows != p.V - 1]
    gq, rq = got['grads']['word_embeddings.weight'][qrows], r64['grads']['word_embeddings.weight'][qrows]
    assert rel_err(gq, rq) < GRAD_TOL, (what, 'word_embeddings (query rows)', rel_err(gq, rq))
    if 'eval' in got:
        assert rel_err(got['eval'], r64['eval']) < EVAL_TOL, (what, 'eval scores', rel_err(got['eval'], r64['eval']))


def print_figures(what, got, r64, r32):
    """The kernel's and the fp32 oracle's error against float64, in the same measure (recorded in
    profiles/saturated_parity.md); a tensor whose kernel error is over three times the fp32 oracle's is a lead."""
    ek, eo = S.errors(got, r64), S.errors(r32, r64)
    gk = [k for k in ek if k not in ('loss', 'logits')]
    wk, wo = S.worst(ek, gk), S.worst(eo, gk)
    print('figures: %s | loss %.1e / %.1e | logits %.1e / %.1e | worst gradient %.1e (%s) / %.1e (%s)'
          % (what, ek['loss'], eo['loss'], ek['logits'], eo['logits'], wk[0], wk[1], wo[0], wo[1]))
    for k in ek:
        if ek[k] > 3 * max(eo[k], 1e-7):                 # (1e-7: an fp32 ulp; below it "three times" means nothing)
            print('lead: %s | %s kernel %.1e fp32 oracle %.1e' % (what, k, ek[k], eo[k]))


@pytest.mark.parametrize('regime', list(S.REGIMES))
@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_step_matches_float64_in_the_regime(name, regime):
    from prodsearch_amd import _lib
    lib = _lib.load()
    p, sd, r64, r32 = S.case(name, regime)
    print('figures: %s %s regime | %s' % (name, regime, S.fmt_stats(S.regime_stats(r64['keep'], p.a))))
    row = None if name == 'qem' else S.row_of(name)
    old = lib.ps_set_fuse_bwd_min(row['fuse_bwd_min']) if row and row['fuse_bwd_min'] is not None else None
    try:
        got = module_step(new_module(p), p, sd, expect=enc_paths.taken_checker(row) if row else None)
    finally:
        if old is not None:
            lib.ps_set_fuse_bwd_min(old)
    print_figures('%s %s' % (name, regime), got, r64, r32)
    assert_step_matches(got, r64, p, (name, regime))


# ------------------------------------------------------------------------------------------------- the loss hand-off
# sep_prod_emb: product_emb feeds the scores and the word loss only, so its factor moves the logits and nothing before them
HANDOFF_ROWS = ('e_2_5_20', 'mf1029', 'e_400_20_9')        # 1, 33 and 263 workgroups of 32 replica rows
UNFOLDED_ROW = 'e_5_33_7'                                  # d = 64: no fused tail, float partials


@functools.lru_cache(maxsize=None)
def handoff_problem(name):
    return S.problem(**dict(enc_paths.oracle_call(S.row_of(name)), sep_prod_emb=True))


@functools.lru_cache(maxsize=None)
def benign64(name, step):
    """The float64 oracle's step on the unscaled weights (shared: the factor search reads its logits, the recovery steps
    compare with it; nobody writes to it)."""
    p = handoff_problem(name)
    return S.oracle_step(p, p.sd, True, step=step, want_eval=False)


def handoff_input(name, kind):
    """(state dict, float64 oracle step, largest workgroup partial) of a hand-off case."""
    p = handoff_problem(name)
    if kind == 'non_finite':
        sd = {k: v.clone() for k, v in p.sd.items()}
        sd['product_emb.weight'][int(p.ni[0, 0]), 0] = float('nan')
        return sd, None, None
    assert p.a.sim_func != 'bias_product'
    base = benign64(name, 1)['logits']
    f = S.product_factor(base, 0.5, 0.9) if kind == 'near_limit' else S.product_factor(base, 2.0, None)
    sd = S.scaled_state_dict(p.sd, product_emb__weight=f)
    r64 = S.oracle_step(p, sd, True, want_eval=False)
    top = float(S.workgroup_partials(S.bce_terms(r64['logits'])).max())
    return sd, r64, top


def assert_recovers(m, name, what):
    """A benign step through the same module matches the oracle: nothing of the step before it is left in the ticket words."""
    p = handoff_problem(name)
    got = module_step(m, p, p.sd, want_eval=False)
    assert_step_matches(got, benign64(name, got['step']), p, (what, 'recovery step'))


@pytest.mark.parametrize('name', HANDOFF_ROWS)
def test_folded_loss_just_under_its_limit(name):
    p = handoff_problem(name)
    sd, r64, top = handoff_input(name, 'near_limit')
    nwg = (p.B * (p.K + 1) + S.MBM - 1) // S.MBM
    print('figures: %s near_limit | %d workgroups, largest partial %.0f = %.2f x 2^19, loss %.6g'
          % (name, nwg, top, top / S.FOLD_LIMIT, float(r64['loss'])))
    assert 0.5 * S.FOLD_LIMIT <= top <= 0.9 * S.FOLD_LIMIT and bool(torch.isfinite(r64['loss']))
    row = S.row_of(name)
    assert 'FS' in row['flags']
    got = module_step(new_module(p), p, sd, expect=enc_paths.taken_checker(row), want_eval=False)
    print_figures('%s near_limit' % name, got, r64, S.oracle_step(p, sd, False, want_eval=False))
    assert_step_matches(got, r64, p, (name, 'near_limit'))


def test_folded_loss_at_the_reduced_scale_with_every_partial_large():
    """More than 512 workgroups (2^18 units), EVERY partial near the limit: the one input at which the scale rule itself is
    live.  The arrival count sits in bits 48+, so a scale left at 2^20 carries into it only once the partials sum to 2^28 —
    which partials below 2^19 cannot reach at 512 workgroups or fewer (263 x 2^19 < 2^28: at 263 workgroups no legal input
    tells 2^19 from 2^20).  A product bias common to all items puts every negative's term at about that bias, so the partials
    are about 30.5 x bias, all alike: 657 of them, the largest at 0.85 x 2^19, sum to 1.07 x 2^28."""
    from prodsearch_amd import _lib
    p = S.problem(B=1000, K=20, L=1, Q=4, sim_func='bias_product')
    base = S.oracle_step(p, p.sd, True, want_eval=False)['logits']           # logits are base + c under a common bias c
    top = lambda c: float(S.workgroup_partials(S.bce_terms(base + c)).max())
    lo, hi = 0.0, float(S.FOLD_LIMIT)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if top(mid) < 0.85 * S.FOLD_LIMIT else (lo, mid)
    sd = {k: v.clone() for k, v in p.sd.items()}
    sd['product_bias'][:p.P_] += float(hi)
    r64 = S.oracle_step(p, sd, True, want_eval=False)
    parts = S.workgroup_partials(S.bce_terms(r64['logits']))
    print('figures: every-partial-large | %d workgroups, partials %.3f .. %.3f x 2^19, sum %.3f x 2^28, loss %.6g'
          % (parts.numel(), float(parts.min()) / S.FOLD_LIMIT, float(parts.max()) / S.FOLD_LIMIT, float(parts.sum()) / 2 ** 28,
             float(r64['loss'])))
    assert parts.numel() > 512 and 0.5 * S.FOLD_LIMIT <= float(parts.max()) <= 0.9 * S.FOLD_LIMIT
    assert float(parts.sum()) >= 1.05 * 2 ** 28 and float(parts.sum()) * 2 ** 18 < 2 ** 47
    lib = _lib.load()

    def folded(backward):
        if not backward and enc_paths.default_switches():
            assert enc_paths.taken(lib, _lib, 0)['fold_score'] == 1
    got = module_step(new_module(p), p, sd, expect=folded, want_eval=False)
    print('figures: every-partial-large | loss rel_err %.1e' % rel_err(got['loss'], r64['loss']))
    assert_step_matches(got, r64, p, 'every-partial-large')


@pytest.mark.parametrize('name', HANDOFF_ROWS)
def test_folded_loss_past_its_limit_is_inf_and_the_next_step_is_clean(name):
    p = handoff_problem(name)
    sd, r64, top = handoff_input(name, 'over_limit')
    assert top >= 2 * S.FOLD_LIMIT and bool(torch.isfinite(r64['loss']))
    m = new_module(p)
    got = module_step(m, p, sd, expect=enc_paths.taken_checker(S.row_of(name)), backward=False, want_eval=False)
    print('figures: %s over_limit | largest partial %.2f x 2^19, float64 loss %.6g, loss %r'
          % (name, top / S.FOLD_LIMIT, float(r64['loss']), float(got['loss'])))
    assert float(got['loss']) == float('inf')
    assert_recovers(m, name, (name, 'over_limit'))


@pytest.mark.parametrize('name', HANDOFF_ROWS)
def test_nan_item_row_gives_a_non_finite_loss_and_the_next_step_is_clean(name):
    p = handoff_problem(name)
    sd, _, _ = handoff_input(name, 'non_finite')
    m = new_module(p)
    got = module_step(m, p, sd, backward=False, want_eval=False)
    assert not bool(torch.isfinite(got['loss']))
    assert_recovers(m, name, (name, 'non_finite'))


@pytest.mark.parametrize('kind', ['near_limit', 'over_limit', 'non_finite'])
def test_unfolded_loss_has_no_such_limit(kind):
    """The same three inputs where the scoring is a launch of its own with float partials (no FS in the path)."""
    p = handoff_problem(UNFOLDED_ROW)
    row = S.row_of(UNFOLDED_ROW)
    assert 'FS' not in row['flags']
    sd, r64, top = handoff_input(UNFOLDED_ROW, kind)
    got = module_step(new_module(p), p, sd, expect=enc_paths.taken_checker(row), backward=False, want_eval=False)
    if kind == 'non_finite':
        assert not bool(torch.isfinite(got['loss']))
        return
    print('figures: %s %s unfolded | largest partial %.2f x 2^19, loss rel_err %.1e'
          % (UNFOLDED_ROW, kind, top / S.FOLD_LIMIT, rel_err(got['loss'], r64['loss'])))
    assert (0.5 <= top / S.FOLD_LIMIT <= 0.9) if kind == 'near_limit' else top >= 2 * S.FOLD_LIMIT
    assert rel_err(got['loss'], r64['loss']) < LOSS_TOL


# ------------------------------------------------------------------------------------------------- review transformer
def rtm_module(p):
    from prodsearch_amd import ProductRanker
    return ProductRanker(p.a, 'cuda', p.V, p.RC, 50, 60, p.rw, None, word_dists=p.wd)


def rtm_module_step(m, p, sd, backward=True):
    m.load_state_dict(sd, strict=False)
    m.train()
    loss = m(p.batch.to('cuda'), train_pv=False)
    out = dict(loss=loss.detach().cpu())
    plan = next(iter(m._plans.values()))
    out['logits'] = m.workspace_view(plan, 'scores', (p.B, p.K + 1)).cpu()
    if backward:
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        out['grads'] = {n: (None if q.grad is None else q.grad.cpu()) for n, q in m.named_parameters()}
    return out


def assert_rtm_step_matches(got, r64, what):
    """tests/test_gpu_rtm_shapes.py's measures and bounds, and the logits, against the float64 oracle."""
    assert rel_err(got['loss'], r64['loss']) < LOSS_TOL, (what, 'loss', float(got['loss']), float(r64['loss']))
    assert rel_err(got['logits'], r64['logits']) < LOGIT_TOL, (what, 'logits')
    checked = 0
    for k, g in r64['grads'].items():
        if g is None or k.endswith('linear_keys.bias') or k not in got['grads'] or float(g.abs().max()) == 0.0:
            continue
        assert got['grads'][k] is not None, (what, k)
        assert bool(torch.isfinite(got['grads'][k]).all()), (what, k)
        assert rel_err(got['grads'][k], g) < GRAD_TOL, (what, k, rel_err(got['grads'][k], g))
        checked += 1
    assert checked >= 16


@pytest.mark.parametrize('name', list(S.RTM_SHAPES))
def test_review_transformer_matches_float64_when_saturated(name):
    p, sd, r64, r32 = S.rtm_case(name, 'saturated')
    print('figures: %s saturated regime | %s' % (name, S.fmt_stats(S.regime_stats(r64['keep'], p.a))))
    got = rtm_module_step(rtm_module(p), p, sd)
    print_figures('%s saturated' % name, got, r64, r32)
    assert_rtm_step_matches(got, r64, (name, 'saturated'))


def rtm_handoff_input(p, kind):
    f, limit = S.rtm_wo_factor(p, 0.5, 0.9) if kind == 'near_limit' else S.rtm_wo_factor(p, 2.0, None)
    sd = S.scaled_state_dict(p.sd, transformer_encoder__wo__weight=f)
    r64 = S.rtm_oracle_step(p, sd, True)
    terms = r64['keep']['weight'].double() * S.bce_terms(r64['logits'])
    return sd, r64, float(S.workgroup_partials(terms, S.RTM_SEQS_PER_WG).max()) / limit


def test_review_transformer_folded_loss_just_under_its_limit():
    p = S.rtm_problem(**S.RTM_SHAPES['rtm_d128'])
    sd, r64, share = rtm_handoff_input(p, 'near_limit')
    print('figures: rtm_d128 near_limit | largest partial %.2f x 2^27 / grid, loss %.6g' % (share, float(r64['loss'])))
    assert 0.5 <= share <= 0.9 and bool(torch.isfinite(r64['loss']))
    got = rtm_module_step(rtm_module(p), p, sd)
    assert_rtm_step_matches(got, r64, ('rtm_d128', 'near_limit'))


def test_review_transformer_folded_loss_past_its_limit_is_inf_and_the_next_step_is_clean():
    p = S.rtm_problem(**S.RTM_SHAPES['rtm_d128'])
    sd, r64, share = rtm_handoff_input(p, 'over_limit')
    assert share >= 2.0 and bool(torch.isfinite(r64['loss']))
    m = rtm_module(p)
    got = rtm_module_step(m, p, sd, backward=False)
    print('figures: rtm_d128 over_limit | largest partial %.2f x 2^27 / grid, float64 loss %.6g, loss %r'
          % (share, float(r64['loss']), float(got['loss'])))
    assert float(got['loss']) == float('inf')
    again = rtm_module_step(m, p, p.sd)
    assert_rtm_step_matches(again, S.rtm_oracle_step(p, p.sd, True), ('rtm_d128', 'recovery step'))
