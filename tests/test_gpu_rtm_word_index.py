"""The review transformer's inverted word index and word-gradient reduce (csrc/rtm_index.hip; the ranks of rtm_embed4_kernel,
csrc/rtm_embed.hip; the slot rows of csrc/rtm_embed_bwd.hip), in every form and at the branches the rest of the suite does
not reach: the forward-counts and the late index (vocabulary above RTM_HIST_MAXV: a workspace without a histogram block),
a second backward over the forward's counts, the LDS histogram at its largest, a partition of more than 1,024 review rows
(the second list of rtm_hist_kernel), a word above WR_DET_LIM occurrences in the default and the ordered reduce at NK = 2 /
4 / 8, word masks that differ from the pad id, and lists of one entry.

One forward and one backward of ``ProductRanker`` (dropout 0, corruption 0) per case; ``ps_rtm_backward_plan`` on the
step's own descriptor names the index form, so no case runs another path unnoticed.  The loss against the float64 oracle
(1e-4), ``word_embeddings.weight.grad`` row by row (tests/rtm_word_rows.py: err_w against 8 x the fp32 oracle's own, the
touched rows exactly), every other gradient with the suite's max-norm (5e-4).  Reference semantics:
``ProductRanker.forward`` (models/ps_model.py:241-358), ``PVC.py:46-61``, models/text_encoder.py."""
import pytest
import torch

import rtm_word_rows as W
from golden_util import rel_err

pytestmark = pytest.mark.gpu

WORD = 'word_embeddings.weight'


def _step(name, det=False, backwards=1):
    """The case's step on the GPU: (module, loss, gradients after the first backward, after the last)."""
    from prodsearch_amd import ProductRanker, _lib
    p = W.problem(name)
    lib = _lib.load()
    old = lib.ps_set_deterministic(1 if det else 0)
    try:
        torch.manual_seed(0)
        m = ProductRanker(p.a, 'cuda', p.V, p.RC, 50, 60, p.rw, None, word_dists=p.wd)
        m.load_state_dict(p.sd)
        m.train()
        loss = m(p.batch.to('cuda'), train_pv=p.train_pv, neg_word_idxs=None if p.neg_words is None else p.neg_words.cuda())
        m.zero_grad()
        first = None
        for i in range(backwards):
            loss.backward(retain_graph=i + 1 < backwards)
            if first is None:
                torch.cuda.synchronize()
                first = {n: q.grad.detach().cpu().clone() for n, q in m.named_parameters() if q.grad is not None}
        torch.cuda.synchronize()
        last = {n: q.grad.detach().cpu().clone() for n, q in m.named_parameters() if q.grad is not None}
        plan = [pl for k, pl in m._plans.items() if k[0] != 'eval'][-1]
        bp = W.backward_plan(plan.desc)
        return m, float(loss.detach().cpu()), first, last, (bp.index, bp.side_fork)
    finally:
        lib.ps_set_deterministic(old)


def _check(name, loss, grads, form, label=''):
    """Loss, word rows and every other gradient of one step against the case's float64 oracle; returns the worst err_w."""
    p, r64, dec = W.reference(name)
    assert form == W.expected_plan(name), (name, form)
    print('figures: %s%s index %d loss %.2e worst err_w %.3e bound %.3e' % (
        name, label, form[0], rel_err(torch.tensor(loss), r64['loss']), float(W.row_errors(grads[WORD], dec).max()), W.bound(name)))
    assert rel_err(torch.tensor(loss), r64['loss']) < 1e-4
    worst = W.compare(grads[WORD], dec, W.bound(name), W.addressed_words(p), what='%s%s (index form %d)' % (name, label, form[0]))
    checked = 0
    for k, g in r64['grads'].items():
        if g is None or k == WORD or k.endswith('linear_keys.bias') or float(g.abs().max()) == 0.0:
            continue
        assert k in grads, k
        assert rel_err(grads[k], g) < 5e-4, k
        checked += 1
    assert checked >= 14, checked
    return worst


@pytest.mark.parametrize('name', ['fc_d64', 'fc_d256', 'fc_d64_pv', 'fc_d256_pv', 'late_d32', 'late_d512', 'hist_limit',
                                  'hist_two_lists', 'masks_avg', 'masks_fs', 'one_review', 'one_review_wl1', 'wl1'])
def test_word_rows_match_the_float64_oracle(name):
    m, loss, g, _, form = _step(name)
    _check(name, loss, g, form)


def test_second_backward_over_the_forward_counts_adds_the_same_rows():
    """``backward(retain_graph=True); backward()`` at V = 38,001: the second build of the index starts the allocator's total
    from 0 (the ``!count`` branch of rtm_build_index) and lays the same list out over the forward's counts and ranks."""
    m, loss, g1, g2, form = _step('fc_d64', backwards=2)
    _check('fc_d64', loss, g1, form, ' first of two backwards')
    for n in g2:
        if float(g1[n].abs().max()) == 0.0:
            continue
        assert rel_err(g2[n], 2 * g1[n]) < 1e-5, n
    assert torch.equal(g2[WORD].ne(0).any(1), g1[WORD].ne(0).any(1))


@pytest.mark.parametrize('name', ['heavy_d64', 'heavy_d256', 'heavy_d512'])
@pytest.mark.parametrize('det', [False, True])
def test_heavy_word_rows_match_the_float64_oracle(name, det):
    """More than WR_DET_LIM real occurrences of one word, several in every review.  Deterministic mode: the one-wave ranks
    (``before`` / ``same``) and rtm_wreduce_heavy_det_kernel, against the oracle and not only against the default path, and
    two runs bit-equal."""
    p, r64, dec = W.reference(name)
    idx, ok, real = W.slot_words(p)
    assert int((idx.eq(W.HEAVY_WORD) & ok & real[:, None]).sum()) > W.WR_DET_LIM
    if det and W.hist_switch_off():
        with pytest.raises(RuntimeError, match='deterministic mode'):
            _step(name, det=True)
        return
    m, loss, g, _, form = _step(name, det=det)
    print('figures: %s%s err_w of the heavy word (%d occurrences) %.3e' % (
        name, ' deterministic' if det else '', int(dec.count[W.HEAVY_WORD]), float(W.row_errors(g[WORD], dec)[W.HEAVY_WORD])))
    _check(name, loss, g, form, ' deterministic' if det else '')
    if det:
        m2, loss2, h, _, _ = _step(name, det=True)
        assert loss2 == loss and sorted(h) == sorted(g)
        for n in g:
            assert torch.equal(g[n], h[n]), n
