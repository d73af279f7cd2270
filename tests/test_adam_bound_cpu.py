"""The float64 yardstick for the clip + Adam kernels (oracle/adam64.py), tried on the CPU before any kernel is judged by it.

* ``step32_numpy`` — ``adam_elem``'s operation sequence in float32 — stays within 1 x ``bound`` of ``step64`` for every element of
  10^6 per setting, 20 settings (t in {1, 2, 10, 1000, 100000}, weight decay 0 / 1e-3, noam on / off; |p| in 1e-6..10, |g| in
  1e-6..1e3 with 30 % exact zeros, m like g, v the square of such values).  Measured: error / bound at most 1.000 for p (the last
  rounding of p' alone reaches it), 0.98 for m, 0.97 for v.
* ``torch.optim.Adam`` in float32 on the CPU (eps 1e-9, with and without weight decay, after ``clip_grad_norm_``, clip active and
  inactive) stays within 2 x ``bound`` of ``step64`` at every t once ``step64`` forms `1 - beta` and the bias corrections the way
  torch does, from its DOUBLE betas (``Hyper(torch_betas=True)``), and takes torch's own clip coefficient (``max_norm / tensor`` is
  reciprocal-then-multiply there: up to one ulp from ``adam_scalars``' division).  Measured: 1.00 / 0.98 / 0.93 for p / m / v.
* The kernel's way — float32 betas throughout, `1 - beta` formed in float32, because PsAdamHyper carries floats — deviates from
  that: 1 - fl32(0.999) is 1.29e-5 below 0.001, and 1 - fl32(0.999)^t is below 1 - 0.999^t by up to the same relative amount at
  small t; each is worth 6.4e-6 on the denominator.  Measured on the inputs above (both conventions in float64): the update moves
  by at most 6.7e-6 relative to its size (cap by reasoning, asserted: 1.4e-5), and by 5e-8 at t = 1 from zero moments, where
  sqrt((1 - b2) / bc2) is 1 either way.  On p' that is up to 13.8 x ``bound`` on these inputs — whose updates are often orders of
  magnitude larger than the parameters — where the float32 torch run itself is at 1.00 x: beyond the factor of 10 that was set as
  the line between a deviation and a defect.  (In training |update| is about lr = 0.002 against |p| of 0.01..1: 1.3e-8 per step,
  under the 6e-8 |p| of p's own rounding.)  Matching torch needs double betas in PsAdamHyper; this file states what the kernel
  does and names the difference.
* Three deliberately wrong variants of ``step64`` fall far outside 2 x ``bound``: eps 1e-8 (3.7e6 x), the second bias correction
  dropped (6e7 x at t <= 10, 5e5 x at t = 1000 — and nothing at t = 1e5, where the factor rounds to 1, which is why kernel
  tests must step at small and mid-range t), weight decay applied after the moments (1e11 x and more).
"""
import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

from oracle import adam64 as A

N = 1000000
N_TORCH = 200000
STEPS = (1, 2, 10, 1000, 100000)
SETTINGS = [(t, wd, noam) for noam in (False, True) for wd in (0.0, 1e-3) for t in STEPS]


def _seed(t, wd, noam):
    return [t, int(wd * 1e6), int(noam)]


@pytest.mark.parametrize('t,wd,noam', SETTINGS)
def test_float32_restatement_is_within_the_bound(t, wd, noam):
    rng = np.random.default_rng(_seed(t, wd, noam))
    p, g, m, v = A.draw_state(rng, N)
    h = A.Hyper(weight_decay=wd, noam=noam)
    for gmul in (1.0, 0.37):
        got = A.step32_numpy(p, g, m, v, h, t, A.f32(gmul))
        r = A.worst_ratios(got, p, g, m, v, h, t, A.f32(gmul))
        print("t %d wd %g noam %d gmul %g: error / bound p %.4f m %.4f v %.4f" % ((t, wd, noam, gmul) + r))
        assert max(r) <= 1.0, r


def _torch_step(p, g, m, v, lr, wd, t, clip):
    """One torch.optim.Adam step in float32 on the CPU from preset moments at step t; returns (p', m', v', pre-clip norm)."""
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([tp], lr=lr, betas=(0.9, 0.999), eps=1e-9, weight_decay=wd)
    opt.state[tp] = {'step': torch.tensor(float(t - 1)), 'exp_avg': torch.from_numpy(m.copy()),
                     'exp_avg_sq': torch.from_numpy(v.copy())}
    norm = clip_grad_norm_([tp], clip)
    # the coefficient as clip_grad_norm_ forms it from its float32 norm (`max_norm / tensor` is reciprocal-then-multiply in torch:
    # up to one ulp from adam_scalars' true division, so the element arithmetic is judged with torch's own coefficient here)
    coef = np.float32(float(torch.clamp(clip / (norm + 1e-6), max=1.0)))
    opt.step()
    st = opt.state[tp]
    return tp.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy(), coef


@pytest.mark.parametrize('t', STEPS)
@pytest.mark.parametrize('wd,clip', [(0.0, 1e9), (1e-3, 1e9), (0.0, 50.0), (1e-3, 50.0)])
def test_torch_adam_float32_is_within_twice_the_bound_and_the_beta_deviation_is_small(t, wd, clip):
    rng = np.random.default_rng(_seed(t, wd, clip > 1e8) + [7])
    p, g, m, v = A.draw_state(rng, N_TORCH)
    if t == 1:
        m[:] = 0.0
        v[:] = 0.0                         # (a first step starts from zero moments: there the two conventions agree)
    lr = 0.002
    tp, tm, tv, gmul = _torch_step(p, g, m, v, lr, wd, t, clip)
    ht = A.Hyper(lr=lr, weight_decay=wd, max_grad_norm=clip, torch_betas=True)
    hk = A.Hyper(lr=lr, weight_decay=wd, max_grad_norm=clip)
    assert (gmul < 1.0) == (clip < 1e8)
    r = A.worst_ratios((tp, tm, tv), p, g, m, v, ht, t, gmul)
    print("t %d wd %g clip %g: torch float32 error / bound p %.4f m %.4f v %.4f" % ((t, wd, clip) + r))
    assert max(r) <= 2.0, r
    # the float32-beta convention of the kernel against torch's double betas, both in float64
    pt, _, _, ut = A.step64(p, g, m, v, ht, t, gmul)
    pk, _, _, uk = A.step64(p, g, m, v, hk, t, gmul)
    # relative to the update's size before m + (1 - b1)(gg - m) cancels (an element where it cancels has no relative error to speak of)
    gg = g.astype(np.float64) * float(gmul) + wd * p.astype(np.float64)
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    ss, isb, _ = [float(x) for x in A.step_scalars(ht, t)]
    size = ss * (np.abs(m64) + 0.1 * np.abs(gg - m64)) / (np.sqrt(v64 * 0.999 + 0.001 * gg * gg) * isb + 1e-9)
    nz = size != 0
    dev_upd = float((np.abs(uk - ut)[nz] / size[nz]).max())
    # ... and on p', in units of the bound, beside the float32 torch run's own error in the same units (r[0])
    dp = A.bound(p, g, m, v, ht, t, gmul)[0]
    dev_p = float((np.abs(pk - pt) / dp).max())
    print("   float32 betas against double betas: update %.3g relative; p' %.2f x bound (the float32 run itself: %.2f x bound)"
          % (dev_upd, dev_p, r[0]))
    # 1 - fl32(b2) is 1.29e-5 below 1 - b2, half of it on sqrt(v'): 6.5e-6; bias correction 2: 6.4e-6; 1 - fl32(b1): 2.3e-7 on m'
    assert dev_upd <= 1.4e-5               # (p' = p - update: the same cap holds for p')
    if t == 1:
        assert dev_upd <= 4 * A.U          # from zero moments sqrt((1 - b2) / bc2) is 1 under either convention


@pytest.mark.parametrize('t', STEPS[1:])
@pytest.mark.parametrize('wd', [0.0, 1e-3])
def test_float32_betas_stay_a_deviation_on_training_range_states(t, wd):
    """The line between a deviation and a defect: the float32-beta effect on p' may be at most 10 x the float32 torch run's own
    error against float64.  Judged where the optimizer works: |p| in 0.01..1, lr 0.002, and moments that belong to their
    gradients — per element a gradient scale s in 1e-4..1, g = s n, m = 0.3 s n', v = s^2 times 0.5..1.5 — so that |update| is
    of the order of the step size, as it is for moments Adam built itself.  Then the effect, 6.7e-6 |update|, is about 1e-8 where
    p's own rounding is up to 6e-8.  Measured: 0.01 .. 0.22 x.  (On the wide synthetic inputs of the test above, with m and v
    drawn independently over nine decades, updates are often orders of magnitude larger than the parameters and the same 6.7e-6
    is up to 13.8 x the bound of p' where the float32 run is at 1.00 x: beyond the line there.  Matching torch on such states
    needs double betas in PsAdamHyper.)"""
    rng = np.random.default_rng([t, int(wd * 1e6), 23])
    n = N_TORCH
    p = A.draw(rng, n, 1e-2, 1.0)
    s = np.exp(rng.uniform(np.log(1e-4), np.log(1.0), n))
    g = (s * rng.standard_normal(n)).astype(np.float32)
    m = (s * (0.3 * rng.standard_normal(n))).astype(np.float32)
    v = (s * s * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    lr = 0.002
    tp, _, _, gmul = _torch_step(p, g, m, v, lr, wd, t, 1e9)
    ht = A.Hyper(lr=lr, weight_decay=wd, torch_betas=True)
    hk = A.Hyper(lr=lr, weight_decay=wd)
    pt, _, _, ut = A.step64(p, g, m, v, ht, t, gmul)
    pk = A.step64(p, g, m, v, hk, t, gmul)[0]
    assert float(np.abs(ut).max()) <= 10 * lr * float(A.step_scalars(ht, t)[0]) / lr       # updates of the order of the step size
    own = float(np.abs(tp.astype(np.float64) - pt).max())
    dev = float(np.abs(pk - pt).max())
    print("t %d wd %g: float32 betas move p' by at most %.3g; the float32 torch run's own error %.3g: %.2f x" % (t, wd, dev, own, dev / own))
    assert dev <= 10.0 * own


@pytest.mark.parametrize('variant,t,wd,least', [('eps8', 1, 0.0, 1e6), ('eps8', 1000, 1e-3, 1e6), ('eps8', 100000, 0.0, 1e6),
                                                ('nobc2', 1, 0.0, 1e7), ('nobc2', 10, 1e-3, 1e7), ('nobc2', 1000, 0.0, 1e5),
                                                ('wd_after', 2, 1e-3, 1e9), ('wd_after', 100000, 1e-3, 1e9)])
def test_the_bound_has_teeth(variant, t, wd, least):
    rng = np.random.default_rng(_seed(t, wd, 0) + [11])
    p, g, m, v = A.draw_state(rng, N // 4)
    h = A.Hyper(weight_decay=wd)
    bad = A.step64(p, g, m, v, h, t, A.f32(1.0), variant=variant)[:3]
    r = A.worst_ratios(bad, p, g, m, v, h, t, A.f32(1.0))
    print("%s at t %d: %.3g x the bound" % (variant, t, max(r)))
    assert max(r) > 2.0 and max(r) >= least


def test_scalars_and_clip_coefficient():
    h = A.Hyper(lr=0.002, noam=True, warmup_steps=100)
    ss, isb, lr = A.step_scalars(h, 10)
    lr0 = float(np.float32(0.002))
    assert lr == np.float32(lr0 * 10 * 100 ** -1.5) and lr.dtype == np.float32        # warm-up: t * warmup^-1.5
    ss, isb, lr = A.step_scalars(h, 1000)
    assert lr == np.float32(lr0 * 1000 ** -0.5)                                       # after it: t^-0.5
    assert ss == np.float32(lr0 * 1000 ** -0.5 / (1.0 - float(np.float32(0.9)) ** 1000))
    assert isb == np.float32(1.0 / (1.0 - float(np.float32(0.999)) ** 1000) ** 0.5)
    h = A.Hyper(max_grad_norm=0.5, grad_scale=0.125)
    assert A.clip_gmul(h, np.float32(0.1)) == np.float32(0.125)                  # clip inactive
    assert A.clip_gmul(h, np.float32(4.0)) == np.float32(0.5) / (np.float32(4.0) + np.float32(1e-6)) * np.float32(0.125)
    assert np.isnan(A.clip_gmul(h, np.float32('nan'))) and A.clip_gmul(h, np.float32('inf')) == 0.0
    assert A.clip_gmul(A.Hyper(max_grad_norm=0.0), np.float32('nan')) == 1.0     # no clip: the norm does not enter
