"""Float64 yardstick for the clip + Adam kernels (csrc/optim_core.h), with a per-element rounding bound.

``adam_elem`` pins one float32 operation sequence (no contraction left to the compiler):

    gg  = fl(g * gmul);  weight_decay != 0:  gg = fl(wd * p + gg)              (one fma)
    m'  = fl(fl(gg - m) * (1 - b1) + m)                                         (one subtraction, one fma)
    v'  = fl(fl(v * b2) + fl(fl((1 - b2) * gg) * gg))
    den = fl(fl(fl(sqrt(v')) * isb) + eps)
    p'  = fl(p - fl(ss * fl(m' / den)))

with ``ss = lr_t / (1 - b1^t)`` and ``isb = 1 / sqrt(1 - b2^t)`` computed in float64 from the FLOAT32 hyper-parameters and then
rounded to float32 (``adam_step_scalars``), and ``1 - b`` formed in float32.  ``step64`` evaluates the same expressions in float64
from the same float32 inputs and the same float32 scalars: what is left between it and a correct kernel is the rounding of the
operations above, and ``bound`` propagates exactly those roundings to first order (u = 2^-24).  ``step32_numpy`` restates the
sequence in float32 on the CPU; it is the yardstick the bound was tried on, never the code under test.

CPU only: numpy, no torch, no GPU.
"""
import math

import numpy as np

U = 2.0 ** -24
f32 = np.float32


class Hyper(object):
    """The fields of PsAdamHyper that enter the arithmetic, each rounded to float32 (the struct carries floats)."""

    def __init__(self, lr=0.002, beta1=0.9, beta2=0.999, eps=1e-9, weight_decay=0.0, max_grad_norm=0.0, noam=False,
                 warmup_steps=4000, grad_scale=1.0, torch_betas=False):
        self.lr, self.beta1, self.beta2, self.eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
        self.weight_decay, self.max_grad_norm = f32(weight_decay), f32(max_grad_norm)
        self.noam, self.warmup_steps = bool(noam), int(warmup_steps)
        self.grad_scale = f32(grad_scale if grad_scale != 0 else 1.0)      # (the entry points read 0 as 1)
        self.omb1 = f32(1.0) - self.beta1                                  # 1 - beta formed in float32, as adam_elem does
        self.omb2 = f32(1.0) - self.beta2
        if torch_betas:
            # torch.optim.Adam keeps its betas as Python floats: `1 - beta` and the bias corrections are formed from the DOUBLE
            # betas (the weights then rounded to float32 by the element kernels), while mul_(beta2) rounds beta2 itself
            self.omb1, self.omb2 = f32(1.0 - float(beta1)), f32(1.0 - float(beta2))
            self.bc_beta1, self.bc_beta2 = float(beta1), float(beta2)
        else:
            self.bc_beta1, self.bc_beta2 = float(self.beta1), float(self.beta2)     # the betas of the bias corrections


def step_scalars(h, t):
    """``adam_step_scalars``: (step_size, 1/sqrt(bias_correction2), lr) of step ``t``: float64, then rounded to float32."""
    t = float(t)
    lr = float(h.lr)
    if h.noam:
        lr = float(h.lr) * min(t ** -0.5, t * float(h.warmup_steps) ** -1.5)
    bc1 = 1.0 - h.bc_beta1 ** t
    bc2 = 1.0 - h.bc_beta2 ** t
    return f32(lr / bc1), f32(1.0 / math.sqrt(bc2)), f32(lr)


def clip_gmul(h, norm):
    """``adam_scalars``' float32 formula: the factor every gradient is multiplied by, from the (float32) norm.  A NaN norm gives a
    NaN factor here, as under ``clip_grad_norm_`` (torch clamps NaN to NaN); the kernel's ``fminf(NaN, 1.f)`` gives 1."""
    coef = f32(1.0)
    if h.max_grad_norm > 0:
        with np.errstate(all='ignore'):
            c = h.max_grad_norm / (f32(norm) + f32(1e-6))
        coef = c if (c < 1.0 or c != c) else f32(1.0)
    return f32(coef * h.grad_scale)


def norm_rel_bound(chain):
    """Relative error bound of a float32 norm whose sum of squares adds non-negative terms, any term passing through at most
    ``chain`` float32 additions: (chain + 2) u on the sum (the additions, the square, and the last rounding of a fused
    square-and-add), half of it plus the rounding of the square root on the norm."""
    return 0.5 * (chain + 2) * U + U


def _f64(*xs):
    return [np.asarray(x, dtype=np.float32).astype(np.float64) for x in xs]


def step64(p, g, m, v, h, t, gmul, variant=None):
    """One Adam step in float64 from the float32 inputs.  Returns (p', m', v', upd) as float64 arrays.
    ``variant`` builds a deliberately WRONG step (the CPU test shows the bound notices): 'eps8' (eps 1e-8), 'nobc2' (the second
    bias correction dropped), 'wd_after' (weight decay added to the update instead of the gradient)."""
    p, g, m, v = _f64(p, g, m, v)
    ss, isb, _ = [float(x) for x in step_scalars(h, t)]
    eps, wd = float(h.eps), float(h.weight_decay)
    if variant == 'eps8':
        eps = float(f32(1e-8))
    if variant == 'nobc2':
        isb = 1.0
    gg = g * float(gmul)
    if wd != 0.0 and variant != 'wd_after':
        gg = wd * p + gg
    m2 = (gg - m) * float(h.omb1) + m
    v2 = v * float(h.beta2) + (float(h.omb2) * gg) * gg
    den = np.sqrt(v2) * isb + eps
    upd = ss * (m2 / den)
    if variant == 'wd_after':
        upd = upd + float(h.lr) * wd * p
    return p - upd, m2, v2, upd


def bound(p, g, m, v, h, t, gmul):
    """First-order propagated rounding bound of ``adam_elem`` per element: (dp, dm, dv) in float64."""
    p, g, m, v = _f64(p, g, m, v)
    ss, isb, _ = [float(x) for x in step_scalars(h, t)]
    eps, wd = float(h.eps), float(h.weight_decay)
    b2, omb1, omb2 = float(h.beta2), float(h.omb1), float(h.omb2)
    gg = g * float(gmul)
    dgg = U * np.abs(gg)                                         # the gmul product
    if wd != 0.0:
        gg = wd * p + gg
        dgg = dgg + U * np.abs(gg)                               # the fma
    m2 = (gg - m) * omb1 + m
    v2 = v * b2 + (omb2 * gg) * gg
    dm = U * np.abs(m2) + omb1 * (U * np.abs(gg - m) + dgg)
    dv = U * (np.abs(v * b2) + 2.0 * omb2 * gg * gg + v2) + 2.0 * omb2 * np.abs(gg) * dgg
    sq = np.sqrt(v2)
    dsq = U * sq + (np.sqrt(v2 + dv) - np.sqrt(np.maximum(v2 - dv, 0.0)))
    den = sq * isb + eps
    dden = isb * dsq + U * isb * sq + U * den
    q = m2 / den
    dq = dm / den + np.abs(q) * dden / den + U * np.abs(q)
    upd = ss * q
    dupd = ss * dq + U * np.abs(upd)
    dp = dupd + U * np.abs(p - upd)
    return dp, dm, dv + U * v2


def step32_numpy(p, g, m, v, h, t, gmul):
    """The same operation sequence in float32 on the CPU (each fma through a float64 product: the product of two float32 is
    exact in float64, and the one rounding of the sum to float32 is the fma's up to double rounding).  Returns float32 (p', m', v')."""
    p, g, m, v = [np.asarray(x, dtype=np.float32) for x in (p, g, m, v)]
    ss, isb, _ = step_scalars(h, t)

    def fma(a, b, c):
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)
    gg = g * f32(gmul)
    if h.weight_decay != 0:
        gg = fma(h.weight_decay, p, gg)
    m2 = fma(gg - m, h.omb1, m)
    v2 = v * h.beta2 + (h.omb2 * gg) * gg
    den = np.sqrt(v2) * isb + h.eps
    p2 = p - ss * (m2 / den)
    assert p2.dtype == np.float32 and m2.dtype == np.float32 and v2.dtype == np.float32
    return p2, m2, v2


def worst_ratios(got, p, g, m, v, h, t, gmul):
    """max over elements of |got - step64| / bound for (p, m, v); ``got`` = the three arrays under test.  An element whose bound
    is 0 (all of its inputs are 0) must be exact: it counts as 0 when it is and as inf when it is not.  NaN anywhere gives nan."""
    p2, m2, v2, _ = step64(p, g, m, v, h, t, gmul)
    out = []
    for x, ref, d in zip(got, (p2, m2, v2), bound(p, g, m, v, h, t, gmul)):
        err = np.abs(np.asarray(x, dtype=np.float64).reshape(ref.shape) - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(d > 0, err / d, np.where(err == 0, 0.0, np.inf))
        out.append(float(r.max()) if r.size else 0.0)
    return tuple(out)


def draw(rng, n, lo, hi, zero_frac=0.0):
    """n float32 values of either sign, |x| log-uniform in [lo, hi], a fraction of them exactly 0."""
    x = np.exp(rng.uniform(math.log(lo), math.log(hi), n)) * rng.choice([-1.0, 1.0], n)
    if zero_frac:
        x[rng.random(n) < zero_frac] = 0.0
    return x.astype(np.float32)


def draw_state(rng, n):
    """The input ranges the bound was tried on: |p| in 1e-6..10, |g| in 1e-6..1e3 with 30 % exact zeros, m drawn like g, v the
    square of such values (no v underflows in float32)."""
    p = draw(rng, n, 1e-6, 10.0)
    g = draw(rng, n, 1e-6, 1e3, 0.3)
    m = draw(rng, n, 1e-6, 1e3, 0.3)
    v = draw(rng, n, 1e-6, 1e3, 0.3)
    return p, g, m, (v * v).astype(np.float32)
