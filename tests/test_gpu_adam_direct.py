"""The dense clip + Adam kernels (csrc/optim.hip, optim_core.h) through the raw C ABI against a float64 Adam, element by element.

Every test writes its own plan (``ps_adam_plan_bytes`` / ``ps_adam_plan_write_host``) over tensors it laid out by hand, presets the
step counter ``state[0]`` and compares every element of p, m, v with ``oracle.adam64.step64`` under 2 x ``oracle.adam64.bound``
(tests/test_adam_bound_cpu.py shows what that bound lets through and what it catches).  The clip norm is judged on its own — its
relative bound is counted from the kernels: a squared gradient passes through at most 16 additions in ``adam_sumsq_chunk`` (the
scalar path: 4096 elements over 256 threads; 7 on the float4 path), 9 in ``block_sum_256`` (6 DPP additions of ``wave_sum`` + 3),
ceil(n_chunks / 256) in ``strided_sum_f32<8>`` and 9 in the final block sum: 45 for the 2,702 chunks here, so (45 + 2) u on the sum
of squares and 47/2 u + u = 24.5 u on the norm (u = 2^-24) — and the elements are then judged with the clip coefficient that
``adam_scalars``' float32 formula gives for the REPORTED norm.

Measured on an MI355X: the figures stand in the docstrings of the tests and in DESIGN.md 5b.
"""
import math

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

from adam_direct_util import (A, Flat, Plan, c_hyper, check_elements, check_lr, check_norm, dense_chain, draw_grads, same_bits,
                              stream)
from prodsearch_amd import _lib

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B, D = 300, 18358, 128
NUMELS = [1, 3, 4, 5, 255, 257, 4095, 4096, 4097, 8191, 8192, 12292, ROWS_A * D, ROWS_B * D] + [1] * 2100
WARM = 100
# (state[0] before the step, noam, weight_decay, max_grad_norm, grad_scale, zero_grads): every value of every option, each step
# count under both schedules, noam below (t = 1, 2, 10) and above (1000, 1e5, 1e6 + 1) its warm-up of 100 steps
COMBOS = [(0, 0, 0.0, 5.0, 1.0, 0), (1, 0, 1e-3, 0.5, 0.125, 1), (9, 1, 0.0, 0.5, 1.0, 1), (999, 1, 1e-3, 5.0, 0.125, 0),
          (99999, 0, 1e-3, 0.0, 1.0, 1), (10 ** 6, 1, 0.0, 0.0, 0.125, 0), (0, 1, 1e-3, 0.0, 1.0, 1), (1, 1, 0.0, 5.0, 0.125, 0),
          (9, 0, 1e-3, 5.0, 1.0, 1), (999, 0, 0.0, 0.5, 1.0, 0), (99999, 1, 0.0, 0.5, 0.125, 1), (10 ** 6, 0, 1e-3, 5.0, 1.0, 1)]


def _zero_runs(g, flat):
    """whole zero runs: table rows without gradient (70 % of them), and runs that start and end inside a chunk at offsets that are
    not multiples of 4 — the non-zero mask then works on 16-byte groups that are all zero, all non-zero and mixed"""
    sl = flat.tensor_slices()
    rng = np.random.default_rng(99)
    for i, rows in ((12, ROWS_A), (13, ROWS_B)):
        x = g[sl[i]].reshape(rows, D)
        x[rng.random(rows) < 0.7] = 0.0
    g[sl[11]][1001:1999] = 0.0                   # 12292 elements: inside its first chunk
    g[sl[10]][4096 + 5:4096 + 1022] = 0.0        # 8192 elements: inside its second chunk
    g[sl[7]][2:4095] = 0.0                       # the one-chunk tensor: all but three elements


@pytest.fixture(scope='module')
def big():
    assert sum((n + 4095) // 4096 for n in NUMELS) > 2048      # strided_sum_f32<8> over 256 threads takes a second trip
    return Flat(NUMELS)


@pytest.mark.parametrize('t0,noam,wd,clip,gs,zero', COMBOS)
def test_one_step_matches_float64_element_by_element(big, t0, noam, wd, clip, gs, zero):
    """Measured on an MI355X over the twelve cases: error / bound at most 0.9991 for p, 0.98 for m, 0.87 for v; the norm within 0.03
    of its bound (chain of 45 additions)."""
    lib, flat = _lib.load(), big
    rng = np.random.default_rng([t0, noam, int(zero)])
    p, _, m, v = A.draw_state(rng, flat.n)
    g = draw_grads(rng, flat.n, 1e-2, gs)
    _zero_runs(g, flat)
    flat.set(p=p, g=g, m=m, v=v)
    flat.upload()
    plan = Plan(flat, step=t0)
    assert plan.n_chunks > 2048
    h = A.Hyper(weight_decay=wd, max_grad_norm=clip, noam=bool(noam), warmup_steps=WARM, grad_scale=gs)
    _lib.check(lib.ps_clip_adam_dense(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, zero), plan.state.data_ptr(),
                                      plan.gnorm.data_ptr(), stream()), 'ps_clip_adam_dense')
    after, clean = flat.download()
    t = t0 + 1
    assert plan.step_count() == t and clean
    norm, lr = [np.float32(x) for x in plan.gnorm.cpu().numpy()]
    check_norm(norm, g, h, dense_chain(plan.n_chunks), 'dense')
    check_lr(lr, h, t)
    gmul = A.clip_gmul(h, norm)
    if clip:                                     # 5.0 leaves the gradients alone, 0.5 clips them
        assert (float(gmul) == gs) == (clip == 5.0), (float(norm), clip)
    check_elements(after, dict(p=p, g=g, m=m, v=v), h, t, gmul, 'dense')
    if zero:
        assert not after['g'].any()
    else:
        assert same_bits(after['g'], g)


@pytest.mark.parametrize('wd', [0.0, 1e-3])
def test_layout_does_not_change_a_bit(wd):
    """The float4 path, the scalar tail and the scalar path of a misaligned tensor are the same arithmetic: one step over a
    full-chunk tensor, one of three chunks and a tail, and a short one — 16-byte aligned, with each of p, g, m, v in turn one
    float off the grid, and with all four off it — gives the same bits."""
    lib = _lib.load()
    numels = [4096, 3 * 4096 + 777, 37]
    rng = np.random.default_rng(5)
    n = sum(numels)
    p, _, m, v = A.draw_state(rng, n)
    g = draw_grads(rng, n, 1e-2, 1.0)
    g[100:1500] = 0.0
    g[4096 + 4096 + 7:4096 + 4096 + 3001] = 0.0
    h = A.Hyper(weight_decay=wd, max_grad_norm=0.0)
    results = []
    for shift in ({}, {'p': 1}, {'g': 1}, {'m': 1}, {'v': 1}, {'p': 1, 'g': 1, 'm': 1, 'v': 1}):
        flat = Flat(numels, shift)
        flat.set(p=p, g=g, m=m, v=v)
        flat.upload()
        plan = Plan(flat, step=6)
        _lib.check(lib.ps_clip_adam_dense(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, 1), plan.state.data_ptr(),
                                          plan.gnorm.data_ptr(), stream()), 'ps_clip_adam_dense')
        after, clean = flat.download()
        assert clean, shift                      # the floats just before and just after every tensor
        assert not after['g'].any()
        results.append(after)
    check_elements(results[0], dict(p=p, g=g, m=m, v=v), h, 7, np.float32(1.0), 'aligned')
    for shift_no, r in enumerate(results[1:]):
        for k in ('p', 'm', 'v'):
            assert same_bits(r[k], results[0][k]), (shift_no + 1, k)


def _fresh(numels, seed, g_hi=0.1):
    rng = np.random.default_rng(seed)
    n = sum(numels)
    p, _, m, v = A.draw_state(rng, n)
    g = draw_grads(rng, n, g_hi, 1.0)
    g[3000:9000] = 0.0
    return dict(p=p, g=g, m=m, v=v)


def test_split_form_equals_the_fused_one_bitwise():
    """ps_adam_sumsq + ps_adam_update_ext fed its own sum = ps_clip_adam_dense: both reduce the chunk partials in the same order."""
    lib = _lib.load()
    numels = [4096 * 3, 5000, 1, 12292] + [3] * 2300        # > 2048 chunks here too
    before = _fresh(numels, 8)
    h = A.Hyper(weight_decay=1e-3, max_grad_norm=0.5)
    out = []
    for split in (False, True):
        flat = Flat(numels)
        flat.set(**before)
        flat.upload()
        plan = Plan(flat, step=41)
        if split:
            total = torch.full((1,), -1.0, device='cuda')
            _lib.check(lib.ps_adam_sumsq(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, 1), plan.state.data_ptr(),
                                         total.data_ptr(), stream()), 'ps_adam_sumsq')
            _lib.check(lib.ps_adam_update_ext(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, 1), plan.state.data_ptr(),
                                              total.data_ptr(), plan.gnorm.data_ptr(), stream()), 'ps_adam_update_ext')
        else:
            _lib.check(lib.ps_clip_adam_dense(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, 1), plan.state.data_ptr(),
                                              plan.gnorm.data_ptr(), stream()), 'ps_clip_adam_dense')
        after, clean = flat.download()
        assert clean and not after['g'].any()
        out.append((after, plan.gnorm.cpu().numpy(), plan.step_count()))
    (a, ga, sa), (b, gb, sb) = out
    assert sa == sb == 42 and same_bits(ga, gb)
    assert float(A.clip_gmul(h, np.float32(ga[0]))) < 1.0   # clipped: the norm enters every element
    for k in ('p', 'm', 'v'):
        assert same_bits(a[k], b[k]), k


def test_split_form_with_the_sum_of_two_half_plans():
    """The sharded optimizer's use: two plans over halves of the tensors, their sums of squares added (the all-reduce), both updated
    with the total: one step64 with the coefficient of the combined norm.  Measured: error / bound 0.99 / 0.94 / 0.61, the norm within 0.02 of its bound."""
    lib = _lib.load()
    numels = [4096 * 2, 5000, 777, 12292, 4096, 3]
    before = _fresh(numels, 9)
    h = A.Hyper(max_grad_norm=0.5, noam=True, warmup_steps=WARM)
    flat = Flat(numels)
    flat.set(**before)
    flat.upload()
    plans = [Plan(flat, which=[0, 1, 2], step=499), Plan(flat, which=[3, 4, 5], step=499)]
    sums = [torch.full((1,), -1.0, device='cuda') for _ in plans]
    for pl, s in zip(plans, sums):
        _lib.check(lib.ps_adam_sumsq(pl.dev.data_ptr(), pl.n_chunks, c_hyper(h, 0), pl.state.data_ptr(), s.data_ptr(), stream()),
                   'ps_adam_sumsq')
    total = sums[0] + sums[1]
    for pl in plans:
        _lib.check(lib.ps_adam_update_ext(pl.dev.data_ptr(), pl.n_chunks, c_hyper(h, 0), pl.state.data_ptr(), total.data_ptr(),
                                          pl.gnorm.data_ptr(), stream()), 'ps_adam_update_ext')
    after, clean = flat.download()
    assert clean and same_bits(after['g'], before['g'])
    g0, g1 = plans[0].gnorm.cpu().numpy(), plans[1].gnorm.cpu().numpy()
    assert same_bits(g0, g1) and plans[0].step_count() == plans[1].step_count() == 500
    # each half: dense_chain of its chunks; the sum of the two: one more addition
    check_norm(g0[0], before['g'], h, dense_chain(max(pl.n_chunks for pl in plans)) + 1, 'two halves')
    check_lr(g0[1], h, 500)
    gmul = A.clip_gmul(h, np.float32(g0[0]))
    assert float(gmul) < 1.0
    check_elements(after, before, h, 500, gmul, 'two halves')


def test_fifty_free_running_steps_against_float64_and_cpu_torch():
    """Fifty steps from zero moments, fresh gradients each step (|g| in 1e-3..10: no element at the eps scale, where Adam turns
    noise into +-lr), weight decay 1e-3.  Yardstick: torch.optim.Adam in float32 on the CPU on the same gradients; both are compared
    with one float64 free run (torch's beta convention).  Per tensor the kernel's largest error may be at most 3 x the CPU run's:
    both are sums of about 50 independent roundings per element, and maxima over 1e5..1e6 such elements differ by tens of per cent,
    not by multiples.  Measured on an MI355X: 1.00 x for each of the three tensors (largest errors 6.6e-7, 6.7e-7, 7.2e-7 on both sides)."""
    lib = _lib.load()
    numels = [1000 * 128, 100003, 262144 + 1]
    steps, lr, wd = 50, 0.002, 1e-3
    rng = np.random.default_rng(21)
    n = sum(numels)
    p0 = A.draw(rng, n, 1e-3, 1.0)
    flat = Flat(numels)
    zeros = np.zeros(n, dtype=np.float32)
    flat.set(p=p0, g=zeros, m=zeros, v=zeros)
    flat.upload()
    plan = Plan(flat, step=0)
    h = A.Hyper(lr=lr, weight_decay=wd, max_grad_norm=0.0)
    ht = A.Hyper(lr=lr, weight_decay=wd, max_grad_norm=0.0, torch_betas=True)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    topt = torch.optim.Adam([tp], lr=lr, betas=(0.9, 0.999), eps=1e-9, weight_decay=wd)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    g_idx = torch.from_numpy(flat.idx + flat.shift['g']).cuda()
    for t in range(1, steps + 1):
        g = A.draw(rng, n, 1e-3, 10.0)
        flat.dev['g'][g_idx] = torch.from_numpy(g).cuda()
        _lib.check(lib.ps_clip_adam_dense(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, 0), plan.state.data_ptr(),
                                          plan.gnorm.data_ptr(), stream()), 'ps_clip_adam_dense')
        tp.grad = torch.from_numpy(g.copy())
        topt.step()
        ss, isb, _ = [float(x) for x in A.step_scalars(ht, t)]
        gg = g.astype(np.float64) + float(ht.weight_decay) * p64                   # float64 throughout: not step64, which
        m64 = m64 + (gg - m64) * float(ht.omb1)                                    # starts every step from float32 inputs
        v64 = v64 * float(ht.beta2) + float(ht.omb2) * gg * gg
        p64 = p64 - ss * (m64 / (np.sqrt(v64) * isb + float(ht.eps)))
    after, clean = flat.download()
    assert clean and plan.step_count() == steps
    cpu = tp.detach().numpy().astype(np.float64)
    for i, sl in enumerate(flat.tensor_slices()):
        e_gpu = float(np.abs(after['p'][sl].astype(np.float64) - p64[sl]).max())
        e_cpu = float(np.abs(cpu[sl] - p64[sl]).max())
        print("tensor %d (%d elements): kernel %.3g, CPU float32 torch %.3g: %.2f x" % (i, numels[i], e_gpu, e_cpu, e_gpu / e_cpu))
        assert e_gpu <= 3.0 * e_cpu, (i, e_gpu, e_cpu)


def _torch_expectation(before, numels, h, t):
    """clip_grad_norm_ + torch.optim.Adam (float32, CPU) from the same state: (p', norm)"""
    ps, o = [], 0
    for n in numels:
        q = torch.nn.Parameter(torch.from_numpy(before['p'][o:o + n].copy()))
        q.grad = torch.from_numpy(before['g'][o:o + n].copy())
        ps.append(q)
        o += n
    opt = torch.optim.Adam(ps, lr=float(h.lr), betas=(0.9, 0.999), eps=1e-9, weight_decay=float(h.weight_decay))
    o = 0
    for q, n in zip(ps, numels):
        opt.state[q] = {'step': torch.tensor(float(t - 1)), 'exp_avg': torch.from_numpy(before['m'][o:o + n].copy()),
                        'exp_avg_sq': torch.from_numpy(before['v'][o:o + n].copy())}
        o += n
    norm = clip_grad_norm_(ps, float(h.max_grad_norm))
    opt.step()
    return np.concatenate([q.detach().numpy() for q in ps]), float(norm)


@pytest.mark.parametrize('bad', ['nan', 'inf'])
def test_non_finite_gradients_behave_as_in_torch(bad):
    """One NaN (or one Inf) in one tensor of the plan; the expectation is what clip_grad_norm_ + torch.optim.Adam do on the CPU.
    NaN: the norm is NaN, the clip coefficient is NaN (torch clamps NaN to NaN) and EVERY parameter of the plan becomes NaN.
    Inf: the norm is Inf, the coefficient 0: the Inf element becomes NaN (Inf * 0) and every other parameter takes the
    zero-gradient step.  On an MI355X the NaN case first gave 1 NaN parameter of 9,133 where torch gives 9,133 — ``fminf(NaN, 1.f)``
    is 1 — and ``adam_scalars`` now hands a NaN norm on to the coefficient."""
    lib = _lib.load()
    numels = [4096, 5000, 37]
    before = _fresh(numels, 31)
    where = 4096 + 1234
    before['g'][where] = np.float32(bad)
    h = A.Hyper(max_grad_norm=5.0, weight_decay=1e-3)
    t = 6
    want_p, want_norm = _torch_expectation(before, numels, h, t)
    flat = Flat(numels)
    flat.set(**before)
    flat.upload()
    plan = Plan(flat, step=t - 1)
    _lib.check(lib.ps_clip_adam_dense(plan.dev.data_ptr(), plan.n_chunks, c_hyper(h, 0), plan.state.data_ptr(),
                                      plan.gnorm.data_ptr(), stream()), 'ps_clip_adam_dense')
    after, clean = flat.download()
    norm = float(plan.gnorm.cpu().numpy()[0])
    assert clean
    print("%s gradient: norm %r (torch %r), NaN parameters %d (torch %d) of %d"
          % (bad, norm, want_norm, int(np.isnan(after['p']).sum()), int(np.isnan(want_p).sum()), want_p.size))
    if bad == 'nan':
        assert math.isnan(want_norm) and np.isnan(want_p).all()                 # what torch does
        assert math.isnan(norm)
        assert np.isnan(after['p']).all()
    else:
        assert math.isinf(want_norm) and np.isnan(want_p).sum() == 1 and np.isnan(want_p[where])
        assert math.isinf(norm) and norm > 0
        assert np.array_equal(np.isnan(after['p']), np.isnan(want_p))
        rest = np.ones(want_p.size, dtype=bool)
        rest[where] = False
        cut = lambda d: {k: x[rest] for k, x in d.items()}
        check_elements(cut(after), cut(before), h, t, A.clip_gmul(h, np.float32(norm)), 'beside the Inf')
        assert float(A.clip_gmul(h, np.float32(norm))) == 0.0
