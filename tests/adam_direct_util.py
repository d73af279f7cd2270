"""Plumbing of the direct optimizer tests (test_gpu_adam_direct.py, test_gpu_adam_rows_direct.py): tensors laid out by hand inside
four flat device buffers with canaries between them, a plan written through the raw C ABI the way ``Optimizer._build_plan`` does
it, and the comparison with oracle/adam64.py."""
import ctypes as C
import math

import numpy as np
import torch

from oracle import adam64 as A
from prodsearch_amd import _lib

CANARY = np.float32(-12345.678)
GUARD = 8                     # canary floats in front of and behind every tensor (a multiple of 4: keeps 16-byte alignment)
NAMES = ('p', 'g', 'm', 'v')


class Flat(object):
    """Tensors of ``numels`` elements inside four flat buffers.  ``shift[name]`` floats move every tensor of that buffer off the
    16-byte grid (float-aligned views into a larger buffer: the scalar path of the kernels)."""

    def __init__(self, numels, shift=None):
        self.numels = [int(n) for n in numels]
        self.shift = dict.fromkeys(NAMES, 0)
        self.shift.update(shift or {})
        self.off, o = [], GUARD
        for n in self.numels:
            self.off.append(o)
            o += (n + 3) // 4 * 4 + GUARD
        self.total = o + 4
        self.n = int(sum(self.numels))
        self.idx = np.concatenate([np.arange(o, o + n) for o, n in zip(self.off, self.numels)])      # flat index of element k
        self.host = {k: np.full(self.total, CANARY, dtype=np.float32) for k in NAMES}
        self.dev = {}

    def set(self, **vals):
        """values of all tensors back to back, per buffer"""
        for k, x in vals.items():
            assert x.shape == (self.n,) and x.dtype == np.float32
            self.host[k][self.idx + self.shift[k]] = x

    def get_host(self, k):
        return self.host[k][self.idx + self.shift[k]].copy()

    def upload(self):
        self.dev = {k: torch.from_numpy(self.host[k]).cuda() for k in NAMES}
        for k in NAMES:
            assert self.dev[k].data_ptr() % 16 == 0

    def ptr(self, k, i):
        return self.dev[k].data_ptr() + 4 * (self.off[i] + self.shift[k])

    def download(self):
        """({name: values of all tensors back to back}, every canary of every buffer intact)"""
        torch.cuda.synchronize()
        out, clean = {}, True
        for k in NAMES:
            full = self.dev[k].cpu().numpy()
            owned = np.zeros(self.total, dtype=bool)
            owned[self.idx + self.shift[k]] = True
            clean = clean and bool(np.all(full[~owned] == CANARY))
            out[k] = full[self.idx + self.shift[k]].copy()
        return out, clean

    def tensor_slices(self):
        o, out = 0, []
        for n in self.numels:
            out.append(slice(o, o + n))
            o += n
        return out


class Plan(object):
    """``ps_adam_plan_*`` over the tensors ``which`` of a Flat (default all), state and gnorm buffers included."""

    def __init__(self, flat, which=None, step=0, extra_state_floats=0):
        lib = _lib.load()
        which = list(range(len(flat.numels))) if which is None else list(which)
        n = len(which)
        numel = torch.tensor([flat.numels[i] for i in which], dtype=torch.int64)
        addr = lambda k: torch.tensor([flat.ptr(k, i) for i in which], dtype=torch.int64)
        pa, ga, ma, va = addr('p'), addr('g'), addr('m'), addr('v')
        nbytes = lib.ps_adam_plan_bytes(n, numel.data_ptr())
        host = torch.zeros(nbytes, dtype=torch.uint8)
        _lib.check(lib.ps_adam_plan_write_host(n, pa.data_ptr(), ga.data_ptr(), ma.data_ptr(), va.data_ptr(), numel.data_ptr(),
                                               host.data_ptr()), 'ps_adam_plan_write_host')
        self.n_chunks = lib.ps_adam_plan_chunks_host(host.data_ptr())
        assert self.n_chunks == sum((flat.numels[i] + 4095) // 4096 for i in which)
        self.dev = host.cuda()
        self.state = torch.zeros(2 + (self.n_chunks + extra_state_floats + 1) // 2 + 1, dtype=torch.int64, device='cuda')
        self.state[0] = int(step)
        self.gnorm = torch.full((2,), -1.0, device='cuda')

    def step_count(self):
        return int(self.state[0].item())


def c_hyper(h, zero_grads=0):
    """oracle Hyper -> PsAdamHyper (the values are float32 already: nothing is rounded again)"""
    hp = _lib.PsAdamHyper()
    hp.lr, hp.beta1, hp.beta2, hp.eps = float(h.lr), float(h.beta1), float(h.beta2), float(h.eps)
    hp.weight_decay, hp.max_grad_norm = float(h.weight_decay), float(h.max_grad_norm)
    hp.noam, hp.warmup_steps, hp.grad_scale = int(h.noam), int(h.warmup_steps), float(h.grad_scale)
    hp.zero_grads, hp.method = int(zero_grads), 0
    return hp


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the clip norm: the longest chain of float32 additions a squared gradient passes through, counted in the kernels
CHUNK_CHAIN = 16      # adam_sumsq_chunk: 4096 elements over 256 threads on the scalar path = 16 `s += x * x` per thread
#                       (the float4 path: 3 additions inside the expression + 4 `s +=` = 7)
BLOCK_CHAIN = 6 + 3   # block_sum_256: wave_sum = 6 DPP additions (row_shr 1, 2, 4, 8, row_bcast 15, 31), then sh[0] + .. + sh[3]


def dense_chain(n_chunks):
    """ps_clip_adam_dense / ps_adam_sumsq: chunk sum, then strided_sum_f32<8> over 256 threads (ceil(n_chunks / 256) additions per
    thread, the padded slots add an exact 0), then block_sum_256 again."""
    return CHUNK_CHAIN + BLOCK_CHAIN + int(math.ceil(n_chunks / 256.0)) + BLOCK_CHAIN


def rows_chain(n_partials, d_max, dense):
    """ps_clip_adam_rowsparse / ps_rowsparse_sumsq: a row lane adds ceil(d / 128) float4 groups (3 additions inside, one `acc +=`
    each), block_sum_256, then rs_finalize / rs_two_sums: strided_sum_f32<8> over 1024 threads, wave_sum (6), 16 serial additions."""
    lane = int(math.ceil(d_max / 128.0)) + 3
    return max(CHUNK_CHAIN if dense else 0, lane) + BLOCK_CHAIN + int(math.ceil(n_partials / 1024.0)) + 6 + 16


def check_norm(got, g, h, chain, what=''):
    """``got`` against the float64 norm of g * grad_scale under the derived bound; returns error / bound."""
    ref = math.sqrt(float(np.sum((g.astype(np.float64) * float(h.grad_scale)) ** 2)))
    lim = A.norm_rel_bound(chain) * ref
    err = abs(float(got) - ref)
    ratio = err / lim if lim > 0 else (0.0 if err == 0 else float('inf'))
    print("%s norm %.9g (float64 %.9g): error / bound %.3f with a chain of %d additions" % (what, float(got), ref, ratio, chain))
    assert ratio <= 1.0, (what, float(got), ref, chain)
    return ratio


def check_sumsq(got, gs, h, chain, what=''):
    """a float32 sum of squares of the arrays ``gs`` (times grad_scale) against float64: (chain + 2) u relative; nothing = exactly 0"""
    ref = float(sum(np.sum((g.astype(np.float64) * float(h.grad_scale)) ** 2) for g in gs))
    lim = (chain + 2) * A.U * ref
    err = abs(float(got) - ref)
    print("%s sum of squares %.9g (float64 %.9g): error / bound %.3f" % (what, float(got), ref, err / lim if lim else err))
    assert err <= lim, (what, float(got), ref, chain)


def check_lr(got, h, t):
    """gnorm_out[1] = the step's learning rate (adam_step_scalars, float64 then float32: one float32 ulp for the device's pow)"""
    want = float(A.step_scalars(h, t)[2])
    assert abs(float(got) - want) <= 2.0 ** -23 * want, (float(got), want, t)


def check_elements(after, before, h, t, gmul, what=''):
    """p, m, v of ``after`` within 2 x bound of step64(before); returns the three worst error / bound ratios."""
    r = A.worst_ratios((after['p'], after['m'], after['v']), before['p'], before['g'], before['m'], before['v'], h, t, gmul)
    print("%s t %d: error / bound p %.4f m %.4f v %.4f" % ((what, t) + r))
    assert max(r) <= 2.0 and not any(math.isnan(x) for x in r), (what, t, r)
    return r


def draw_grads(rng, n, g_hi, grad_scale):
    """|g| log-uniform in 1e-6..g_hi with 30 % exact zeros, divided by grad_scale (a power of two) so that the clip sees g_hi"""
    return (A.draw(rng, n, 1e-6, g_hi, 0.3) / np.float32(grad_scale)).astype(np.float32)


def row_table(p, g, m, v, rows, count, cap, d):
    t = _lib.PsRowTable()
    t.p, t.g, t.m, t.v = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
    t.rows, t.count, t.cap, t.d = rows.data_ptr(), count.data_ptr(), int(cap), int(d)
    return t


def tables(ts):
    arr = (_lib.PsRowTable * max(len(ts), 1))()
    for i, t in enumerate(ts):
        for f, _ in _lib.PsRowTable._fields_:
            setattr(arr[i], f, getattr(t, f))
    return arr


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


__all__ = ['A', 'C', 'Flat', 'Plan', 'c_hyper', 'stream', 'dense_chain', 'rows_chain', 'check_norm', 'check_lr', 'check_elements',
           'draw_grads', 'row_table', 'tables', 'same_bits', 'CANARY']
