"""The row-sparse clip + Adam and the lazy catch-up (csrc/optim_rows.hip) through the raw C ABI.

* ``ps_clip_adam_rowsparse`` and its split form against ``oracle.adam64.step64`` under 2 x ``bound``, at row widths beside the
  128 / 256 of the models, with touched-row counts of 0, below the capacity and off the 8 rows of a block; untouched rows, the
  dense plan's gradients and everything outside keep their bits.  The norm bound is counted as in test_gpu_adam_direct.py: a row
  lane adds ceil(d / 128) float4 groups (3 additions inside, one per group), ``block_sum_256`` 9, ``rs_finalize`` /
  ``rs_two_sums`` ceil(n_blocks / 1024) + 6 (``wave_sum``) + 16 serial additions; with a dense plan its chunk sum (16) is the
  longer start: 16 + 9 + 1 + 6 + 16 = 48 here (36 without a dense plan at d <= 128, one more for the split form's sum of two).
* ``ps_rowsparse_catchup`` against the dense kernel stepped T = 3000 times with a zero gradient, bit for bit — through a gap in
  which noam's rate keeps growing (warm-up 4000), and with betas (0.5, 0.9) under which the moments reach their fixed point long
  before T, so that the replay's early stop is taken and has to be right about everything after it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from adam_direct_util import (A, Flat, Plan, c_hyper, check_elements, check_lr, check_norm, check_sumsq, draw_grads, row_table,
                              rows_chain, same_bits, stream, tables)
from prodsearch_amd import _lib

pytestmark = pytest.mark.gpu

N_ROWS, CAP = 5000, 512
DENSE = [4096, 700, 3]


class Table(object):
    def __init__(self, rng, d, count, n_rows=N_ROWS, cap=CAP):
        self.d, self.count, self.n_rows, self.cap = d, count, n_rows, cap
        n = n_rows * d
        p, _, m, v = A.draw_state(rng, n)
        g = draw_grads(rng, n, 1e-2, 1.0)                    # untouched rows hold non-zero gradients too: canaries
        self.host = {k: x.reshape(n_rows, d) for k, x in dict(p=p, g=g, m=m, v=v).items()}
        if count == 1:
            rows = np.array([n_rows - 1])
        elif count:
            mid = np.sort(rng.choice(np.arange(1, n_rows - 1), count - 2, replace=False))
            rows = np.concatenate([[0], mid, [n_rows - 1]])              # sorted, unique, first and last row of the table
        else:
            rows = np.zeros(0, dtype=np.int64)
        self.rows = rows.astype(np.int64)
        spare = np.setdiff1d(np.arange(n_rows), self.rows)[:1]           # past `count` the list names an UNTOUCHED row: a kernel
        lst = np.concatenate([self.rows, np.repeat(spare, cap - count)]).astype(np.int64)     # that read it would be noticed
        self.dev = {k: torch.from_numpy(x.copy()).cuda() for k, x in self.host.items()}
        self.rows_dev = torch.from_numpy(lst).cuda()
        self.count_dev = torch.tensor([count], dtype=torch.int32, device='cuda')

    def c(self):
        return row_table(self.dev['p'], self.dev['g'], self.dev['m'], self.dev['v'], self.rows_dev, self.count_dev, self.cap, self.d)

    def touched(self, k):
        return self.host[k][self.rows].reshape(-1)

    def check(self, h, t, gmul, what):
        torch.cuda.synchronize()
        after = {k: x.cpu().numpy() for k, x in self.dev.items()}
        un = np.ones(self.n_rows, dtype=bool)
        un[self.rows] = False
        for k in ('p', 'g', 'm', 'v'):
            assert same_bits(after[k][un], self.host[k][un]), (what, k, 'an untouched row changed')
        assert not after['g'][self.rows].any(), (what, 'a touched gradient row is not zero')
        if self.count:
            check_elements({k: after[k][self.rows].reshape(-1) for k in 'pmv'}, {k: self.touched(k) for k in 'pgmv'}, h, t, gmul, what)
        return after


def _dense(rng, use):
    if not use:
        return None, None, None
    flat = Flat(DENSE)
    p, _, m, v = A.draw_state(rng, flat.n)
    before = dict(p=p, g=draw_grads(rng, flat.n, 1e-2, 1.0), m=m, v=v)
    flat.set(**before)
    flat.upload()
    return flat, before, Plan(flat, step=0)


def _state(lib, n_chunks, tabs, n_tables, step):
    need = lib.ps_adam_rowsparse_state_floats(n_chunks, tabs, n_tables)
    assert need >= 4 + n_chunks
    st = torch.zeros(2 + (need + 1) // 2 + 1, dtype=torch.int64, device='cuda')
    st[0] = step
    return st, need - 4


@pytest.mark.parametrize('count', [0, 1, 7, 8, 9, 511, 512])
@pytest.mark.parametrize('ds,dense', [((4,), True), ((96, 128), True), ((256,), True), ((260, 128), True), ((128, 96), False)])
def test_rowsparse_step_matches_float64_and_leaves_the_rest_alone(count, ds, dense):
    """Measured on an MI355X over the 35 cases: error / bound at most 0.998 / 0.98 / 0.98 (p / m / v), the norm within 0.07 of its
    bound."""
    lib = _lib.load()
    rng = np.random.default_rng([count, len(ds), ds[0], int(dense)])
    tabs_py = [Table(rng, d, count if i == 0 else CAP - count) for i, d in enumerate(ds)]
    flat, before, plan = _dense(rng, dense)
    tabs = tables([t.c() for t in tabs_py])
    n_chunks = plan.n_chunks if dense else 0
    t0 = 999
    state, n_partial = _state(lib, n_chunks, tabs, len(ds), t0)
    gnorm = torch.full((2,), -1.0, device='cuda')
    h = A.Hyper(weight_decay=1e-3, max_grad_norm=0.5, noam=True, warmup_steps=100)
    _lib.check(lib.ps_clip_adam_rowsparse(plan.dev.data_ptr() if dense else None, n_chunks, tabs, len(ds), c_hyper(h, 1),
                                          state.data_ptr(), gnorm.data_ptr(), stream()), 'ps_clip_adam_rowsparse')
    torch.cuda.synchronize()
    assert int(state[0].item()) == t0 + 1
    norm, lr = [np.float32(x) for x in gnorm.cpu().numpy()]
    allg = np.concatenate([t.touched('g') for t in tabs_py] + ([before['g']] if dense else []))
    what = 'rows d %s count %d%s' % (ds, count, '' if dense else ' (no dense plan)')
    if allg.size:
        check_norm(norm, allg, h, rows_chain(n_partial, max(ds), dense), what)
    else:
        assert float(norm) == 0.0
    check_lr(lr, h, t0 + 1)
    gmul = A.clip_gmul(h, norm)
    for i, t in enumerate(tabs_py):
        t.check(h, t0 + 1, gmul, what + ' table %d' % i)
    if dense:
        after, clean = flat.download()
        assert clean and same_bits(after['g'], before['g'])          # the dense plan's gradients are left alone
        check_elements(after, before, h, t0 + 1, gmul, what + ' dense plan')


def _split_run(lib, seed, clip, n_shared, fused):
    rng = np.random.default_rng(seed)
    tabs_py = [Table(rng, 128, 300), Table(rng, 260, 77)]
    flat, before, plan = _dense(rng, True)
    tabs = tables([t.c() for t in tabs_py])
    state, n_partial = _state(lib, plan.n_chunks, tabs, 2, 41)
    gnorm = torch.full((2,), -1.0, device='cuda')
    sums = torch.full((2,), -1.0, device='cuda')
    h = A.Hyper(weight_decay=1e-3, max_grad_norm=clip)
    if fused:
        _lib.check(lib.ps_clip_adam_rowsparse(plan.dev.data_ptr(), plan.n_chunks, tabs, 2, c_hyper(h), state.data_ptr(),
                                              gnorm.data_ptr(), stream()), 'ps_clip_adam_rowsparse')
    else:
        _lib.check(lib.ps_rowsparse_sumsq(plan.dev.data_ptr(), plan.n_chunks, tabs, 2, n_shared, c_hyper(h), state.data_ptr(),
                                          sums.data_ptr(), stream()), 'ps_rowsparse_sumsq')
        _lib.check(lib.ps_rowsparse_update_ext(plan.dev.data_ptr(), plan.n_chunks, tabs, 2, c_hyper(h), state.data_ptr(),
                                               sums.data_ptr(), gnorm.data_ptr(), stream()), 'ps_rowsparse_update_ext')
    torch.cuda.synchronize()
    return dict(tabs=tabs_py, flat=flat, before=before, h=h, step=int(state[0].item()), gnorm=gnorm.cpu().numpy(),
                sums=sums.cpu().numpy(), n_partial=n_partial)


def test_rowsparse_split_form_without_clipping_equals_the_fused_one_bitwise():
    lib = _lib.load()
    a = _split_run(lib, 3, 0.0, 1, fused=True)
    b = _split_run(lib, 3, 0.0, 1, fused=False)
    assert a['step'] == b['step'] == 42
    assert a['gnorm'][1] == b['gnorm'][1]
    for ta, tb in zip(a['tabs'], b['tabs']):
        for k in ('p', 'g', 'm', 'v'):
            assert same_bits(ta.dev[k].cpu().numpy(), tb.dev[k].cpu().numpy()), k
    fa, ca = a['flat'].download()
    fb, cb = b['flat'].download()
    assert ca and cb
    for k in ('p', 'g', 'm', 'v'):
        assert same_bits(fa[k], fb[k]), k
    for i, t in enumerate(a['tabs']):
        t.check(a['h'], 42, np.float32(1.0), 'fused, no clip, table %d' % i)


@pytest.mark.parametrize('n_shared', [0, 1, 2])
def test_rowsparse_split_form_with_clipping(n_shared):
    """sums[0] = dense plan + the first n_shared tables, sums[1] = the others, each a fixed-order float32 sum; the update takes the
    coefficient of sqrt(sums[0] + sums[1]).  Measured: sums within 0.03 of their bound, elements 0.997 / 0.94 / 0.84."""
    lib = _lib.load()
    r = _split_run(lib, 4, 0.1, n_shared, fused=False)
    tabs_py, h, before = r['tabs'], r['h'], r['before']
    chain = rows_chain(r['n_partial'], 260, True)
    common = [before['g']] + [t.touched('g') for t in tabs_py[:n_shared]]
    owned = [t.touched('g') for t in tabs_py[n_shared:]]
    check_sumsq(r['sums'][0], common, h, chain, 'n_shared %d: sums[0]' % n_shared)
    if owned:
        check_sumsq(r['sums'][1], owned, h, chain, 'n_shared %d: sums[1]' % n_shared)
    else:
        assert float(r['sums'][1]) == 0.0
    norm = np.float32(r['gnorm'][0])
    check_norm(norm, np.concatenate(common + owned), h, chain + 1, 'n_shared %d' % n_shared)      # + the addition of the two sums
    check_lr(r['gnorm'][1], h, 42)
    gmul = A.clip_gmul(h, norm)
    assert float(gmul) < 1.0 and r['step'] == 42
    for i, t in enumerate(tabs_py):
        t.check(h, 42, gmul, 'split, n_shared %d, table %d' % (n_shared, i))
    after, clean = r['flat'].download()
    assert clean and same_bits(after['g'], before['g'])
    check_elements(after, before, h, 42, gmul, 'split, n_shared %d, dense plan' % n_shared)


# ---------------------------------------------------------------- lazy catch-up
T_GAP, R_CATCH = 3000, 24
DS = (100, 128, 256, 512)
SPECIAL = (0.0, 1e-30, 1e-25, 1e-10, 1.0)            # |p| of whole rows 0..4: below, at and above the replay's 1e-20 guard


def _catch_values(seed):
    rng = np.random.default_rng(seed)
    out = []
    for d in DS:
        p, _, m, v = A.draw_state(rng, R_CATCH * d)
        p = p.reshape(R_CATCH, d)
        for r, mag in enumerate(SPECIAL):
            p[r] = np.float32(mag) * np.where(np.arange(d) % 2, -1, 1).astype(np.float32)
        out.append(dict(p=p.reshape(-1), m=m, v=v))
    return out


def _dense_gap(lib, vals, h):
    """the same [rows, d] values as tensors of a dense plan, stepped T_GAP times with a zero gradient and no clipping"""
    flat = Flat([R_CATCH * d for d in DS])
    cat = lambda k: np.concatenate([x[k] for x in vals])
    flat.set(p=cat('p'), g=np.zeros(flat.n, dtype=np.float32), m=cat('m'), v=cat('v'))
    flat.upload()
    plan = Plan(flat, step=0)
    hp = c_hyper(h, 0)
    st = stream()
    for _ in range(T_GAP):
        rc = lib.ps_clip_adam_dense(plan.dev.data_ptr(), plan.n_chunks, hp, plan.state.data_ptr(), plan.gnorm.data_ptr(), st)
        if rc:
            _lib.check(rc, 'ps_clip_adam_dense')
    after, clean = flat.download()
    assert clean and plan.step_count() == T_GAP and not after['g'].any()
    return [{k: after[k][sl].reshape(R_CATCH, -1) for k in 'pmv'} for sl in flat.tensor_slices()]


def _fixed_point_step(vals, h):
    """first step (CPU, step32_numpy) after which neither m nor v of any element changes any more, or None"""
    p, m, v = [np.concatenate([x[k] for x in vals]) for k in 'pmv']
    g = np.zeros_like(p)
    for t in range(1, T_GAP + 1):
        p, m2, v2 = A.step32_numpy(p, g, m, v, h, t, np.float32(1.0))
        if same_bits(m2, m) and same_bits(v2, v):
            return t
        m, v = m2, v2
    return None


def _catchup(lib, vals, h, all_rows, advance):
    """one ps_rowsparse_catchup call over the four tables from last = 0 (rows 20, 21: already at T; 22, 23: at T + 1)"""
    devs, lasts, tabs_c = [], [], []
    listed = np.array([0, 1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 17, 20, 22, 23], dtype=np.int64)       # count 15 < cap 20
    lst = torch.from_numpy(np.concatenate([listed, np.repeat([6], 5)])).cuda()                     # (row 6 is not listed)
    cnt = torch.tensor([len(listed)], dtype=torch.int32, device='cuda')
    last0 = np.zeros(R_CATCH, dtype=np.int32)
    last0[20:22] = T_GAP
    last0[22:24] = T_GAP + 1
    for x, d in zip(vals, DS):
        dev = {k: torch.from_numpy(x[k].reshape(R_CATCH, d).copy()).cuda() for k in 'pmv'}
        devs.append(dev)
        lasts.append(torch.from_numpy(last0.copy()).cuda())
        t = row_table(dev['p'], dev['p'], dev['m'], dev['v'], lst, cnt, 20, d)
        t.g = 0                                                                                     # not read by the catch-up
        tabs_c.append(t)
    tabs = tables(tabs_c)
    last_ptrs = (C.c_void_p * 4)(*[x.data_ptr() for x in lasts])
    nrows = (C.c_int64 * 4)(*[R_CATCH] * 4)
    state = torch.tensor([T_GAP, 0], dtype=torch.int64, device='cuda')
    _lib.check(lib.ps_rowsparse_catchup(tabs, 4, last_ptrs, nrows, c_hyper(h, 0), state.data_ptr(), int(advance), int(all_rows),
                                        stream()), 'ps_rowsparse_catchup')
    torch.cuda.synchronize()
    replay = np.zeros(R_CATCH, dtype=bool)
    replay[:20] = True
    want_last = last0.copy()
    want_last[20:22] = T_GAP + advance
    if not all_rows:
        on = np.zeros(R_CATCH, dtype=bool)
        on[listed] = True
        replay &= on
        want_last[~on] = last0[~on]
    want_last[replay] = T_GAP + advance
    return ([{k: x.cpu().numpy() for k, x in dev.items()} for dev in devs], [x.cpu().numpy() for x in lasts], replay, want_last)


CATCH_CASES = [('real betas, adam', dict(), False), ('real betas, noam', dict(noam=True, weight_decay=1e-3), False),
               ('early stop, adam', dict(beta1=0.5, beta2=0.9), True),
               ('early stop, adam, wd', dict(beta1=0.5, beta2=0.9, weight_decay=1e-3), False),
               ('early stop, noam', dict(beta1=0.5, beta2=0.9, noam=True), True),
               ('early stop, noam, wd', dict(beta1=0.5, beta2=0.9, noam=True, weight_decay=1e-3), False)]


@pytest.mark.parametrize('name,kw,stops', CATCH_CASES, ids=[c[0] for c in CATCH_CASES])
def test_catchup_equals_the_dense_kernel_bitwise(name, kw, stops):
    """One catch-up call over a gap of T = 3000 steps = 3000 dense steps with a zero gradient, for d = 100 / 128 / 256 / 512, listed
    rows and all rows, advance 0 and 1; rows already at T or T + 1 keep their values.  With warmup_steps = 4000 noam's rate grows
    through the whole gap.  Under betas (0.5, 0.9) m and v of every element stop changing after step 1,096 on the CPU
    (``step32_numpy``; m is exactly 0 from step 160 on) — well before T, so the replay's early stop is taken wherever p stands
    still too (with weight decay only the rows with p = 0 do: wd * p keeps feeding the others' moments) — and rows with |p| = 0, 1e-30, 1e-25, 1e-10 and 1 sit on both sides of its 1e-20 guard.  On an MI355X all six regimes are bitwise
    equal to the dense run: the early-stop rule needed no change."""
    lib = _lib.load()
    h = A.Hyper(warmup_steps=4000, max_grad_norm=0.0, **kw)
    vals = _catch_values(13)
    if stops:
        fp = _fixed_point_step(vals, h)
        print("%s: m and v stand still from step %s on" % (name, fp))
        assert fp is not None and fp < T_GAP // 2
    dense = _dense_gap(lib, vals, h)
    for all_rows in (0, 1):
        for advance in (0, 1):
            got, last, replay, want_last = _catchup(lib, vals, h, all_rows, advance)
            for i, d in enumerate(DS):
                assert np.array_equal(last[i], want_last), (name, d, all_rows, advance, last[i])
                for k in 'pmv':
                    x0 = vals[i][k].reshape(R_CATCH, d)
                    assert same_bits(got[i][k][~replay], x0[~replay]), (name, d, k, 'a row that was not to be replayed changed')
                    bad = [r for r in np.nonzero(replay)[0] if not same_bits(got[i][k][r], dense[i][k][r])]
                    assert not bad, (name, 'd %d all_rows %d advance %d' % (d, all_rows, advance), k, 'rows', bad)
