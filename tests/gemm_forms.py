"""The GEMM dispatcher's cases (csrc/gemm.hip, gemm_plan): one list shared by tools/gemm_forms.py (launches every case and
prints a hash of its output), tests/test_gemm_plan_cpu.py (ps_gemm_plan against the table, no device) and
tests/test_gpu_gemm_forms.py (plan, launch, float64 check).  A case describes a launch twice: as what the driver calls
(`kind` and its arguments) and as the group ps_launch_gemm then sees (`members`, `flat`, `prefer`, `planes`) — for the
weight-gradient groups that second description is derived by hand from run_wgrads' split rules (csrc/wgrad.hip) and says so.
`plan` is the expected PsGemmPlan; the rows of the launchable cases are what the kernel trace of the commit before the plan
existed showed for them (profiles/gemm_plan_forms.md), the rows of CPU_ONLY are derived by reading that commit's dispatcher."""
F32, X3, X3D, X3W = 0, 1, 2, 3
PLAN_FIELDS = ('family', 'ta', 'tb', 'full', 'idx', 'bk', 'pf', 'tile_m', 'tile_n', 'flat', 'redirected', 'grid_x', 'grid_y',
               'grid_z', 'lds_bytes', 'flat_xcd', 'split_xcd')
BOUND = 6e-7            # of sum |a||b|: tests/test_gpu_gemm_x3.py's bound for reductions of at most 1,024 terms


def P(family, lay, grid, bk=32, pf=1, tile=(64, 64), flat=0, redir=0, fxcd=0, sxcd=0):
    ta, tb, full, idx = lay
    return dict(zip(PLAN_FIELDS, (family, ta, tb, full, idx, bk, pf, tile[0], tile[1], flat, redir, grid[0], grid[1], grid[2], 0,
                                  fxcd, sxcd)))


def member(M, N, K, ksplit=1, ta=0, tb=0, full=0, listed=0, accumulate=0, split_stride=0, no_deep=0, kseg=0):
    return dict(M=M, N=N, K=K, ksplit=ksplit, ta=ta, tb=tb, full=full, listed=listed, accumulate=accumulate,
                split_stride=split_stride, no_deep=no_deep, kseg=kseg)


def _cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------- products through ps_gemm_f32 / ps_gemm_f32_weight
def gemm(name, M, N, K, ta, tb, plan, acc=0, bias=1, x3=(1, -1), kind='gemm'):
    # ps_gemm_f32: an atomic product (accumulate 2) is split four ways (PS_GEMM_KSPLIT's default), anything else is one split
    m = member(M, N, K, ksplit=4 if acc == 2 else 1, ta=ta, tb=tb, accumulate=acc)
    return dict(name=name, kind=kind, M=M, N=N, K=K, ta=ta, tb=tb, acc=acc, bias=bias, x3=x3, det=0, members=[m], flat=0,
                prefer=0, planes=1 if kind == 'weight' else 0, plan=plan)


CASES = []
# the fp32 kernel, plain layouts: N = K = 64; one workgroup (<= 64: one 128-deep slab) against 65 (32-deep slabs, two in flight)
for M, deep in ((64, 1), (4160, 0)):
    gy, slab = _cdiv(M, 64), dict(bk=128, pf=1) if deep else dict(bk=32, pf=2)
    for ta, tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        CASES.append(gemm('f32_m%d_t%d%d' % (M, ta, tb), M, 64, 64, ta, tb, P(F32, (ta, tb, 0, 0), (1, gy, 1), **slab)))
    CASES.append(gemm('f32_m%d_t00_nobias' % M, M, 64, 64, 0, 0, P(F32, (0, 0, 0, 0), (1, gy, 1), **slab), bias=0))
    for ta, tb in ((0, 0), (1, 1)):
        CASES.append(gemm('f32_m%d_t%d%d_acc1' % (M, ta, tb), M, 64, 64, ta, tb, P(F32, (ta, tb, 0, 0), (1, gy, 1), **slab), acc=1))
        CASES.append(gemm('f32_m%d_t%d%d_acc2' % (M, ta, tb), M, 64, 64, ta, tb, P(F32, (ta, tb, 0, 0), (1, gy, 4), **slab), acc=2))
# bf16x3 by the size rule, N = K = 256: 127 x 4 = 508 tiles of 64 x 64 stay fp32 (PS_GEMM_X3_T11 = 512), 128 x 4 take the 64 x 64
# tile, 96 x 4 = 384 tiles of 128 x 64 take that one (T21 = 384); and the tall rule (>= 32,768 rows) at N = K = 64
for tb in (0, 1):
    for bias in (1, 0):
        sfx = '_t0%d%s' % (tb, '' if bias else '_nobias')
        CASES.append(gemm('rule_m8128' + sfx, 8128, 256, 256, 0, tb, P(F32, (0, tb, 0, 0), (4, 127, 1), bk=32, pf=2), bias=bias))
        CASES.append(gemm('rule_m8192' + sfx, 8192, 256, 256, 0, tb, P(X3, (0, tb, 0, 0), (4, 128, 1)), bias=bias))
        CASES.append(gemm('rule_m12288' + sfx, 12288, 256, 256, 0, tb, P(X3, (0, tb, 0, 0), (4, 96, 1), tile=(128, 64)), bias=bias))
        CASES.append(gemm('rule_tall' + sfx, 32768, 64, 64, 0, tb, P(X3, (0, tb, 0, 0), (1, 512, 1)), bias=bias))
# bf16x3 forced (ps_gemm_x3_config(1, s)): the three layouts with instantiations, and (ta, tb) = (1, 0), which has none
for s, fam, tile in ((0, X3, (64, 64)), (1, X3, (128, 64)), (2, X3, (128, 128)), (3, X3D, (128, 128))):
    for tb in (0, 1):
        CASES.append(gemm('force%d_t0%d' % (s, tb), 200, 136, 256, 0, tb,
                          P(fam, (0, tb, 0, 0), (_cdiv(136, tile[1]), _cdiv(200, tile[0]), 1), tile=tile), x3=(1, s)))
    CASES.append(gemm('force%d_t11' % s, 256, 256, 256, 1, 1, P(fam, (1, 1, 0, 0), (256 // tile[1], 256 // tile[0], 1), tile=tile), x3=(1, s)))
    CASES.append(gemm('force%d_t10_falls_to_f32' % s, 256, 256, 256, 1, 0, P(F32, (1, 0, 0, 0), (4, 4, 1), bk=128, pf=1), x3=(1, s)))
# pre-split weights (ps_gemm_x3_config(1, 4), ps_gemm_f32_weight): from 4,096 rows (PS_GEMM_X3W_MIN_ROWS)
for tb in (0, 1):
    CASES.append(gemm('planes_m4096_t0%d' % tb, 4096, 64, 64, 0, tb, P(X3W, (0, tb, 0, 0), (1, 32, 1), tile=(128, 128)), x3=(1, 4), kind='weight'))
    CASES.append(gemm('planes_m4092_t0%d' % tb, 4092, 64, 64, 0, tb, P(F32, (0, tb, 0, 0), (1, 64, 1), bk=128, pf=1), x3=(1, 4), kind='weight'))


# ---------------------------------------------------------------- weight-gradient groups through ps_wgrad_group_test
def wgrad(name, n_out, k_in, rows, ks, plan, listed=None, flat=0, prefer=0, det=0, kvq=1, count='full'):
    """dW_i[n_out, k_in] += dY_i[rows_i, n_out]^T . X_i[rows_i, k_in].  ks / flat / prefer: what run_wgrads hands ps_launch_gemm
    (hand-derived); deterministic mode stores per-split partials (accumulate 0 with a split stride) wherever it splits."""
    listed = listed or [0] * len(rows)
    parts = det and (flat or max(ks) > 1)
    ms = [member(n_out, k_in, r, ksplit=k, ta=1, tb=1, listed=l, accumulate=0 if parts else 2, split_stride=1 if parts else 0)
          for r, k, l in zip(rows, ks, listed)]
    return dict(name=name + ('_det' if det else ''), kind='wgrad', n_out=n_out, k_in=k_in, rows=rows, listed=listed, det=det, kvq=kvq,
                count=count, x3=(1, -1), members=ms, flat=flat, prefer=prefer, planes=0, plan=plan)


W = (1, 1, 0, 0)        # a plain weight gradient's instantiation
WL = (1, 1, 0, 1)       # ... with row lists
for det in (0, 1):
    # one member, 128 x 128 over 1,024 rows: pick_ksplit(4 tiles, 1024) = 8 (fill: at most one split per 128 rows)
    CASES.append(wgrad('wg_one', 128, 128, [1024], [8], P(F32, W, (2, 2, 8), bk=128, pf=1, sxcd=1), det=det))
    # different row counts: the flat form, every member the split count it would take alone (4, 8, 12; 8 and 16)
    CASES.append(wgrad('wg_flat3', 128, 128, [512, 1024, 1536], [4, 8, 12], P(X3, W, (96, 1, 1), flat=1), flat=1, det=det))
    CASES.append(wgrad('wg_flat2_xcd', 128, 128, [1024, 2048], [8, 16], P(X3, W, (96, 1, 1), flat=1, fxcd=3), flat=1, det=det))
    # one 512 x 512 member over 4,096 rows: 8 splits x 64 tiles = 512 workgroups of 64 x 64: the size rule says shape 0, the
    # split count is a multiple of 8: redirected to the flat grid
    CASES.append(wgrad('wg_redirect_rule', 512, 512, [4096], [8], P(X3, W, (512, 1, 1), flat=1, redir=1, fxcd=1), det=det))
# three same-shape 512 x 512 members.  4,096 rows: 48 tiles of 128 x 128 x 8 splits = 384: run_wgrads prefers the 128 x 128 form
# (prefer_x3d) with 8 splits -> redirected to the flat grid; deterministic mode never prefers: pick_ksplit(192, 4096) = 2
CASES.append(wgrad('wg_same3_ks8', 512, 512, [4096] * 3, [8] * 3, P(X3D, W, (384, 1, 1), tile=(128, 128), flat=1, redir=1, fxcd=7), prefer=1))
CASES.append(wgrad('wg_same3_ks8', 512, 512, [4096] * 3, [2] * 3, P(F32, W, (8, 8, 6), bk=32, pf=2), det=1))
# ... 3,072 rows: 48 x 6 = 288 < 384, no preference; 2 splits on the 3-D grid
for det in (0, 1):
    CASES.append(wgrad('wg_same3_ks2', 512, 512, [3072] * 3, [2] * 3, P(F32, W, (8, 8, 6), bk=32, pf=2), det=det))
# the smallest group run_wgrads prefers the 128 x 128 form for: 64 tiles x 6 splits = 384 (not a multiple of 8: the 3-D grid);
# deterministic mode: 2 splits, 16 x 16 x 2 = 512 tiles of 64 x 64 by the size rule
CASES.append(wgrad('wg_prefer_x3d', 1024, 1024, [3072], [6], P(X3D, W, (8, 8, 6), tile=(128, 128)), prefer=1))
CASES.append(wgrad('wg_prefer_x3d', 1024, 1024, [3072], [2], P(X3, W, (16, 16, 2)), det=1))
# K / V listed (1,152 positions) + Q plain (256 rows), 128 x 128: per-member splits on the flat grid (cdiv(1152, 288) = 4 and
# 256 / 64 = 4), an empty and a full list; ps_set_kvq_split(0): pick_ksplit(12, 1152) = 9 -> 16 on the 3-D grid; deterministic: 9
for count in ('full', 'empty'):
    CASES.append(wgrad('wg_listed3_' + count, 128, 128, [1152, 1152, 256], [4, 4, 4], P(F32, WL, (48, 1, 1), pf=3, flat=1),
                       listed=[1, 1, 0], flat=1, count=count))
    CASES.append(wgrad('wg_listed3_common_' + count, 128, 128, [1152, 1152, 256], [16] * 3, P(F32, WL, (2, 2, 48), pf=2, sxcd=1),
                       listed=[1, 1, 0], kvq=0, count=count))
    CASES.append(wgrad('wg_listed3_' + count, 128, 128, [1152, 1152, 256], [9] * 3, P(F32, WL, (2, 2, 27), pf=2),
                       listed=[1, 1, 0], det=1, count=count))
# K / V / Q / f_W: four members; deterministic: pick_ksplit(16, 1152) = 8
CASES.append(wgrad('wg_kvqf', 128, 128, [1152, 1152, 256, 256], [4] * 4, P(F32, WL, (64, 1, 1), pf=3, flat=1), listed=[1, 1, 0, 0], flat=1))
CASES.append(wgrad('wg_kvqf', 128, 128, [1152, 1152, 256, 256], [8] * 4, P(F32, WL, (2, 2, 32), pf=2, sxcd=1), listed=[1, 1, 0, 0], det=1))


# ---------------------------------------------------------------- cases no cheap launch reaches: rows derived by reading the dispatcher
def only(name, members, plan=None, error=None, flat=0, prefer=0, planes=0, x3=(1, -1)):
    return dict(name=name, kind=None, members=members, flat=flat, prefer=prefer, planes=planes, x3=x3, det=0, plan=plan, error=error)


_wg = lambda M, N, K, ks, **kw: member(M, N, K, ksplit=ks, ta=1, tb=1, accumulate=2, **kw)
CPU_ONLY = [
    only('grid_too_large', [member(64 * 65535 + 1, 64, 64)], error='gemm: grid too large'),
    only('group_of_0', [], error='gemm: group size 0'),
    only('group_of_5', [member(64, 64, 64)] * 5, error='gemm: group size 5'),
    only('unequal_layout', [member(64, 64, 64), member(64, 64, 64, tb=1)], error='gemm: group members must share layout and ksplit'),
    only('unequal_ksplit', [_wg(64, 64, 256, 2), _wg(64, 64, 256, 4)], error='gemm: group members must share layout and ksplit'),
    only('listed_dropout', [member(64, 64, 64, tb=1, full=2, listed=1)],
         error='gemm: row-list problems take no dropout / column sums / pre-activation output'),
    only('flat_full', [member(64, 64, 64, ta=1, tb=1, full=1)], flat=1, error='gemm: the flat group form takes weight-gradient problems'),
    only('kidx_max_3d', [_wg(64, 64, 2080, 1, listed=1)], error='gemm: row-list weight gradient: 2080 rows per split > 2048'),
    only('kidx_max_flat', [_wg(64, 64, 2080, 1, listed=1)], flat=1,
         error='gemm: flat row-list weight gradient: one segment, no bias, 2080 rows per split <= 2048'),
    only('listed_no_instantiation', [member(64, 64, 64, listed=1, full=1)], error='gemm: no row-list instantiation for ta=0 tb=0 full=1'),
    # four plain 256 x 256 members over 4,096 rows in 8 splits: 16 tiles x 32 = 512 workgroups, shape 0 -> the redirect, which
    # once refused groups of four after the caller's scatter had been launched
    only('redirect_4_members', [_wg(256, 256, 4096, 8)] * 4, P(X3, W, (512, 1, 1), flat=1, redir=1, fxcd=15)),
    only('no_deep', [member(64, 64, 64, no_deep=1)], P(F32, (0, 0, 0, 0), (1, 1, 1), bk=32, pf=2)),
    # prefer_x3d needs whole 32-deep slabs: 3,080 rows are not taken; the size rule then picks for 8 x 16 x 6 = 768 tiles of 128 x 64
    only('prefer_x3d_ragged', [_wg(1024, 1024, 3080, 6)], P(X3, W, (16, 8, 6), tile=(128, 64)), prefer=1),
    # the full epilogue (an activation), which the test entries cannot ask for: the fp32 kernel's two depths, the bf16x3 rule, the
    # row-list dX product (tb = 1, full), the K / V projection over a list as one deep slab, K-concatenated B operands
    only('full_deep', [member(64, 64, 64, full=1)], P(F32, (0, 0, 1, 0), (1, 1, 1), bk=128, pf=1)),
    only('full_shallow', [member(4160, 64, 64, tb=1, full=1)], P(F32, (0, 1, 1, 0), (1, 65, 1), bk=32, pf=2)),
    only('full_rule_128x64', [member(12288, 256, 256, full=1)], P(X3, (0, 0, 1, 0), (4, 96, 1), tile=(128, 64))),
    only('full_planes', [member(4096, 64, 64, full=1, listed=1)], P(X3W, (0, 0, 1, 1), (1, 32, 1), tile=(128, 128)), planes=1, x3=(1, 4)),
    only('listed_dx', [member(8064, 128, 256, tb=1, full=1, listed=1, kseg=128)], P(F32, (0, 1, 1, 1), (2, 126, 1), bk=32, pf=2)),
    only('listed_kv_deep', [member(8064, 128, 128, listed=1)] * 2, P(F32, (0, 0, 0, 1), (2, 126, 2), bk=128, pf=1)),
    only('listed_kv_shallow', [member(8064, 128, 256, listed=1)] * 2, P(F32, (0, 0, 0, 1), (2, 126, 2), bk=32, pf=2)),
    only('listed_rule_x3', [member(32768, 64, 64, tb=1, full=1, listed=1)], P(X3, (0, 1, 1, 1), (1, 512, 1))),
    only('force3_segments_fall_to_128x64', [member(200, 136, 256, kseg=128)], P(X3, (0, 0, 0, 0), (3, 2, 1), tile=(128, 64)), x3=(1, 3)),
    only('flat_force3', [_wg(128, 128, 512, 4), _wg(128, 128, 1024, 8)], P(X3D, W, (12, 1, 1), tile=(128, 128), flat=1), flat=1, x3=(1, 3)),
    only('x3_off_flat', [_wg(128, 128, 512, 4), _wg(128, 128, 1024, 8)], P(F32, W, (48, 1, 1), pf=2, flat=1), flat=1, x3=(0, -1)),
    only('x3_off_no_redirect', [_wg(512, 512, 4096, 8)], P(F32, W, (8, 8, 8), bk=32, pf=2, sxcd=1), x3=(0, -1)),
]
ALL = CASES + CPU_ONLY
assert len({c['name'] for c in ALL}) == len(ALL)


# ---------------------------------------------------------------- asking the plan
def plan_of(lib, _lib, case, config=True):
    """(PsGemmPlan as a dict, None) or (None, the refusal's message) for the case's described group, under the case's
    ps_gemm_x3_config (the configuration is put back); config=False: under the process's own PS_GEMM_X3 / PS_GEMM_X3_SHAPE."""
    import ctypes as C
    n = len(case['members'])
    ms = (_lib.PsGemmMember * max(n, 1))()
    for i, m in enumerate(case['members']):
        for k, v in m.items():
            setattr(ms[i], k, v)
    out = _lib.PsGemmPlan()
    if config:
        lib.ps_gemm_x3_config(*case['x3'])
    try:
        rc = lib.ps_gemm_plan(n, ms, case['flat'], case['prefer'], case['planes'], C.byref(out))
    finally:
        if config:
            lib.ps_gemm_x3_config(1, -1)
    if rc != 0:
        return None, lib.ps_last_error().decode('utf-8', 'replace')
    return {f: getattr(out, f) for f in PLAN_FIELDS}, None


# ---------------------------------------------------------------- launching a case (GPU)
def run_case(lib, _lib, case, want_ref=True):
    """Launches the case on the current device.  Returns [(got, ref, mag)] per output, float64 on the device: ref the float64
    result, mag = sum |a||b| + |bias| + |what the output held before| (the measure of tests/test_gpu_gemm_x3.py)."""
    import ctypes as C
    import torch
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case['name']))
    gen = torch.Generator(device='cuda').manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    lib.ps_gemm_x3_config(*case['x3'])
    old_det = lib.ps_set_deterministic(case['det'])
    try:
        if case['kind'] in ('gemm', 'weight'):
            M, N, K, ta, tb, acc = (case[k] for k in ('M', 'N', 'K', 'ta', 'tb', 'acc'))
            A, Bm = rnd(M, K), rnd(K, N) * 0.1                              # logical [M][K], [K][N]
            Ad = A.t().contiguous() if ta else A
            Bd = Bm if tb else Bm.t().contiguous()
            bias = rnd(N) if case['bias'] else None
            C0 = rnd(M, N) if acc else torch.zeros(M, N, device='cuda')
            out = C0.clone()
            bp = bias.data_ptr() if bias is not None else None
            if case['kind'] == 'weight':
                rc = lib.ps_gemm_f32_weight(Ad.data_ptr(), K, Bd.data_ptr(), tb, out.data_ptr(), N, M, N, K, bp, 0.5, st)
            else:
                rc = lib.ps_gemm_f32(Ad.data_ptr(), M if ta else K, ta, Bd.data_ptr(), N if tb else K, tb, out.data_ptr(), N,
                                     M, N, K, bp, 0.5, acc, st)
            _lib.check(rc, case['name'])
            torch.cuda.synchronize()
            if not want_ref:
                return [(out, None, None)]
            b64 = bias.double() if bias is not None else torch.zeros(N, dtype=torch.float64, device='cuda')
            ref = (A.double() @ Bm.double() + b64) * 0.5 + C0.double()
            mag = (A.double().abs() @ Bm.double().abs() + b64.abs()) * 0.5 + C0.double().abs()
            return [(out.double(), ref, mag)]
        n, n_out, k_in = len(case['rows']), case['n_out'], case['k_in']
        dY = [rnd(r, n_out) for r in case['rows']]
        X = [rnd(r, k_in) * 0.1 for r in case['rows']]
        dW0 = [rnd(n_out, k_in) for _ in range(n)]
        dW = [w.clone() for w in dW0]
        nl = max([r for r, l in zip(case['rows'], case['listed']) if l] or [1])
        ridx = torch.randperm(nl, generator=gen, device='cuda').to(torch.int32)
        length = nl if case['count'] == 'full' else 0
        rcount = torch.tensor([length], dtype=torch.int32, device='cuda')
        arr = lambda ts: (C.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - n)))
        i32 = lambda v: (C.c_int32 * 4)(*(list(v) + [0] * (4 - n)))
        old_kvq = lib.ps_set_kvq_split(case['kvq'])
        try:
            rc = lib.ps_wgrad_group_test(n, arr(dY), arr(X), arr(dW), i32(case['rows']), i32(case['listed']),
                                         C.c_void_p(ridx.data_ptr()), C.c_void_p(rcount.data_ptr()), n_out, k_in, 0, 0, C.c_void_p(st))
        finally:
            lib.ps_set_kvq_split(old_kvq)
        _lib.check(rc, case['name'])
        torch.cuda.synchronize()
        res = []
        for i in range(n):
            if not want_ref:
                res.append((dW[i], None, None))
                continue
            sel = ridx[:length].long() if case['listed'][i] else slice(None)
            a, b = dY[i][sel].double(), X[i][sel].double()
            res.append((dW[i].double(), dW0[i].double() + a.t() @ b, dW0[i].double().abs() + a.abs().t() @ b.abs()))
        return res
    finally:
        lib.ps_set_deterministic(old_det)
        lib.ps_gemm_x3_config(1, -1)


def bound_of(case):
    """A reduction of at most 1,024 terms, split or not, is held to BOUND itself (6e-7 of sum |a||b|), the bound's own domain.  The
    redirect and the 128 x 128 preference only exist for longer ones (>= 256 rows in each of >= 8 splits), so those cases get
    a bound built from the project's two: one split accumulates `depth` terms in fp32, whose rounding error grows with
    sqrt(depth) on zero-mean data — interpolated in sqrt(depth) between BOUND at 1,024 terms and tests/test_gpu_gemm_x3.py's
    2e-6 at 21,504 — plus one rounding (2^-24 of a running sum that is at most sum |a||b|) per addition of a split's partial
    result onto the output, by atomics or by the deterministic mode's ordered sum."""
    if max(m['K'] for m in case['members']) <= 1024:
        return BOUND
    ks = max(m['ksplit'] for m in case['members'])
    depth = max(_cdiv(m['K'], m['ksplit']) for m in case['members'])
    per_split = BOUND + (2e-6 - BOUND) * max(0.0, depth ** 0.5 - 32.0) / (21504 ** 0.5 - 32.0)
    return per_split + ks * 2.0 ** -24


def atomic(case):
    """The output goes through fp32 atomics: its bits depend on their order."""
    return any(m['accumulate'] == 2 and m['ksplit'] > 1 for m in case['members'])
