"""Launch every launchable case of tests/gemm_forms.py once and print, per case, its name and a SHA-256 of its output(s); for
the cases whose output goes through fp32 atomics (order-dependent bits) also the largest error against float64 in units of
sum |a||b|, and whether it is within the case's bound.  Uses only entries older than ps_gemm_plan, so it runs against any
build of the library:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_forms.py [--lib PATH]

Two libraries that dispatch alike give the same kernel sequence (names with template arguments, grids, workgroups, LDS) in
their traces and the same hashes for the non-atomic cases (profiles/gemm_plan_forms.md)."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import gemm_forms as gf                     # noqa: E402
from prodsearch_amd import _lib             # noqa: E402

ENTRIES = ('ps_gemm_f32', 'ps_gemm_f32_weight', 'ps_wgrad_group_test', 'ps_gemm_x3_config', 'ps_set_kvq_split', 'ps_set_deterministic',
           'ps_last_error')


def load(path):
    if not path:
        return _lib.load()
    lib = C.CDLL(path)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    _lib._lib = lib                          # _lib.check reads the error text from the library in use
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libprodsearch_hip.so')
    ap.add_argument('--only', default=None, help='substring of the case names to run')
    a = ap.parse_args()
    lib = load(a.lib)
    bad = 0
    for case in gf.CASES:
        if a.only and a.only not in case['name']:
            continue
        atomic = gf.atomic(case)
        outs = gf.run_case(lib, _lib, case, want_ref=atomic)
        h = hashlib.sha256()
        for got, _, _ in outs:
            h.update(got.float().cpu().numpy().tobytes())
        line = '%-34s %s' % (case['name'], 'atomic' + ' ' * 58 if atomic else h.hexdigest())
        if atomic:
            err = max(float(((got - ref).abs() / mag).max()) for got, ref, mag in outs)
            ok = err < gf.bound_of(case)
            bad += not ok
            line += '  err %.3g of sum|a||b| (bound %.3g) %s' % (err, gf.bound_of(case), 'ok' if ok else 'EXCEEDED')
        print(line, flush=True)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
