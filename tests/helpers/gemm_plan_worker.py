"""Child process of tests/test_gemm_plan_cpu.py: PS_GEMM_X3 and PS_GEMM_X3_SHAPE are read once per process, so each of their
values gets a process of its own.

  gemm_plan_worker.py NAME...   no GPU: ps_gemm_plan of the named cases of tests/gemm_forms.py under this process's
                                environment (ps_gemm_x3_config is not called), one JSON object {name: plan or message}"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import gemm_forms as gf                     # noqa: E402
from prodsearch_amd import _lib             # noqa: E402


def main(names):
    lib = _lib.load()
    cases = {c['name']: c for c in gf.ALL}
    out = {}
    for n in names:
        plan, err = gf.plan_of(lib, _lib, cases[n], config=False)
        out[n] = plan if plan is not None else err
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
