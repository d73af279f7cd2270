"""Child process of tests/test_enc_plan_cpu.py and tests/test_gpu_enc_paths.py: the plan-relevant switches are read once per
process, so each of them gets a process of its own.

  enc_path_worker.py plan NAME...   no GPU: ps_tem_plan of the named rows of tests/enc_paths.py, one JSON object
  enc_path_worker.py gpu NAME       one oracle comparison of the row (check_against_oracle) under this process's switches; the
                                    taken records of its training forward and backward as one JSON object"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import enc_paths as ep                      # noqa: E402
from prodsearch_amd import _lib             # noqa: E402


def main(mode, names):
    lib = _lib.load()
    rows = {r['name']: r for r in ep.ALL_ROWS}
    if mode == 'plan':
        print(json.dumps({n: ep.plan_of(lib, _lib, ep.desc_of(rows[n], _lib)) for n in names}))
        return
    from test_gpu_tem_options import check_against_oracle
    rec = {}

    def record(backward):
        rec['bwd' if backward else 'fwd'] = ep.taken(lib, _lib, backward)
    check_against_oracle(expect=record, **ep.oracle_call(rows[names[0]]))
    print(json.dumps(rec))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2:])
