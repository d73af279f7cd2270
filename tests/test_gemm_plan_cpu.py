"""The GEMM launch plan (csrc/gemm.hip: gemm_plan, through ps_gemm_plan — host only, no device) against the hand-written table of
tests/gemm_forms.py, for every case of the table: the launchable ones, whose rows are what the kernel trace of the commit before
the plan showed (profiles/gemm_plan_forms.md; tests/test_gpu_gemm_forms.py launches them), and the ones no cheap launch
reaches (gemm_forms.CPU_ONLY), whose rows and refusal messages are derived by reading that commit's dispatcher.  Then the
table's own coverage of the plan's cells, and PS_GEMM_X3 / PS_GEMM_X3_SHAPE, one child process per value (read once per process)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import gemm_forms as gf
from gemm_forms import F32, X3, X3D, X3W, P
from prodsearch_amd import _lib
from prodsearch_amd import build as pbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'helpers', 'gemm_plan_worker.py')


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


def test_struct_sizes():
    assert C.sizeof(_lib.PsGemmPlan) == 4 * 17 == 4 * len(gf.PLAN_FIELDS)
    assert C.sizeof(_lib.PsGemmMember) == 4 * 12


@pytest.mark.parametrize('name', [c['name'] for c in gf.ALL])
def test_plan_equals_table(lib, name):
    case = next(c for c in gf.ALL if c['name'] == name)
    got, err = gf.plan_of(lib, _lib, case)
    if case.get('error'):
        assert got is None and err == case['error'], (got, err)      # the text the launch itself refuses with
    else:
        assert err is None and got == case['plan'], (err, {k: (got[k], case['plan'][k]) for k in got if got[k] != case['plan'][k]})


def test_plan_refuses_null_arguments(lib):
    assert lib.ps_gemm_plan(1, None, 0, 0, 0, None) != 0 and b'null argument' in lib.ps_last_error()


def test_table_covers_the_plan():
    """The table stays a cover of the plan's cells, not a subset of them."""
    plans = [c['plan'] for c in gf.ALL if c['plan']]
    cell = lambda *ks: {tuple(p[k] for k in ks) for p in plans}
    assert cell('family') == {(F32,), (X3,), (X3D,), (X3W,)}
    assert {(X3, 64, 64), (X3, 128, 64), (X3, 128, 128), (X3D, 128, 128), (X3W, 128, 128), (F32, 64, 64)} == cell('family', 'tile_m', 'tile_n')
    assert cell('bk') == {(32,), (128,)} and {p['pf'] for p in plans if p['family'] == F32} == {1, 2, 3}
    assert cell('flat', 'redirected') == {(0, 0), (1, 0), (1, 1)}
    for fam in (F32, X3, X3D):                                         # every family that has a flat form, flat and 3-D
        assert {p['flat'] for p in plans if p['family'] == fam} == {0, 1}, fam
    assert {p['redirected'] for p in plans if p['family'] in (X3, X3D) and p['flat']} == {0, 1}
    assert cell('full') == {(0,), (1,)} and cell('idx') == {(0,), (1,)}
    assert cell('ta', 'tb') == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {p['flat_xcd'] for p in plans} >= {0, 1, 3, 7, 15} and cell('split_xcd') == {(0,), (1,)}
    # every row-list instantiation of the fp32 kernel, and the three of the bf16x3 kernel's that the rule can reach
    assert {(p['ta'], p['tb'], p['full'], p['bk'], p['pf']) for p in plans if p['family'] == F32 and p['idx']} == \
           {(0, 1, 1, 32, 2), (1, 1, 0, 32, 2), (1, 1, 0, 32, 3), (0, 0, 0, 32, 2), (0, 0, 0, 128, 1)}
    # both sides of each threshold the launchable list names
    names = {c['name'] for c in gf.CASES}
    assert {'f32_m64_t00', 'f32_m4160_t00', 'rule_m8128_t00', 'rule_m8192_t00', 'rule_m12288_t00', 'rule_tall_t00', 'planes_m4096_t00',
            'planes_m4092_t00', 'wg_same3_ks8', 'wg_same3_ks2', 'wg_listed3_full', 'wg_listed3_common_empty', 'wg_kvqf_det'} <= names
    assert {c['error'] for c in gf.CPU_ONLY if c['error']} >= {'gemm: grid too large', 'gemm: group size 0', 'gemm: group size 5'}


# ---- the two supported switches: each child plans these probes under its environment and nothing else
PROBES = ('f32_m64_t00', 'rule_m8192_t00', 'wg_flat3', 'wg_redirect_rule', 'planes_m4096_t00')
W = (1, 1, 0, 0)
# switch value -> {probe: plan}; a probe not named keeps its table row — but for planes_m4096_t00, whose row holds under
# ps_gemm_x3_config(1, 4) only: without it the fp32 kernel's 32-deep slabs take the product (64 workgroups would still be deep,
# 4,096 rows are 64 tiles: deep)
NO_PLANES = P(F32, (0, 0, 0, 0), (1, 64, 1), bk=128, pf=1)
SWITCH_PLANS = {
    ('PS_GEMM_X3', '0'): {'rule_m8192_t00': P(F32, (0, 0, 0, 0), (4, 128, 1), bk=32, pf=2),
                          'wg_flat3': P(F32, W, (96, 1, 1), pf=2, flat=1),
                          'wg_redirect_rule': P(F32, W, (8, 8, 8), bk=32, pf=2, sxcd=1), 'planes_m4096_t00': NO_PLANES},
    ('PS_GEMM_X3_SHAPE', '2'): {'f32_m64_t00': P(X3, (0, 0, 0, 0), (1, 1, 1), tile=(128, 128)),
                                'rule_m8192_t00': P(X3, (0, 0, 0, 0), (2, 64, 1), tile=(128, 128)),
                                # a forced tile is not shape 0: no redirect; the 3-D grid of 128 x 128 tiles, splits placed by XCD
                                'wg_redirect_rule': P(X3, W, (4, 4, 8), tile=(128, 128), sxcd=1),
                                'planes_m4096_t00': P(X3, (0, 0, 0, 0), (1, 32, 1), tile=(128, 128))},
    ('PS_GEMM_X3_SHAPE', '3'): {'f32_m64_t00': P(X3D, (0, 0, 0, 0), (1, 1, 1), tile=(128, 128)),
                                'rule_m8192_t00': P(X3D, (0, 0, 0, 0), (2, 64, 1), tile=(128, 128)),
                                'wg_flat3': P(X3D, W, (24, 1, 1), tile=(128, 128), flat=1),
                                'wg_redirect_rule': P(X3D, W, (4, 4, 8), tile=(128, 128), sxcd=1),
                                'planes_m4096_t00': P(X3D, (0, 0, 0, 0), (1, 32, 1), tile=(128, 128))},
    ('PS_GEMM_X3_SHAPE', '4'): {},          # the rule everywhere, and planes_m4096_t00's own row
}


def _probe_plans(env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ('PS_GEMM_X3', 'PS_GEMM_X3_SHAPE', 'PS_DIAG_LIB')}
    env.update(env_extra)
    res = subprocess.run([sys.executable, WORKER] + list(PROBES), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.parametrize('switch', [None] + list(SWITCH_PLANS), ids=lambda s: 'default' if s is None else '%s=%s' % s)
def test_switch_changes_the_plan_exactly_so(lib, switch):
    got = _probe_plans({} if switch is None else {switch[0]: switch[1]})
    changed = {} if switch is None else SWITCH_PLANS[switch]
    table = {c['name']: c['plan'] for c in gf.ALL}
    for name in PROBES:
        want = changed.get(name, table[name])
        if name == 'planes_m4096_t00' and name not in changed and switch != ('PS_GEMM_X3_SHAPE', '4'):
            want = NO_PLANES
        assert got[name] == want, (switch, name, got[name], want)
