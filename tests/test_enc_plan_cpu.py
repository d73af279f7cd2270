"""The encoder plan (csrc/encoder.hip: enc_plan, through ps_tem_plan — host only, no device) against the hand-written table of
tests/enc_paths.py, for every case of the table; the table's own coverage of the plan's cells; deterministic mode; and every
supported switch's effect on the plan, one child process per switch (the switches are read once per process).  The GPU tests
assert the same rows against what a step really launched (tests/test_gpu_enc_paths.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import enc_paths as ep
from enc_paths import GEN, SQ1, W1, WF, KVQ
from prodsearch_amd import _lib
from prodsearch_amd import build as pbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'helpers', 'enc_path_worker.py')


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


@pytest.mark.skipif(not ep.default_switches(), reason="the table holds the plan under default switches")
@pytest.mark.parametrize('name', [r['name'] for r in ep.ALL_ROWS])
def test_plan_equals_table(lib, name):
    r = next(r for r in ep.ALL_ROWS if r['name'] == name)
    old = lib.ps_set_fuse_bwd_min(r['fuse_bwd_min']) if r['fuse_bwd_min'] is not None else None
    try:
        got = ep.plan_of(lib, _lib, ep.desc_of(r, _lib))
    finally:
        if old is not None:
            lib.ps_set_fuse_bwd_min(old)
    want = ep.expected_plan(r)
    assert got == want, (name, '(got, expected)', ep.diff(got, want))


def test_plan_reads_null_tensors_and_the_mask(lib):
    """What the plan reads beside the shapes: which tensors are null (the final LayerNorm's: no fused last layer in the forward,
    so no folded scoring; the backward's form stays) and a key-padding mask (the review transformer's callers: no kvq form)."""
    if not ep.default_switches():
        pytest.skip("default switches only")
    r = next(r for r in ep.ALL_ROWS if r['name'] == 'e_50_20_9')
    d = ep.desc_of(r, _lib)
    full = ep.plan_of(lib, _lib, d)
    p = _lib.PsEncPath()
    t = _lib.PsTemTensors()
    for n in _lib.TOP_FIELDS:
        setattr(t, n, 64)
    for n in _lib.LAYER_FIELDS:
        setattr(t.layer[0], n, 64)
    _lib.check(lib.ps_tem_plan(d, t, 0, C.byref(p)), 'ps_tem_plan')
    assert ep.path_dict(p) == full                      # every tensor given == params NULL
    t.final_ln_g = None
    _lib.check(lib.ps_tem_plan(d, t, 0, C.byref(p)), 'ps_tem_plan')
    got = ep.path_dict(p)
    assert got['fwd_fuse_last'] == 0 and got['fold_score'] == 0
    assert {k: v for k, v in got.items() if k not in ('fwd_fuse_last', 'fold_score')} == \
           {k: v for k, v in full.items() if k not in ('fwd_fuse_last', 'fold_score')}
    _lib.check(lib.ps_tem_plan(d, None, 1, C.byref(p)), 'ps_tem_plan')
    got = ep.path_dict(p)
    assert got['attn'] == (WF,) and ep.diff(got, dict(full, attn=(WF,))) == {}
    assert lib.ps_tem_plan(d, None, 0, None) != 0 and b'null argument' in lib.ps_last_error()


def test_eval_call_plans_without_replicas(lib):
    """C > 0 describes an eval scoring call: no dropout is drawn, so no replicas — the 50,20,9 row's shape then plans what a
    no-dropout training step at d = 128 does (w1, the fused forward, no folded scoring: the e_6_4_40_nodrop row's flags),
    whatever the descriptor's training field says."""
    if not ep.default_switches():
        pytest.skip("default switches only")
    r = next(r for r in ep.ALL_ROWS if r['name'] == 'e_50_20_9')
    want = ep.expected_plan(dict(r, attn=(W1,), flags=frozenset('RL FF QF LI'.split())))
    for training in (1, 0):
        d = ep.desc_of(r, _lib)
        d.C, d.training = 9, training
        assert ep.diff(ep.plan_of(lib, _lib, d), want) == {}, training


def test_table_covers_the_plan():
    """The table stays a cover of the plan's cells, not a subset of them."""
    rows = ep.ALL_ROWS
    assert {r['attn'][0] for r in rows} == {GEN, SQ1, W1, WF, KVQ}
    # a last layer has one query row.  As the single layer every form can stand there; behind other layers it has B * R sequences
    # without replicas of their own, which leaves generic, sq1 and w1 (wf needs replicas, kvq is a one-layer form)
    assert {r['attn'][-1] for r in rows if r['layers'] == 1} == {GEN, SQ1, W1, WF, KVQ}
    assert {r['attn'][-1] for r in rows if r['layers'] > 1} == {GEN, SQ1, W1}
    assert any(r['layers'] == 3 and r['attn'][1] == GEN for r in rows)
    assert any(r['layers'] == 2 and r['d'] == 256 for r in rows)
    for letter in ep.FLAGS:
        assert {letter in r['flags'] for r in rows} == {True, False}, letter

    def forms(**want):
        return {r['attn'][0] for r in rows if r['layers'] == 1 and r['dropout'] > 0 and r['H'] == 8 and
                all((r['L'] + 1 if k == 'S' else r['K'] + 1 if k == 'fan' else r[k]) == v for k, v in want.items())}
    # the boundary pairs, both sides
    assert forms(d=128, S=24) == {KVQ} and forms(d=128, S=25) == {KVQ}          # the wf kernels' two instances
    assert forms(d=128, S=32) == {KVQ} and forms(d=128, S=33) == {SQ1}
    assert forms(d=128, S=64) == {SQ1} and forms(d=256, S=64) == {GEN}
    assert forms(d=128, S=2) == {KVQ}
    assert forms(d=128, fan=24) == {KVQ} and forms(d=128, fan=25) == {SQ1}
    assert forms(d=128, fan=4) >= {KVQ} and forms(d=128, fan=3) == {SQ1}
    assert forms(d=256, S=24) == {WF} and forms(d=256, S=25) == {SQ1}
    assert forms(d=256, fan=3) == {SQ1}
    assert any(r['dropout'] == 0 and r['L'] == 63 and r['attn'] == (W1,) for r in rows)
    # the fused backward's row minimum, both sides
    mf = {r['B'] * (r['K'] + 1): 'BF' in r['flags'] for r in rows if r['fuse_bwd_min'] == ep.PS_FUSE_BWD_MIN}
    assert mf == {1008: False, 1029: True}
    # generic attention with replicas and one query row; sq1 with 4 and with 16 heads
    assert any(r['attn'] == (GEN,) and r['dropout'] > 0 for r in rows)
    assert {r['H'] for r in rows if r['attn'] == (SQ1,) and r['d'] == 128} >= {4, 8, 16}


def test_deterministic_mode_drops_the_two_unordered_forms(lib):
    if not ep.default_switches():
        pytest.skip("default switches only")
    r = next(r for r in ep.ALL_ROWS if r['name'] == 'e_50_20_9')
    base = ep.plan_of(lib, _lib, ep.desc_of(r, _lib))
    old = lib.ps_set_deterministic(1)
    try:
        det = ep.plan_of(lib, _lib, ep.desc_of(r, _lib))
    finally:
        lib.ps_set_deterministic(old)
    assert base['item_scatter'] == 1 and base['dx_fused'] == 1
    assert ep.diff(det, base) == {'item_scatter': (0, 1), 'dx_fused': (0, 1)}


def test_a_setter_between_two_calls_changes_the_next_plan(lib):
    """The call context is built per entry call and latches no setter: ps_set_item_scatter_fused(0) changes the very next plan,
    by that cell alone, and restoring it restores the plan in the same process."""
    if not ep.default_switches():
        pytest.skip("default switches only")
    r = next(r for r in ep.ALL_ROWS if r['name'] == 'e_50_20_9')
    base = ep.plan_of(lib, _lib, ep.desc_of(r, _lib))
    old = lib.ps_set_item_scatter_fused(0)
    try:
        off = ep.plan_of(lib, _lib, ep.desc_of(r, _lib))
    finally:
        lib.ps_set_item_scatter_fused(old)
    assert old == 1 and base['item_scatter'] == 1
    assert ep.diff(off, base) == {'item_scatter': (0, 1)}
    assert ep.plan_of(lib, _lib, ep.desc_of(r, _lib)) == base


# ---- the supported switches: each child calls ps_tem_plan on these four rows and nothing else
PROBES = ('e_50_20_9', 'mf1008', 'w_d256', 'e_6_4_40_nodrop')
# switch -> {probe: (layer-0 form, flags)}; a probe not named keeps its table row
SWITCH_PLANS = {
    'PS_NO_FUSE': ('1', {'e_50_20_9': (WF, 'RL LI PR'), 'mf1008': (WF, 'RL LI PR'), 'e_6_4_40_nodrop': (W1, 'RL LI')}),
    'PS_NO_FUSE_BWD': ('1', {'e_50_20_9': (KVQ, 'RL FF FS QF LI DX')}),
    'PS_NO_ROWLIST': ('1', {'e_50_20_9': (WF, 'FF FS BF IS M ML QF'), 'mf1008': (WF, 'FF FS QF'), 'w_d256': (WF, ''),
                            'e_6_4_40_nodrop': (W1, 'FF QF')}),
    'PS_NO_FOLD_SCORE': ('1', {'e_50_20_9': (KVQ, 'RL FF BF IS M ML QF LI DX'), 'mf1008': (KVQ, 'RL FF QF LI DX')}),
    'PS_KVQ_FUSED': ('0', {'e_50_20_9': (WF, ep.C2_FLAGS), 'mf1008': (WF, ep.FUSED_D128)}),
    'PS_KVDX_FUSED': ('0', {'e_50_20_9': (KVQ, 'RL FF FS BF IS M ML QF LI'), 'mf1008': (KVQ, 'RL FF FS QF LI')}),
    'PS_ATTN_WF': ('0', {'e_50_20_9': (SQ1, 'RL FF FS BF IS M ML QF LI'), 'mf1008': (SQ1, 'RL FF FS QF LI'),
                         'w_d256': (SQ1, 'RL LI PR')}),
    'PS_ATTN_W1': ('0', {'e_6_4_40_nodrop': (SQ1, 'RL FF LI')}),
    'PS_ATTN_WK': ('0', {}),
}


def _probe_plans(env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ep.PLAN_SWITCHES}
    env.update(env_extra)
    res = subprocess.run([sys.executable, WORKER, 'plan'] + list(PROBES), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.fixture(scope='module')
def default_plans(lib):
    got = _probe_plans({})
    for name in PROBES:
        r = next(r for r in ep.ALL_ROWS if r['name'] == name)
        want = ep.expected_plan(r)
        assert ep.diff(ep.from_json(got[name]), want) == {}, name
    return got


@pytest.mark.parametrize('switch', list(SWITCH_PLANS))
def test_switch_changes_the_plan_exactly_so(lib, default_plans, switch):
    value, changed = SWITCH_PLANS[switch]
    got = _probe_plans({switch: value})
    for name in PROBES:
        r = next(r for r in ep.ALL_ROWS if r['name'] == name)
        want = ep.expected_plan(r)
        if name in changed:
            form, flags = changed[name]
            want = ep.expected_plan(dict(r, attn=(form,), flags=frozenset(flags.split())))
            assert want != ep.expected_plan(r), (switch, name)
        assert ep.diff(ep.from_json(got[name]), want) == {}, (switch, name)
