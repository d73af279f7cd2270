"""The cells of the encoder plan (csrc/encoder.h: EncPlan) no other oracle-compared case reaches — tests/enc_paths.py, NEW_ROWS:
generic attention with replicas, the unfused d = 128 forms, the sq1 form with 4 / 16 heads and with the fan-in pre-sum, the shape
boundaries of every attention form, three layers, two layers at d = 256, the fused backward's row minimum — each through the module
API against oracle.tem exactly as tests/test_gpu_tem_options.py (loss 1e-4, every gradient 5e-4, touched rows, the query words'
rows, eval scores), and each asserting the path its training forward and backward really took (ps_enc_path_taken).

Two shipped kernels only a switch reaches, one child process each: the fused forward without folded scoring at R >= 2
(PS_NO_FOLD_SCORE=1) and the replica-split d = 256 attention backward (PS_ATTN_WK=0)."""
import json
import os
import subprocess
import sys

import pytest

import enc_paths as ep
from test_gpu_tem_options import check_against_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'helpers', 'enc_path_worker.py')


@pytest.mark.parametrize('name', [r['name'] for r in ep.NEW_ROWS])
def test_new_cell_matches_oracle_on_its_path(name):
    from prodsearch_amd import _lib
    lib = _lib.load()
    r = next(r for r in ep.NEW_ROWS if r['name'] == name)
    old = lib.ps_set_fuse_bwd_min(r['fuse_bwd_min']) if r['fuse_bwd_min'] is not None else None
    try:
        check_against_oracle(expect=ep.taken_checker(r), **ep.oracle_call(r))
    finally:
        if old is not None:
            lib.ps_set_fuse_bwd_min(old)


_child_died = []     # a child killed by a signal or by its time limit: nothing more is started on the device


def _leg(switch, value, name):
    if _child_died:
        pytest.skip("an earlier child ended abnormally (%s)" % _child_died[0])
    env = {k: v for k, v in os.environ.items() if k not in ep.PLAN_SWITCHES}
    env[switch] = value
    try:
        res = subprocess.run([sys.executable, WORKER, 'gpu', name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             env=env, timeout=240)
    except subprocess.TimeoutExpired:
        _child_died.append('%s=%s: time limit' % (switch, value))
        pytest.fail("child hung under %s=%s" % (switch, value))
    if res.returncode < 0:
        _child_died.append('%s=%s: signal %d' % (switch, value, -res.returncode))
    assert res.returncode == 0, res.stderr[-3000:]           # (the oracle comparison runs in the child)
    rec = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('{')][-1])
    r = next(r for r in ep.ALL_ROWS if r['name'] == name)
    return r, ep.from_json(rec['fwd']), ep.from_json(rec['bwd'])


def test_fused_forward_without_folded_scoring():
    """PS_NO_FOLD_SCORE=1 at 1,050 replica rows: the fused last layer with the score and loss launches of their own."""
    r, fwd, bwd = _leg('PS_NO_FOLD_SCORE', '1', 'e_50_20_9')
    assert fwd['fwd_fuse_last'] == 1 and fwd['fold_score'] == 0
    unfolded = dict(r, flags=r['flags'] - {'FS'})
    assert ep.diff(fwd, ep.expected_taken(unfolded, 0)) == {} and ep.diff(bwd, ep.expected_taken(unfolded, 1)) == {}


def test_replica_split_attention_backward_at_d256():
    """PS_ATTN_WK=0: the wf backward's replica-split kernel at 32 columns per head instead of the key-split one, which the
    default process takes at this shape (the w_d256 and d256_s24 rows assert wf_key_split = 1)."""
    r, fwd, bwd = _leg('PS_ATTN_WK', '0', 'w_d256')
    assert ep.expected_taken(r, 1)['wf_key_split'] == 1
    assert bwd['wf_key_split'] == 0 and bwd['attn'] == (ep.WF,)
    assert ep.diff(fwd, ep.expected_taken(r, 0)) == {} and ep.diff(bwd, ep.expected_taken(r, 1, wk_on=False)) == {}
