"""The one-message row exchange (``dist.TablesGradExchange``, ``make_exchange(mode='tables')``) under data parallelism on the
GPU, in the manner of tests/test_gpu_dp.py: the ranks are fresh child processes (gloo over 127.0.0.1, all on cuda:0, at most
four of them beside this process), the single-rank run happens here.  The review transformer with the pv encoder and user /
item tables has four row-sparse tables; both loss terms are batch means, so the mean of the ranks' gradients is the
gradient of the global batch."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'helpers', 'dp_tables_worker.py')
TABLES = ('review_encoder.review_embeddings.weight', 'user_emb.weight', 'product_emb.weight', 'word_embeddings.weight')


class _NoExchange(object):
    def __call__(self):
        return None


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(out, world, args, env_extra=None):
    """Start the ranks, wait for them with a timeout; on expiry every rank is killed and the test fails (no second try)."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK='0', WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        env.pop('PS_DP_EXCHANGE', None)
        env.update(env_extra or {})
        procs.append(subprocess.Popen([sys.executable, WORKER, '--out', out] + list(args), env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank did not finish within 300 s; all ranks were killed")
        logs.append(o)
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, logs[r][-4000:])
    return [dict(np.load(out + '.rank%d.npz' % r)) for r in range(world)]


def _assert_replicas_equal(ranks):
    for r in ranks[1:]:
        for k in ranks[0]:
            if not k.startswith('__'):
                assert np.array_equal(ranks[0][k], r[k]), "replicas diverged: " + k           # bitwise lock step


@pytest.fixture(scope='module')
def two_ranks(tmp_path_factory):
    """Case 1's two ranks of 32, two steps without the PV loss, collectives counted: shared by the tests below."""
    out = str(tmp_path_factory.mktemp('dp_tables') / 'rtm2')
    return _run_ranks(out, 2, ['--global-batch', '64', '--pv-steps', '0,0'])


def test_review_transformer_two_ranks_of_32_equal_one_rank_of_64(two_ranks):
    sys.path.insert(0, os.path.join(HERE, 'helpers'))
    import dp_tables_worker
    lr, steps = 0.002, 2
    single = dp_tables_worker.run_rtm(64, [False] * steps, 0, 1, lambda m, o: _NoExchange())
    r0, r1 = two_ranks
    assert set(TABLES) <= set(r0)
    _assert_replicas_equal(two_ranks)
    checked = 0
    for k, ref in single.items():
        if k.startswith('__') or k.endswith('linear_keys.bias') or float(np.abs(ref).max()) == 0.0:
            continue
        got = r0[k]
        assert got.shape == ref.shape, k
        tol = 2e-3 * float(np.abs(ref).max()) + 0.02 * lr * steps           # the project's data-parallel tolerance (test_gpu_dp.py)
        err = float(np.abs(got - ref).max())
        print("%s: max |2 ranks - 1 rank| = %.3e (tolerance %.3e)" % (k, err, tol))
        assert err < tol, (k, err, tol)
        checked += 1
    assert checked >= 18
    print("loss: ranks %.6f %.6f, single %.6f" % (r0['__loss'], r1['__loss'], single['__loss']))
    assert abs(0.5 * (r0['__loss'] + r1['__loss']) - single['__loss']) < 2e-3 * abs(single['__loss'])
    # the ranks' union is the global batch's touched list, table by table, exactly
    for name in TABLES:
        key = '__touched__' + name
        assert np.array_equal(r0[key], single[key]), name
        assert np.array_equal(r1[key], single[key]), name
        assert single[key].size > 0


def test_one_all_reduce_and_one_all_gather_per_step(two_ranks):
    """(all-reduces, all-gathers) each exchange entered: the first one carries the capacity agreement as well."""
    for r in two_ranks:
        assert r['__collectives'].tolist() == [[2, 1], [1, 1]]


def test_review_transformer_four_ranks_with_a_pv_step_and_a_short_last_batch(tmp_path):
    ranks = _run_ranks(str(tmp_path / 'rtm4'), 4, ['--global-batch', '64', '--pv-steps', '1,0', '--ragged', '5'])
    _assert_replicas_equal(ranks)                # (the worker's check_index_errors() raised nothing on any rank)
    assert all(np.isfinite(r['__loss']) for r in ranks)
    assert all(r['__collectives'].tolist() == [[2, 1], [1, 1]] for r in ranks)


def test_item_transformer_tables_mode_equals_the_table_by_table_exchange_bit_for_bit(tmp_path):
    """PS_DETERMINISTIC=1 makes the step reproducible; the two exchanges then add the same rows in the same (rank) order and
    hand the optimizer the same union, so every parameter agrees bit for bit."""
    env = {'PS_DETERMINISTIC': '1'}
    args = ['--model', 'tem', '--global-batch', '384', '--pv-steps', '0,0']
    tables = _run_ranks(str(tmp_path / 'tem_tables'), 2, args + ['--xmode', 'tables'], env)
    default = _run_ranks(str(tmp_path / 'tem_default'), 2, args + ['--xmode', 'default'], env)
    _assert_replicas_equal(tables)
    checked = 0
    for r in range(2):
        for k in default[r]:
            if not k.startswith('__'):
                assert np.array_equal(tables[r][k], default[r][k]), k
                checked += 1
    assert checked >= 40
