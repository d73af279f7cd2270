"""The grouped weight-gradient launch with row-list members (csrc/wgrad.hip, run_wgrads), driven through ps_wgrad_group_test:
two listed members (the K and V gradients: the same list of valid positions, entries past its length pointing at a row of NaN
operands) and two plain ones (Q and f_W: one row per sequence), 128 x 128 outputs over 168 positions.  Every member has its
own split count in one flat launch (PS_KVQ_SPLIT / ps_set_kvq_split, the default); with the switch off the group takes one
common count on the 3-D grid, and both forms must give the float64 product over the listed rows.

Error measure: |got - ref| / (sum_k |a_k b_k| + |dW0|) per element (the launch accumulates onto the pre-filled dW0, which is
one more term of the sum); an element whose sum has no term must come back bit for bit.
Bound: the common-count form of the commit before the per-member counts, on these same inputs (all 36 cases), had a largest
error of PARENT_ERR = 2.371e-07 by this measure (profiles/kvq_wgrad_notes.md); the bound is twice that — the factor covers the
order of the fp32 atomics, which differs from run to run.  (The fp32 MFMA at the step's own shapes: 1.13e-7, DESIGN.md.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128                       # outputs are D x D: four 64 x 64 tiles per member
NPOS = 168                    # 8 sequences x 21 positions
LENGTHS = (0, 1, 31, 32, 33, 95, 96, 97, 168)
PLAIN_ROWS = (8, 24, 33, 384)
GUARD = 64                    # canary floats in front of and behind every dW
CANARY = -12345.678
PARENT_ERR = 2.371e-07
BOUND = 2 * PARENT_ERR


@functools.lru_cache(maxsize=None)
def base():
    """Operands of the whole file, drawn once: listed dY (K, V) and their shared X over NPOS rows, plain dY / X over 384 rows,
    the pre-filled dW of the four members."""
    rng = np.random.RandomState(1234)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(dy_l=[f(NPOS, D), f(NPOS, D)], x_l=f(NPOS, D), dy_p=[f(384, D), f(384, D)], x_p=[f(384, D), f(384, D)],
                dw0=[f(D, D) for _ in range(4)], perm=rng.permutation(NPOS))


@functools.lru_cache(maxsize=None)
def listed_rows(length):
    """The list: `length` distinct positions in ascending order, and the row the entries past the length point at."""
    perm = base()['perm']
    rows = np.sort(perm[:length]).astype(np.int32)
    poison = int(perm[length]) if length < NPOS else -1
    ridx = np.full(NPOS, poison if poison >= 0 else 0, dtype=np.int32)
    ridx[:length] = rows
    return rows, poison, ridx


def product64(dy, x):
    """float64 dY^T X and sum |dy| |x| per output element."""
    a, b = dy.astype(np.float64), x.astype(np.float64)
    return a.T @ b, np.abs(a).T @ np.abs(b)


@functools.lru_cache(maxsize=None)
def ref_listed(length):
    b = base()
    rows = listed_rows(length)[0]
    return [product64(b['dy_l'][m][rows], b['x_l'][rows]) for m in range(2)]


@functools.lru_cache(maxsize=None)
def ref_plain(nrows):
    b = base()
    return [product64(b['dy_p'][m][:nrows], b['x_p'][m][:nrows]) for m in range(2)]


def run_group(lib, length, nrows, ks_listed=0, ks_plain=0):
    """One launch: members 0, 1 listed with `length` list entries, members 2, 3 plain over `nrows` rows.  Returns the four dW
    (numpy) and the four guarded buffers."""
    b = base()
    rows, poison, ridx = listed_rows(length)
    dy_l = [a.copy() for a in b['dy_l']]
    x_l = b['x_l'].copy()
    if poison >= 0:
        for a in dy_l + [x_l]:
            a[poison] = np.nan
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x_ld = dev(x_l)
    dY = [dev(dy_l[0]), dev(dy_l[1]), dev(b['dy_p'][0][:nrows]), dev(b['dy_p'][1][:nrows])]
    X = [x_ld, x_ld, dev(b['x_p'][0][:nrows]), dev(b['x_p'][1][:nrows])]
    bufs = []
    for m in range(4):
        g = torch.full((GUARD + D * D + GUARD,), CANARY, dtype=torch.float32, device='cuda')
        g[GUARD:GUARD + D * D] = dev(b['dw0'][m]).view(-1)
        bufs.append(g)
    ridx_d, rcount_d = dev(ridx), torch.tensor([length], dtype=torch.int32, device='cuda')
    arr = lambda ps: (C.c_void_p * 4)(*ps)
    i32 = lambda v: (C.c_int32 * 4)(*v)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.ps_wgrad_group_test(4, arr([t.data_ptr() for t in dY]), arr([t.data_ptr() for t in X]),
                                 arr([g.data_ptr() + 4 * GUARD for g in bufs]), i32([NPOS, NPOS, nrows, nrows]), i32([1, 1, 0, 0]),
                                 C.c_void_p(ridx_d.data_ptr()), C.c_void_p(rcount_d.data_ptr()), D, D, ks_listed, ks_plain,
                                 C.c_void_p(st))
    assert rc == 0, lib.ps_last_error().decode('utf-8', 'replace')
    torch.cuda.synchronize()
    host = [g.cpu().numpy() for g in bufs]
    return [h[GUARD:GUARD + D * D].reshape(D, D) for h in host], host


def errors(lib, length, nrows, ks_listed=0, ks_plain=0):
    """The largest error of each member by the file's measure; asserts the canaries and the bit-for-bit cases."""
    b = base()
    dws, host = run_group(lib, length, nrows, ks_listed, ks_plain)
    refs = ref_listed(length) + ref_plain(nrows)
    out = []
    for m in range(4):
        assert (host[m][:GUARD] == np.float32(CANARY)).all() and (host[m][-GUARD:] == np.float32(CANARY)).all(), \
            "member %d: canary overwritten" % m
        prod, mag = refs[m]
        dw0 = b['dw0'][m]
        assert np.isfinite(dws[m]).all(), "member %d: a row past the list's length was read" % m
        if length == 0 and m < 2:
            assert np.array_equal(dws[m].view(np.uint32), dw0.view(np.uint32)), "member %d: empty list changed dW" % m
        err = np.abs(dws[m].astype(np.float64) - (dw0.astype(np.float64) + prod)) / (mag + np.abs(dw0.astype(np.float64)))
        out.append(float(err.max()))
    return out


@pytest.fixture
def lib():
    from prodsearch_amd import _lib
    lb = _lib.load()
    was = lb.ps_set_kvq_split(1)
    yield lb
    lb.ps_set_kvq_split(was)


@pytest.mark.parametrize('switch', [1, 0])
@pytest.mark.parametrize('nrows', PLAIN_ROWS)
@pytest.mark.parametrize('length', LENGTHS)
def test_group_matches_float64_over_the_listed_rows(lib, length, nrows, switch):
    """Per-member split counts (switch 1) and the common count (switch 0): both within the bound of the float64 product."""
    lib.ps_set_kvq_split(switch)
    e = errors(lib, length, nrows)
    print("length %d rows %d switch %d: max error per member %s" % (length, nrows, switch, ' '.join('%.3g' % v for v in e)))
    assert max(e) <= BOUND, e


@pytest.mark.parametrize('switch', [1, 0])
def test_more_splits_than_slabs(lib, switch):
    """8 splits for a 33-entry list (two slabs) and 4 for 24 plain rows (one): the workgroups without a slab leave at once."""
    lib.ps_set_kvq_split(switch)
    e = errors(lib, 33, 24, ks_listed=8, ks_plain=4)
    print("switch %d: max error per member %s" % (switch, ' '.join('%.3g' % v for v in e)))
    assert max(e) <= BOUND, e


@pytest.mark.parametrize('switch', [1, 0])
def test_empty_list_leaves_dw_bit_for_bit(lib, switch):
    """rcount = 0 for both listed members, more splits than anything needs: their dW unchanged bit for bit (errors() asserts
    it), the plain members still within the bound."""
    lib.ps_set_kvq_split(switch)
    e = errors(lib, 0, 8, ks_listed=8, ks_plain=4)
    assert e[0] == 0.0 and e[1] == 0.0 and max(e) <= BOUND, e
