"""The small kernels of the data-parallel exchanges, called directly: ``ps_sum_slices`` (local half of the peer-to-peer
reduce-scatter) and ``ps_shard_bucket`` / ``ps_shard_remap`` (requests and slots of a row-sharded table).  Elsewhere they run only
inside multi-process tests; here every result is exact and is compared with a plain numpy restatement, with canaries behind every
buffer."""
import numpy as np
import pytest
import torch

from prodsearch_amd import _lib

pytestmark = pytest.mark.gpu

CANARY_F = np.float32(-777.25)
CANARY_I = -424242
TAIL = 16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(x, canary):
    """device copy of x with TAIL canary elements behind it"""
    buf = np.concatenate([x.reshape(-1), np.full(TAIL, canary, dtype=x.dtype)])
    return torch.from_numpy(buf).cuda()


def _tail_ok(t, n, canary):
    return bool((t[n:].cpu().numpy() == canary).all())


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n,zero', [(n, z) for n in (0, 4, 1020, 1024, 4 * 600001) for z in ('none', 'smaller', 'larger')
                                    if (n, z) != (0, 'smaller')])             # (there is no zero_n below n = 0)
def test_sum_slices_adds_in_rank_order_and_clears_exactly_zero_n(world, n, zero):
    lib = _lib.load()
    rng = np.random.default_rng([world, n % 9973])
    recv = (rng.standard_normal((world, n)) * np.exp(rng.uniform(-8, 8, (world, n)))).astype(np.float32)
    want = recv[0].copy() if n else np.zeros(0, dtype=np.float32)
    for r in range(1, world):
        want = want + recv[r]                                         # float32, rank order
    recv_d = _padded(recv, CANARY_F)
    out_d = _padded(np.full(n, 3.5, dtype=np.float32), CANARY_F)
    zero_n = {'none': 0, 'smaller': n // 2 // 4 * 4, 'larger': n + 1028}[zero]
    zero_d = _padded(np.full(zero_n + 8, 7.0, dtype=np.float32), CANARY_F) if zero != 'none' else None
    _lib.check(lib.ps_sum_slices(recv_d.data_ptr(), world, n, out_d.data_ptr(), zero_d.data_ptr() if zero_d is not None else None,
                                 zero_n, _stream()), 'ps_sum_slices')
    torch.cuda.synchronize()
    got = out_d[:n].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _tail_ok(out_d, n, CANARY_F) and _tail_ok(recv_d, world * n, CANARY_F)
    assert np.array_equal(recv_d[:world * n].cpu().numpy().view(np.uint32), recv.reshape(-1).view(np.uint32))
    if zero_d is not None:
        z = zero_d.cpu().numpy()
        assert not z[:zero_n].any() and (z[zero_n:zero_n + 8] == 7.0).all() and _tail_ok(zero_d, zero_n + 8, CANARY_F)


def _bucket_numpy(rows, world, capp):
    """request o = local rows (id // world) of the ids with id % world == o, ascending, then -1; slot_of[u] = o * capp + position;
    entries past capp go to the pad slot world * capp"""
    send = np.full((world, capp), -1, dtype=np.int64)
    slot = np.zeros(len(rows), dtype=np.int32)
    over = False
    for o in range(world):
        mine = np.nonzero(rows % world == o)[0]
        for pos, u in enumerate(mine):
            if pos < capp:
                send[o, pos] = rows[u] // world
                slot[u] = o * capp + pos
            else:
                slot[u] = world * capp
                over = True
    return send, slot, over


def _bucket(lib, rows, world, capp):
    n = len(rows)
    rows_d = _padded(rows, CANARY_I)
    count_d = torch.tensor([n], dtype=torch.int32, device='cuda')
    send_d = _padded(np.full(world * capp, -5, dtype=np.int64), CANARY_I)
    slot_d = _padded(np.full(n, -5, dtype=np.int32), CANARY_I)
    bad_d = torch.zeros(4, dtype=torch.int32, device='cuda')
    _lib.check(lib.ps_shard_bucket(rows_d.data_ptr(), count_d.data_ptr(), world, capp, send_d.data_ptr(), slot_d.data_ptr(),
                                   bad_d.data_ptr(), _stream()), 'ps_shard_bucket')
    torch.cuda.synchronize()
    assert _tail_ok(send_d, world * capp, CANARY_I) and _tail_ok(slot_d, n, CANARY_I) and _tail_ok(rows_d, n, CANARY_I)
    assert not bad_d[1:].any()
    return send_d[:world * capp].cpu().numpy().reshape(world, capp), slot_d[:n].cpu().numpy(), int(bad_d[0]), rows_d, count_d, slot_d


def _rows(n, world):
    rng = np.random.default_rng([n, world])
    return np.sort(rng.choice(40000, n, replace=False)).astype(np.int64)


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 5000])
def test_shard_bucket_and_remap_equal_the_numpy_restatement(world, n):
    lib = _lib.load()
    rows = _rows(n, world)
    capp = int(max([np.sum(rows % world == o) for o in range(world)] + [1])) + 3
    send, slot, bad, rows_d, count_d, slot_d = _bucket(lib, rows, world, capp)
    want_send, want_slot, over = _bucket_numpy(rows, world, capp)
    assert not over and bad == 0
    assert np.array_equal(send, want_send) and np.array_equal(slot, want_slot)
    filled = np.nonzero(send.reshape(-1) >= 0)[0]
    assert np.array_equal(np.sort(slot), filled)                      # slot_of: a bijection onto the filled slots
    # remap: ids of the list in any order and with repeats, the pad, and (separately) an id that is not in the list
    rng = np.random.default_rng([n, world, 1])
    pad_in, pad_out = 40000, world * capp
    m = 3001
    pick = rng.integers(0, max(n, 1), m)
    idx = rows[pick] if n else np.full(m, pad_in, dtype=np.int64)
    idx[rng.random(m) < 0.2] = pad_in
    want = np.where(idx == pad_in, pad_out, want_slot[pick] if n else pad_out).astype(np.int64)
    for missing in (False, True):
        idx2, want2 = idx.copy(), want.copy()
        if missing:
            absent = np.setdiff1d(np.arange(40001, 40010), rows)[0]  # above every id of the list; and one below / between
            idx2[5], want2[5] = absent, pad_out
            if n:
                gap = np.setdiff1d(np.arange(0, 40000), rows)[0]
                idx2[77], want2[77] = gap, pad_out
        idx_d = _padded(idx2, CANARY_I)
        out_d = _padded(np.full(m, -9, dtype=np.int64), CANARY_I)
        bad_d = torch.zeros(4, dtype=torch.int32, device='cuda')
        _lib.check(lib.ps_shard_remap(idx_d.data_ptr(), m, pad_in, rows_d.data_ptr(), count_d.data_ptr(), slot_d.data_ptr(), pad_out,
                                      out_d.data_ptr(), bad_d.data_ptr(), _stream()), 'ps_shard_remap')
        torch.cuda.synchronize()
        assert np.array_equal(out_d[:m].cpu().numpy(), want2), missing
        assert int(bad_d[0]) == (1 if missing else 0) and not bad_d[1:].any()
        assert _tail_ok(out_d, m, CANARY_I) and _tail_ok(idx_d, m, CANARY_I)


@pytest.mark.parametrize('world', [2, 8])
def test_a_request_over_its_capacity_is_flagged_and_goes_to_the_pad_slot(world):
    lib = _lib.load()
    rows = _rows(5000, world)
    capp = int(min(np.sum(rows % world == o) for o in range(world))) - 10      # every owner's request overflows
    send, slot, bad, _, _, _ = _bucket(lib, rows, world, capp)
    want_send, want_slot, over = _bucket_numpy(rows, world, capp)
    assert over and bad == 2
    assert np.array_equal(send, want_send) and np.array_equal(slot, want_slot)
    assert (slot == world * capp).sum() == 5000 - world * capp
