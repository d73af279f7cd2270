"""``ps_pack_tables`` / ``ps_union_tables`` / ``ps_merge_tables`` against numpy, in one process and without a process group:
the W ranks are simulated.  For every rank a sorted touched list and a gradient table per table are packed into slot r of a
"gathered" [W, msg_bytes] buffer; the union and the merge then run over it as they do after the all-gather.

Shapes — the smallest that can go wrong: four tables together, widths 128 / 8 / 128 / 4 (one float4 per lane; two lanes of
32; one lane of 32), rows 70 / 1000 / 65 / 4097 (bitmap tail words: 70 and 65 end six and one bits into their second word,
4097 one bit into its 65th), capacities 5 / 64 / 1 / 130 (no multiples of 8 among 5, 1 and 130: the last row block of a table
is partial; 5 and 1 are odd: their id sections are rounded up to 16 bytes); 1000 + 4097 rows put the tables' bitmap blocks
side by side in one count / emit grid.  Worlds 1, 2, 3, 8; one run with a single table."""
import ctypes as C

import numpy as np
import pytest
import torch

from prodsearch_amd import _lib, dist as pdist

pytestmark = pytest.mark.gpu

TABLES = ((70, 5, 128), (1000, 64, 8), (65, 1, 128), (4097, 130, 4))       # (rows, cap, d)
SENTINEL = 777.0


def _lists(rng, world, tables, empty):
    """[table][rank] -> ascending int64 ids.  Every table but ``empty`` holds: its LAST row (the bitmap's tail word) on every
    rank, row 0 on the last rank only, and on rank 0 exactly ``cap`` ids (no -1 padding in that section).  A table of capacity
    1 cannot hold all of that: its last row is on every rank in an even world and on the last rank only in an odd one."""
    out = []
    for ti, (rows, cap, _) in enumerate(tables):
        per = []
        for r in range(world):
            last = r == world - 1
            if ti == empty:
                ids = []
            elif cap < 3:
                ids = [rows - 1] if (world % 2 == 0 or last) else []
            else:
                special = [rows - 1] + ([0] if last else [])
                n = cap if r == 0 else int(rng.integers(len(special), cap + 1))
                ids = special + rng.choice(np.arange(1, rows - 1), size=n - len(special), replace=False).tolist()
            per.append(np.array(sorted(ids), dtype=np.int64))
        out.append(per)
    return out


class _Sim(object):
    """Device state of the simulated ranks for one set of tables."""

    def __init__(self, lib, tables, world, empty, seed):
        self.lib, self.tables, self.world = lib, tables, world
        rng = np.random.default_rng(seed)
        self.ids = _lists(rng, world, tables, empty)
        self.grads = [[rng.standard_normal((rows, d)).astype(np.float32) for _ in range(world)] for rows, _, d in tables]
        caps, ds = [t[1] for t in tables], [t[2] for t in tables]
        self.ids_off, self.vals_off, self.nbytes = pdist.row_msg_layout(caps, ds)
        dev = 'cuda'
        self.keep = []
        # per rank: its own table array (gradient, list); all ranks share the union outputs and the merge destination
        self.dst = [torch.full((rows, d), SENTINEL, device=dev) for rows, _, d in tables]
        self.ws = [torch.zeros(lib.ps_coalesce_ws_bytes(rows), device=dev, dtype=torch.uint8) for rows, _, _ in tables]
        self.ucap = [max(1, min(world * cap, rows)) for rows, cap, _ in tables]
        self.urows = [torch.full((uc,), -5, device=dev, dtype=torch.int64) for uc in self.ucap]
        self.ucount = [torch.full((1,), -1, device=dev, dtype=torch.int32) for _ in tables]
        self.rank_tabs = []
        for r in range(world):
            arr = (_lib.PsRowMsgTable * len(tables))()
            for ti, (rows, cap, d) in enumerate(tables):
                ids = self.ids[ti][r]
                list_cap = cap if r == 0 else max(1, len(ids))          # a list buffer shorter than the message's capacity
                buf = np.full(list_cap, -7 if r % 2 else rows - 2, dtype=np.int64)      # garbage past the count, both kinds
                buf[:len(ids)] = ids
                g = torch.from_numpy(self.grads[ti][r]).to(dev)
                lst, cnt = torch.from_numpy(buf).to(dev), torch.tensor([len(ids)], device=dev, dtype=torch.int32)
                self.keep += [g, lst, cnt]
                self._fill(arr[ti], ti, g, lst, cnt, list_cap)
            self.rank_tabs.append(arr)
        self.merge_tabs = (_lib.PsRowMsgTable * len(tables))()
        for ti in range(len(tables)):
            self._fill(self.merge_tabs[ti], ti, self.dst[ti], None, None, 1)

    def _fill(self, t, ti, grad, lst, cnt, list_cap):
        rows, cap, d = self.tables[ti]
        t.cap, t.d, t.n_rows, t.grad_dev = cap, d, rows, grad.data_ptr()
        t.rows_dev, t.count_dev, t.list_cap = (None if lst is None else lst.data_ptr()), (None if cnt is None else cnt.data_ptr()), list_cap
        t.ws_dev, t.union_rows_dev, t.union_cap = self.ws[ti].data_ptr(), self.urows[ti].data_ptr(), self.ucap[ti]
        t.union_count_dev = self.ucount[ti].data_ptr()

    def pack(self, fill):
        """Every rank's message packed into its slot of a [world, msg_bytes] buffer that held ``fill`` in every byte."""
        buf = torch.full((self.world, self.nbytes), fill, device='cuda', dtype=torch.uint8)
        for r in range(self.world):
            _lib.check(self.lib.ps_pack_tables(self.rank_tabs[r], len(self.tables), buf[r].data_ptr(), self.nbytes, None),
                       'ps_pack_tables')
        torch.cuda.synchronize()
        return buf

    def union(self, buf):
        _lib.check(self.lib.ps_union_tables(self.merge_tabs, len(self.tables), buf.data_ptr(), self.nbytes, self.world, None),
                   'ps_union_tables')

    def merge(self, buf):
        _lib.check(self.lib.ps_merge_tables(self.merge_tabs, len(self.tables), buf.data_ptr(), self.nbytes, self.world, None),
                   'ps_merge_tables')

    def status(self, ti):
        ws, rows = self.ws[ti], self.tables[ti][0]
        off = self.lib.ps_coalesce_bad_flag(ws.data_ptr(), rows) - ws.data_ptr()
        return int(ws[off:off + 4].view(torch.int32)[0])

    def expected_union(self, ti):
        return np.unique(np.concatenate(self.ids[ti]))

    def expected_row(self, ti, row):
        """fp32 sum of the ranks' rows in rank order, from zero — the kernel's addends in the kernel's order."""
        acc = np.zeros(self.tables[ti][2], dtype=np.float32)
        for r in range(self.world):
            if row in self.ids[ti][r]:
                acc = acc + self.grads[ti][r][row]
        return acc


def _check_messages(sim, buf):
    host = buf.cpu().numpy()
    for r in range(sim.world):
        for ti, (rows, cap, d) in enumerate(sim.tables):
            ids = sim.ids[ti][r]
            sec = host[r, sim.ids_off[ti]:sim.ids_off[ti] + 8 * cap].view(np.int64)
            assert np.array_equal(sec[:len(ids)], ids) and (sec[len(ids):] == -1).all(), (r, ti)
            vals = host[r, sim.vals_off[ti]:sim.vals_off[ti] + 4 * cap * d].view(np.float32).reshape(cap, d)
            assert np.array_equal(vals[:len(ids)].view(np.uint32), sim.grads[ti][r][ids].view(np.uint32)), (r, ti)
            assert (vals[len(ids):].view(np.uint32) == 0).all(), (r, ti)


def _check_union_and_merge(sim):
    torch.cuda.synchronize()
    for ti, (rows, cap, d) in enumerate(sim.tables):
        want = sim.expected_union(ti)
        n = int(sim.ucount[ti][0])
        assert n == len(want), (ti, n, len(want))
        assert np.array_equal(sim.urows[ti][:n].cpu().numpy(), want), ti
        assert sim.status(ti) == 0, ti
        got = sim.dst[ti].cpu().numpy()
        outside = np.setdiff1d(np.arange(rows), want)
        assert (got[outside] == SENTINEL).all(), ti                         # rows outside the union: untouched
        for row in want:
            assert np.array_equal(got[row].view(np.uint32), sim.expected_row(ti, int(row)).view(np.uint32)), (ti, int(row))


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('world', [1, 2, 3, 8])
def test_four_tables_pack_union_merge_against_numpy(lib, world):
    empty = 2 if world in (1, 3) else 1          # one table empty on every rank (the capacity-1 one, or the 64-wide one)
    sim = _Sim(lib, TABLES, world, empty, seed=100 + world)
    assert all(len(sim.ids[ti][0]) == cap for ti, (_, cap, _) in enumerate(TABLES) if ti != empty and cap >= 3)
    assert all(len(sim.ids[empty][r]) == 0 for r in range(world))
    a, b = sim.pack(0xA5), sim.pack(0x3C)
    assert torch.equal(a, b)                     # the bytes on the wire are a function of the gradient only
    _check_messages(sim, a)
    sim.union(a)
    sim.merge(a)
    _check_union_and_merge(sim)
    # the union left its bitmaps clean: the same call again gives the same lists
    first = [u.clone() for u in sim.urows]
    sim.union(a)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, sim.urows))


def test_a_single_table(lib):
    sim = _Sim(lib, (TABLES[3],), 3, None, seed=7)
    a, b = sim.pack(0x00), sim.pack(0xFF)
    assert torch.equal(a, b)
    _check_messages(sim, a)
    sim.union(a)
    sim.merge(a)
    _check_union_and_merge(sim)


def test_a_union_larger_than_its_output_sets_the_status_word_and_returns(lib):
    """Output capacity below the union's size for one table: status 2 for that table only (``ps_coalesce_bad_flag``), the ids
    that fit are written, the count is the full one, the calls return normally and the merge touches the written rows only."""
    world = 3
    sim = _Sim(lib, TABLES, world, 2, seed=55)
    buf = sim.pack(0x77)
    want = sim.expected_union(1)
    short = len(want) - 3
    assert short >= 1
    sim.merge_tabs[1].union_cap = short
    sim.union(buf)
    sim.merge(buf)
    torch.cuda.synchronize()
    assert [sim.status(ti) for ti in range(4)] == [0, 2, 0, 0]
    assert int(sim.ucount[1][0]) == len(want)
    assert np.array_equal(sim.urows[1][:short].cpu().numpy(), want[:short])
    assert (sim.urows[1][short:].cpu().numpy() == -5).all()                 # nothing written past the capacity
    got = sim.dst[1].cpu().numpy()
    assert (got[want[short:]] == SENTINEL).all()
    for row in want[:short]:
        assert np.array_equal(got[row].view(np.uint32), sim.expected_row(1, int(row)).view(np.uint32))
    # the status word is the caller's to clear; with room for the whole union the same buffers give the whole result
    ws, rows = sim.ws[1], TABLES[1][0]
    off = lib.ps_coalesce_bad_flag(ws.data_ptr(), rows) - ws.data_ptr()
    ws[off:off + 4].zero_()
    sim.merge_tabs[1].union_cap = sim.ucap[1]
    sim.union(buf)
    sim.merge(buf)
    _check_union_and_merge(sim)
