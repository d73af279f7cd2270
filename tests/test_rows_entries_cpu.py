"""CPU-only checks of the one-table row entries (``ps_coalesce_rows``, ``ps_pack_rows``, ``ps_merge_rows``): host adaptors over
the kernels of the ``ps_*_tables`` entries.  What they refuse comes back as an error code and a message before anything is
launched; the device addresses here are made up (the style of tests/test_rtm_rowsparse_cpu.py)."""
import pytest

from prodsearch_amd import _lib
from prodsearch_amd import build as pbuild


@pytest.fixture(scope='module')
def lib():
    pbuild.build()
    return _lib.load()


def _refused(lib, rc, prefix, match):
    assert rc != 0
    msg = lib.ps_last_error().decode()
    assert msg.startswith(prefix) and match in msg, msg


def _lists(n_lists, n=4, idx=0x1000):
    arr = (_lib.PsIdxList * max(n_lists, 1))()
    for i in range(n_lists):
        arr[i].idx, arr[i].n = idx, n
    return arr


def test_coalesce_rows_refuses_before_launching(lib):
    def call(arr, n_lists, n_rows=100, cap=8, ws=0x2000, rows=0x3000, count=0x4000):
        return lib.ps_coalesce_rows(arr, n_lists, n_rows, n_rows - 1, ws, rows, cap, count, None)
    _refused(lib, call(_lists(1), 0), 'coalesce:', '1..8 index lists')
    _refused(lib, call(_lists(9), 9), 'coalesce:', '1..8 index lists')
    _refused(lib, call(None, 1), 'coalesce:', '1..8 index lists')
    _refused(lib, call(_lists(2, idx=None), 2), 'coalesce:', 'list 0 null')              # a null list with n > 0
    arr = _lists(2)
    arr[1].idx = None
    _refused(lib, call(arr, 2), 'coalesce:', 'list 1 null')
    _refused(lib, call(_lists(2), 2, cap=7), 'coalesce:', 'rows_out capacity 7 < 8')      # cap below min(total, n_rows) = 8
    _refused(lib, call(_lists(2, n=400), 2, n_rows=100, cap=99), 'coalesce:', 'rows_out capacity 99 < 100')     # ... = n_rows
    _refused(lib, call(_lists(1), 1, n_rows=0), 'coalesce:', 'bad argument')
    for field in ('ws', 'rows', 'count'):
        _refused(lib, call(_lists(1), 1, **{field: None}), 'coalesce:', 'bad argument')


def test_pack_rows_refuses_before_launching(lib):
    def call(d=8, n_rows=100, list_cap=4, cap=8, grad=0x10000, rows=0x20000, count=0x30000, msg_rows=0x40000, msg_vals=0x50000):
        return lib.ps_pack_rows(grad, d, n_rows, rows, count, list_cap, cap, msg_rows, msg_vals, None)
    _refused(lib, call(list_cap=0), 'pack_rows:', 'list capacity 0, message capacity 8')
    _refused(lib, call(list_cap=9), 'pack_rows:', 'list capacity 9, message capacity 8')  # a touched list longer than the message
    _refused(lib, call(n_rows=0), 'pack_rows:', 'n_rows 0')
    _refused(lib, call(d=6), 'pack_rows:', 'width 6')
    _refused(lib, call(d=0), 'pack_rows:', 'width 0')
    _refused(lib, call(cap=0), 'pack_rows:', 'capacity 0')
    _refused(lib, call(msg_vals=0x50008), 'pack_rows:', '16-byte alignment')
    _refused(lib, call(grad=0x10004), 'pack_rows:', '16-byte alignment')
    for field in ('grad', 'rows', 'count', 'msg_rows', 'msg_vals'):
        _refused(lib, call(**{field: None}), 'pack_rows:', 'null argument')


def test_merge_rows_refuses_before_launching(lib):
    def call(world=2, cap=8, d=8, ucap=16, all_rows=0x10000, all_vals=0x20000, grad=0x30000, urows=0x40000, ucount=0x50000):
        return lib.ps_merge_rows(all_rows, all_vals, world, cap, d, grad, urows, ucount, ucap, None)
    for world in (0, 33):
        _refused(lib, call(world=world), 'merge_rows:', 'world %d (<= 32)' % world)
    _refused(lib, call(d=6), 'merge_rows:', 'd 6')
    _refused(lib, call(cap=0), 'merge_rows:', 'cap 0')
    _refused(lib, call(ucap=0), 'merge_rows:', 'world 2')
    _refused(lib, call(all_vals=0x20008), 'merge_rows:', '16-byte alignment')
    for field in ('all_rows', 'all_vals', 'grad', 'urows', 'ucount'):
        _refused(lib, call(**{field: None}), 'merge_rows:', 'null argument')
