"""The device-counted probes (rpt_bf_probe_sel_strategy_for, rpt_bf_probe_chain_sel_workspace_bytes,
rpt_bf_probe_chain_sel_ws, rpt_bf_transfer_sel_ws, rpt_bf_transfer_insert_sel_ws) without a GPU: the symbols are
declared, exported and bound, the Python names exist, and every argument check that needs no look into a handle refuses
before a handle is looked into. The handles and device pointers here are made-up values, never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

NEW = ("rpt_bf_probe_sel_strategy_for", "rpt_bf_probe_chain_sel_workspace_bytes", "rpt_bf_probe_chain_sel_ws",
       "rpt_bf_transfer_sel_ws", "rpt_bf_transfer_insert_sel_ws")
BF, BF2, BF3 = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000  # "filters"
KEYS, SEL, COUNT = 0x7F0000100000, 0x7F0000300000, 0x7F0000400000  # "device memory", 16-byte aligned
OUT_SEL, OUT_COUNT, WS, IWS = 0x7F0000500000, 0x7F0000600000, 0x7F0000700000, 0x7F0000800000
INVALID, OK, ERR_HIP = _lib.RPT_ERR_INVALID_ARGUMENT, _lib.RPT_OK, _lib.RPT_ERR_HIP


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def col(key_type=_lib.RPT_KEY_I64, keys=KEYS):
    return _lib.KeyColumn(key_type, keys, None, None)


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def columns(k):
    return (_lib.KeyColumn * k)(*[col() for _ in range(k)])


def refused(lib, status, message):
    assert status == INVALID
    assert message in lib.rpt_last_error(), lib.rpt_last_error()


def chain(lib, filters, cols, k, sel=SEL, count=COUNT, max_rows=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_probe_chain_sel_ws(filters, cols, k, sel, count, max_rows, out_sel, out_count, WS, 1 << 20, None)


def transfer(lib, filters, cols, k, dst, dst_cols, n_dst, sel=SEL, count=COUNT, max_rows=1000, out_sel=OUT_SEL,
             out_count=OUT_COUNT, routed=False):
    if routed:
        return lib.rpt_bf_transfer_insert_sel_ws(filters, cols, k, dst, dst_cols, n_dst, sel, count, max_rows, out_sel,
                                                 out_count, WS, 1 << 20, IWS, 1 << 20, None)
    return lib.rpt_bf_transfer_sel_ws(filters, cols, k, dst, dst_cols, n_dst, sel, count, max_rows, out_sel, out_count,
                                      WS, 1 << 20, None)


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["rpt_bf_probe_chain_sel_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["rpt_bf_probe_sel_strategy_for"][0] is ctypes.c_int
    # sel + count_dev + max_rows take the place of row_sel + n
    assert len(_lib.SIGNATURES["rpt_bf_probe_chain_sel_ws"][1]) == len(_lib.SIGNATURES["rpt_bf_probe_chain_ws"][1]) + 1
    assert len(_lib.SIGNATURES["rpt_bf_transfer_sel_ws"][1]) == len(_lib.SIGNATURES["rpt_bf_transfer_ws"][1]) + 1
    assert (len(_lib.SIGNATURES["rpt_bf_transfer_insert_sel_ws"][1])
            == len(_lib.SIGNATURES["rpt_bf_transfer_sel_ws"][1]) + 2)
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_python_names_exist():
    import rpt_amd

    for name in ("probe_chain_sel_workspace_bytes", "probe_chain_sel_ws", "transfer_sel_ws", "transfer_insert_sel_ws"):
        assert callable(getattr(rpt_amd, name)), name
    assert callable(rpt_amd.BloomFilter.probe_sel_strategy_for)


def test_strategy_and_sizing_of_null_or_invalid_arguments(lib):
    assert lib.rpt_bf_probe_sel_strategy_for(None, 1000) == -INVALID
    assert b"null filter" in lib.rpt_last_error()
    size = lib.rpt_bf_probe_chain_sel_workspace_bytes
    assert size(None, 1, 1000) == 0
    assert b"null" in lib.rpt_last_error()
    assert size(handles(None), 1, 1000) == 0
    assert b"null filter 0" in lib.rpt_last_error()
    for k in (0, 9, 2**32 - 1):
        assert size(handles(*[None] * 9), k, 1000) == 0
        assert b"n_filters" in lib.rpt_last_error() and b"1..8" in lib.rpt_last_error()


def test_chain_null_arguments_are_refused(lib):
    cols = columns(2)
    refused(lib, chain(lib, None, cols, 1), b"null")
    refused(lib, chain(lib, handles(BF), None, 1), b"null")
    refused(lib, chain(lib, handles(BF), cols, 1, out_count=None), b"null")
    refused(lib, chain(lib, handles(None), cols, 1), b"null filter 0")
    refused(lib, chain(lib, handles(BF, None), cols, 2), b"null filter 1")
    refused(lib, chain(lib, handles(None), cols, 1, max_rows=0), b"null filter 0")  # ... whatever max_rows is
    refused(lib, chain(lib, handles(BF), cols, 1, count=None), b"null count_dev")
    refused(lib, chain(lib, handles(BF), cols, 1, count=None, max_rows=0), b"null count_dev")
    refused(lib, chain(lib, handles(BF), cols, 1, sel=None), b"null sel")
    refused(lib, chain(lib, handles(BF), cols, 1, out_sel=None), b"null out_sel")


def test_transfer_null_arguments_are_refused(lib):
    cols, dcols = columns(1), columns(1)
    for routed in (False, True):
        for args in ((None, cols, 1, handles(BF2), dcols, 1), (handles(BF), None, 1, handles(BF2), dcols, 1),
                     (handles(BF), cols, 1, None, dcols, 1), (handles(BF), cols, 1, handles(BF2), None, 1)):
            refused(lib, transfer(lib, *args, routed=routed), b"null argument")
        ok = (handles(BF), cols, 1, handles(BF2), dcols, 1)
        refused(lib, transfer(lib, *ok, out_count=None, routed=routed), b"null argument")
        refused(lib, transfer(lib, handles(None), cols, 1, handles(BF2), dcols, 1, routed=routed), b"null filter 0")
        refused(lib, transfer(lib, handles(BF), cols, 1, handles(None), dcols, 1, routed=routed),
                b"null destination filter 0")
        refused(lib, transfer(lib, *ok, count=None, routed=routed), b"null count_dev")
        refused(lib, transfer(lib, *ok, sel=None, routed=routed), b"null sel")
        refused(lib, transfer(lib, *ok, out_sel=None, routed=routed), b"null out_sel")


def test_filter_and_destination_counts_outside_the_limit_are_refused(lib):
    nine, dst, cols = handles(*[BF] * 9), handles(*[BF2 + 4096 * j for j in range(9)]), columns(9)
    for k in (0, 9, 2**32 - 1):
        refused(lib, chain(lib, nine, cols, k), b"n_filters=%d outside 1..8" % k)
        for routed in (False, True):
            refused(lib, transfer(lib, nine, cols, k, dst, cols, 1, routed=routed), b"n_filters=%d outside 1..8" % k)
    for n_dst in (0, 9, 2**32 - 1):
        for routed in (False, True):
            refused(lib, transfer(lib, nine, cols, 1, dst, cols, n_dst, routed=routed), b"n_dst=%d outside 1..8" % n_dst)


def test_row_counts_past_uint32_are_refused(lib):
    cols = columns(1)
    for max_rows in (2**32, 2**32 + 1, 2**63):
        refused(lib, chain(lib, handles(BF), cols, 1, max_rows=max_rows), b"exceeds uint32")
        for routed in (False, True):
            refused(lib, transfer(lib, handles(BF), cols, 1, handles(BF2), cols, 1, max_rows=max_rows, routed=routed),
                    b"exceeds uint32")


def test_overlapping_out_sel_and_sel_are_refused(lib):
    """The two ranges of max_rows 4-byte entries are compared: equal, overlapping from either side, and touching by a
    single entry are refused; ranges that only abut are not an overlap (the next check then fails: the made-up
    handle is the only thing left, so those calls are not made here)."""
    cols, dcols = columns(1), columns(1)
    n = 1000
    for out_sel in (SEL, SEL + 4, SEL - 4, SEL + 4 * (n - 1), SEL - 4 * (n - 1), SEL + 2000):
        refused(lib, chain(lib, handles(BF), cols, 1, max_rows=n, out_sel=out_sel), b"out_sel overlaps sel")
        for routed in (False, True):
            refused(lib, transfer(lib, handles(BF), cols, 1, handles(BF2), dcols, 1, max_rows=n, out_sel=out_sel,
                                  routed=routed), b"out_sel overlaps sel")


def test_transfer_into_a_probed_filter_is_refused(lib):
    """The handles are compared before any of them is looked into: made-up handles are enough."""
    cols = columns(3)
    probed = handles(BF, BF2, BF3)
    for routed in (False, True):
        refused(lib, transfer(lib, probed, cols, 3, handles(BF3), cols, 1, routed=routed),
                b"destination filter 0 is probed filter 2 of the same call")
        refused(lib, transfer(lib, probed, cols, 2, handles(BF3, BF), cols, 2, routed=routed),
                b"destination filter 1 is probed filter 0 of the same call")
        refused(lib, transfer(lib, probed, cols, 1, handles(BF2, BF), cols, 2, max_rows=0, routed=routed),
                b"destination filter 1 is probed filter 0")  # ... whatever max_rows is


def test_zero_max_rows_passes_every_argument_check(lib):
    """max_rows == 0 looks into no handle, needs no sel, out_sel or workspace, and only sets the count: the call returns
    RPT_OK for a non-null filter list. Setting the count is a stream-ordered device memset, which this file, run without
    a GPU, cannot see succeed: where no device is present the one thing that may fail is that memset (RPT_ERR_HIP naming
    it), never an argument check. tests/test_gpu_probe_sel.py asserts RPT_OK and the zeroed count on the GPU. The count
    here is real host memory, so nothing made-up is ever handed to the runtime."""
    count = ctypes.c_uint64(0xDEADBEEF)
    out = ctypes.cast(ctypes.pointer(count), ctypes.c_void_p)
    cols = columns(1)
    calls = [
        lambda: lib.rpt_bf_probe_chain_sel_ws(handles(BF), cols, 1, None, COUNT, 0, None, out, None, 0, None),
        lambda: lib.rpt_bf_transfer_sel_ws(handles(BF), cols, 1, handles(BF2), cols, 1, None, COUNT, 0, None, out, None, 0,
                                           None),
        lambda: lib.rpt_bf_transfer_insert_sel_ws(handles(BF), cols, 1, handles(BF2), cols, 1, None, COUNT, 0, None, out,
                                                  None, 0, None, 0, None),
    ]
    for call in calls:
        status = call()
        assert status != INVALID, lib.rpt_last_error()
        assert status == OK or (status == ERR_HIP and b"hipMemsetAsync" in lib.rpt_last_error()), lib.rpt_last_error()
