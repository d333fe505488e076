"""The one-launch device-counted probes (rpt_bf_probe_chain_sel, rpt_bf_transfer_sel) without a GPU: the symbols are
declared, exported and bound, the Python names exist, and every argument check that needs no look into a handle refuses
before a handle is looked into, in the order and with the messages of the workspace calls (tests/test_probe_sel_abi.py).
The handles and device pointers here are made-up values, never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

NEW = ("rpt_bf_probe_chain_sel", "rpt_bf_transfer_sel")
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
BF, BF2, BF3 = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000  # "filters"
KEYS, SEL, COUNT = 0x7F0000100000, 0x7F0000300000, 0x7F0000400000  # "device memory", 16-byte aligned
OUT_SEL, OUT_COUNT = 0x7F0000500000, 0x7F0000600000
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
    return lib.rpt_bf_probe_chain_sel(filters, cols, k, sel, count, max_rows, out_sel, out_count, None)


def transfer(lib, filters, cols, k, dst, dst_cols, n_dst, sel=SEL, count=COUNT, max_rows=1000, out_sel=OUT_SEL,
             out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_sel(filters, cols, k, dst, dst_cols, n_dst, sel, count, max_rows, out_sel, out_count, None)


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    assert int(re.search(r"#define\s+RPT_SMALL_PROBE_ROWS\s+(\d+)", header).group(1)) == SMALL_ROWS
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    # the workspace calls' arguments less the workspace and its size
    for name in NEW:
        assert _lib.SIGNATURES[name][1] == (_lib.SIGNATURES[name + "_ws"][1][:-3] + _lib.SIGNATURES[name + "_ws"][1][-1:])
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_python_names_exist():
    import rpt_amd

    for name in ("probe_chain_sel", "transfer_sel"):
        assert callable(getattr(rpt_amd, name)), name


def test_chain_null_arguments_are_refused(lib):
    cols = columns(2)
    refused(lib, chain(lib, None, cols, 1), b"null argument")
    refused(lib, chain(lib, handles(BF), None, 1), b"null argument")
    refused(lib, chain(lib, handles(BF), cols, 1, out_count=None), b"null argument")
    refused(lib, chain(lib, handles(None), cols, 1), b"null filter 0")
    refused(lib, chain(lib, handles(BF, None), cols, 2), b"null filter 1")
    refused(lib, chain(lib, handles(None), cols, 1, max_rows=0), b"null filter 0")  # ... whatever max_rows is
    refused(lib, chain(lib, handles(BF), cols, 1, count=None), b"null count_dev")
    refused(lib, chain(lib, handles(BF), cols, 1, count=None, max_rows=0), b"null count_dev")
    refused(lib, chain(lib, handles(BF), cols, 1, count=None, max_rows=2**40), b"null count_dev")  # before the size
    refused(lib, chain(lib, handles(BF), cols, 1, sel=None), b"null sel")
    refused(lib, chain(lib, handles(BF), cols, 1, out_sel=None), b"null out_sel")


def test_transfer_null_arguments_are_refused(lib):
    cols, dcols = columns(1), columns(1)
    for args in ((None, cols, 1, handles(BF2), dcols, 1), (handles(BF), None, 1, handles(BF2), dcols, 1),
                 (handles(BF), cols, 1, None, dcols, 1), (handles(BF), cols, 1, handles(BF2), None, 1)):
        refused(lib, transfer(lib, *args), b"null argument")
    ok = (handles(BF), cols, 1, handles(BF2), dcols, 1)
    refused(lib, transfer(lib, *ok, out_count=None), b"null argument")
    refused(lib, transfer(lib, handles(None), cols, 1, handles(BF2), dcols, 1), b"null filter 0")
    refused(lib, transfer(lib, handles(BF), cols, 1, handles(None), dcols, 1), b"null destination filter 0")
    refused(lib, transfer(lib, handles(BF), cols, 1, handles(BF2, None), columns(2), 2), b"null destination filter 1")
    refused(lib, transfer(lib, *ok, count=None), b"null count_dev")
    refused(lib, transfer(lib, *ok, sel=None), b"null sel")
    refused(lib, transfer(lib, *ok, out_sel=None), b"null out_sel")


def test_filter_and_destination_counts_outside_the_limit_are_refused(lib):
    nine, dst, cols = handles(*[BF] * 9), handles(*[BF2 + 4096 * j for j in range(9)]), columns(9)
    for k in (0, 9, 2**32 - 1):
        refused(lib, chain(lib, nine, cols, k), b"n_filters=%d outside 1..8" % k)
        refused(lib, transfer(lib, nine, cols, k, dst, cols, 1), b"n_filters=%d outside 1..8" % k)
    for n_dst in (0, 9, 2**32 - 1):
        refused(lib, transfer(lib, nine, cols, 1, dst, cols, n_dst), b"n_dst=%d outside 1..8" % n_dst)


def test_max_rows_past_the_small_batch_limit_is_refused(lib):
    cols = columns(1)
    for max_rows in (SMALL_ROWS + 1, 2**32, 2**63):
        refused(lib, chain(lib, handles(BF), cols, 1, max_rows=max_rows), b"exceeds RPT_SMALL_PROBE_ROWS")
        assert b"max_rows=%d" % max_rows in lib.rpt_last_error()
        refused(lib, transfer(lib, handles(BF), cols, 1, handles(BF2), cols, 1, max_rows=max_rows),
                b"exceeds RPT_SMALL_PROBE_ROWS")
        # ... before sel and out_sel are looked at
        refused(lib, chain(lib, handles(BF), cols, 1, max_rows=max_rows, sel=None, out_sel=None),
                b"exceeds RPT_SMALL_PROBE_ROWS")


def test_overlapping_out_sel_and_sel_are_refused(lib):
    """The two ranges of max_rows 4-byte entries are compared: equal, overlapping from either side, and touching by a
    single entry are refused, at 1000 entries and at the limit; ranges that only abut are not an overlap (the next
    check then looks into the made-up handle, so those calls are not made here)."""
    cols, dcols = columns(1), columns(1)
    for n in (1000, SMALL_ROWS):
        for out_sel in (SEL, SEL + 4, SEL - 4, SEL + 4 * (n - 1), SEL - 4 * (n - 1), SEL + 2000):
            refused(lib, chain(lib, handles(BF), cols, 1, max_rows=n, out_sel=out_sel), b"out_sel overlaps sel")
            refused(lib, transfer(lib, handles(BF), cols, 1, handles(BF2), dcols, 1, max_rows=n, out_sel=out_sel),
                    b"out_sel overlaps sel")


def test_transfer_into_a_probed_filter_is_refused(lib):
    """The handles are compared before any of them is looked into: made-up handles are enough."""
    cols = columns(3)
    probed = handles(BF, BF2, BF3)
    refused(lib, transfer(lib, probed, cols, 3, handles(BF3), cols, 1),
            b"destination filter 0 is probed filter 2 of the same call")
    refused(lib, transfer(lib, probed, cols, 2, handles(BF3, BF), cols, 2),
            b"destination filter 1 is probed filter 0 of the same call")
    refused(lib, transfer(lib, probed, cols, 1, handles(BF2, BF), cols, 2, max_rows=0),
            b"destination filter 1 is probed filter 0")  # ... even at max_rows = 0
    refused(lib, transfer(lib, probed, cols, 1, handles(BF2, BF), cols, 2, max_rows=2**40),
            b"destination filter 1 is probed filter 0")  # ... and before the size check


def test_zero_max_rows_passes_every_argument_check(lib):
    """max_rows == 0 looks into no handle, needs no sel or out_sel, and only sets the count: RPT_OK for a non-null
    filter list. Setting the count is a stream-ordered device memset, which this file, run without a GPU, cannot see
    succeed: where no device is present the one thing that may fail is that memset (RPT_ERR_HIP naming it), never an
    argument check. tests/test_gpu_probe_sel_small.py asserts RPT_OK and the zeroed count on the GPU. The count here is
    real host memory, so nothing made-up is ever handed to the runtime."""
    count = ctypes.c_uint64(0xDEADBEEF)
    out = ctypes.cast(ctypes.pointer(count), ctypes.c_void_p)
    cols = columns(1)
    calls = [
        lambda: lib.rpt_bf_probe_chain_sel(handles(BF), cols, 1, None, COUNT, 0, None, out, None),
        lambda: lib.rpt_bf_transfer_sel(handles(BF), cols, 1, handles(BF2), cols, 1, None, COUNT, 0, None, out, None),
        # a destination listed twice is no argument error
        lambda: lib.rpt_bf_transfer_sel(handles(BF), cols, 1, handles(BF2, BF2), columns(2), 2, None, COUNT, 0, None, out,
                                        None),
    ]
    for call in calls:
        status = call()
        assert status != INVALID, lib.rpt_last_error()
        assert status == OK or (status == ERR_HIP and b"hipMemsetAsync" in lib.rpt_last_error()), lib.rpt_last_error()
