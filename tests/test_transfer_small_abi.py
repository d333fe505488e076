"""The one-launch row-list transfer and the multi-filter sink (rpt_bf_transfer, rpt_bf_transfer_range,
rpt_bf_insert_multi) without a GPU: the symbols are declared, exported and bound, the two transfers' signatures are
their _ws twins' less the workspace, the Python names exist, and every argument check that needs no look into a handle
refuses before a handle is looked into, in the documented order (of two faults the earlier check wins) and with the
family's messages (tests/test_probe_sel_small_abi.py, tests/test_probe_sel_range_abi.py). The handles and device
pointers here are made-up values, never dereferenced. n == 0 passes every argument check only after the handles have
been looked into (the filters' devices and the destinations come first), so that part needs real handles:
tests/test_gpu_transfer_small.py::test_zero_rows_only_set_the_count; what n == 0 does not excuse is checked here."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

NEW = ("rpt_bf_transfer", "rpt_bf_transfer_range", "rpt_bf_insert_multi")
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
BF, BF2, BF3 = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000  # "filters"
KEYS, SEL = 0x7F0000100000, 0x7F0000300000  # "device memory", 16-byte aligned
OUT_SEL, OUT_COUNT = 0x7F0000500000, 0x7F0000600000
INVALID = _lib.RPT_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def columns(k, hash_at=None, bad_at=None):
    return (_lib.KeyColumn * k)(*[
        _lib.KeyColumn(_lib.RPT_KEY_HASH if f == hash_at else 77 if f == bad_at else _lib.RPT_KEY_I64,
                       None if f == bad_at else KEYS, None, None) for f in range(k)])


def refused(lib, status, message):
    assert status == INVALID
    assert message in lib.rpt_last_error(), lib.rpt_last_error()


def plain(lib, filters, cols, k, dst, dcols, n_dst, mask=0, row_sel=None, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    assert mask == 0
    return lib.rpt_bf_transfer(filters, cols, k, dst, dcols, n_dst, row_sel, n, out_sel, out_count, None)


def ranged(lib, filters, cols, k, dst, dcols, n_dst, mask=1, row_sel=None, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_range(filters, cols, k, mask, dst, dcols, n_dst, row_sel, n, out_sel, out_count, None)


def zero_mask(lib, *args, **kw):
    """rpt_bf_transfer_range with range_mask == 0: hands over to rpt_bf_transfer."""
    return ranged(lib, *args, mask=0, **kw)


TRANSFERS = (plain, ranged, zero_mask)


def multi(lib, dst, dcols, n_dst, row_sel=None, n=1000):
    return lib.rpt_bf_insert_multi(dst, dcols, n_dst, row_sel, n, None)


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    assert int(re.search(r"#define\s+RPT_SMALL_PROBE_ROWS\s+(\d+)", header).group(1)) == SMALL_ROWS
    assert "There is no one-launch row-list transfer" not in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    # the workspace calls' arguments less the workspace and its size
    for name in ("rpt_bf_transfer", "rpt_bf_transfer_range"):
        ws = _lib.SIGNATURES[name + "_ws"][1]
        assert _lib.SIGNATURES[name][1] == ws[:-3] + ws[-1:], name
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_the_header_declares_each_transfer_as_its_ws_twin_less_the_workspace():
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)

    def params(name):
        text = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        return [" ".join(p.split()) for p in text.split(",")]

    for name in ("rpt_bf_transfer", "rpt_bf_transfer_range"):
        want = [p for p in params(name + "_ws") if p not in ("void* workspace", "size_t workspace_bytes")]
        assert len(want) == len(params(name + "_ws")) - 2
        assert params(name) == want, name
    assert params("rpt_bf_insert_multi") == ["rpt_bf* const* dst_filters", "const rpt_key_column* dst_cols",
                                             "uint32_t n_dst", "const uint32_t* row_sel", "uint64_t n",
                                             "rpt_stream_t stream"]


def test_python_names_exist():
    import rpt_amd

    for name in ("transfer", "transfer_range", "insert_multi"):
        assert callable(getattr(rpt_amd, name)), name


def test_null_lists_and_handles_are_refused(lib):
    cols, dst, dcols = columns(2), handles(BF3), columns(1)
    for call in TRANSFERS:
        refused(lib, call(lib, None, cols, 1, dst, dcols, 1), b"null argument")
        refused(lib, call(lib, handles(BF), None, 1, dst, dcols, 1), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, None, dcols, 1), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, dst, None, 1), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, out_count=None), b"null argument")
        refused(lib, call(lib, handles(None), cols, 1, dst, dcols, 1), b"null filter 0")
        refused(lib, call(lib, handles(BF, None), cols, 2, dst, dcols, 1), b"null filter 1")
        refused(lib, call(lib, handles(None), cols, 1, dst, dcols, 1, n=0), b"null filter 0")  # ... whatever n is
        refused(lib, call(lib, handles(BF), cols, 1, handles(None), dcols, 1), b"null destination filter 0")
        refused(lib, call(lib, handles(BF), cols, 1, handles(BF2, None), columns(2), 2), b"null destination filter 1")
    refused(lib, multi(lib, None, dcols, 1), b"null argument")
    refused(lib, multi(lib, dst, None, 1), b"null argument")
    refused(lib, multi(lib, handles(None), dcols, 1), b"null destination filter 0")
    refused(lib, multi(lib, handles(BF, None), columns(2), 2), b"null destination filter 1")
    refused(lib, multi(lib, handles(None), dcols, 1, n=0), b"null destination filter 0")  # ... whatever n is


def test_filter_and_destination_counts_outside_the_limit_are_refused(lib):
    nine, dst, cols = handles(*[BF] * 9), handles(*[BF2 + 4096 * j for j in range(9)]), columns(9)
    for k in (0, 9, 2**32 - 1):
        for call in TRANSFERS:
            refused(lib, call(lib, nine, cols, k, dst, cols, 1), b"n_filters=%d outside 1..8" % k)
    for n_dst in (0, 9, 2**32 - 1):
        for call in TRANSFERS:
            refused(lib, call(lib, nine, cols, 1, dst, cols, n_dst), b"n_dst=%d outside 1..8" % n_dst)
        refused(lib, multi(lib, dst, cols, n_dst), b"n_dst=%d outside 1..8" % n_dst)


def test_transfer_into_a_probed_filter_is_refused(lib):
    """The handles are compared before any of them is looked into: made-up handles are enough."""
    cols = columns(3)
    probed = handles(BF, BF2, BF3)
    for call in TRANSFERS:
        refused(lib, call(lib, probed, cols, 3, handles(BF3), cols, 1),
                b"destination filter 0 is probed filter 2 of the same call")
        refused(lib, call(lib, probed, cols, 2, handles(BF3, BF), cols, 2),
                b"destination filter 1 is probed filter 0 of the same call")
        refused(lib, call(lib, probed, cols, 1, handles(BF2, BF), cols, 2, n=0),
                b"destination filter 1 is probed filter 0")  # ... even at n = 0
        refused(lib, call(lib, probed, cols, 1, handles(BF2, BF), cols, 2, n=2**40),
                b"destination filter 1 is probed filter 0")  # ... and before the size check


def test_the_mask_is_checked_before_the_size(lib):
    dst, dcols = handles(BF3), columns(1)
    for k, mask in ((1, 0b10), (2, 0b101), (3, 1 << 3), (8, 1 << 8), (1, 1 << 31), (2, 0xFFFFFFFF)):
        filters = handles(*[BF + 4096 * f for f in range(k)])
        for n in (1000, 0, SMALL_ROWS + 1):
            refused(lib, ranged(lib, filters, columns(8), k, dst, dcols, 1, mask=mask, n=n),
                    b"at or above n_filters=%d" % k)
    for hash_at in (0, 1):
        for mask in (1 << hash_at, 0b11):
            for n in (1000, 0, SMALL_ROWS + 1):
                refused(lib, ranged(lib, handles(BF, BF2), columns(2, hash_at=hash_at), 2, dst, dcols, 1, mask=mask, n=n),
                        b"range_mask flags filter %d" % hash_at)
    # ... and after the lists: of two faults the earlier check wins
    refused(lib, ranged(lib, handles(BF), columns(1), 1, handles(BF), dcols, 1, mask=0b10),
            b"destination filter 0 is probed filter 0")
    refused(lib, ranged(lib, handles(BF), columns(1), 1, dst, dcols, 9, mask=0b10), b"n_dst=9 outside 1..8")


def test_rows_past_the_small_batch_limit_are_refused(lib):
    cols, dst, dcols = columns(1), handles(BF2), columns(1)
    for n in (SMALL_ROWS + 1, 2**32, 2**63):
        for call in TRANSFERS:
            refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, n=n), b"exceeds RPT_SMALL_PROBE_ROWS")
            assert b"n=%d rows" % n in lib.rpt_last_error()
            # ... before row_sel and out_sel are looked at: a null out_sel, and ranges that would overlap
            refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, n=n, out_sel=None), b"exceeds RPT_SMALL_PROBE_ROWS")
            refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, n=n, row_sel=SEL, out_sel=SEL),
                    b"exceeds RPT_SMALL_PROBE_ROWS")
        refused(lib, multi(lib, dst, dcols, 1, n=n), b"exceeds RPT_SMALL_PROBE_ROWS")
        assert b"n=%d rows" % n in lib.rpt_last_error()
        refused(lib, multi(lib, dst, dcols, 1, n=n, row_sel=SEL), b"exceeds RPT_SMALL_PROBE_ROWS")


def test_overlapping_out_sel_and_row_sel_are_refused(lib):
    """The two ranges of n 4-byte entries are compared: equal, overlapping from either side, and touching by a single
    entry are refused, at 1000 entries and at the limit; ranges that only abut are not an overlap (the next check then
    looks into the made-up handle, so those calls are not made here)."""
    cols, dst, dcols = columns(1), handles(BF2), columns(1)
    for n in (1000, SMALL_ROWS):
        for out_sel in (SEL, SEL + 4, SEL - 4, SEL + 4 * (n - 1), SEL - 4 * (n - 1), SEL + 2000):
            for call in TRANSFERS:
                refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, n=n, row_sel=SEL, out_sel=out_sel),
                        b"out_sel overlaps row_sel")
    # the earlier checks win
    refused(lib, ranged(lib, handles(BF), cols, 1, dst, dcols, 1, mask=0b10, row_sel=SEL, out_sel=SEL),
            b"at or above n_filters=1")
    refused(lib, plain(lib, handles(BF), columns(1, bad_at=0), 1, dst, dcols, 1, row_sel=SEL, out_sel=SEL), b"")
    assert b"overlaps" not in lib.rpt_last_error()  # the probed column's own refusal
