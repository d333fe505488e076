"""The range calls of the device-counted probes and of the one-launch chains (rpt_bf_probe_chain_sel_range_ws,
rpt_bf_transfer_sel_range_ws, rpt_bf_transfer_insert_sel_range_ws, rpt_bf_probe_chain_sel_range,
rpt_bf_transfer_sel_range, rpt_bf_probe_chain_range) without a GPU: the symbols are declared, exported and bound, each
signature is its twin's with the mask after n_filters, the Python names exist, and every argument check that needs no
look into a handle refuses before a handle is looked into, the mask checks among them, also at max_rows == 0 / n == 0
(tests/test_probe_range_abi.py does the same for the row-list range calls). The handles and device pointers here are
made-up values, never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

TWINS = {"rpt_bf_probe_chain_sel_range_ws": "rpt_bf_probe_chain_sel_ws",
         "rpt_bf_transfer_sel_range_ws": "rpt_bf_transfer_sel_ws",
         "rpt_bf_transfer_insert_sel_range_ws": "rpt_bf_transfer_insert_sel_ws",
         "rpt_bf_probe_chain_sel_range": "rpt_bf_probe_chain_sel",
         "rpt_bf_transfer_sel_range": "rpt_bf_transfer_sel",
         "rpt_bf_probe_chain_range": "rpt_bf_probe_chain"}
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
BF, BF2, BF3 = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000  # "filters"
KEYS, SEL, COUNT = 0x7F0000100000, 0x7F0000300000, 0x7F0000400000  # "device memory", 16-byte aligned
OUT_SEL, OUT_COUNT = 0x7F0000500000, 0x7F0000600000
WS, IWS = 0x7F0000700000, 0x7F0000800000
INVALID = _lib.RPT_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def columns(k, hash_at=None):
    return (_lib.KeyColumn * k)(
        *[_lib.KeyColumn(_lib.RPT_KEY_HASH if f == hash_at else _lib.RPT_KEY_I64, KEYS, None, None) for f in range(k)])


def refused(lib, status, message):
    assert status == INVALID
    assert message in lib.rpt_last_error(), lib.rpt_last_error()


# ---- the five device-counted calls, as (lib, filters, cols, k, dst, dst_cols, n_dst, **kw); chains ignore the dsts
def chain_ws(lib, filters, cols, k, _dst=None, _dcols=None, _n_dst=0, mask=1, sel=SEL, count=COUNT, max_rows=1000,
             out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_probe_chain_sel_range_ws(filters, cols, k, mask, sel, count, max_rows, out_sel, out_count, WS,
                                               1 << 20, None)


def transfer_ws(lib, filters, cols, k, dst, dcols, n_dst, mask=1, sel=SEL, count=COUNT, max_rows=1000, out_sel=OUT_SEL,
                out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_sel_range_ws(filters, cols, k, mask, dst, dcols, n_dst, sel, count, max_rows, out_sel,
                                            out_count, WS, 1 << 20, None)


def transfer_insert_ws(lib, filters, cols, k, dst, dcols, n_dst, mask=1, sel=SEL, count=COUNT, max_rows=1000,
                       out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_insert_sel_range_ws(filters, cols, k, mask, dst, dcols, n_dst, sel, count, max_rows,
                                                   out_sel, out_count, WS, 1 << 20, IWS, 1 << 20, None)


def chain_small(lib, filters, cols, k, _dst=None, _dcols=None, _n_dst=0, mask=1, sel=SEL, count=COUNT, max_rows=1000,
                out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_probe_chain_sel_range(filters, cols, k, mask, sel, count, max_rows, out_sel, out_count, None)


def transfer_small(lib, filters, cols, k, dst, dcols, n_dst, mask=1, sel=SEL, count=COUNT, max_rows=1000,
                   out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_sel_range(filters, cols, k, mask, dst, dcols, n_dst, sel, count, max_rows, out_sel,
                                         out_count, None)


# ---- the row-list one-launch chain
def chain_rows(lib, filters, cols, k, mask=1, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_probe_chain_range(filters, cols, k, mask, None, n, out_sel, out_count, None)


COUNTED = (chain_ws, transfer_ws, transfer_insert_ws, chain_small, transfer_small)
TRANSFERS = (transfer_ws, transfer_insert_ws, transfer_small)
SMALL = (chain_small, transfer_small)


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, twin in TWINS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
        # the twin's argument list with the 32-bit mask after n_filters
        want = list(_lib.SIGNATURES[twin][1])
        want.insert(want.index(ctypes.c_uint32) + 1, ctypes.c_uint32)
        assert _lib.SIGNATURES[name][1] == want, name
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_the_header_declares_each_call_as_its_twin_with_the_mask():
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)

    def params(name):
        text = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        return [" ".join(p.split()) for p in text.split(",")]

    for name, twin in TWINS.items():
        want = params(twin)
        at = [i for i, p in enumerate(want) if p.endswith(" n_filters")]
        assert len(at) == 1, twin
        want.insert(at[0] + 1, "uint32_t range_mask")
        assert params(name) == want, name


def test_python_names_exist():
    import rpt_amd

    for name in ("probe_chain_sel_range_ws", "transfer_sel_range_ws", "transfer_insert_sel_range_ws",
                 "probe_chain_sel_range", "transfer_sel_range", "probe_chain_range"):
        assert callable(getattr(rpt_amd, name)), name


def test_a_mask_bit_at_or_above_n_filters_is_refused(lib):
    cols, dst, dcols = columns(8), handles(BF3), columns(1)
    for k, mask in ((1, 0b10), (2, 0b101), (3, 1 << 3), (8, 1 << 8), (1, 1 << 31), (2, 0xFFFFFFFF)):
        filters = handles(*[BF + 4096 * f for f in range(k)])
        for call in COUNTED:
            for max_rows in (1000, 0):  # ... even at max_rows = 0
                refused(lib, call(lib, filters, cols, k, dst, dcols, 1, mask=mask, max_rows=max_rows),
                        b"at or above n_filters=%d" % k)
        for n in (1000, 0):
            refused(lib, chain_rows(lib, filters, cols, k, mask=mask, n=n), b"at or above n_filters=%d" % k)


def test_a_flagged_hash_column_is_refused(lib):
    filters, dst, dcols = handles(BF, BF2), handles(BF3), columns(1)
    for hash_at in (0, 1):
        cols = columns(2, hash_at=hash_at)
        for mask in (1 << hash_at, 0b11):
            for call in COUNTED:
                for max_rows in (1000, 0):
                    refused(lib, call(lib, filters, cols, 2, dst, dcols, 1, mask=mask, max_rows=max_rows),
                            b"range_mask flags filter %d" % hash_at)
            for n in (1000, 0):
                refused(lib, chain_rows(lib, filters, cols, 2, mask=mask, n=n), b"range_mask flags filter %d" % hash_at)


def test_null_lists_handles_and_row_sources_are_refused(lib):
    cols, dst, dcols = columns(2), handles(BF3), columns(1)
    for call in COUNTED:
        refused(lib, call(lib, None, cols, 1, dst, dcols, 1), b"null argument")
        refused(lib, call(lib, handles(BF), None, 1, dst, dcols, 1), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, out_count=None), b"null argument")
        refused(lib, call(lib, handles(None), cols, 1, dst, dcols, 1), b"null filter 0")
        refused(lib, call(lib, handles(BF, None), cols, 2, dst, dcols, 1, mask=2), b"null filter 1")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, count=None), b"null count_dev")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, count=None, max_rows=0), b"null count_dev")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, sel=None), b"null sel")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, out_sel=None), b"null out_sel")
    for call in TRANSFERS:
        refused(lib, call(lib, handles(BF), cols, 1, None, dcols, 1), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, dst, None, 1), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, handles(None), dcols, 1), b"null destination filter 0")
    refused(lib, chain_rows(lib, None, cols, 1), b"null argument")
    refused(lib, chain_rows(lib, handles(BF), None, 1), b"null argument")
    refused(lib, chain_rows(lib, handles(BF), cols, 1, out_count=None), b"null argument")
    refused(lib, chain_rows(lib, handles(None), cols, 1), b"null filter 0")
    refused(lib, chain_rows(lib, handles(None), cols, 1, n=0), b"null filter 0")  # ... whatever n is


def test_filter_and_destination_counts_outside_the_limit_are_refused(lib):
    nine, dst, cols = handles(*[BF] * 9), handles(*[BF2 + 4096 * j for j in range(9)]), columns(9)
    for k in (0, 9, 2**32 - 1):
        for call in COUNTED:
            refused(lib, call(lib, nine, cols, k, dst, cols, 1), b"n_filters=%d outside 1..8" % k)
        refused(lib, chain_rows(lib, nine, cols, k), b"n_filters=%d outside 1..8" % k)
    for n_dst in (0, 9, 2**32 - 1):
        for call in TRANSFERS:
            refused(lib, call(lib, nine, cols, 1, dst, cols, n_dst), b"n_dst=%d outside 1..8" % n_dst)


def test_rows_past_the_limits_are_refused(lib):
    cols, dst, dcols = columns(1), handles(BF2), columns(1)
    for rows in (SMALL_ROWS + 1, 2**32, 2**63):
        for call in SMALL:
            refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, max_rows=rows), b"exceeds RPT_SMALL_PROBE_ROWS")
            assert b"max_rows=%d" % rows in lib.rpt_last_error()
            # ... before sel and out_sel are looked at
            refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, max_rows=rows, sel=None, out_sel=None),
                    b"exceeds RPT_SMALL_PROBE_ROWS")
        refused(lib, chain_rows(lib, handles(BF), cols, 1, n=rows), b"exceeds RPT_SMALL_PROBE_ROWS")
        assert b"n=%d" % rows in lib.rpt_last_error()
    for call in (chain_ws, transfer_ws, transfer_insert_ws):
        for rows in (2**32, 2**63):
            refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, max_rows=rows), b"exceeds uint32 sel_t")


def test_overlapping_out_sel_and_sel_are_refused(lib):
    cols, dst, dcols = columns(1), handles(BF2), columns(1)
    for n in (1000, SMALL_ROWS):
        for out_sel in (SEL, SEL + 4, SEL - 4, SEL + 4 * (n - 1), SEL - 4 * (n - 1), SEL + 2000):
            for call in COUNTED:
                refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, max_rows=n, out_sel=out_sel),
                        b"out_sel overlaps sel")


def test_transfer_into_a_probed_filter_is_refused(lib):
    """The handles are compared before any of them is looked into: made-up handles are enough."""
    cols = columns(3)
    probed = handles(BF, BF2, BF3)
    for call in TRANSFERS:
        refused(lib, call(lib, probed, cols, 3, handles(BF3), cols, 1),
                b"destination filter 0 is probed filter 2 of the same call")
        refused(lib, call(lib, probed, cols, 2, handles(BF3, BF), cols, 2),
                b"destination filter 1 is probed filter 0 of the same call")
        refused(lib, call(lib, probed, cols, 1, handles(BF2, BF), cols, 2, max_rows=0),
                b"destination filter 1 is probed filter 0")  # ... even at max_rows = 0
        refused(lib, call(lib, probed, cols, 1, handles(BF2, BF), cols, 2, max_rows=2**40),
                b"destination filter 1 is probed filter 0")  # ... and before the size check


def test_a_zero_mask_takes_the_twins_checks(lib):
    """range_mask == 0 hands over to the twin: its refusals, its messages."""
    cols, dst, dcols = columns(1), handles(BF2), columns(1)
    for call in COUNTED:
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, mask=0, count=None), b"null count_dev")
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, mask=0, out_sel=SEL), b"out_sel overlaps sel")
    for call in SMALL:
        refused(lib, call(lib, handles(BF), cols, 1, dst, dcols, 1, mask=0, max_rows=SMALL_ROWS + 1),
                b"exceeds RPT_SMALL_PROBE_ROWS")
    refused(lib, chain_rows(lib, handles(BF), cols, 1, mask=0, n=SMALL_ROWS + 1), b"exceeds RPT_SMALL_PROBE_ROWS")
    refused(lib, chain_rows(lib, handles(None), cols, 1, mask=0), b"null filter 0")
