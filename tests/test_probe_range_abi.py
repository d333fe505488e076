"""The min/max range calls (rpt_bf_range_bits, rpt_bf_probe_chain_range_workspace_bytes, rpt_bf_probe_chain_range_ws,
rpt_bf_transfer_range_ws, rpt_bf_transfer_insert_range_ws) without a GPU: the symbols are declared, exported and bound,
the Python names exist, and every argument check that needs no look into a handle refuses before a handle is looked
into (tests/test_probe_sel_small_abi.py does the same for the one-launch device-counted probes). The handles and device
pointers here are made-up values, never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

NEW = ("rpt_bf_range_bits", "rpt_bf_probe_chain_range_workspace_bytes", "rpt_bf_probe_chain_range_ws",
       "rpt_bf_transfer_range_ws", "rpt_bf_transfer_insert_range_ws")
TWINS = {"rpt_bf_probe_chain_range_ws": "rpt_bf_probe_chain_ws", "rpt_bf_transfer_range_ws": "rpt_bf_transfer_ws",
         "rpt_bf_transfer_insert_range_ws": "rpt_bf_transfer_insert_ws",
         "rpt_bf_probe_chain_range_workspace_bytes": "rpt_bf_probe_chain_workspace_bytes"}
BF, BF2, BF3 = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000  # "filters"
KEYS, OUT_SEL, OUT_COUNT = 0x7F0000100000, 0x7F0000500000, 0x7F0000600000  # "device memory", 16-byte aligned
WS, IWS, BITS = 0x7F0000700000, 0x7F0000800000, 0x7F0000900000
INVALID = _lib.RPT_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def col(key_type=_lib.RPT_KEY_I64, keys=KEYS):
    return _lib.KeyColumn(key_type, keys, None, None)


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def columns(k, hash_at=None):
    return (_lib.KeyColumn * k)(*[col(_lib.RPT_KEY_HASH if f == hash_at else _lib.RPT_KEY_I64) for f in range(k)])


def refused(lib, status, message):
    assert status == INVALID
    assert message in lib.rpt_last_error(), lib.rpt_last_error()


def chain(lib, filters, cols, k, mask=1, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_probe_chain_range_ws(filters, cols, k, mask, None, n, out_sel, out_count, WS, 1 << 20, None)


def transfer(lib, filters, cols, k, dst, dst_cols, n_dst, mask=1, n=1000, out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_range_ws(filters, cols, k, mask, dst, dst_cols, n_dst, None, n, OUT_SEL, out_count, WS,
                                        1 << 20, None)


def transfer_insert(lib, filters, cols, k, dst, dst_cols, n_dst, mask=1, n=1000, out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_insert_range_ws(filters, cols, k, mask, dst, dst_cols, n_dst, None, n, OUT_SEL, out_count,
                                               WS, 1 << 20, IWS, 1 << 20, None)


TRANSFERS = (transfer, transfer_insert)


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["rpt_bf_probe_chain_range_workspace_bytes"][0] is ctypes.c_size_t
    for name in NEW:
        if name != "rpt_bf_probe_chain_range_workspace_bytes":
            assert _lib.SIGNATURES[name][0] is ctypes.c_int
    # each range call is its twin's argument list with the 32-bit mask after n_filters
    for name, twin in TWINS.items():
        want = list(_lib.SIGNATURES[twin][1])
        want.insert(want.index(ctypes.c_uint32) + 1, ctypes.c_uint32)
        assert _lib.SIGNATURES[name][1] == want, name
    # rpt_bf_range_bits: rpt_bf_probe_bits without the workspace and its size
    bits = _lib.SIGNATURES["rpt_bf_probe_bits"][1]
    assert _lib.SIGNATURES["rpt_bf_range_bits"][1] == bits[:-3] + bits[-1:]
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_python_names_exist():
    import rpt_amd

    for name in ("probe_chain_range_workspace_bytes", "probe_chain_range_ws", "transfer_range_ws",
                 "transfer_insert_range_ws"):
        assert callable(getattr(rpt_amd, name)), name
    assert callable(rpt_amd.BloomFilter.range_bits)


def test_range_mask_as_int_or_bools():
    from rpt_amd.bloom import _range_mask_of

    assert _range_mask_of(0b101, 3) == 0b101
    assert _range_mask_of([True, False, True], 3) == 0b101
    assert _range_mask_of((False, False), 2) == 0
    assert _range_mask_of(1 << 7, 2) == 1 << 7  # an int is handed on as it is: the library refuses the bit
    with pytest.raises(_lib.RptError):
        _range_mask_of([True], 2)
    with pytest.raises(_lib.RptError):
        _range_mask_of(-1, 2)


def test_range_bits_refusals(lib):
    c = col()
    refused(lib, lib.rpt_bf_range_bits(None, ctypes.byref(c), None, 10, BITS, None), b"null argument")
    refused(lib, lib.rpt_bf_range_bits(BF, ctypes.byref(c), None, 10, None, None), b"null argument")
    refused(lib, lib.rpt_bf_range_bits(BF, ctypes.byref(c), None, 2**32, BITS, None), b"exceeds uint32 sel_t")
    assert lib.rpt_bf_range_bits(BF, ctypes.byref(c), None, 0, BITS, None) == _lib.RPT_OK  # n == 0: a no-op
    refused(lib, lib.rpt_bf_range_bits(BF, None, None, 10, BITS, None), b"null key column")
    h = col(_lib.RPT_KEY_HASH)
    refused(lib, lib.rpt_bf_range_bits(BF, ctypes.byref(h), None, 10, BITS, None), b"hashes")
    bad = col(key_type=7)
    refused(lib, lib.rpt_bf_range_bits(BF, ctypes.byref(bad), None, 10, BITS, None), b"bad key_type")


def test_chain_null_lists_and_handles_are_refused(lib):
    cols = columns(2)
    refused(lib, chain(lib, None, cols, 1), b"null argument")
    refused(lib, chain(lib, handles(BF), None, 1), b"null argument")
    refused(lib, chain(lib, handles(BF), cols, 1, out_count=None), b"null argument")
    refused(lib, chain(lib, handles(None), cols, 1), b"null filter 0")
    refused(lib, chain(lib, handles(BF, None), cols, 2, mask=2), b"null filter 1")
    refused(lib, chain(lib, handles(None), cols, 1, n=0), b"null filter 0")  # ... whatever n is


def test_transfer_null_lists_and_handles_are_refused(lib):
    cols, dcols = columns(1), columns(1)
    for call in TRANSFERS:
        for args in ((None, cols, 1, handles(BF2), dcols, 1), (handles(BF), None, 1, handles(BF2), dcols, 1),
                     (handles(BF), cols, 1, None, dcols, 1), (handles(BF), cols, 1, handles(BF2), None, 1)):
            refused(lib, call(lib, *args), b"null argument")
        refused(lib, call(lib, handles(BF), cols, 1, handles(BF2), dcols, 1, out_count=None), b"null argument")
        refused(lib, call(lib, handles(None), cols, 1, handles(BF2), dcols, 1), b"null filter 0")
        refused(lib, call(lib, handles(BF), cols, 1, handles(None), dcols, 1), b"null destination filter 0")
        refused(lib, call(lib, handles(BF), cols, 1, handles(BF2, None), columns(2), 2), b"null destination filter 1")


def test_filter_and_destination_counts_outside_the_limit_are_refused(lib):
    nine, dst, cols = handles(*[BF] * 9), handles(*[BF2 + 4096 * j for j in range(9)]), columns(9)
    for k in (0, 9, 2**32 - 1):
        refused(lib, chain(lib, nine, cols, k), b"n_filters=%d outside 1..8" % k)
        for call in TRANSFERS:
            refused(lib, call(lib, nine, cols, k, dst, cols, 1), b"n_filters=%d outside 1..8" % k)
    for n_dst in (0, 9, 2**32 - 1):
        for call in TRANSFERS:
            refused(lib, call(lib, nine, cols, 1, dst, cols, n_dst), b"n_dst=%d outside 1..8" % n_dst)


def test_a_mask_bit_at_or_above_n_filters_is_refused(lib):
    cols, dst = columns(8), handles(BF3)
    for k, mask in ((1, 0b10), (2, 0b101), (3, 1 << 3), (8, 1 << 8), (1, 1 << 31), (2, 0xFFFFFFFF)):
        filters = handles(*[BF + 4096 * f for f in range(k)])
        refused(lib, chain(lib, filters, cols, k, mask=mask), b"at or above n_filters=%d" % k)
        for call in TRANSFERS:
            refused(lib, call(lib, filters, cols, k, dst, columns(1), 1, mask=mask), b"at or above n_filters=%d" % k)
        assert lib.rpt_bf_probe_chain_range_workspace_bytes(filters, k, mask, 1000) == 0
        assert b"at or above n_filters" in lib.rpt_last_error()
    refused(lib, chain(lib, handles(BF), cols, 1, mask=0b10, n=0), b"at or above n_filters=1")  # ... even at n = 0


def test_a_flagged_hash_column_is_refused(lib):
    filters, dst = handles(BF, BF2), handles(BF3)
    for hash_at in (0, 1):
        cols = columns(2, hash_at=hash_at)
        for mask in (1 << hash_at, 0b11):
            refused(lib, chain(lib, filters, cols, 2, mask=mask), b"range_mask flags filter %d" % hash_at)
            for call in TRANSFERS:
                refused(lib, call(lib, filters, cols, 2, dst, columns(1), 1, mask=mask),
                        b"range_mask flags filter %d" % hash_at)
    refused(lib, chain(lib, filters, columns(2, hash_at=1), 2, mask=0b10, n=0), b"range_mask flags filter 1")


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


def test_workspace_bytes_is_zero_on_invalid_arguments(lib):
    for mask in (0, 1):
        assert lib.rpt_bf_probe_chain_range_workspace_bytes(None, 1, mask, 1000) == 0
        assert lib.rpt_bf_probe_chain_range_workspace_bytes(handles(BF), 0, mask, 1000) == 0
        assert lib.rpt_bf_probe_chain_range_workspace_bytes(handles(*[BF] * 9), 9, mask, 1000) == 0
        assert lib.rpt_bf_probe_chain_range_workspace_bytes(handles(None), 1, mask, 1000) == 0
