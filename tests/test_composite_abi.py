"""The composite-key calls (rpt_hash_keys_composite, rpt_bf_insert_composite, rpt_bf_probe_chain_composite,
rpt_bf_transfer_composite, rpt_bf_insert_multi_composite) without a GPU: the symbols are declared, exported and bound,
the three one-launch calls' signatures are their single-column twins' with a key list for each column list, the Python
names exist, and every argument check that needs no look into a handle refuses before a handle is looked into, names
the argument in rpt_last_error, and comes in the documented order (of two faults the earlier check wins), after the
pattern of tests/test_transfer_small_abi.py. The handles and device pointers here are made-up values, never
dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

NEW = ("rpt_hash_keys_composite", "rpt_bf_insert_composite", "rpt_bf_probe_chain_composite",
       "rpt_bf_transfer_composite", "rpt_bf_insert_multi_composite")
TWINS = {"rpt_bf_probe_chain_composite": "rpt_bf_probe_chain", "rpt_bf_transfer_composite": "rpt_bf_transfer",
         "rpt_bf_insert_multi_composite": "rpt_bf_insert_multi"}
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
MAX_KEY_COLUMNS, MAX_CHAIN_KEY_COLUMNS = 4, 16
BF, BF2, BF3 = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000  # "filters"
KEYS, SEL = 0x7F0000100000, 0x7F0000300000  # "device memory", 16-byte aligned
OUT, OUT_SEL, OUT_COUNT = 0x7F0000400000, 0x7F0000500000, 0x7F0000600000
INVALID = _lib.RPT_ERR_INVALID_ARGUMENT
I64, I32, HASH = _lib.RPT_KEY_I64, _lib.RPT_KEY_I32, _lib.RPT_KEY_HASH


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def key(*types, null_cols=False, null_keys_at=None, n_cols=None):
    """One rpt_composite_key whose columns have the given key types; the column array stays alive with it."""
    arr = (_lib.KeyColumn * max(len(types), 1))(*[
        _lib.KeyColumn(t, None if j == null_keys_at else KEYS + 4096 * j, None, None) for j, t in enumerate(types)])
    k = _lib.CompositeKey(None if null_cols else arr, len(types) if n_cols is None else n_cols)
    k._arr = arr
    return k


def keys(*ks):
    arr = (_lib.CompositeKey * len(ks))(*ks)
    arr._ks = ks
    return arr


def refused(lib, status, *messages):
    assert status == INVALID
    for message in messages:
        assert message in lib.rpt_last_error(), lib.rpt_last_error()


def chain(lib, filters, ks, k, row_sel=None, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    return lib.rpt_bf_probe_chain_composite(filters, ks, k, row_sel, n, out_sel, out_count, None)


def transfer(lib, filters, ks, k, dst=None, dks=None, n_dst=1, row_sel=None, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT):
    dst = handles(BF3) if dst is None else dst
    dks = keys(key(I64)) if dks is None else dks
    return lib.rpt_bf_transfer_composite(filters, ks, k, dst, dks, n_dst, row_sel, n, out_sel, out_count, None)


def transfer_dst(lib, dst, dks, n_dst, **kw):
    """rpt_bf_transfer_composite with a good probed side: the destination side is what is checked."""
    return transfer(lib, handles(BF), keys(key(I64)), 1, dst, dks, n_dst, **kw)


def multi(lib, dst, dks, n_dst, row_sel=None, n=1000):
    return lib.rpt_bf_insert_multi_composite(dst, dks, n_dst, row_sel, n, None)


PROBED = (chain, transfer)  # (filters, keys, n_filters, ...)
SINKS = (transfer_dst, multi)  # (dst_filters, dst_keys, n_dst, ...)


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    assert int(re.search(r"#define\s+RPT_MAX_KEY_COLUMNS\s+(\d+)", header).group(1)) == MAX_KEY_COLUMNS
    assert int(re.search(r"#define\s+RPT_MAX_CHAIN_KEY_COLUMNS\s+(\d+)", header).group(1)) == MAX_CHAIN_KEY_COLUMNS
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct rpt_composite_key \{\s*const rpt_key_column\* cols;\s*uint32_t n_cols;\s*\} rpt_composite_key;",
                     header)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert [f[0] for f in _lib.CompositeKey._fields_] == ["cols", "n_cols"]
    assert ctypes.sizeof(_lib.CompositeKey) == 16
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_the_one_launch_calls_are_their_twins_with_keys_for_columns():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rpt_gpu.h")).read(), flags=re.S)

    def params(name):
        text = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        return [" ".join(p.split()) for p in text.split(",")]

    for name, twin in TWINS.items():
        want = [p.replace("const rpt_key_column* cols", "const rpt_composite_key* keys")
                .replace("const rpt_key_column* dst_cols", "const rpt_composite_key* dst_keys") for p in params(twin)]
        assert params(name) == want, name
        col, ckey = ctypes.POINTER(_lib.KeyColumn), ctypes.POINTER(_lib.CompositeKey)
        assert _lib.SIGNATURES[name][1] == [ckey if t is col else t for t in _lib.SIGNATURES[twin][1]], name
    assert params("rpt_hash_keys_composite") == ["const rpt_composite_key* key", "uint64_t n", "uint64_t* out_hashes",
                                                 "rpt_stream_t stream"]
    assert params("rpt_bf_insert_composite") == ["rpt_bf* bf", "const rpt_composite_key* key", "uint64_t n",
                                                 "rpt_stream_t stream"]


def test_python_names_exist():
    import rpt_amd

    for name in ("composite_key", "hash_columns_fused", "probe_chain_composite", "transfer_composite",
                 "insert_multi_composite"):
        assert callable(getattr(rpt_amd, name)), name
    assert callable(rpt_amd.BloomFilter.insert_composite)
    assert callable(rpt_amd.hash_columns)  # the two-pass baseline stays


def test_a_bad_single_key_is_refused_before_the_filter_or_the_output_is_looked_at(lib):
    """rpt_hash_keys_composite and rpt_bf_insert_composite: the key checks come first, whatever else is wrong."""
    calls = (lambda k, n=1000: lib.rpt_hash_keys_composite(k, n, OUT, None),
             lambda k, n=1000: lib.rpt_hash_keys_composite(k, n, None, None),
             lambda k, n=1000: lib.rpt_bf_insert_composite(BF, k, n, None),
             lambda k, n=1000: lib.rpt_bf_insert_composite(None, k, n, None))
    for call in calls:
        for n in (1000, 0, 2**40):
            refused(lib, call(None, n), b"null key")
            refused(lib, call(ctypes.byref(key(I64, I64, null_cols=True)), n), b"null cols")
            refused(lib, call(ctypes.byref(key(I64, n_cols=0)), n), b"n_cols=0 outside 1..4")
            refused(lib, call(ctypes.byref(key(I64, I32, I64, I32, I64)), n), b"n_cols=5 outside 1..4")
            refused(lib, call(ctypes.byref(key(I64, n_cols=2**32 - 1)), n), b"n_cols=4294967295 outside 1..4")
            refused(lib, call(ctypes.byref(key(I64, HASH)), n), b"HASH column at position 1")
            refused(lib, call(ctypes.byref(key(HASH, I64, I32, HASH)), n), b"HASH column at position 3")
            refused(lib, call(ctypes.byref(key(I64, 77)), n), b"bad key_type 77", b"column 1")
            refused(lib, call(ctypes.byref(key(I64, -1)), n), b"bad key_type -1")
            refused(lib, call(ctypes.byref(key(I64, I32, null_keys_at=1)), n), b"null keys pointer", b"column 1")
            refused(lib, call(ctypes.byref(key(I64, null_keys_at=0)), n), b"null keys pointer", b"column 0")
    # a good key of two columns: the output, then the filter
    good = key(HASH, I32)
    refused(lib, lib.rpt_hash_keys_composite(ctypes.byref(good), 1000, None, None), b"null out")
    refused(lib, lib.rpt_bf_insert_composite(None, ctypes.byref(good), 1000, None), b"null filter")
    # ... and one column forwards to the single-column call, whose refusals these are
    refused(lib, lib.rpt_hash_keys_composite(ctypes.byref(key(I64)), 1000, None, None), b"null out")
    refused(lib, lib.rpt_bf_insert_composite(None, ctypes.byref(key(I64)), 1000, None), b"null filter")
    assert lib.rpt_hash_keys_composite(ctypes.byref(good), 0, OUT, None) == _lib.RPT_OK  # nothing to do


def test_null_lists_and_counts_outside_the_limit_are_refused(lib):
    nine = handles(*[BF + 4096 * f for f in range(9)])
    ks = keys(*[key(I64, I32) for _ in range(9)])
    for call in PROBED:
        refused(lib, call(lib, None, ks, 1), b"null argument")
        refused(lib, call(lib, nine, None, 1), b"null argument")
        refused(lib, call(lib, nine, ks, 1, out_count=None), b"null argument")
        for k in (0, 9, 2**32 - 1):
            refused(lib, call(lib, nine, ks, k), b"n_filters=%d outside 1..8" % k)
            refused(lib, call(lib, nine, ks, k, n=0), b"n_filters=%d outside 1..8" % k)  # ... whatever n is
    refused(lib, lib.rpt_bf_transfer_composite(nine, ks, 1, None, ks, 1, None, 1000, OUT_SEL, OUT_COUNT, None), b"null argument")
    refused(lib, lib.rpt_bf_transfer_composite(nine, ks, 1, nine, None, 1, None, 1000, OUT_SEL, OUT_COUNT, None), b"null argument")
    refused(lib, multi(lib, None, ks, 1), b"null argument")
    refused(lib, multi(lib, nine, None, 1), b"null argument")
    for n_dst in (0, 9, 2**32 - 1):
        for call in SINKS:
            refused(lib, call(lib, nine, ks, n_dst), b"n_dst=%d outside 1..8" % n_dst)
    # the counts come before the keys they let the call read
    refused(lib, chain(lib, nine, keys(key(I64, HASH)), 9), b"n_filters=9 outside 1..8")


def test_a_bad_key_in_a_list_is_refused_and_named(lib):
    two = handles(BF, BF2)
    good = key(I64, I32)
    for call, side in ((chain, b"key 1"), (transfer, b"key 1")):
        refused(lib, call(lib, two, keys(good, key(I64, I64, null_cols=True)), 2), b"null cols", side)
        refused(lib, call(lib, two, keys(good, key(I64, n_cols=0)), 2), b"n_cols=0 outside 1..4", side)
        refused(lib, call(lib, two, keys(good, key(I64, I32, I64, I32, I64)), 2), b"n_cols=5 outside 1..4", side)
        refused(lib, call(lib, two, keys(good, key(I32, HASH)), 2), b"HASH column at position 1", side)
        refused(lib, call(lib, two, keys(good, key(I32, 77)), 2), b"bad key_type 77", side)
        refused(lib, call(lib, two, keys(good, key(I32, I64, null_keys_at=1)), 2), b"null keys pointer", side)
        # before any handle is looked at or compared, before the size, the overlap and n == 0
        refused(lib, call(lib, handles(None, None), keys(good, key(I32, HASH)), 2), b"HASH column at position 1")
        refused(lib, call(lib, two, keys(good, key(I32, HASH)), 2, n=2**40), b"HASH column at position 1")
        refused(lib, call(lib, two, keys(good, key(I32, HASH)), 2, n=0), b"HASH column at position 1")
        refused(lib, call(lib, two, keys(good, key(I32, HASH)), 2, row_sel=SEL, out_sel=SEL), b"HASH column at position 1")
    dst = handles(BF2, BF3)
    for call in SINKS:
        refused(lib, call(lib, dst, keys(good, key(I64, I64, null_cols=True)), 2), b"null cols", b"destination key 1")
        refused(lib, call(lib, dst, keys(good, key(I64, n_cols=0)), 2), b"n_cols=0 outside 1..4", b"destination key 1")
        refused(lib, call(lib, dst, keys(good, key(I64, I32, I64, I32, I64)), 2), b"n_cols=5 outside 1..4", b"destination key 1")
        refused(lib, call(lib, dst, keys(key(I32, HASH), good), 2), b"HASH column at position 1", b"destination key 0")
        refused(lib, call(lib, handles(None, None), keys(good, key(I32, HASH)), 2, n=2**40), b"HASH column at position 1")
    # a transfer into a probed filter is found after the keys ...
    refused(lib, transfer(lib, handles(BF), keys(good), 1, handles(BF), keys(key(I32, HASH)), 1), b"HASH column at position 1")
    # ... and the probed keys are checked before the destination keys
    refused(lib, transfer(lib, handles(BF), keys(key(I64, n_cols=0)), 1, handles(BF2), keys(key(I32, HASH)), 1),
            b"n_cols=0 outside 1..4", b"in key 0")


def test_more_than_sixteen_columns_on_a_side_are_refused(lib):
    five = handles(*[BF + 4096 * f for f in range(5)])
    seventeen = keys(key(I64, I32, I64, I32), key(I32, I64, I64, I32), key(HASH, I32, I64, I32), key(I64, I32, I64, I32),
                     key(I64))
    assert sum(k.n_cols for k in seventeen) == MAX_CHAIN_KEY_COLUMNS + 1
    for call in PROBED:
        for n in (1000, 0, SMALL_ROWS + 1):
            refused(lib, call(lib, five, seventeen, 5, n=n), b"17 columns over the keys exceed RPT_MAX_CHAIN_KEY_COLUMNS")
    for call in SINKS:
        refused(lib, call(lib, five, seventeen, 5), b"17 columns over the destination keys exceed RPT_MAX_CHAIN_KEY_COLUMNS")
    # each side has its own total: 16 probed columns and a 17-column destination side
    sixteen = keys(*[key(I64, I32, I64, I32) for _ in range(4)])
    refused(lib, transfer(lib, five, sixteen, 4, handles(*[BF3 + 4096 * j for j in range(5)]), seventeen, 5),
            b"over the destination keys")
    # 32 columns over the call, 16 a side, pass the cap: the next check (the size) is what refuses
    refused(lib, transfer(lib, five, sixteen, 4, handles(*[BF3 + 4096 * j for j in range(4)]), sixteen, 4, n=SMALL_ROWS + 1),
            b"exceeds RPT_SMALL_PROBE_ROWS")


def test_null_handles_and_a_probed_destination_are_refused(lib):
    ks = keys(key(I64, I32), key(I32), key(HASH, I64))
    probed = handles(BF, BF2, BF3)
    refused(lib, transfer(lib, handles(None), ks, 1), b"null filter 0")
    refused(lib, transfer(lib, handles(BF, None), ks, 2), b"null filter 1")
    refused(lib, transfer(lib, handles(None), ks, 1, n=0), b"null filter 0")  # ... whatever n is
    for call in SINKS:
        refused(lib, call(lib, handles(None), ks, 1), b"null destination filter 0")
        refused(lib, call(lib, handles(BF2, None), ks, 2), b"null destination filter 1")
        refused(lib, call(lib, handles(BF2, None), ks, 2, n=2**40), b"null destination filter 1")  # before the size
    refused(lib, transfer(lib, probed, ks, 3, handles(BF3), ks, 1), b"destination filter 0 is probed filter 2 of the same call")
    refused(lib, transfer(lib, probed, ks, 2, handles(BF3, BF), ks, 2), b"destination filter 1 is probed filter 0 of the same call")
    refused(lib, transfer(lib, probed, ks, 1, handles(BF2, BF), ks, 2, n=0), b"destination filter 1 is probed filter 0")
    refused(lib, transfer(lib, probed, ks, 1, handles(BF2, BF), ks, 2, n=2**40), b"destination filter 1 is probed filter 0")


def test_rows_past_the_small_batch_limit_are_refused(lib):
    ks, dst, dks = keys(key(I64, I32)), handles(BF2), keys(key(I32, I64, I32))
    for n in (SMALL_ROWS + 1, 2**32, 2**63):
        for call in PROBED:
            refused(lib, call(lib, handles(BF), ks, 1, n=n), b"exceeds RPT_SMALL_PROBE_ROWS", b"n=%d rows" % n)
            # ... before row_sel and out_sel are looked at: a null out_sel, and ranges that would overlap
            refused(lib, call(lib, handles(BF), ks, 1, n=n, out_sel=None), b"exceeds RPT_SMALL_PROBE_ROWS")
            refused(lib, call(lib, handles(BF), ks, 1, n=n, row_sel=SEL, out_sel=SEL), b"exceeds RPT_SMALL_PROBE_ROWS")
        refused(lib, multi(lib, dst, dks, 1, n=n), b"exceeds RPT_SMALL_PROBE_ROWS", b"n=%d rows" % n)
        refused(lib, multi(lib, dst, dks, 1, n=n, row_sel=SEL), b"exceeds RPT_SMALL_PROBE_ROWS")


def test_overlapping_out_sel_and_row_sel_are_refused_by_the_transfer(lib):
    """As rpt_bf_transfer: the two ranges of n 4-byte entries are compared; ranges that only abut are not an overlap
    (the next check then looks into the made-up handle, so those calls are not made here)."""
    ks = keys(key(I64, I32))
    for n in (1000, SMALL_ROWS):
        for out_sel in (SEL, SEL + 4, SEL - 4, SEL + 4 * (n - 1), SEL - 4 * (n - 1), SEL + 2000):
            refused(lib, transfer(lib, handles(BF), ks, 1, n=n, row_sel=SEL, out_sel=out_sel), b"out_sel overlaps row_sel")
    # the earlier checks win
    refused(lib, transfer(lib, handles(BF), keys(key(I64, HASH)), 1, row_sel=SEL, out_sel=SEL), b"HASH column at position 1")
    refused(lib, transfer(lib, handles(BF), ks, 1, handles(BF), ks, 1, row_sel=SEL, out_sel=SEL),
            b"destination filter 0 is probed filter 0")
