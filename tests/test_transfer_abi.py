"""rpt_bf_insert_bits / rpt_bf_insert_sel / rpt_bf_transfer_ws argument checks that need no GPU: the three symbols
are declared, exported and bound; null and out-of-range arguments are refused (RPT_ERR_INVALID_ARGUMENT) before any
device is touched, and rpt_last_error() names the problem. The non-null pointers and filter handles here are
made-up values that are never dereferenced (every check under test comes before the first look into a handle)."""
import ctypes

from rpt_amd import _lib

INVALID = _lib.RPT_ERR_INVALID_ARGUMENT
OK = _lib.RPT_OK

BF, BF2 = 0x7F0000010000, 0x7F0000020000  # made-up rpt_bf handles
KEYS, BITS, SEL, COUNT = 0x7F0000100000, 0x7F0000200000, 0x7F0000300000, 0x7F0000400000
OUT_SEL, OUT_COUNT, WS = 0x7F0000500000, 0x7F0000600000, 0x7F0000700000


def column(key_type=_lib.RPT_KEY_I64, keys=KEYS):
    return _lib.KeyColumn(key_type, keys, None, None)


def transfer(lib, filters, cols, k, dst, dst_cols, n_dst, n=1000, out_count=OUT_COUNT):
    return lib.rpt_bf_transfer_ws(filters, cols, k, dst, dst_cols, n_dst, None, n, OUT_SEL, out_count, WS, 1 << 20, None)


def test_the_three_functions_are_bound_and_exported():
    lib = _lib.load()
    for name in ("rpt_bf_insert_bits", "rpt_bf_insert_sel", "rpt_bf_transfer_ws"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible
    import rpt_amd

    assert callable(rpt_amd.transfer_ws)
    assert callable(rpt_amd.BloomFilter.insert_bits) and callable(rpt_amd.BloomFilter.insert_sel)


def test_insert_bits_null_arguments_are_refused():
    lib = _lib.load()
    col = column()
    assert lib.rpt_bf_insert_bits(None, ctypes.byref(col), None, 10, BITS, None) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert lib.rpt_bf_insert_bits(BF, None, None, 10, BITS, None) == INVALID
    assert b"null" in lib.rpt_last_error()
    nokeys = column(keys=None)
    assert lib.rpt_bf_insert_bits(BF, ctypes.byref(nokeys), None, 10, BITS, None) == INVALID
    assert b"null keys" in lib.rpt_last_error()
    assert lib.rpt_bf_insert_bits(BF, ctypes.byref(col), None, 10, None, None) == INVALID
    assert b"null row_bits" in lib.rpt_last_error()


def test_insert_sel_null_arguments_are_refused():
    lib = _lib.load()
    col = column()
    assert lib.rpt_bf_insert_sel(None, ctypes.byref(col), SEL, COUNT, 10, None) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert lib.rpt_bf_insert_sel(BF, None, SEL, COUNT, 10, None) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert lib.rpt_bf_insert_sel(BF, ctypes.byref(col), None, COUNT, 10, None) == INVALID
    assert b"null sel" in lib.rpt_last_error()
    assert lib.rpt_bf_insert_sel(BF, ctypes.byref(col), SEL, None, 10, None) == INVALID
    assert b"null count_dev" in lib.rpt_last_error()


def test_bad_key_types_are_refused():
    lib = _lib.load()
    for kt in (-1, 3, 99):
        col = column(key_type=kt)
        assert lib.rpt_bf_insert_bits(BF, ctypes.byref(col), None, 10, BITS, None) == INVALID
        assert b"key_type" in lib.rpt_last_error()
        assert lib.rpt_bf_insert_sel(BF, ctypes.byref(col), SEL, COUNT, 10, None) == INVALID
        assert b"key_type" in lib.rpt_last_error()


def test_row_counts_past_uint32_are_refused():
    lib = _lib.load()
    col = column()
    for n in (2**32, 2**32 + 1, 2**63):
        assert lib.rpt_bf_insert_bits(BF, ctypes.byref(col), None, n, BITS, None) == INVALID
        assert b"exceeds uint32" in lib.rpt_last_error()
        assert lib.rpt_bf_insert_sel(BF, ctypes.byref(col), SEL, COUNT, n, None) == INVALID
        assert b"exceeds uint32" in lib.rpt_last_error()


def test_zero_rows_is_a_no_op():
    lib = _lib.load()
    col = column()
    assert lib.rpt_bf_insert_bits(BF, ctypes.byref(col), None, 0, BITS, None) == OK
    assert lib.rpt_bf_insert_sel(BF, ctypes.byref(col), SEL, COUNT, 0, None) == OK
    # ... but not for a null filter
    assert lib.rpt_bf_insert_bits(None, ctypes.byref(col), None, 0, BITS, None) == INVALID
    assert lib.rpt_bf_insert_sel(None, ctypes.byref(col), SEL, COUNT, 0, None) == INVALID


def test_transfer_null_arguments_are_refused():
    lib = _lib.load()
    handles = (ctypes.c_void_p * 1)(BF)
    dst = (ctypes.c_void_p * 1)(BF2)
    cols = (_lib.KeyColumn * 1)(column())
    dcols = (_lib.KeyColumn * 1)(column())
    for args in ((None, cols, 1, dst, dcols, 1), (handles, None, 1, dst, dcols, 1), (handles, cols, 1, None, dcols, 1),
                 (handles, cols, 1, dst, None, 1)):
        assert transfer(lib, *args) == INVALID
        assert b"null" in lib.rpt_last_error()
    assert transfer(lib, handles, cols, 1, dst, dcols, 1, out_count=None) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert transfer(lib, (ctypes.c_void_p * 1)(None), cols, 1, dst, dcols, 1) == INVALID
    assert b"null filter 0" in lib.rpt_last_error()
    assert transfer(lib, handles, cols, 1, (ctypes.c_void_p * 1)(None), dcols, 1) == INVALID
    assert b"null destination filter 0" in lib.rpt_last_error()


def test_transfer_filter_and_destination_counts_outside_the_limit_are_refused():
    lib = _lib.load()
    handles = (ctypes.c_void_p * 9)(*[BF] * 9)
    dst = (ctypes.c_void_p * 9)(*[BF2] * 9)
    cols = (_lib.KeyColumn * 9)(*[column()] * 9)
    for n_dst in (0, 9, 2**32 - 1):
        assert transfer(lib, handles, cols, 1, dst, cols, n_dst) == INVALID
        assert b"n_dst" in lib.rpt_last_error() and b"1..8" in lib.rpt_last_error()
    for k in (0, 9):
        assert transfer(lib, handles, cols, k, dst, cols, 1) == INVALID
        assert b"n_filters" in lib.rpt_last_error() and b"1..8" in lib.rpt_last_error()


def test_transfer_into_a_probed_filter_is_refused():
    """The handles are compared before any of them is looked into: made-up handles are enough."""
    lib = _lib.load()
    a, b, c = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000
    cols = (_lib.KeyColumn * 3)(*[column()] * 3)
    handles = (ctypes.c_void_p * 3)(a, b, c)
    assert transfer(lib, handles, cols, 3, (ctypes.c_void_p * 1)(c), cols, 1) == INVALID
    assert b"destination filter 0 is probed filter 2" in lib.rpt_last_error()
    assert transfer(lib, handles, cols, 2, (ctypes.c_void_p * 2)(c, a), cols, 2) == INVALID
    assert b"destination filter 1 is probed filter 0" in lib.rpt_last_error()
    assert transfer(lib, handles, cols, 1, (ctypes.c_void_p * 2)(b, a), cols, 2, n=0) == INVALID  # ... whatever n is
