"""rpt_bf_probe_chain_ws / rpt_bf_probe_chain_workspace_bytes argument checks that need no GPU: null and
out-of-range arguments are refused (RPT_ERR_INVALID_ARGUMENT, or 0 bytes) before any device is touched, and
rpt_last_error() names the problem. The pointers here are never dereferenced."""
import ctypes

from rpt_amd import _lib

INVALID = _lib.RPT_ERR_INVALID_ARGUMENT


def chain_ws(lib, filters, cols, k, n=1000, out_sel=0x7F0000001000, out_count=0x7F0000002000, ws=0x7F0000100000,
             ws_bytes=1 << 20):
    return lib.rpt_bf_probe_chain_ws(filters, cols, k, None, n, out_sel, out_count, ws, ws_bytes, None)


def test_both_functions_are_bound_and_declared():
    lib = _lib.load()
    assert "rpt_bf_probe_chain_ws" in _lib.SIGNATURES and "rpt_bf_probe_chain_workspace_bytes" in _lib.SIGNATURES
    assert lib.rpt_bf_probe_chain_workspace_bytes.restype is ctypes.c_size_t
    assert lib.rpt_abi_version() == 1  # the additions are backward compatible


def test_null_arguments_are_refused():
    lib = _lib.load()
    handles = (ctypes.c_void_p * 2)(None, None)
    cols = (_lib.KeyColumn * 2)(_lib.KeyColumn(0, None, None, None), _lib.KeyColumn(0, None, None, None))
    assert chain_ws(lib, None, cols, 1) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert chain_ws(lib, handles, None, 1) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert chain_ws(lib, handles, cols, 1, out_count=None) == INVALID
    assert b"null" in lib.rpt_last_error()
    assert chain_ws(lib, handles, cols, 1) == INVALID  # filters[0] is null
    assert b"null filter 0" in lib.rpt_last_error()
    assert chain_ws(lib, handles, cols, 2, n=0) == INVALID  # ... whatever n is
    assert b"null filter 0" in lib.rpt_last_error()


def test_filter_count_outside_the_chain_limit_is_refused():
    lib = _lib.load()
    handles = (ctypes.c_void_p * 9)(*[None] * 9)
    cols = (_lib.KeyColumn * 9)()
    for k in (0, 9, 2**32 - 1):
        assert chain_ws(lib, handles, cols, k) == INVALID
        assert b"n_filters" in lib.rpt_last_error() and b"1..8" in lib.rpt_last_error()
        assert lib.rpt_bf_probe_chain_workspace_bytes(handles, k, 1000) == 0
        assert b"n_filters" in lib.rpt_last_error()


def test_workspace_bytes_of_null_arguments_is_zero():
    lib = _lib.load()
    assert lib.rpt_bf_probe_chain_workspace_bytes(None, 1, 1000) == 0
    assert b"null" in lib.rpt_last_error()
    handles = (ctypes.c_void_p * 1)(None)
    assert lib.rpt_bf_probe_chain_workspace_bytes(handles, 1, 1000) == 0
    assert b"null filter 0" in lib.rpt_last_error()
