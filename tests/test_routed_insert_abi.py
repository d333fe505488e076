"""The routed device-side inserts (rpt_bf_insert_bits_ws, rpt_bf_insert_sel_ws, rpt_bf_transfer_insert_ws and its
sizing function) without a GPU: the symbols are declared, exported and bound, the Python names exist, and every
argument check that needs no look into a handle refuses before a handle is looked into. The handles and pointers
here are made-up values, never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from rpt_amd import _lib

NEW = ("rpt_bf_insert_bits_ws", "rpt_bf_insert_sel_ws", "rpt_bf_transfer_insert_workspace_bytes",
       "rpt_bf_transfer_insert_ws")
BF, BF2 = 0x7F0000010000, 0x7F0000020000  # "filters"
PTR = 0x7F0000100000                      # "device memory", 16-byte aligned
INVALID = _lib.RPT_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def col(key_type=0, keys=PTR):
    return _lib.KeyColumn(key_type, keys, None, None)


def refused(lib, status, message):
    assert status == INVALID
    assert message in lib.rpt_last_error(), lib.rpt_last_error()


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "rpt_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["rpt_bf_transfer_insert_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES["rpt_bf_insert_bits_ws"][1]) == 8
    assert len(_lib.SIGNATURES["rpt_bf_insert_sel_ws"][1]) == 8
    assert len(_lib.SIGNATURES["rpt_bf_transfer_insert_ws"][1]) == len(_lib.SIGNATURES["rpt_bf_transfer_ws"][1]) + 2
    assert lib.rpt_abi_version() == 1


def test_python_names_exist():
    import rpt_amd

    assert callable(rpt_amd.transfer_insert_ws) and callable(rpt_amd.transfer_insert_workspace_bytes)
    assert callable(rpt_amd.BloomFilter.insert_bits_ws) and callable(rpt_amd.BloomFilter.insert_sel_ws)


def test_insert_bits_ws_refusals(lib):
    c = col()
    call = lib.rpt_bf_insert_bits_ws
    refused(lib, call(None, ctypes.byref(c), None, 10, PTR, PTR, 1 << 20, None), b"null filter")
    refused(lib, call(BF, ctypes.byref(c), None, 1 << 32, PTR, PTR, 1 << 20, None), b"exceeds uint32 sel_t")
    refused(lib, call(BF, None, None, 10, PTR, PTR, 1 << 20, None), b"null key column")
    refused(lib, call(BF, ctypes.byref(col(keys=None)), None, 10, PTR, PTR, 1 << 20, None), b"null keys pointer")
    for kt in (-1, 3):
        refused(lib, call(BF, ctypes.byref(col(key_type=kt)), None, 10, PTR, PTR, 1 << 20, None), b"bad key_type")
    refused(lib, call(BF, ctypes.byref(c), None, 10, None, PTR, 1 << 20, None), b"null row_bits")
    # n == 0 is a no-op, whatever else is passed
    assert call(BF, ctypes.byref(c), None, 0, PTR, None, 0, None) == _lib.RPT_OK
    assert call(BF, None, None, 0, None, None, 0, None) == _lib.RPT_OK


def test_insert_sel_ws_refusals(lib):
    c = col(key_type=1)
    call = lib.rpt_bf_insert_sel_ws
    refused(lib, call(None, ctypes.byref(c), PTR, PTR, 10, PTR, 1 << 20, None), b"null filter")
    refused(lib, call(BF, ctypes.byref(c), PTR, PTR, 1 << 32, PTR, 1 << 20, None), b"exceeds uint32 sel_t")
    refused(lib, call(BF, None, PTR, PTR, 10, PTR, 1 << 20, None), b"null key column")
    refused(lib, call(BF, ctypes.byref(col(keys=None)), PTR, PTR, 10, PTR, 1 << 20, None), b"null keys pointer")
    refused(lib, call(BF, ctypes.byref(col(key_type=7)), PTR, PTR, 10, PTR, 1 << 20, None), b"bad key_type")
    refused(lib, call(BF, ctypes.byref(c), None, PTR, 10, PTR, 1 << 20, None), b"null sel")
    refused(lib, call(BF, ctypes.byref(c), PTR, None, 10, PTR, 1 << 20, None), b"null count_dev")
    assert call(BF, ctypes.byref(c), PTR, PTR, 0, None, 0, None) == _lib.RPT_OK
    assert call(BF, None, None, None, 0, None, 0, None) == _lib.RPT_OK


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def test_transfer_insert_ws_refusals(lib):
    cols = (_lib.KeyColumn * 1)(col())
    many = (_lib.KeyColumn * 9)(*[col() for _ in range(9)])
    call = lib.rpt_bf_transfer_insert_ws

    def run(filters, n_filters, dst, n_dst, dst_cols=cols, out_count=PTR):
        return call(filters, cols, n_filters, dst, dst_cols, n_dst, None, 100, PTR, out_count, PTR, 1 << 20, PTR, 1 << 20,
                    None)

    refused(lib, run(None, 1, handles(BF2), 1), b"null argument")
    refused(lib, run(handles(BF), 1, None, 1), b"null argument")
    refused(lib, run(handles(BF), 1, handles(BF2), 1, dst_cols=None), b"null argument")
    refused(lib, run(handles(BF), 1, handles(BF2), 1, out_count=None), b"null argument")
    refused(lib, run(handles(BF), 0, handles(BF2), 1), b"n_filters=0 outside 1..8")
    for n_dst in (0, 9):
        refused(lib, run(handles(BF), 1, handles(*[BF2 + 4096 * j for j in range(9)]), n_dst, dst_cols=many),
                b"n_dst=%d outside 1..8" % n_dst)
    refused(lib, run(handles(None), 1, handles(BF2), 1), b"null filter 0")
    refused(lib, run(handles(BF), 1, handles(None), 1), b"null destination filter 0")
    refused(lib, run(handles(BF), 1, handles(BF), 1), b"destination filter 0 is probed filter 0 of the same call")
    two = (_lib.KeyColumn * 2)(col(), col())
    assert call(handles(BF, BF2), two, 2, handles(BF2 + 4096, BF2), two, 2, None, 100, PTR, PTR, PTR, 1 << 20, PTR,
                1 << 20, None) == INVALID
    assert b"destination filter 1 is probed filter 1 of the same call" in lib.rpt_last_error()


def test_transfer_insert_workspace_bytes_is_zero_on_null_or_invalid_arguments(lib):
    size = lib.rpt_bf_transfer_insert_workspace_bytes
    assert size(None, 1, 1 << 20) == 0
    assert size(handles(None), 1, 1 << 20) == 0
    assert size(handles(BF), 0, 1 << 20) == 0
    assert size(handles(*[BF + 4096 * j for j in range(9)]), 9, 1 << 20) == 0
    assert size(handles(BF), 1, 1 << 32) == 0
