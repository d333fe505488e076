"""Python mirror of the PTBloomFilter seam over librpt_gpu.so, on torch device tensors.

Mirrors the reference interface (src/include/bloom_filter.hpp:22-57):
    Initialize(est_num_rows)            -> BloomFilter(est_num_rows, device=...)
    Insert(chunk, cols)                 -> BloomFilter.insert(keys, key_sel=, validity=)
    LookupSel(chunk, sel, cols, _)      -> BloomFilter.lookup_sel(keys, ...) -> ascending sel
    ReinitializeAndRehash(rows, data)   -> BloomFilter.reinitialize_and_rehash(rows, chunks)
    SizedForRows() / IsEmpty() / finalized_
Errors surface as RptError (the reference raises DuckDB exceptions).
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from ._lib import (
    RPT_KEY_HASH,
    RPT_KEY_I32,
    RPT_KEY_I64,
    BfInfo,
    CompositeKey,
    KeyColumn,
    RptError,
    check,
    load,
)

SEG_ROWS = 512


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(device: torch.device, stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def key_type_of(keys: torch.Tensor, key_type: Optional[int]) -> int:
    if key_type is not None:
        return key_type
    if keys.dtype == torch.int64:
        return RPT_KEY_I64
    if keys.dtype == torch.int32:
        return RPT_KEY_I32
    raise RptError(1, f"unsupported key dtype {keys.dtype}; pass key_type=RPT_KEY_HASH for hashes")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _check_lists(filters, columns, message: str) -> None:
    if not filters or len(filters) != len(columns):
        raise RptError(1, message)


def _list_args(filters, columns):
    """(handle array, rpt_key_column array) of a filter list and its columns: device key tensors, or dicts of
    make_column's arguments (keys, key_type, key_sel, validity)."""
    cols = [make_column(**c) if isinstance(c, dict) else make_column(c) for c in columns]
    return (ctypes.c_void_p * len(filters))(*[f._h for f in filters]), (KeyColumn * len(cols))(*cols)


def _row_list_rows(columns, row_sel, n) -> int:
    """n of a row-list call (None: the length of row_sel, else of the first column's key_sel, else of its keys), with
    the row_sel check."""
    if n is None:
        c0 = columns[0] if isinstance(columns[0], dict) else {"keys": columns[0]}
        n = (row_sel.numel() if row_sel is not None else
             (c0["key_sel"].numel() if c0.get("key_sel") is not None else c0["keys"].numel()))
    if row_sel is not None and (row_sel.element_size() != 4 or not row_sel.is_cuda):
        raise RptError(1, "row_sel must be a 32-bit device tensor")
    return int(n)


def _probed_call_args(filters, columns, row_sel, n, out_sel, out_count):
    """The probed side of every chain and transfer call: the checked lists as arrays, n (None: the length of row_sel,
    else of the first column's key_sel, else of its keys), the row_sel check, and out_sel / out_count (allocated here
    when None)."""
    _check_lists(filters, columns, "one key column per filter, at least one filter")
    handles, arr = _list_args(filters, columns)
    n = _row_list_rows(columns, row_sel, n)
    device = filters[0].device
    if out_sel is None:
        out_sel = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    if out_count is None:
        out_count = torch.zeros(1, dtype=torch.int64, device=device)
    return filters[0]._lib, device, handles, arr, n, out_sel, out_count


def _dst_call_args(dst_filters, dst_columns):
    """The destination side of every transfer: the checked lists as arrays."""
    _check_lists(dst_filters, dst_columns, "one key column per destination filter, at least one destination")
    return _list_args(dst_filters, dst_columns)


def _workspace_or_new(workspace: Optional[torch.Tensor], need, device, stream) -> torch.Tensor:
    """The caller's workspace, or one of need() bytes (at least 256) allocated here."""
    if workspace is None:
        workspace = torch.empty(max(int(need()), 256), dtype=torch.uint8, device=device)
        if isinstance(stream, torch.cuda.Stream):
            workspace.record_stream(stream)  # freed on return while the call may still run on `stream`
    return workspace


def probe_chain(filters, columns, *, row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                out_sel: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None,
                stream=None) -> torch.Tensor:
    """USE_BF's filter chain in one launch (rpt_bf_probe_chain): ascending ids (int32) of the rows passing
    every filters[i] on its own key column. columns[i]: a device key tensor, or a dict of make_column's
    arguments (keys, key_type, key_sel, validity). n <= RPT_SMALL_PROBE_ROWS, 1..RPT_MAX_CHAIN filters."""
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    check(lib.rpt_bf_probe_chain(handles, arr, len(filters), _ptr(row_sel), n, out_sel.data_ptr(),
                                 out_count.data_ptr(), _stream(device, stream)))
    return out_sel[: int(out_count.item())]


def probe_chain_workspace_bytes(filters, n: int) -> int:
    """Device workspace probe_chain_ws needs for these filters (their strategies resolved for n) and n rows
    (rpt_bf_probe_chain_workspace_bytes)."""
    if not filters:
        raise RptError(1, "at least one filter")
    handles = (ctypes.c_void_p * len(filters))(*[f._h for f in filters])
    return int(filters[0]._lib.rpt_bf_probe_chain_workspace_bytes(handles, len(filters), int(n)))


def probe_chain_ws(filters, columns, *, row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                   out_sel: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """probe_chain for batches of any size (rpt_bf_probe_chain_ws): the survivors stay on the device as result
    bits between the filters, each filter runs its own probe strategy, and the selection vector is written once
    at the end. Arguments as probe_chain, plus a device workspace of probe_chain_workspace_bytes(filters, n) bytes
    (allocated here when None). Returns out_sel[:count] (reads the count back)."""
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    workspace = _workspace_or_new(
        workspace, lambda: lib.rpt_bf_probe_chain_workspace_bytes(handles, len(filters), n), device, stream)
    check(lib.rpt_bf_probe_chain_ws(handles, arr, len(filters), _ptr(row_sel), n, out_sel.data_ptr(),
                                    out_count.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                    _stream(device, stream)), lib)
    return out_sel[: int(out_count.item())]


def transfer_ws(filters, columns, dst_filters, dst_columns, *, row_sel: Optional[torch.Tensor] = None,
                n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
                out_count: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, stream=None):
    """One USE_BF -> CREATE_BF step on the device (rpt_bf_transfer_ws): probe_chain_ws over filters / columns,
    then the survivors inserted into dst_filters[j] on its own key column dst_columns[j]. Nothing is read back:
    returns the device tensors (out_sel, out_count), the count not synchronized (out_sel[:int(out_count)] are
    the survivors once the stream has run). Columns as in probe_chain; the destination columns are indexed by
    the same row ids as the probed ones. A destination's is_empty() is False afterwards even if no row survived
    (set_has_data(False) restores it once a zero count has been read)."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    workspace = _workspace_or_new(
        workspace, lambda: lib.rpt_bf_probe_chain_workspace_bytes(handles, len(filters), n), device, stream)
    check(lib.rpt_bf_transfer_ws(handles, arr, len(filters), dst_handles, darr, len(dst_filters), _ptr(row_sel), n,
                                 out_sel.data_ptr(), out_count.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                 _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_insert_workspace_bytes(dst_filters, n: int) -> int:
    """Insert workspace transfer_insert_ws needs for these destinations and n rows: the largest need of the
    destinations whose insert strategy routes for n, 0 if none does (rpt_bf_transfer_insert_workspace_bytes)."""
    if not dst_filters:
        raise RptError(1, "at least one destination filter")
    handles = (ctypes.c_void_p * len(dst_filters))(*[f._h for f in dst_filters])
    return int(dst_filters[0]._lib.rpt_bf_transfer_insert_workspace_bytes(handles, len(dst_filters), int(n)))


def transfer_insert_ws(filters, columns, dst_filters, dst_columns, *, row_sel: Optional[torch.Tensor] = None,
                       n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
                       out_count: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                       insert_workspace: Optional[torch.Tensor] = None, stream=None):
    """transfer_ws with each destination's insert strategy honoured (rpt_bf_transfer_insert_ws): a destination that
    resolves to RPT_INSERT_PARTITIONED for n rows takes the routed insert (partition, LDS slice merge) from the
    survivors' result bits, the others one atomic OR per row. Arguments and result as transfer_ws, plus the insert
    workspace of transfer_insert_workspace_bytes(dst_filters, n) bytes the destinations share (allocated here when
    None). Nothing is read back."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    workspace = _workspace_or_new(
        workspace, lambda: lib.rpt_bf_probe_chain_workspace_bytes(handles, len(filters), n), device, stream)
    insert_workspace = _workspace_or_new(
        insert_workspace, lambda: lib.rpt_bf_transfer_insert_workspace_bytes(dst_handles, len(dst_filters), n), device,
        stream)
    check(lib.rpt_bf_transfer_insert_ws(handles, arr, len(filters), dst_handles, darr, len(dst_filters), _ptr(row_sel),
                                        n, out_sel.data_ptr(), out_count.data_ptr(), workspace.data_ptr(),
                                        _nbytes(workspace), insert_workspace.data_ptr(), _nbytes(insert_workspace),
                                        _stream(device, stream)), lib)
    return out_sel, out_count


def _range_mask_of(range_mask, n_filters: int) -> int:
    """range_mask as the C-ABI takes it: an int as it is, a sequence of bools (one per filter) as its bits."""
    if isinstance(range_mask, (int, np.integer)) and not isinstance(range_mask, (bool, np.bool_)):
        mask = int(range_mask)
    else:
        flags = list(range_mask)
        if len(flags) != n_filters:
            raise RptError(1, f"range_mask has {len(flags)} entries for {n_filters} filters")
        mask = sum(1 << f for f, flag in enumerate(flags) if flag)
    if mask < 0 or mask >= 1 << 32:
        raise RptError(1, f"range_mask={mask} is not a 32-bit mask")
    return mask


def probe_chain_range_workspace_bytes(filters, range_mask, n: int) -> int:
    """Device workspace the range calls need for these filters, this mask and n rows
    (rpt_bf_probe_chain_range_workspace_bytes); probe_chain_workspace_bytes when the mask is 0."""
    if not filters:
        raise RptError(1, "at least one filter")
    handles = (ctypes.c_void_p * len(filters))(*[f._h for f in filters])
    return int(filters[0]._lib.rpt_bf_probe_chain_range_workspace_bytes(
        handles, len(filters), _range_mask_of(range_mask, len(filters)), int(n)))


def probe_chain_range_ws(filters, columns, *, range_mask, row_sel: Optional[torch.Tensor] = None,
                         n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
                         out_count: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                         stream=None) -> torch.Tensor:
    """probe_chain_ws restricted to the rows that also lie in the min/max range of every flagged filter on its own
    column (rpt_bf_probe_chain_range_ws). range_mask: an int (bit f flags filters[f]) or a sequence of bools, one per
    filter. The range is read on the device when the kernels run. Workspace: probe_chain_range_workspace_bytes
    (allocated here when None). Returns out_sel[:count] (reads the count back)."""
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    mask = _range_mask_of(range_mask, len(filters))
    workspace = _workspace_or_new(
        workspace, lambda: lib.rpt_bf_probe_chain_range_workspace_bytes(handles, len(filters), mask, n), device, stream)
    check(lib.rpt_bf_probe_chain_range_ws(handles, arr, len(filters), mask, _ptr(row_sel), n, out_sel.data_ptr(),
                                          out_count.data_ptr(), workspace.data_ptr(), _nbytes(workspace),
                                          _stream(device, stream)), lib)
    return out_sel[: int(out_count.item())]


def transfer_range_ws(filters, columns, dst_filters, dst_columns, *, range_mask,
                      row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                      out_sel: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None, stream=None):
    """transfer_ws over the rows that also pass the flagged filters' range tests (rpt_bf_transfer_range_ws);
    range_mask and workspace as in probe_chain_range_ws. Nothing is read back: returns (out_sel, out_count)."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    mask = _range_mask_of(range_mask, len(filters))
    workspace = _workspace_or_new(
        workspace, lambda: lib.rpt_bf_probe_chain_range_workspace_bytes(handles, len(filters), mask, n), device, stream)
    check(lib.rpt_bf_transfer_range_ws(handles, arr, len(filters), mask, dst_handles, darr, len(dst_filters),
                                       _ptr(row_sel), n, out_sel.data_ptr(), out_count.data_ptr(),
                                       workspace.data_ptr(), _nbytes(workspace), _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_insert_range_ws(filters, columns, dst_filters, dst_columns, *, range_mask,
                             row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                             out_sel: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None,
                             workspace: Optional[torch.Tensor] = None,
                             insert_workspace: Optional[torch.Tensor] = None, stream=None):
    """transfer_insert_ws over the rows that also pass the flagged filters' range tests
    (rpt_bf_transfer_insert_range_ws); range_mask and workspace as in probe_chain_range_ws, the insert workspace as in
    transfer_insert_ws. Nothing is read back: returns (out_sel, out_count)."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    mask = _range_mask_of(range_mask, len(filters))
    workspace = _workspace_or_new(
        workspace, lambda: lib.rpt_bf_probe_chain_range_workspace_bytes(handles, len(filters), mask, n), device, stream)
    insert_workspace = _workspace_or_new(
        insert_workspace, lambda: lib.rpt_bf_transfer_insert_workspace_bytes(dst_handles, len(dst_filters), n), device,
        stream)
    check(lib.rpt_bf_transfer_insert_range_ws(handles, arr, len(filters), mask, dst_handles, darr, len(dst_filters),
                                              _ptr(row_sel), n, out_sel.data_ptr(), out_count.data_ptr(),
                                              workspace.data_ptr(), _nbytes(workspace), insert_workspace.data_ptr(),
                                              _nbytes(insert_workspace), _stream(device, stream)), lib)
    return out_sel, out_count


def probe_chain_sel_workspace_bytes(filters, max_rows: int) -> int:
    """Device workspace the device-counted calls need for a selection of max_rows entries
    (rpt_bf_probe_chain_sel_workspace_bytes): result bits, segment counts and the tail's sums; no stage area."""
    if not filters:
        raise RptError(1, "at least one filter")
    handles = (ctypes.c_void_p * len(filters))(*[f._h for f in filters])
    return int(filters[0]._lib.rpt_bf_probe_chain_sel_workspace_bytes(handles, len(filters), int(max_rows)))


def _sel_call_args(filters, columns, sel, count, max_rows, out_sel, out_count, workspace=None):
    """The checked arguments the device-counted calls share; every buffer is the caller's (nothing is allocated here,
    so the calls can be captured into a graph). workspace None (the one-launch calls, which take none): 0 bytes."""
    _check_lists(filters, columns, "one key column per filter, at least one filter")
    for name, t in (("sel", sel), ("out_sel", out_sel)):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != 4:
            raise RptError(1, f"{name} must be a contiguous 32-bit device tensor")
    for name, t in (("count", count), ("out_count", out_count)):
        if not t.is_cuda or t.element_size() != 8 or t.numel() < 1:
            raise RptError(1, f"{name} must be a 64-bit device tensor")
    if workspace is not None and (not workspace.is_cuda or not workspace.is_contiguous()):
        raise RptError(1, "workspace must be a contiguous device tensor")
    max_rows = sel.numel() if max_rows is None else int(max_rows)
    if max_rows > sel.numel() or max_rows > out_sel.numel():
        raise RptError(1, f"max_rows={max_rows} exceeds the entries of sel ({sel.numel()}) or out_sel ({out_sel.numel()})")
    lib, device, handles, arr, max_rows, _, _ = _probed_call_args(filters, columns, sel, max_rows, out_sel, out_count)
    return lib, device, handles, arr, max_rows, 0 if workspace is None else _nbytes(workspace)


def probe_chain_sel_ws(filters, columns, sel: torch.Tensor, count: torch.Tensor, *, out_sel: torch.Tensor,
                       out_count: torch.Tensor, workspace: torch.Tensor, max_rows: Optional[int] = None, stream=None):
    """Probe the survivors of an earlier probe again without their count reaching the host
    (rpt_bf_probe_chain_sel_ws): rows sel[0 .. min(count, max_rows)) of every columns[f] through filters[f]; `sel` and
    `count` are what probe_async / probe_chain_ws / transfer_ws left on the device, max_rows the capacity of sel
    (default: its length). out_sel (>= max_rows entries, not overlapping sel), out_count (may be `count` itself) and
    workspace (probe_chain_sel_workspace_bytes(filters, max_rows) bytes) are the caller's. Never reads the count back
    and never synchronizes: returns the device tensors (out_sel, out_count)."""
    lib, device, handles, arr, max_rows, ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                   out_count, workspace)
    check(lib.rpt_bf_probe_chain_sel_ws(handles, arr, len(filters), sel.data_ptr(), count.data_ptr(), max_rows,
                                        out_sel.data_ptr(), out_count.data_ptr(), workspace.data_ptr(), ws_bytes,
                                        _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_sel_ws(filters, columns, dst_filters, dst_columns, sel: torch.Tensor, count: torch.Tensor, *,
                    out_sel: torch.Tensor, out_count: torch.Tensor, workspace: torch.Tensor,
                    max_rows: Optional[int] = None, stream=None):
    """probe_chain_sel_ws, then the survivors inserted into dst_filters[j] on dst_columns[j] (rpt_bf_transfer_sel_ws):
    the backward pass of predicate transfer over a device-resident table. One atomic OR per row. Arguments and result
    as probe_chain_sel_ws; the destination columns are indexed by the same row ids as the probed ones."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, max_rows, ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                   out_count, workspace)
    check(lib.rpt_bf_transfer_sel_ws(handles, arr, len(filters), dst_handles, darr, len(dst_filters), sel.data_ptr(),
                                     count.data_ptr(), max_rows, out_sel.data_ptr(), out_count.data_ptr(),
                                     workspace.data_ptr(), ws_bytes, _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_insert_sel_ws(filters, columns, dst_filters, dst_columns, sel: torch.Tensor, count: torch.Tensor, *,
                           out_sel: torch.Tensor, out_count: torch.Tensor, workspace: torch.Tensor,
                           insert_workspace: Optional[torch.Tensor] = None, max_rows: Optional[int] = None,
                           stream=None):
    """transfer_sel_ws with each destination's insert strategy honoured (rpt_bf_transfer_insert_sel_ws): a destination
    that resolves to RPT_INSERT_PARTITIONED for max_rows takes the routed insert through insert_workspace, the
    caller's buffer of transfer_insert_workspace_bytes(dst_filters, max_rows) bytes (None where no destination
    routes)."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, max_rows, ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                   out_count, workspace)
    iws_bytes = 0 if insert_workspace is None else _nbytes(insert_workspace)
    check(lib.rpt_bf_transfer_insert_sel_ws(handles, arr, len(filters), dst_handles, darr, len(dst_filters),
                                            sel.data_ptr(), count.data_ptr(), max_rows, out_sel.data_ptr(),
                                            out_count.data_ptr(), workspace.data_ptr(), ws_bytes, _ptr(insert_workspace),
                                            iws_bytes, _stream(device, stream)), lib)
    return out_sel, out_count


def probe_chain_sel(filters, columns, sel: torch.Tensor, count: torch.Tensor, *, out_sel: torch.Tensor,
                    out_count: torch.Tensor, max_rows: Optional[int] = None, stream=None):
    """probe_chain_sel_ws for a small batch in one launch with no workspace (rpt_bf_probe_chain_sel): max_rows (default:
    the length of sel) at most RPT_SMALL_PROBE_ROWS. Every filter is gathered from L2 whatever its probe strategy.
    Arguments and result as probe_chain_sel_ws; nothing is allocated, read back or synchronized."""
    lib, device, handles, arr, max_rows, _ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                    out_count)
    check(lib.rpt_bf_probe_chain_sel(handles, arr, len(filters), sel.data_ptr(), count.data_ptr(), max_rows,
                                     out_sel.data_ptr(), out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_sel(filters, columns, dst_filters, dst_columns, sel: torch.Tensor, count: torch.Tensor, *,
                 out_sel: torch.Tensor, out_count: torch.Tensor, max_rows: Optional[int] = None, stream=None):
    """transfer_sel_ws for a small batch in one launch with no workspace (rpt_bf_transfer_sel): the chain over
    sel[0 .. min(count, max_rows)) and the insert of its survivors into every dst_filters[j] on dst_columns[j] in the
    same kernel; a whole backward step of predicate transfer for one vector. max_rows at most RPT_SMALL_PROBE_ROWS.
    Arguments and result as transfer_sel_ws; nothing is allocated, read back or synchronized."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, max_rows, _ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                    out_count)
    check(lib.rpt_bf_transfer_sel(handles, arr, len(filters), dst_handles, darr, len(dst_filters), sel.data_ptr(),
                                  count.data_ptr(), max_rows, out_sel.data_ptr(), out_count.data_ptr(),
                                  _stream(device, stream)), lib)
    return out_sel, out_count


def probe_chain_sel_range_ws(filters, columns, sel: torch.Tensor, count: torch.Tensor, *, range_mask,
                             out_sel: torch.Tensor, out_count: torch.Tensor, workspace: torch.Tensor,
                             max_rows: Optional[int] = None, stream=None):
    """probe_chain_sel_ws restricted to the positions that also lie in the min/max range of every flagged filter on its
    own column (rpt_bf_probe_chain_sel_range_ws). range_mask as in probe_chain_range_ws (0: probe_chain_sel_ws itself);
    the workspace is probe_chain_sel_workspace_bytes(filters, max_rows) bytes whatever the mask. Everything else as
    probe_chain_sel_ws."""
    lib, device, handles, arr, max_rows, ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                   out_count, workspace)
    mask = _range_mask_of(range_mask, len(filters))
    check(lib.rpt_bf_probe_chain_sel_range_ws(handles, arr, len(filters), mask, sel.data_ptr(), count.data_ptr(),
                                              max_rows, out_sel.data_ptr(), out_count.data_ptr(), workspace.data_ptr(),
                                              ws_bytes, _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_sel_range_ws(filters, columns, dst_filters, dst_columns, sel: torch.Tensor, count: torch.Tensor, *,
                          range_mask, out_sel: torch.Tensor, out_count: torch.Tensor, workspace: torch.Tensor,
                          max_rows: Optional[int] = None, stream=None):
    """transfer_sel_ws over the positions that also pass the flagged filters' range tests
    (rpt_bf_transfer_sel_range_ws); range_mask and workspace as in probe_chain_sel_range_ws."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, max_rows, ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                   out_count, workspace)
    mask = _range_mask_of(range_mask, len(filters))
    check(lib.rpt_bf_transfer_sel_range_ws(handles, arr, len(filters), mask, dst_handles, darr, len(dst_filters),
                                           sel.data_ptr(), count.data_ptr(), max_rows, out_sel.data_ptr(),
                                           out_count.data_ptr(), workspace.data_ptr(), ws_bytes,
                                           _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_insert_sel_range_ws(filters, columns, dst_filters, dst_columns, sel: torch.Tensor, count: torch.Tensor, *,
                                 range_mask, out_sel: torch.Tensor, out_count: torch.Tensor, workspace: torch.Tensor,
                                 insert_workspace: Optional[torch.Tensor] = None, max_rows: Optional[int] = None,
                                 stream=None):
    """transfer_insert_sel_ws over the positions that also pass the flagged filters' range tests
    (rpt_bf_transfer_insert_sel_range_ws); range_mask and workspace as in probe_chain_sel_range_ws, the insert
    workspace as in transfer_insert_sel_ws."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, max_rows, ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                   out_count, workspace)
    mask = _range_mask_of(range_mask, len(filters))
    iws_bytes = 0 if insert_workspace is None else _nbytes(insert_workspace)
    check(lib.rpt_bf_transfer_insert_sel_range_ws(handles, arr, len(filters), mask, dst_handles, darr, len(dst_filters),
                                                  sel.data_ptr(), count.data_ptr(), max_rows, out_sel.data_ptr(),
                                                  out_count.data_ptr(), workspace.data_ptr(), ws_bytes,
                                                  _ptr(insert_workspace), iws_bytes, _stream(device, stream)), lib)
    return out_sel, out_count


def probe_chain_sel_range(filters, columns, sel: torch.Tensor, count: torch.Tensor, *, range_mask,
                          out_sel: torch.Tensor, out_count: torch.Tensor, max_rows: Optional[int] = None, stream=None):
    """probe_chain_sel with the flagged filters' range tests, in one launch (rpt_bf_probe_chain_sel_range): a flagged
    filter's keys are loaded once for both tests, and a row outside the range gathers no filter word. range_mask as in
    probe_chain_range_ws (0: probe_chain_sel itself); everything else as probe_chain_sel."""
    lib, device, handles, arr, max_rows, _ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                    out_count)
    mask = _range_mask_of(range_mask, len(filters))
    check(lib.rpt_bf_probe_chain_sel_range(handles, arr, len(filters), mask, sel.data_ptr(), count.data_ptr(), max_rows,
                                           out_sel.data_ptr(), out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_sel_range(filters, columns, dst_filters, dst_columns, sel: torch.Tensor, count: torch.Tensor, *,
                       range_mask, out_sel: torch.Tensor, out_count: torch.Tensor, max_rows: Optional[int] = None,
                       stream=None):
    """transfer_sel with the flagged filters' range tests, in one launch (rpt_bf_transfer_sel_range); range_mask as in
    probe_chain_sel_range, everything else as transfer_sel."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, max_rows, _ws_bytes = _sel_call_args(filters, columns, sel, count, max_rows, out_sel,
                                                                    out_count)
    mask = _range_mask_of(range_mask, len(filters))
    check(lib.rpt_bf_transfer_sel_range(handles, arr, len(filters), mask, dst_handles, darr, len(dst_filters),
                                        sel.data_ptr(), count.data_ptr(), max_rows, out_sel.data_ptr(),
                                        out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel, out_count


def probe_chain_range(filters, columns, *, range_mask, row_sel: Optional[torch.Tensor] = None,
                      n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
                      out_count: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """probe_chain with the flagged filters' range tests, in one launch (rpt_bf_probe_chain_range): the result of
    probe_chain_range_ws for n <= RPT_SMALL_PROBE_ROWS with no workspace. range_mask as in probe_chain_range_ws
    (0: probe_chain itself). Returns out_sel[:count] (reads the count back)."""
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    mask = _range_mask_of(range_mask, len(filters))
    check(lib.rpt_bf_probe_chain_range(handles, arr, len(filters), mask, _ptr(row_sel), n, out_sel.data_ptr(),
                                       out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel[: int(out_count.item())]


def transfer(filters, columns, dst_filters, dst_columns, *, row_sel: Optional[torch.Tensor] = None,
             n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
             out_count: Optional[torch.Tensor] = None, stream=None):
    """transfer_ws for a small batch in one launch with no workspace (rpt_bf_transfer): the chain over rows 0..n-1 or
    row_sel[0..n) and the insert of its survivors into every dst_filters[j] on dst_columns[j] in the same kernel; a
    whole forward step of predicate transfer for one vector. n at most RPT_SMALL_PROBE_ROWS; out_sel must not overlap
    row_sel. Arguments and result as transfer_ws; with the caller's out_sel and out_count nothing is allocated, read
    back or synchronized."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    check(lib.rpt_bf_transfer(handles, arr, len(filters), dst_handles, darr, len(dst_filters), _ptr(row_sel), n,
                              out_sel.data_ptr(), out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_range(filters, columns, dst_filters, dst_columns, *, range_mask, row_sel: Optional[torch.Tensor] = None,
                   n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
                   out_count: Optional[torch.Tensor] = None, stream=None):
    """transfer with the flagged filters' range tests, in one launch (rpt_bf_transfer_range); range_mask as in
    probe_chain_range_ws (0: transfer itself), everything else as transfer."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    lib, device, handles, arr, n, out_sel, out_count = _probed_call_args(filters, columns, row_sel, n, out_sel, out_count)
    mask = _range_mask_of(range_mask, len(filters))
    check(lib.rpt_bf_transfer_range(handles, arr, len(filters), mask, dst_handles, darr, len(dst_filters),
                                    _ptr(row_sel), n, out_sel.data_ptr(), out_count.data_ptr(),
                                    _stream(device, stream)), lib)
    return out_sel, out_count


def insert_multi(dst_filters, dst_columns, *, row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                 stream=None) -> None:
    """The sink of one vector into one filter per build column, in one launch (rpt_bf_insert_multi): rows 0..n-1, or
    row_sel[0..n), of every dst_columns[j] into dst_filters[j], as one insert per destination would leave them. n
    (default: the length of row_sel, else of the first column) at most RPT_SMALL_PROBE_ROWS, 1..RPT_MAX_CHAIN
    destinations. Columns as in probe_chain."""
    dst_handles, darr = _dst_call_args(dst_filters, dst_columns)
    n = _row_list_rows(dst_columns, row_sel, n)
    lib, device = dst_filters[0]._lib, dst_filters[0].device
    check(lib.rpt_bf_insert_multi(dst_handles, darr, len(dst_filters), _ptr(row_sel), n, _stream(device, stream)), lib)


def _column_rows(c) -> int:
    c = c if isinstance(c, dict) else {"keys": c}
    return c["key_sel"].numel() if c.get("key_sel") is not None else c["keys"].numel()


def composite_key(columns: Sequence) -> CompositeKey:
    """rpt_composite_key of one key's columns: device key tensors, or dicts of make_column's arguments (keys, key_type,
    key_sel, validity), the shape hash_columns accepts. The returned structure keeps its column array alive (the
    tensors stay the caller's to keep)."""
    if not columns:
        raise RptError(1, "a composite key needs at least one column")
    arr = (KeyColumn * len(columns))(*[make_column(**c) if isinstance(c, dict) else make_column(c) for c in columns])
    key = CompositeKey(arr, len(columns))
    key._columns = arr
    return key


def _composite_list_args(filters, keys, message: str):
    """(handle array, rpt_composite_key array) of a filter list and one list of columns per filter."""
    _check_lists(filters, keys, message)
    built = [composite_key(k) for k in keys]
    arr = (CompositeKey * len(built))(*built)
    arr._keys = built  # the column arrays the structures point to
    return (ctypes.c_void_p * len(filters))(*[f._h for f in filters]), arr


def probe_chain_composite(filters, keys, *, row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                          out_sel: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None,
                          stream=None):
    """probe_chain with a composite key per filter, hashed in the kernel (rpt_bf_probe_chain_composite): keys[i] is the
    list of filters[i]'s key columns (tensors or make_column dicts, 1..RPT_MAX_KEY_COLUMNS, at most
    RPT_MAX_CHAIN_KEY_COLUMNS over the call). Returns (out_sel, out_count); with the caller's buffers nothing is
    allocated, read back or synchronized."""
    handles, arr = _composite_list_args(filters, keys, "one key per filter, at least one filter")
    n = _row_list_rows(keys[0], row_sel, n)
    lib, device = filters[0]._lib, filters[0].device
    if out_sel is None:
        out_sel = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    if out_count is None:
        out_count = torch.zeros(1, dtype=torch.int64, device=device)
    check(lib.rpt_bf_probe_chain_composite(handles, arr, len(filters), _ptr(row_sel), n, out_sel.data_ptr(),
                                           out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel, out_count


def transfer_composite(filters, keys, dst_filters, dst_keys, *, row_sel: Optional[torch.Tensor] = None,
                       n: Optional[int] = None, out_sel: Optional[torch.Tensor] = None,
                       out_count: Optional[torch.Tensor] = None, stream=None):
    """transfer with a composite key per probed filter and per destination (rpt_bf_transfer_composite); a destination
    key of two or more columns folds no min/max. Arguments as probe_chain_composite, result as transfer."""
    dst_handles, darr = _composite_list_args(dst_filters, dst_keys, "one key per destination filter, at least one destination")
    handles, arr = _composite_list_args(filters, keys, "one key per filter, at least one filter")
    n = _row_list_rows(keys[0], row_sel, n)
    lib, device = filters[0]._lib, filters[0].device
    if out_sel is None:
        out_sel = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    if out_count is None:
        out_count = torch.zeros(1, dtype=torch.int64, device=device)
    check(lib.rpt_bf_transfer_composite(handles, arr, len(filters), dst_handles, darr, len(dst_filters), _ptr(row_sel), n,
                                        out_sel.data_ptr(), out_count.data_ptr(), _stream(device, stream)), lib)
    return out_sel, out_count


def insert_multi_composite(dst_filters, dst_keys, *, row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                           stream=None) -> None:
    """insert_multi with a composite key per destination (rpt_bf_insert_multi_composite)."""
    dst_handles, darr = _composite_list_args(dst_filters, dst_keys, "one key per destination filter, at least one destination")
    n = _row_list_rows(dst_keys[0], row_sel, n)
    lib, device = dst_filters[0]._lib, dst_filters[0].device
    check(lib.rpt_bf_insert_multi_composite(dst_handles, darr, len(dst_filters), _ptr(row_sel), n,
                                            _stream(device, stream)), lib)


def make_column(keys: torch.Tensor, key_type: Optional[int] = None, key_sel: Optional[torch.Tensor] = None,
                validity: Optional[torch.Tensor] = None) -> KeyColumn:
    """rpt_key_column for a FLAT (key_sel None) or DICTIONARY (key_sel uint32/int32) key vector."""
    if not keys.is_cuda:
        raise RptError(1, "keys must be a device tensor")
    if not keys.is_contiguous():
        raise RptError(1, "keys must be contiguous")
    for name, t in (("key_sel", key_sel), ("validity", validity)):
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.device != keys.device):
            raise RptError(1, f"{name} must be a contiguous tensor on {keys.device}")
    if key_sel is not None and key_sel.element_size() != 4:
        raise RptError(1, "key_sel must be 32-bit")
    if validity is not None and validity.element_size() != 8:
        raise RptError(1, "validity must be 64-bit words")
    return KeyColumn(key_type_of(keys, key_type), keys.data_ptr(), _ptr(key_sel), _ptr(validity))


def validity_from_mask(valid: torch.Tensor) -> torch.Tensor:
    """Pack a bool row mask into DuckDB ValidityMask words (bit i%64 of word i/64 = row i valid)."""
    n = valid.numel()
    nw = (n + 63) // 64
    v = torch.zeros(nw * 64, dtype=torch.int64, device=valid.device)
    v[:n] = valid.to(torch.int64)
    v = v.view(nw, 64)
    shifts = torch.arange(64, device=valid.device, dtype=torch.int64)
    # bit 63 wraps to the sign bit of int64 (two's complement), which is what the device reads.
    return (v << shifts).sum(dim=1, dtype=torch.int64)


class ProbeWorkspace:
    """Device workspace reused across probes (grown on demand)."""

    def __init__(self, device: torch.device):
        self.device = device
        self.buf: Optional[torch.Tensor] = None

    def get_bytes(self, need: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < need:
            self.buf = None  # release before growing
            self.buf = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return self.buf

    def get(self, n: int, log_num_blocks: int) -> torch.Tensor:
        """Enough for any strategy on a 2^log_num_blocks-block filter."""
        return self.get_bytes(int(load().rpt_probe_workspace_bytes(n, log_num_blocks)))


class BloomFilter:
    """A device-resident blocked Bloom filter (PTBloomFilter)."""

    def __init__(self, est_num_rows: Optional[int] = None, *, log_num_blocks: Optional[int] = None,
                 device=None, lib=None):
        lib = lib if lib is not None else load()  # lib: a build bound by _lib.load_variant (tests)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RptError(1, "BloomFilter lives on a GPU device")
        h = ctypes.c_void_p()
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if log_num_blocks is not None:
            check(lib.rpt_bf_create_log_blocks(dev, int(log_num_blocks), ctypes.byref(h)))
        else:
            check(lib.rpt_bf_create(dev, int(est_num_rows or 0), ctypes.byref(h)))
        self._h = h
        self._lib = lib
        self._ws = ProbeWorkspace(self.device)
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)

    # ---- lifecycle -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.rpt_bf_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def info(self) -> BfInfo:
        i = BfInfo()
        check(self._lib.rpt_bf_get_info(self._h, ctypes.byref(i)))
        return i

    @property
    def log_num_blocks(self) -> int:
        return self.info().log_num_blocks

    @property
    def num_blocks(self) -> int:
        return self.info().num_blocks

    def sized_for_rows(self) -> int:
        return self.info().sized_for_rows

    def is_empty(self) -> bool:
        return not self.info().has_data

    @property
    def finalized(self) -> bool:
        return bool(self.info().finalized)

    @finalized.setter
    def finalized(self, v: bool) -> None:
        check(self._lib.rpt_bf_set_finalized(self._h, int(bool(v))))

    @property
    def probe_strategy(self) -> int:
        """The strategy a probe runs now (RPT_PROBE_*; AUTO resolved by filter size)."""
        v = self._lib.rpt_bf_probe_strategy(self._h)
        if v < 0:
            check(-v)
        return v

    @probe_strategy.setter
    def probe_strategy(self, strategy: int) -> None:
        check(self._lib.rpt_bf_set_probe_strategy(self._h, int(strategy)))

    def workspace_bytes(self, n: int) -> int:
        """Probe workspace for n rows with the strategy this filter would run (AUTO resolved with n)."""
        return int(self._lib.rpt_bf_probe_workspace_bytes(self._h, n))

    def probe_strategy_for(self, n: int) -> int:
        v = self._lib.rpt_bf_probe_strategy_for(self._h, n)
        if v < 0:
            check(-v)
        return v

    def probe_sel_strategy_for(self, max_rows: int) -> int:
        """The strategy this filter runs in a device-counted chain (rpt_bf_probe_sel_strategy_for): probe_strategy_for
        with PARTITIONED and BUCKETED replaced by GATHER."""
        v = self._lib.rpt_bf_probe_sel_strategy_for(self._h, int(max_rows))
        if v < 0:
            check(-v)
        return v

    def insert_strategy_for(self, n: int) -> int:
        v = self._lib.rpt_bf_insert_strategy_for(self._h, n)
        if v < 0:
            check(-v)
        return v

    def needs_resize(self, actual_rows: int) -> bool:
        """CREATE_BF Finalize's resize predicate on this filter's real allocation: fewer than 8 allocated
        bits per actual row (physical_create_bf.cpp:383; rpt_bf_needs_resize_alloc)."""
        v = self._lib.rpt_bf_needs_resize_alloc(self._h, int(actual_rows))
        if v < 0:
            check(-v)
        return bool(v)

    def set_has_data(self, v: bool) -> None:
        check(self._lib.rpt_bf_set_has_data(self._h, int(bool(v))))

    # ---- build -----------------------------------------------------------------------------
    def insert(self, keys: torch.Tensor, *, key_type: Optional[int] = None, key_sel=None, validity=None,
               n: Optional[int] = None, stream=None, strategy: Optional[int] = None) -> None:
        """PTBloomFilter::Insert. Large batches use the partitioned / bucketed insert (workspace
        allocated here) unless strategy=RPT_INSERT_ATOMIC; results are identical."""
        n = keys.numel() if (n is None and key_sel is None) else (key_sel.numel() if n is None else n)
        col = make_column(keys, key_type, key_sel, validity)
        if strategy is not None:
            check(self._lib.rpt_bf_set_insert_strategy(self._h, int(strategy)))
        ws_bytes = int(self._lib.rpt_bf_insert_workspace_bytes(self._h, n))  # 0: atomic insert
        if ws_bytes:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            if isinstance(stream, torch.cuda.Stream):
                ws.record_stream(stream)  # freed below while the insert may still run on `stream`
            check(self._lib.rpt_bf_insert_ws(self._h, ctypes.byref(col), n, ws.data_ptr(), ws_bytes,
                                             _stream(self.device, stream)))
        else:
            check(self._lib.rpt_bf_insert(self._h, ctypes.byref(col), n, _stream(self.device, stream)))

    def insert_composite(self, columns: Sequence, *, n: Optional[int] = None, stream=None) -> None:
        """Insert rows 0..n-1 (default: the first column's length) of a composite key, hashed in the insert kernel
        (rpt_bf_insert_composite): one atomic OR per row, no min/max for two or more columns. Columns as in
        hash_columns."""
        n = _column_rows(columns[0]) if n is None else int(n)
        key = composite_key(columns)
        check(self._lib.rpt_bf_insert_composite(self._h, ctypes.byref(key), n, _stream(self.device, stream)), self._lib)

    def insert_bits(self, keys: torch.Tensor, bits: torch.Tensor, *, n: Optional[int] = None,
                    row_sel: Optional[torch.Tensor] = None, key_type: Optional[int] = None, key_sel=None,
                    validity=None, stream=None) -> None:
        """Insert the rows i < n (row i, or row_sel[i]) whose bit i is set in `bits` (rpt_bf_insert_bits): 64-bit
        device words in the layout of rpt_bf_probe_bits, ceil(n / 512) * 8 of them; bits past n are ignored.
        Stream-ordered, nothing is read back; is_empty() is False afterwards whatever the bits held."""
        if n is None:
            n = row_sel.numel() if row_sel is not None else (key_sel.numel() if key_sel is not None else keys.numel())
        col = make_column(keys, key_type, key_sel, validity)
        if row_sel is not None and (row_sel.element_size() != 4 or not row_sel.is_cuda):
            raise RptError(1, "row_sel must be a 32-bit device tensor")
        need = ((n + SEG_ROWS - 1) // SEG_ROWS) * (SEG_ROWS // 64)
        if not bits.is_cuda or not bits.is_contiguous() or bits.element_size() != 8 or bits.numel() < need:
            raise RptError(1, f"bits must be a contiguous device tensor of at least {need} 64-bit words")
        check(self._lib.rpt_bf_insert_bits(self._h, ctypes.byref(col), _ptr(row_sel), n, bits.data_ptr(),
                                           _stream(self.device, stream)), self._lib)

    def insert_sel(self, keys: torch.Tensor, sel: torch.Tensor, count: torch.Tensor, *,
                   max_rows: Optional[int] = None, key_type: Optional[int] = None, key_sel=None, validity=None,
                   stream=None) -> None:
        """Insert rows sel[0 .. min(count, max_rows)) (rpt_bf_insert_sel): `sel` a 32-bit device tensor of row ids,
        `count` a one-element 64-bit device tensor read when the kernel runs (what probe_async returns), max_rows
        the capacity of sel (default: its length). Stream-ordered, nothing is read back; is_empty() is False
        afterwards whatever the count held."""
        col = make_column(keys, key_type, key_sel, validity)
        if not sel.is_cuda or not sel.is_contiguous() or sel.element_size() != 4:
            raise RptError(1, "sel must be a contiguous 32-bit device tensor")
        if not count.is_cuda or count.element_size() != 8 or count.numel() < 1:
            raise RptError(1, "count must be a 64-bit device tensor")
        max_rows = sel.numel() if max_rows is None else int(max_rows)
        if max_rows > sel.numel():
            raise RptError(1, f"max_rows={max_rows} exceeds the {sel.numel()} entries of sel")
        check(self._lib.rpt_bf_insert_sel(self._h, ctypes.byref(col), sel.data_ptr(), count.data_ptr(), max_rows,
                                          _stream(self.device, stream)), self._lib)

    def _insert_workspace(self, n: int, workspace: Optional[torch.Tensor], stream):
        """(pointer, bytes) of the workspace a routed device-side insert of n rows gets: the caller's, or one of
        rpt_bf_insert_workspace_bytes(n) bytes allocated here (none when the strategy for n does not route)."""
        if workspace is None:
            need = int(self._lib.rpt_bf_insert_workspace_bytes(self._h, n))
            if not need:
                return None, 0
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            if isinstance(stream, torch.cuda.Stream):
                workspace.record_stream(stream)  # freed on return while the insert may still run on `stream`
        return workspace.data_ptr(), workspace.numel() * workspace.element_size()

    def insert_bits_ws(self, keys: torch.Tensor, bits: torch.Tensor, *, n: Optional[int] = None,
                       row_sel: Optional[torch.Tensor] = None, key_type: Optional[int] = None, key_sel=None,
                       validity=None, workspace: Optional[torch.Tensor] = None, stream=None,
                       strategy: Optional[int] = None) -> None:
        """insert_bits with the filter's insert strategy honoured (rpt_bf_insert_bits_ws): where it resolves to
        RPT_INSERT_PARTITIONED for n rows, the selected rows are partitioned by filter slice and merged through
        LDS instead of one atomic OR per row; the result is identical. `workspace`: device bytes of
        rpt_bf_insert_workspace_bytes(n) (allocated here when None); strategy: as insert()."""
        if n is None:
            n = row_sel.numel() if row_sel is not None else (key_sel.numel() if key_sel is not None else keys.numel())
        col = make_column(keys, key_type, key_sel, validity)
        if row_sel is not None and (row_sel.element_size() != 4 or not row_sel.is_cuda):
            raise RptError(1, "row_sel must be a 32-bit device tensor")
        need = ((n + SEG_ROWS - 1) // SEG_ROWS) * (SEG_ROWS // 64)
        if not bits.is_cuda or not bits.is_contiguous() or bits.element_size() != 8 or bits.numel() < need:
            raise RptError(1, f"bits must be a contiguous device tensor of at least {need} 64-bit words")
        if strategy is not None:
            check(self._lib.rpt_bf_set_insert_strategy(self._h, int(strategy)))
        ws_ptr, ws_bytes = self._insert_workspace(n, workspace, stream)
        check(self._lib.rpt_bf_insert_bits_ws(self._h, ctypes.byref(col), _ptr(row_sel), n, bits.data_ptr(), ws_ptr,
                                              ws_bytes, _stream(self.device, stream)), self._lib)

    def insert_sel_ws(self, keys: torch.Tensor, sel: torch.Tensor, count: torch.Tensor, *,
                      max_rows: Optional[int] = None, key_type: Optional[int] = None, key_sel=None, validity=None,
                      workspace: Optional[torch.Tensor] = None, stream=None, strategy: Optional[int] = None) -> None:
        """insert_sel with the filter's insert strategy honoured (rpt_bf_insert_sel_ws), resolved with max_rows:
        the count stays on the device. `workspace`: device bytes of rpt_bf_insert_workspace_bytes(max_rows)
        (allocated here when None); strategy: as insert()."""
        col = make_column(keys, key_type, key_sel, validity)
        if not sel.is_cuda or not sel.is_contiguous() or sel.element_size() != 4:
            raise RptError(1, "sel must be a contiguous 32-bit device tensor")
        if not count.is_cuda or count.element_size() != 8 or count.numel() < 1:
            raise RptError(1, "count must be a 64-bit device tensor")
        max_rows = sel.numel() if max_rows is None else int(max_rows)
        if max_rows > sel.numel():
            raise RptError(1, f"max_rows={max_rows} exceeds the {sel.numel()} entries of sel")
        if strategy is not None:
            check(self._lib.rpt_bf_set_insert_strategy(self._h, int(strategy)))
        ws_ptr, ws_bytes = self._insert_workspace(max_rows, workspace, stream)
        check(self._lib.rpt_bf_insert_sel_ws(self._h, ctypes.byref(col), sel.data_ptr(), count.data_ptr(), max_rows,
                                             ws_ptr, ws_bytes, _stream(self.device, stream)), self._lib)

    def reinitialize(self, actual_rows: int) -> None:
        check(self._lib.rpt_bf_reinitialize(self._h, int(actual_rows)))

    def reinitialize_and_rehash(self, actual_rows: int, chunks: Iterable[dict]) -> None:
        """PTBloomFilter::ReinitializeAndRehash (bloom_filter.cpp:34-58): reallocate for
        actual_rows, then re-insert every materialized chunk (dicts of insert() kwargs)."""
        self.reinitialize(actual_rows)
        for ch in chunks:
            ch = dict(ch)
            self.insert(ch.pop("keys"), **ch)

    def clear(self, stream=None) -> None:
        check(self._lib.rpt_bf_clear(self._h, _stream(self.device, stream)))

    def settle(self, stream=None) -> None:
        """Settle a deferred clear now (rpt_bf_settle; before a stream capture reads the filter)."""
        check(self._lib.rpt_bf_settle(self._h, _stream(self.device, stream)))

    def minmax(self, stream=None) -> Optional[tuple[int, int]]:
        """(min, max) of the valid I32/I64 keys inserted so far, or None (the CREATE_BF min/max
        dynamic filter, physical_create_bf.cpp:82-176, computed inside the insert kernels)."""
        mn, mx, has = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        check(self._lib.rpt_bf_get_minmax(self._h, ctypes.byref(mn), ctypes.byref(mx), ctypes.byref(has),
                                          _stream(self.device, stream)))
        return (mn.value, mx.value) if has.value else None

    def set_minmax(self, value: Optional[tuple[int, int]], stream=None) -> None:
        mn, mx = value if value is not None else (0, 0)
        check(self._lib.rpt_bf_set_minmax(self._h, int(mn), int(mx), int(value is not None),
                                          _stream(self.device, stream)))

    # ---- probe -----------------------------------------------------------------------------
    def probe_async(self, keys: torch.Tensor, *, key_type: Optional[int] = None, key_sel=None, validity=None,
                    row_sel: Optional[torch.Tensor] = None, n: Optional[int] = None,
                    out_sel: Optional[torch.Tensor] = None, out_count: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None, stream=None):
        """Enqueue a probe; returns (out_sel, out_count) device tensors (count not synchronized)."""
        if n is None:
            n = row_sel.numel() if row_sel is not None else (key_sel.numel() if key_sel is not None else keys.numel())
        col = make_column(keys, key_type, key_sel, validity)
        if row_sel is not None and (row_sel.element_size() != 4 or not row_sel.is_cuda):
            raise RptError(1, "row_sel must be a 32-bit device tensor")
        if out_sel is None:
            out_sel = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        if out_count is None:
            out_count = self._count
        ws = workspace if workspace is not None else self._ws.get_bytes(self.workspace_bytes(n))
        if workspace is None and isinstance(stream, torch.cuda.Stream):
            ws.record_stream(stream)  # the filter's workspace may be regrown (freed) while this probe runs
        check(self._lib.rpt_bf_probe(self._h, ctypes.byref(col), _ptr(row_sel), n, out_sel.data_ptr(),
                                     out_count.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                                     _stream(self.device, stream)))
        return out_sel, out_count

    def probe_phase1(self, keys: torch.Tensor, workspace: torch.Tensor, *, n: Optional[int] = None,
                     key_type: Optional[int] = None, key_sel=None, validity=None, row_sel=None, stream=None) -> None:
        """Hash + gather + result bits (rpt_bf_probe_phase1)."""
        if n is None:
            n = row_sel.numel() if row_sel is not None else (key_sel.numel() if key_sel is not None else keys.numel())
        col = make_column(keys, key_type, key_sel, validity)
        check(self._lib.rpt_bf_probe_phase1(self._h, ctypes.byref(col), _ptr(row_sel), n, workspace.data_ptr(),
                                            workspace.numel() * workspace.element_size(),
                                            _stream(self.device, stream)))

    def probe_phase2(self, n: int, out_sel: torch.Tensor, out_count: torch.Tensor, workspace: torch.Tensor, *,
                     row_sel=None, stream=None) -> None:
        """Selection-vector expansion (rpt_bf_probe_phase2)."""
        check(self._lib.rpt_bf_probe_phase2(self._h, _ptr(row_sel), n, out_sel.data_ptr(), out_count.data_ptr(),
                                            workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                            _stream(self.device, stream)))

    def lookup_sel(self, keys: torch.Tensor, **kw) -> torch.Tensor:
        """LookupSel: ascending ids (int32 tensor) of the rows that may match."""
        sel, cnt = self.probe_async(keys, **kw)
        c = int(cnt.item())
        return sel[:c]

    def find_bits(self, keys: torch.Tensor, *, key_type: Optional[int] = None, key_sel=None, validity=None,
                  n: Optional[int] = None, stream=None) -> torch.Tensor:
        """Arrow Find(...) bit vector as int64 words (bit i of the LSB-first stream = row i)."""
        if n is None:
            n = key_sel.numel() if key_sel is not None else keys.numel()
        nw = ((n + SEG_ROWS - 1) // SEG_ROWS) * (SEG_ROWS // 64)
        out = torch.zeros(max(nw, 1), dtype=torch.int64, device=self.device)
        col = make_column(keys, key_type, key_sel, validity)
        check(self._lib.rpt_bf_find_bits(self._h, ctypes.byref(col), n, out.data_ptr(),
                                         _stream(self.device, stream)))
        return out

    def range_bits(self, keys: torch.Tensor, *, n: Optional[int] = None, row_sel: Optional[torch.Tensor] = None,
                   key_type: Optional[int] = None, key_sel=None, validity=None, out: Optional[torch.Tensor] = None,
                   stream=None) -> torch.Tensor:
        """The filter's min/max range test alone (rpt_bf_range_bits): bit i of the returned int64 words (the layout
        of rpt_bf_probe_bits, ceil(n / 512) * 8 words) is set iff row i (or row_sel[i]) is not NULL and lies in
        [min, max]; a filter without a value passes every row. The range is read on the device when the kernel runs.
        `out`: a contiguous 64-bit device tensor of at least that many words (allocated here when None)."""
        if n is None:
            n = row_sel.numel() if row_sel is not None else (key_sel.numel() if key_sel is not None else keys.numel())
        col = make_column(keys, key_type, key_sel, validity)
        if row_sel is not None and (row_sel.element_size() != 4 or not row_sel.is_cuda):
            raise RptError(1, "row_sel must be a 32-bit device tensor")
        need = ((n + SEG_ROWS - 1) // SEG_ROWS) * (SEG_ROWS // 64)
        if out is None:
            out = torch.empty(max(need, 1), dtype=torch.int64, device=self.device)
        elif not out.is_cuda or not out.is_contiguous() or out.element_size() != 8 or out.numel() < need:
            raise RptError(1, f"out must be a contiguous device tensor of at least {need} 64-bit words")
        check(self._lib.rpt_bf_range_bits(self._h, ctypes.byref(col), _ptr(row_sel), n, out.data_ptr(),
                                          _stream(self.device, stream)), self._lib)
        return out

    # ---- merge / fold / export -------------------------------------------------------------
    def merge_or(self, other: "BloomFilter", stream=None) -> None:
        check(self._lib.rpt_bf_merge_or(self._h, other._h, _stream(self.device, stream)))

    def count_bits(self) -> int:
        v = ctypes.c_uint64()
        check(self._lib.rpt_bf_count_bits(self._h, ctypes.byref(v)))
        return v.value

    def is_same_as(self, other: "BloomFilter") -> bool:
        """BlockedBloomFilter::IsSameAs on the device (rpt_bf_is_same_as): same geometry, every word equal."""
        same, diff = ctypes.c_int(), ctypes.c_uint64()
        check(self._lib.rpt_bf_is_same_as(self._h, other._h, ctypes.byref(same), ctypes.byref(diff)))
        return bool(same.value)

    def diff_words(self, other: "BloomFilter") -> int:
        """Number of words that differ from `other` (rpt_bf_is_same_as; 2^64 - 1 for different geometry)."""
        same, diff = ctypes.c_int(), ctypes.c_uint64()
        check(self._lib.rpt_bf_is_same_as(self._h, other._h, ctypes.byref(same), ctypes.byref(diff)))
        return diff.value

    def fold(self) -> int:
        v = ctypes.c_int()
        check(self._lib.rpt_bf_fold(self._h, ctypes.byref(v)))
        return v.value

    def export_words(self) -> np.ndarray:
        nw = self.num_blocks
        out = np.zeros(nw, dtype=np.uint64)
        check(self._lib.rpt_bf_export_words(self._h, out.ctypes.data, nw))
        return out

    def import_words(self, words: np.ndarray) -> None:
        w = np.ascontiguousarray(words, dtype=np.uint64)
        check(self._lib.rpt_bf_import_words(self._h, w.ctypes.data, w.size))

    def copy_words_to(self, dst: torch.Tensor, stream=None) -> None:
        check(self._lib.rpt_bf_copy_words_to(self._h, dst.data_ptr(), self.num_blocks, _stream(self.device, stream)))

    def copy_words_from(self, src: torch.Tensor, stream=None) -> None:
        check(self._lib.rpt_bf_copy_words_from(self._h, src.data_ptr(), self.num_blocks,
                                               _stream(self.device, stream)))


def hash_keys(keys: torch.Tensor, *, key_type: Optional[int] = None, key_sel=None, validity=None,
              stream=None) -> torch.Tensor:
    n = key_sel.numel() if key_sel is not None else keys.numel()
    out = torch.empty(max(n, 1), dtype=torch.int64, device=keys.device)
    col = make_column(keys, key_type, key_sel, validity)
    check(load().rpt_hash_keys(ctypes.byref(col), n, out.data_ptr(), _stream(keys.device, stream)))
    return out[:n]


def hash_columns(columns: Sequence, stream=None) -> torch.Tensor:
    """HashColumns (reference src/bloom_filter.cpp:11-24) for one or more key columns: Hash(col_0),
    then CombineHash with col_1, col_2, ... on the device. Each column is a tensor or a dict of
    make_column kwargs (keys=, key_type=, key_sel=, validity=). Insert / probe the result with
    key_type=RPT_KEY_HASH."""
    cols = [c if isinstance(c, dict) else {"keys": c} for c in columns]
    if not cols:
        raise RptError(1, "hash_columns needs at least one column")
    first = cols[0]
    out = hash_keys(first["keys"], key_type=first.get("key_type"), key_sel=first.get("key_sel"),
                    validity=first.get("validity"), stream=stream)
    n = out.numel()
    for c in cols[1:]:
        cn = c["key_sel"].numel() if c.get("key_sel") is not None else c["keys"].numel()
        if cn != n:
            raise RptError(1, f"composite key columns differ in length ({cn} vs {n})")
        col = make_column(c["keys"], c.get("key_type"), c.get("key_sel"), c.get("validity"))
        check(load().rpt_hash_combine(ctypes.byref(col), n, out.data_ptr(), _stream(out.device, stream)))
    return out


def hash_columns_fused(columns: Sequence, stream=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hash_columns in one launch (rpt_hash_keys_composite): every column is read once and the combined hash written
    once. Bit-identical to hash_columns; at most RPT_MAX_KEY_COLUMNS columns, a HASH column only first. `out`: the
    caller's int64 buffer of at least n entries."""
    if not columns:
        raise RptError(1, "hash_columns_fused needs at least one column")
    n = _column_rows(columns[0])
    for c in columns[1:]:
        if _column_rows(c) != n:
            raise RptError(1, f"composite key columns differ in length ({_column_rows(c)} vs {n})")
    key = composite_key(columns)
    device = (columns[0]["keys"] if isinstance(columns[0], dict) else columns[0]).device
    if out is None:
        out = torch.empty(max(n, 1), dtype=torch.int64, device=device)
    check(load().rpt_hash_keys_composite(ctypes.byref(key), n, out.data_ptr(), _stream(device, stream)))
    return out[:n]


def words_or_slices(dst: torch.Tensor, srcs: torch.Tensor, k: int, n_words: int, stream=None) -> None:
    """dst[:n_words] = OR of k consecutive n_words slices of srcs (device tensors, 64-bit)."""
    check(load().rpt_words_or_slices(dst.data_ptr(), srcs.data_ptr(), int(k), int(n_words),
                                     _stream(dst.device, stream)))


def synth_build_keys(n: int, start: int = 0, device=None, out: Optional[torch.Tensor] = None,
                     stream=None) -> torch.Tensor:
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if out is None else out
    check(load().rpt_synth_build_keys(out.data_ptr(), start, n, _stream(dev, stream)))
    return out[:n]


def synth_probe_keys(n: int, n_build: int, p_permille: int = 100, start: int = 0, device=None,
                     out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if out is None else out
    check(load().rpt_synth_probe_keys(out.data_ptr(), n_build, p_permille, start, n, _stream(dev, stream)))
    return out[:n]


def log_num_blocks_for_rows(n: int) -> int:
    return int(load().rpt_bf_log_num_blocks_for_rows(n))


def needs_resize(sized_for_rows: int, actual_rows: int) -> bool:
    return bool(load().rpt_bf_needs_resize(sized_for_rows, actual_rows))


__all__: Sequence[str] = [
    "BloomFilter",
    "ProbeWorkspace",
    "make_column",
    "transfer_ws",
    "probe_chain_sel_workspace_bytes",
    "probe_chain_sel_ws",
    "transfer_sel_ws",
    "transfer_insert_sel_ws",
    "validity_from_mask",
    "hash_keys",
    "hash_columns",
    "words_or_slices",
    "synth_build_keys",
    "synth_probe_keys",
    "log_num_blocks_for_rows",
    "needs_resize",
]
