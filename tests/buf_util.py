"""Helpers of the GPU tests that check what the library does with caller buffers (imported as a plain
module; not a conftest):

  GuardedBuffer   an exactly sized device buffer between two guard bands, with poison patterns for its payload
  hip_graph_api / stream_capture / graph_instantiate / graph_launch / graph_destroy
                  the HIP stream-capture calls torch does not expose for a caller-owned stream (ctypes)
  FilterCache     one (BloomFilter, oracle words, build keys) triple per log_num_blocks, built once

torch rounds every allocation up, so a kernel that writes a few vector widths past an output or a workspace
lands in slack nobody looks at. A GuardedBuffer puts the payload at its exact size inside one larger
allocation, guard bytes directly behind its last byte (and in front of its first), and compares the guards
on the device afterwards."""
from __future__ import annotations

import ctypes
import gc

import numpy as np
import torch

import rpt_oracle as orc

GUARD_BYTE = 0xC3
GUARD_BYTES = 64 << 10

# Poison patterns (GuardedBuffer.poison): names, or (name, value) for the two valued uint32 patterns
FF, A5, RAMP = "ff", "a5", "ramp"


def const32(v: int):
    """Every uint32 word = v."""
    return ("const", v & 0xFFFFFFFF)


def alt32(v: int):
    """uint32 words v, ~v, v, ~v, ..."""
    return ("alt", v & 0xFFFFFFFF)


def pattern_id(p) -> str:
    return p if isinstance(p, str) else f"{p[0]}{p[1]:08x}"


def _as_i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def fill_bytes(t: torch.Tensor, pattern) -> None:
    """Fill the uint8 tensor t (4-byte aligned start) with a poison pattern; a tail of fewer than 4 bytes
    gets the pattern's low bytes."""
    assert t.dtype == torch.uint8 and t.is_contiguous()
    n = t.numel()
    if n == 0:
        return
    if pattern == FF:
        t.fill_(0xFF)
        return
    if pattern == A5:
        t.fill_(0xA5)
        return
    nw = n // 4
    words = t[: nw * 4].view(torch.int32)
    if pattern == RAMP:
        if nw:
            words.copy_(torch.arange(nw, device=t.device, dtype=torch.int64).to(torch.int32))
        tail = nw
    else:
        kind, v = pattern
        assert kind in ("const", "alt"), pattern
        words.fill_(_as_i32(v))
        if kind == "alt" and nw > 1:
            words[1::2] = _as_i32(~v)
        tail = v if (kind == "const" or nw % 2 == 0) else ~v
    for i in range(nw * 4, n):
        t[i] = (tail >> (8 * (i - nw * 4))) & 0xFF


class GuardedBuffer:
    """`nbytes` of device memory at a 256-B-aligned address inside one allocation: guard | payload | guard.
    The back guard starts at the byte after the payload, so a one-byte overrun is seen."""

    def __init__(self, nbytes: int, device="cuda:0", guard: int = GUARD_BYTES):
        self.nbytes, self.guard = int(nbytes), int(guard)
        self._raw = torch.empty(self.guard + 256 + self.nbytes + self.guard, dtype=torch.uint8, device=device)
        base = self._raw.data_ptr()
        self._off = ((base + self.guard + 255) & ~255) - base  # front guard: [_off - guard, _off)
        self._front = self._raw[self._off - self.guard: self._off]
        self._back = self._raw[self._off + self.nbytes: self._off + self.nbytes + self.guard]
        self._raw.fill_(GUARD_BYTE)
        assert self.ptr % 256 == 0

    @property
    def ptr(self) -> int:
        return self._raw.data_ptr() + self._off

    def bytes(self) -> torch.Tensor:
        return self._raw[self._off: self._off + self.nbytes]

    def view(self, dtype: torch.dtype) -> torch.Tensor:
        """The payload as a tensor of `dtype` (its size must divide the payload)."""
        return self.bytes().view(dtype)

    def poison(self, pattern) -> "GuardedBuffer":
        fill_bytes(self.bytes(), pattern)
        return self

    def assert_guards_intact(self, what: str = "buffer") -> None:
        for name, g, origin in (("front", self._front, -self.guard), ("back", self._back, self.nbytes)):
            bad = g != GUARD_BYTE
            if bool(bad.any()):
                first = int(bad.nonzero()[0])
                raise AssertionError(
                    f"{what}: {name} guard damaged, first at payload offset {origin + first} "
                    f"(payload is {self.nbytes} bytes), {int(bad.sum())} guard bytes changed")


# ---- HIP graphs over a caller-owned stream ---------------------------------------------------------
CAPTURE_MODE_GLOBAL, CAPTURE_MODE_RELAXED = 0, 2  # hipStreamCaptureModeGlobal (torch's default), ...Relaxed

_hip = None


def hip_graph_api() -> ctypes.CDLL:
    """libamdhip64 with the stream-capture / graph entry points typed (int status results)."""
    global _hip
    if _hip is None:
        hip = ctypes.CDLL("libamdhip64.so")
        for fn in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphInstantiate", "hipGraphLaunch",
                   "hipGraphExecDestroy", "hipGraphDestroy"):
            getattr(hip, fn).restype = ctypes.c_int
        _hip = hip
    return _hip


def stream_capture(stream_handle: ctypes.c_void_p, mode: int, graph: ctypes.c_void_p, op):
    """Capture what op() enqueues on the stream into `graph`; returns (hipStreamEndCapture's status, op's
    result). As torch.cuda.graph prepares a capture: garbage is collected first (a filter an earlier test left
    to the cycle collector is freed by rpt_bf_destroy -> hipFree, which would invalidate a global-mode capture
    from any thread of the process) and the collector stays off inside the capture window."""
    hip = hip_graph_api()
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        assert hip.hipStreamBeginCapture(stream_handle, mode) == 0
        result = op()
        status = hip.hipStreamEndCapture(stream_handle, ctypes.byref(graph))
    finally:
        gc.enable()
    return status, result


def graph_instantiate(graph: ctypes.c_void_p, exe: ctypes.c_void_p) -> int:
    return hip_graph_api().hipGraphInstantiate(ctypes.byref(exe), graph, None, None, ctypes.c_size_t(0))


def graph_launch(exe: ctypes.c_void_p, stream_handle: ctypes.c_void_p) -> int:
    return hip_graph_api().hipGraphLaunch(exe, stream_handle)


def graph_destroy(exe: ctypes.c_void_p, graph: ctypes.c_void_p) -> bool:
    hip = hip_graph_api()
    return hip.hipGraphExecDestroy(exe) == 0 and hip.hipGraphDestroy(graph) == 0


# ---- filters shared by a test module ---------------------------------------------------------------
def build_keys_for(log_nb: int) -> np.ndarray:
    """min(4 * blocks, 300_000) random int64 keys; the first quarter lies in [0, 2^32), so an INTEGER probe
    column can hit them too (int32 keys hash zero-extended through uint32, as the same BIGINT value does)."""
    n = min(1 << (log_nb + 2), 300_000)
    rng = np.random.default_rng(1000 + log_nb)
    keys = rng.integers(-(2**62), 2**62, size=n, dtype=np.int64)
    keys[: n // 4] = rng.integers(0, 2**32, size=n // 4, dtype=np.int64)
    return keys


def int32_build_keys(build_keys: np.ndarray) -> np.ndarray:
    """The build keys an int32 probe key can equal, as int32 bit patterns."""
    return build_keys[: build_keys.size // 4].astype(np.uint32).view(np.int32)


class FilterCache:
    """get(log_nb) -> (BloomFilter, oracle words, build keys): min(4 * blocks, 300_000) random int64 keys,
    inserted with atomics; the device words are compared with the oracle's once, when the filter is made.
    The words are shared: tests must not insert into these filters (the probe strategy may be set freely)."""

    def __init__(self, lib=None):
        self._lib = lib
        self._made = {}

    def get(self, log_nb: int):
        if log_nb not in self._made:
            import rpt_amd

            keys = build_keys_for(log_nb)
            bf = rpt_amd.BloomFilter(log_num_blocks=log_nb, lib=self._lib)
            bf.insert(torch.from_numpy(keys).to(bf.device), strategy=1)  # RPT_INSERT_ATOMIC
            words = orc.new_words(log_nb)
            orc.insert_keys(words, log_nb, keys)
            assert np.array_equal(bf.export_words(), words), f"2^{log_nb}-block filter differs from the oracle"
            words.setflags(write=False)
            self._made[log_nb] = (bf, words, keys)
        return self._made[log_nb]

    def close(self) -> None:
        for bf, _w, _k in self._made.values():
            bf.close()
        self._made.clear()
