"""Results must not depend on what a caller's workspace or output buffers hold on entry, and nothing may be
written outside their documented sizes (include/rpt_gpu.h, "Caller buffers").

Nearly every other GPU test hands the library a fresh torch.empty buffer, used once: fresh device memory usually
reads as zero and a recycled block holds the leftovers of the same call shape, so a kernel that read a counter,
stamp, run table or pass byte nobody wrote would pass them all. Here every workspace is exactly
rpt_bf_probe_workspace_bytes / rpt_bf_insert_workspace_bytes bytes, every output exactly its documented size,
each between guard bands (buf_util.GuardedBuffer), and each filled with a poison pattern before the call.
Everything is bit-exact against rpt_oracle: no tolerances.

Geometries are the smallest that reach each code path (log2 blocks, forced strategy): 2^4 gather; 2^14 whole
filter in LDS; 2^15 / 2^17 hybrid LDS + L2; partitioned with 1 slice (2^14, wave-aggregated counters), 16 slices
(2^18, the first with skew items), 128 slices (2^21, 16 Ki-row tiles) and 256 slices (2^22, 32 Ki-row tiles);
bucketed with 1 and 2 buckets (2^22, 2^23). Row counts: 16385 (just past the fused kernel, two tiles), 131073 (one
256-segment scan group + 1 row), 200001, and for 2^18 partitioned 256 * 16384 + 16385 (a second block of 256 tiles).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import rpt_oracle as orc
from buf_util import (A5, CAPTURE_MODE_RELAXED, FF, RAMP, FilterCache, GuardedBuffer, alt32, build_keys_for, const32,
                      graph_destroy, graph_instantiate, graph_launch, int32_build_keys, pattern_id, stream_capture)
from conftest import REPO

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED, BUCKETED = 0, 1, 2, 3, 4
INS_PARTITIONED, INS_BUCKETED = 2, 3
STRATEGY_NAME = {AUTO: "auto", GATHER: "gather", LDS: "lds", PARTITIONED: "part", BUCKETED: "buck"}
TEST_LIB = os.path.join(REPO, "tests", "loopback", "build", "librpt_gpu_testing.so")

GEOMS = [(4, GATHER), (14, LDS), (15, LDS), (17, LDS), (14, PARTITIONED), (18, PARTITIONED), (21, PARTITIONED),
         (22, PARTITIONED), (22, BUCKETED), (23, BUCKETED)]
ROWS = [16385, 131073, 200001]
BIG_ROWS = 256 * 16384 + 16385  # crosses a block of 256 tiles: the second block's offset is used
PASS = [0.0, 0.3, 1.0]
# in the order a first run should meet them: bytes that are no small integer, then small indices, then all-ones
PATTERNS = [A5, RAMP, FF, const32(0x00010001), alt32(0x55555555)]
ENTRIES = ("probe", "bits", "phases")


def geom_id(g):
    return f"2^{g[0]}-{STRATEGY_NAME[g[1]]}"


def rows_of(geom):
    return ROWS + ([BIG_ROWS] if geom == (18, PARTITIONED) else [])


def dev(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def cur_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def filters(rpt):
    fc = FilterCache()
    yield fc
    fc.close()


@pytest.fixture(scope="module")
def tlib(rpt):
    from rpt_amd import _lib

    t = _lib.load_variant(TEST_LIB)
    t.rpt_testing_next_skew_epoch.restype = ctypes.c_uint32
    t.rpt_testing_next_skew_epoch.argtypes = []
    t.rpt_testing_bucketed_insert_batch.restype = ctypes.c_uint64
    return t


@pytest.fixture(scope="module")
def tfilters(tlib):
    fc = FilterCache(lib=tlib)
    yield fc
    fc.close()


# ---- probe batches and their oracle results, made once and shared (never modified) -------------------
class Batch:
    """A probe batch on host and device with the oracle's answer: `sel` (the ids rpt_bf_probe must write) and
    `bits` (the ceil(n/512)*8 words rpt_bf_probe_bits must write, zero past n)."""

    def __init__(self, words, log_nb, keys, key_sel=None, valid=None, row_sel=None):
        self.keys, self.key_sel, self.row_sel = keys, key_sel, row_sel
        self.vw = gu.validity_words(valid) if valid is not None else None
        # physical key index of the i-th probed row
        eff = key_sel if row_sel is None else (key_sel[row_sel] if key_sel is not None else row_sel)
        self.n = int(eff.size if eff is not None else keys.size)
        idx = orc.probe_keys(words, log_nb, keys, key_sel=eff, validity=self.vw).copy()
        self.sel = idx if row_sel is None else row_sel[idx]
        flags = np.zeros(-(-self.n // 512) * 512, dtype=np.uint8)
        flags[idx] = 1
        self.bits = np.packbits(flags, bitorder="little").view(np.uint64)
        for a in (self.sel, self.bits):
            a.setflags(write=False)
        self._dev = None

    def column(self, rpt):
        """(rpt_key_column, row_sel device pointer or None); the device tensors stay alive with the batch."""
        if self._dev is None:
            self._dev = tuple(None if a is None else dev(a) for a in (self.keys, self.key_sel, self.vw, self.row_sel))
        k, ks, vw, rs = self._dev
        return rpt.make_column(k, None, ks, vw), (None if rs is None else rs.data_ptr())


_BATCHES = {}


def flat_batch(filters, log_nb, n, pf, dtype=np.int64, hot=False):
    """n keys of which about pf come from the filter's build keys (pf = 1.0: all of them); hot: 30 % of the rows
    carry ONE build key (probe keys skewed onto a slice)."""
    key = (id(filters), log_nb, n, pf, np.dtype(dtype).name, hot)
    if key not in _BATCHES:
        _bf, words, build = filters.get(log_nb)
        rng = np.random.default_rng([log_nb, n, int(pf * 10), np.dtype(dtype).itemsize])
        if dtype == np.int64:
            pool, miss = build, rng.integers(-(2**62), 2**62, size=n, dtype=np.int64)
        else:
            pool, miss = int32_build_keys(build), rng.integers(-(2**31), 2**31, size=n, dtype=np.int32)
        hit = pool[rng.integers(0, pool.size, n)]
        keys = hit if pf >= 1.0 else (miss if pf <= 0.0 else np.where(rng.random(n) < pf, hit, miss))
        if hot:
            keys = np.where(rng.random(n) < 0.3, pool[7 % pool.size], keys)
        _BATCHES[key] = Batch(words, log_nb, np.ascontiguousarray(keys, dtype=dtype))
    return _BATCHES[key]


def vector_batch(filters, log_nb, n=200001):
    """A DuckDB-shaped vector: DICTIONARY keys with NULLs, probed through a row selection (n of n + 5000 rows)."""
    key = (id(filters), log_nb, n, "vector")
    if key not in _BATCHES:
        _bf, words, build = filters.get(log_nb)
        rng = np.random.default_rng([log_nb, n, 77])
        d = 60_000
        dict_keys = np.where(rng.random(d) < 0.3, build[rng.integers(0, build.size, d)],
                             rng.integers(-(2**62), 2**62, size=d, dtype=np.int64))
        valid = rng.random(d) > 0.1
        rows = n + 5000
        key_sel = rng.integers(0, d, rows).astype(np.uint32)
        row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32)
        _BATCHES[key] = Batch(words, log_nb, dict_keys, key_sel=key_sel, valid=valid, row_sel=row_sel)
    return _BATCHES[key]


# ---- one guarded, poisoned call of each probe entry point -----------------------------------------
class ProbeBuffers:
    """Exactly sized guarded buffers of a probe of n rows: workspace (ws_bytes), out_sel (n entries), out_bits
    (ceil(n/512)*8 words), out_count (one uint64)."""

    def __init__(self, n, ws_bytes):
        self.n = n
        self.ws = GuardedBuffer(ws_bytes)
        self.sel = GuardedBuffer(4 * n)
        self.bits = GuardedBuffer(8 * 8 * -(-n // 512))
        self.cnt = GuardedBuffer(8)

    def poison(self, pattern, workspace=True):
        for b in (self.sel, self.bits, self.cnt) + ((self.ws,) if workspace else ()):
            b.poison(pattern)

    def assert_guards(self, what):
        for name in ("ws", "sel", "bits", "cnt"):
            getattr(self, name).assert_guards_intact(f"{what}: {name}")


def run_entry(rpt, lib, bf, batch, bufs, entry, what, stream=None):
    """Run one probe entry point into bufs (as poisoned by the caller) and check it against the oracle."""
    col, rs = batch.column(rpt)
    n, ws, ws_bytes = batch.n, bufs.ws.ptr, bufs.ws.nbytes
    s = cur_stream() if stream is None else stream
    if entry == "bits":
        st = lib.rpt_bf_probe_bits(bf.handle, ctypes.byref(col), rs, n, bufs.bits.ptr, ws, ws_bytes, s)
    elif entry == "phases":
        st = lib.rpt_bf_probe_phase1(bf.handle, ctypes.byref(col), rs, n, ws, ws_bytes, s)
        assert st == 0, f"{what}: phase 1: {lib.rpt_last_error().decode()}"
        st = lib.rpt_bf_probe_phase2(bf.handle, rs, n, bufs.sel.ptr, bufs.cnt.ptr, ws, ws_bytes, s)
    else:
        st = lib.rpt_bf_probe(bf.handle, ctypes.byref(col), rs, n, bufs.sel.ptr, bufs.cnt.ptr, ws, ws_bytes, s)
    assert st == 0, f"{what}: {lib.rpt_last_error().decode()}"
    check_entry(batch, bufs, entry, what)


def check_entry(batch, bufs, entry, what):
    torch.cuda.synchronize()
    if entry == "bits":
        got = bufs.bits.view(torch.int64).cpu().numpy().view(np.uint64)
        diff = np.flatnonzero(got != batch.bits)
        assert diff.size == 0, f"{what}: {diff.size} result words differ, first word {diff[0]} of {got.size}"
    else:
        cnt = int(bufs.cnt.view(torch.int64)[0])
        assert cnt == batch.sel.size, f"{what}: count {cnt}, oracle {batch.sel.size}"
        got = bufs.sel.view(torch.int32)[:cnt].cpu().numpy().view(np.uint32)
        diff = np.flatnonzero(got != batch.sel)
        assert diff.size == 0, f"{what}: {diff.size} sel entries differ, first at {diff[0]} of {cnt}"
    bufs.assert_guards(what)


def strategy_filter(fc, lib, geom):
    log_nb, strategy = geom
    bf, _words, _keys = fc.get(log_nb)
    bf.probe_strategy = strategy
    return bf


def sweep(rpt, lib, fc, geom, batches, patterns, entries=ENTRIES):
    bf = strategy_filter(fc, lib, geom)
    bufs = {}
    for batch in batches:
        n = batch.n
        if n not in bufs:
            bufs[n] = ProbeBuffers(n, int(lib.rpt_bf_probe_workspace_bytes(bf.handle, n)))
        for pattern in patterns:
            for entry in entries:
                bufs[n].poison(pattern)
                run_entry(rpt, lib, bf, batch, bufs[n], entry,
                          f"{geom_id(geom)} n={n} {entry} poison={pattern_id(pattern)} survivors={batch.sel.size}")


# ---- a. poisoned, exactly sized, guarded workspace and outputs --------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=geom_id)
@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
def test_probe_int64_poisoned_exact_buffers(rpt, filters, geom, pattern):
    """int64 keys: every row count x pass fraction (0, ~0.3, 1.0) x entry point of the geometry."""
    batches = [flat_batch(filters, geom[0], n, pf) for n in rows_of(geom) for pf in PASS]
    sweep(rpt, rpt.load(), filters, geom, batches, [pattern])


@pytest.mark.parametrize("geom", GEOMS, ids=geom_id)
def test_probe_int32_poisoned_exact_buffers(rpt, filters, geom):
    sweep(rpt, rpt.load(), filters, geom, [flat_batch(filters, geom[0], 200001, 0.3, np.int32)], PATTERNS)


@pytest.mark.parametrize("geom", GEOMS, ids=geom_id)
def test_probe_dictionary_nulls_row_sel_poisoned_exact_buffers(rpt, filters, geom):
    sweep(rpt, rpt.load(), filters, geom, [vector_batch(filters, geom[0])], PATTERNS)


@pytest.mark.parametrize("log_nb", [4, 18])
def test_find_bits_poisoned_exact_output(rpt, filters, log_nb):
    """rpt_bf_find_bits takes no workspace: ceil(n/512)*8 words exactly, bits past n zero, whatever they held."""
    lib = rpt.load()
    bf, _w, _k = filters.get(log_nb)
    for n in (1, 513, 16385, 200001):
        out = GuardedBuffer(8 * 8 * -(-n // 512))
        for i, pf in enumerate(PASS):
            batch = flat_batch(filters, log_nb, n, pf)
            col, _rs = batch.column(rpt)
            for pattern in (PATTERNS[i], FF):
                out.poison(pattern)
                st = lib.rpt_bf_find_bits(bf.handle, ctypes.byref(col), n, out.ptr, cur_stream())
                assert st == 0, lib.rpt_last_error().decode()
                torch.cuda.synchronize()
                got = out.view(torch.int64).cpu().numpy().view(np.uint64)
                assert np.array_equal(got, batch.bits), f"n={n} pf={pf} poison={pattern_id(pattern)}"
                out.assert_guards_intact(f"find_bits n={n}")


# ---- b. stale skew stamps ---------------------------------------------------------------------------
@pytest.mark.parametrize("hot", [False, True], ids=["uniform", "skewed"])
@pytest.mark.parametrize("fill", ["every-slice-heavy", "alternate-slices-heavy", "previous-call"])
@pytest.mark.parametrize("log_nb", [18, 21])
def test_stale_skew_stamps_do_not_change_results(rpt, tlib, tfilters, log_nb, fill, hot):
    """The skewed partitioned probe stamps the slices its keys overload with a per-call epoch in workspace words
    no eager call clears. A stale word equal to the call's epoch sends a slice that is NOT overloaded down the
    fine-item path and empties its base items: the work is divided differently, the result must not change. The
    whole workspace is filled with the coming epoch E (every slice looks heavy), with (E, ~E) (every other
    slice), or with E - 1 (what the previous call left)."""
    geom = (log_nb, PARTITIONED)
    bf = strategy_filter(tfilters, tlib, geom)
    for n in (16385, 200001):
        batch = flat_batch(tfilters, log_nb, n, 0.3, hot=hot)
        bufs = ProbeBuffers(n, int(tlib.rpt_bf_probe_workspace_bytes(bf.handle, n)))
        for entry in ENTRIES:
            e = tlib.rpt_testing_next_skew_epoch()
            assert e >= 2  # 1 is the captured probes' stamp
            pattern = {"every-slice-heavy": const32(e), "alternate-slices-heavy": alt32(e),
                       "previous-call": const32(e - 1)}[fill]
            bufs.poison(pattern)
            run_entry(rpt, tlib, bf, batch, bufs, entry, f"{geom_id(geom)} n={n} {entry} {fill} epoch={e}")
            assert tlib.rpt_testing_next_skew_epoch() == e + 1  # the probe used the stamp the fill anticipated


# ---- c. one workspace reused across filters, strategies, entry points and batch sizes -----------------
SEQUENCE = [  # (log_nb, strategy, entry point, rows, pass fraction): n descending, then ascending, ...
    (18, PARTITIONED, "probe", BIG_ROWS, 0.3),
    (14, LDS, "bits", 16385, 1.0),
    (22, BUCKETED, "probe", 200001, 0.3),
    (21, PARTITIONED, "phases", 131073, 0.0),
    (4, GATHER, "probe", 16385, 0.3),
    (22, AUTO, "probe", 513, 1.0),  # the fused small probe in between: leaves the workspace as it is
    (22, PARTITIONED, "bits", 200001, 1.0),
    (17, LDS, "probe", 131073, 0.3),
    (18, PARTITIONED, "probe", 16385, 1.0),
    (23, BUCKETED, "phases", 200001, 0.3),
    (21, PARTITIONED, "probe", 200001, 1.0),
    (14, PARTITIONED, "probe", 131073, 0.3),
    (18, PARTITIONED, "bits", BIG_ROWS, 0.0),
]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_workspace_reused_across_calls(rpt, filters, order):
    """What a long-running host does: one grow-on-demand device buffer serves every probe. Poisoned once, then
    each call finds what the previous ones left. Every call against the oracle, every guard after every call."""
    lib = rpt.load()
    steps = SEQUENCE if order == "forward" else SEQUENCE[::-1]
    need = 0
    for log_nb, strategy, _entry, n, _pf in steps:
        bf = strategy_filter(filters, lib, (log_nb, strategy))
        need = max(need, int(lib.rpt_bf_probe_workspace_bytes(bf.handle, n)))
    ws = GuardedBuffer(need).poison(A5)
    for i, (log_nb, strategy, entry, n, pf) in enumerate(steps):
        bf = strategy_filter(filters, lib, (log_nb, strategy))
        batch = flat_batch(filters, log_nb, n, pf)
        bufs = ProbeBuffers(n, 0)
        bufs.ws = ws  # the shared one, passed at its full size
        bufs.poison(A5, workspace=False)
        run_entry(rpt, lib, bf, batch, bufs, entry, f"{order} step {i}: {geom_id((log_nb, strategy))} n={n} {entry}")


# ---- d. graph replays over a dirtied workspace --------------------------------------------------------
@pytest.mark.parametrize("log_nb,strategy,n,hot", [(14, LDS, 200_000, False), (18, PARTITIONED, 300_001, True),
                                                   (21, PARTITIONED, 300_001, False)],
                         ids=["2^14-lds", "2^18-part-skewed", "2^21-part"])
def test_graph_replays_over_a_dirtied_workspace(rpt, filters, log_nb, strategy, n, hot):
    """A captured rpt_bf_probe owns its workspace only while a replay runs: between replays the host may have
    used it for anything. Before each replay the workspace and out_sel are filled with another pattern, one of
    them the constant 1 (the skew epoch every captured probe uses). One stream, so the graph is linear."""
    lib = rpt.load()
    bf = strategy_filter(filters, lib, (log_nb, strategy))
    batch = flat_batch(filters, log_nb, n, 0.3, hot=hot)
    bufs = ProbeBuffers(n, int(lib.rpt_bf_probe_workspace_bytes(bf.handle, n)))
    col, rs = batch.column(rpt)
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    bufs.poison(A5)

    def op():
        return lib.rpt_bf_probe(bf.handle, ctypes.byref(col), rs, n, bufs.sel.ptr, bufs.cnt.ptr, bufs.ws.ptr,
                                bufs.ws.nbytes, sh)

    end, st = stream_capture(sh, CAPTURE_MODE_RELAXED, graph, op)
    assert st == 0, lib.rpt_last_error().decode()
    assert end == 0
    assert graph_instantiate(graph, exe) == 0
    for pattern in (const32(1), RAMP, FF):
        bufs.poison(pattern)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        check_entry(batch, bufs, "probe", f"{geom_id((log_nb, strategy))} replay after {pattern_id(pattern)}")
    assert graph_destroy(exe, graph)


# ---- e. routed inserts --------------------------------------------------------------------------------
def insert_keys_for(rng, n, dtype, nulls):
    info = np.iinfo(dtype)
    keys = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    valid = (rng.random(n) > 0.1) if nulls else None
    return keys, (gu.validity_words(valid) if valid is not None else None)


def merged_minmax(a, b):
    if a is None or b is None:
        return a if b is None else b
    return min(a[0], b[0]), max(a[1], b[1])


@pytest.mark.parametrize("n", [1, 16385, 300_001])
@pytest.mark.parametrize("strategy,log_nb", [(INS_PARTITIONED, 14), (INS_PARTITIONED, 18), (INS_PARTITIONED, 22),
                                             (INS_BUCKETED, 22), (INS_BUCKETED, 23)])
def test_routed_insert_poisoned_exact_workspace(rpt, strategy, log_nb, n):
    """rpt_bf_insert_ws, int64 / int32 keys with and without NULLs, each into a fresh filter, after rpt_bf_clear
    (the whole-slice store modes) and into a filter that already holds other keys (the atomic and adaptive
    merges): words and key min/max against the oracle. Pad records of a run are stale by design: the insert
    must OR none of them, whatever the workspace held."""
    lib = rpt.load()
    case = 0
    for dtype in (np.int64, np.int32):
        for nulls in (False, True):
            rng = np.random.default_rng([log_nb, n, strategy, np.dtype(dtype).itemsize, int(nulls)])
            bf = rpt.BloomFilter(log_num_blocks=log_nb)
            assert lib.rpt_bf_set_insert_strategy(bf.handle, strategy) == 0
            need = int(lib.rpt_bf_insert_workspace_bytes(bf.handle, n))
            assert need > 0
            ws = GuardedBuffer(need)
            words, mm = orc.new_words(log_nb), None
            for state in ("fresh", "cleared", "holding-keys"):
                keys, vw = insert_keys_for(rng, n, dtype, nulls)
                what = f"{np.dtype(dtype).name} nulls={nulls} {state}"
                if state == "cleared":
                    bf.clear()
                    words, mm = orc.new_words(log_nb), None
                pattern = PATTERNS[case % len(PATTERNS)]
                case += 1
                ws.poison(pattern)
                dk, dv = dev(keys), (dev(vw) if vw is not None else None)
                col = rpt.make_column(dk, None, None, dv)
                st = lib.rpt_bf_insert_ws(bf.handle, ctypes.byref(col), n, ws.ptr, need, cur_stream())
                assert st == 0, f"{what}: {lib.rpt_last_error().decode()}"
                torch.cuda.synchronize()
                orc.insert_keys(words, log_nb, keys, validity=vw)
                mm = merged_minmax(mm, orc.minmax(keys, validity=vw))
                got = bf.export_words()
                diff = np.flatnonzero(got != words)
                assert diff.size == 0, f"{what} poison={pattern_id(pattern)}: {diff.size} filter words differ"
                assert bf.minmax() == mm, what
                ws.assert_guards_intact(f"{what}: insert workspace")
            bf.close()


def test_batched_bucketed_insert_poisoned_workspace(rpt, tlib):
    """The test build's batched bucketed insert (batches of 2^20 rows reuse ONE workspace, each finding the
    previous batch's lists, cursors and run tables): 2^25 blocks, 2_100_003 rows through a dictionary."""
    log_nb, n = 25, 2_100_003
    assert tlib.rpt_testing_bucketed_insert_batch() == 1 << 20
    rng = np.random.default_rng(n)
    dict_keys = rng.integers(-(2**63), 2**63 - 1, size=300_000, dtype=np.int64, endpoint=True)
    key_sel = rng.integers(0, dict_keys.size, n).astype(np.uint32)
    vw = gu.validity_words(rng.random(dict_keys.size) > 0.1)
    bf = rpt.BloomFilter(log_num_blocks=log_nb, lib=tlib)
    assert tlib.rpt_bf_set_insert_strategy(bf.handle, INS_BUCKETED) == 0
    need = int(tlib.rpt_bf_insert_workspace_bytes(bf.handle, n))
    ws = GuardedBuffer(need).poison(RAMP)
    dk, ds, dv = dev(dict_keys), dev(key_sel), dev(vw)
    col = rpt.make_column(dk, None, ds, dv)
    assert tlib.rpt_bf_insert_ws(bf.handle, ctypes.byref(col), n, ws.ptr, need, cur_stream()) == 0, tlib.rpt_last_error()
    torch.cuda.synchronize()
    words = orc.new_words(log_nb)
    orc.insert_keys(words, log_nb, dict_keys, key_sel=key_sel, validity=vw)
    assert np.array_equal(bf.export_words(), words)
    assert bf.minmax() == orc.minmax(dict_keys, key_sel=key_sel, validity=vw)
    ws.assert_guards_intact("batched bucketed insert workspace")
    bf.close()


# ---- f. fused small probe and chain ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 513, 16384])
def test_fused_small_probe_leaves_the_workspace_untouched(rpt, filters, n):
    lib = rpt.load()
    bf = strategy_filter(filters, lib, (18, AUTO))
    assert lib.rpt_bf_probe_is_fused(bf.handle, n) == 1
    batch = flat_batch(filters, 18, n, 1.0)  # every row passes: out_sel is written to its last entry
    assert batch.sel.size == n
    bufs = ProbeBuffers(n, int(lib.rpt_bf_probe_workspace_bytes(bf.handle, n)))
    bufs.poison(RAMP)
    before = bufs.ws.bytes().clone()
    run_entry(rpt, lib, bf, batch, bufs, "probe", f"fused n={n}")
    assert torch.equal(bufs.ws.bytes(), before), "the fused probe wrote into the workspace"
    # no workspace at all
    col, rs = batch.column(rpt)
    bufs.poison(FF, workspace=False)
    st = lib.rpt_bf_probe(bf.handle, ctypes.byref(col), rs, n, bufs.sel.ptr, bufs.cnt.ptr, None, 0, cur_stream())
    assert st == 0, lib.rpt_last_error().decode()
    check_entry(batch, bufs, "probe", f"fused n={n}, NULL workspace")


def test_probe_chain_exact_out_sel(rpt, filters):
    """rpt_bf_probe_chain over 3 filters, every row passing every filter: out_sel of exactly n entries."""
    chain = [filters.get(log_nb) for log_nb in (14, 18, 21)]
    for n in (1, 513, 16384):
        rng = np.random.default_rng(n)
        cols_host = [k[rng.integers(0, k.size, n)] for _bf, _w, k in chain]
        want = np.arange(n, dtype=np.uint32)
        for (_bf, w, _k), keys in zip(chain, cols_host):
            want = np.intersect1d(want, orc.probe_keys(w, int(np.log2(w.size)), keys)).astype(np.uint32)
        assert want.size == n
        sel, cnt = GuardedBuffer(4 * n).poison(A5), GuardedBuffer(8).poison(A5)
        got = rpt.probe_chain([bf for bf, _w, _k in chain], [dev(k) for k in cols_host], n=n,
                              out_sel=sel.view(torch.int32), out_count=cnt.view(torch.int64))
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
        sel.assert_guards_intact(f"chain n={n}: out_sel")
        cnt.assert_guards_intact(f"chain n={n}: out_count")


# ---- g. plain outputs ---------------------------------------------------------------------------------
SIZES = [1, 3, 513, 100_003]


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_hash_outputs_exact(rpt, dtype):
    lib = rpt.load()
    for n in SIZES:
        rng = np.random.default_rng(n)
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
        b = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
        vw = gu.validity_words(rng.random(n) > 0.2)
        da, db, dv = dev(a), dev(b), dev(vw)
        out = GuardedBuffer(8 * n).poison(RAMP)
        ca, cb = rpt.make_column(da, None, None, dv), rpt.make_column(db)
        assert lib.rpt_hash_keys(ctypes.byref(ca), n, out.ptr, cur_stream()) == 0
        torch.cuda.synchronize()
        h = orc.hash_keys(a, validity=vw)
        assert np.array_equal(out.view(torch.int64).cpu().numpy().view(np.uint64), h), n
        assert lib.rpt_hash_combine(ctypes.byref(cb), n, out.ptr, cur_stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.view(torch.int64).cpu().numpy().view(np.uint64), orc.hash_combine(h, b)), n
        out.assert_guards_intact(f"hashes n={n}")


def test_keys_widen_exact_output(rpt):
    lib = rpt.load()
    row0 = np.array([0, 1, 4, 517, 517, 100_003], dtype=np.uint32)  # ragged chunks, one empty
    n = int(row0[-1])
    rng = np.random.default_rng(3)
    lo = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    hi = rng.integers(0, 2**32, size=row0.size - 1, dtype=np.uint64).astype(np.uint32)
    want = lo.astype(np.uint64)
    for c in range(hi.size):
        want[row0[c]: row0[c + 1]] |= np.uint64(hi[c]) << np.uint64(32)
    out = GuardedBuffer(8 * n).poison(A5)
    dl, dh, dr = dev(lo), dev(hi), dev(row0)
    assert lib.rpt_keys_widen(dl.data_ptr(), dh.data_ptr(), dr.data_ptr(), hi.size, out.ptr, cur_stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.view(torch.int64).cpu().numpy().view(np.uint64), want)
    out.assert_guards_intact("keys_widen")


def test_words_or_exact_outputs(rpt):
    lib = rpt.load()
    for n in SIZES:  # rpt_words_or: dst |= src, odd word counts included
        rng = np.random.default_rng(n)
        a, b = (rng.integers(0, 2**63, size=n, dtype=np.uint64) for _ in range(2))
        dst = GuardedBuffer(8 * n)
        dst.view(torch.int64).copy_(dev(a))
        db = dev(b)
        assert lib.rpt_words_or(dst.ptr, db.data_ptr(), n, cur_stream()) == 0, lib.rpt_last_error().decode()
        torch.cuda.synchronize()
        assert np.array_equal(dst.view(torch.int64).cpu().numpy().view(np.uint64), a | b), n
        dst.assert_guards_intact(f"words_or n={n}")
    for n in (2, 4, 514, 100_004):  # rpt_words_or_slices: dst = OR of k slices, even word counts
        rng = np.random.default_rng(n)
        k = 3
        srcs = rng.integers(0, 2**63, size=k * n, dtype=np.uint64)
        dst = GuardedBuffer(8 * n).poison(FF)
        ds = dev(srcs)
        assert lib.rpt_words_or_slices(dst.ptr, ds.data_ptr(), k, n, cur_stream()) == 0, lib.rpt_last_error().decode()
        torch.cuda.synchronize()
        want = srcs[:n] | srcs[n: 2 * n] | srcs[2 * n:]
        assert np.array_equal(dst.view(torch.int64).cpu().numpy().view(np.uint64), want), n
        dst.assert_guards_intact(f"words_or_slices n={n}")


@pytest.mark.parametrize("log_nb", [4, 14])
def test_copy_words_to_exact_output(rpt, filters, log_nb):
    bf, words, _k = filters.get(log_nb)
    out = GuardedBuffer(8 << log_nb).poison(RAMP)
    bf.copy_words_to(out.view(torch.int64))
    torch.cuda.synchronize()
    assert np.array_equal(out.view(torch.int64).cpu().numpy().view(np.uint64), words)
    out.assert_guards_intact("copy_words_to")


# ---- workspace alignment ------------------------------------------------------------------------------
def test_misaligned_workspace_is_rejected(rpt, filters):
    """Workspaces must be 16-byte aligned (rpt_gpu.h): another base is refused before anything is launched.
    Only the returned status is checked."""
    lib = rpt.load()
    n = 16385
    bf = strategy_filter(filters, lib, (18, PARTITIONED))
    batch = flat_batch(filters, 18, n, 0.3)
    col, rs = batch.column(rpt)
    need = int(lib.rpt_bf_probe_workspace_bytes(bf.handle, n))
    raw = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    bits = torch.empty(8 * -(-n // 512), dtype=torch.int64, device="cuda:0")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    s = cur_stream()
    for off in (1, 4, 8):
        ws = raw.data_ptr() + off
        assert lib.rpt_bf_probe(bf.handle, ctypes.byref(col), rs, n, sel.data_ptr(), cnt.data_ptr(), ws, need, s) == 1
        assert b"aligned" in lib.rpt_last_error()
        assert lib.rpt_bf_probe_bits(bf.handle, ctypes.byref(col), rs, n, bits.data_ptr(), ws, need, s) == 1
        assert lib.rpt_bf_probe_phase1(bf.handle, ctypes.byref(col), rs, n, ws, need, s) == 1
        assert lib.rpt_bf_probe_phase2(bf.handle, rs, n, sel.data_ptr(), cnt.data_ptr(), ws, need, s) == 1
    ins = rpt.BloomFilter(log_num_blocks=18)
    assert lib.rpt_bf_set_insert_strategy(ins.handle, INS_PARTITIONED) == 0
    ineed = int(lib.rpt_bf_insert_workspace_bytes(ins.handle, n))
    assert 0 < ineed <= need + 240
    assert lib.rpt_bf_insert_ws(ins.handle, ctypes.byref(col), n, raw.data_ptr() + 8, ineed, s) == 1
    assert b"aligned" in lib.rpt_last_error()
    torch.cuda.synchronize()
    assert ins.is_empty() and ins.export_words().sum() == 0  # refused before anything ran
    assert cnt.item() == 0
    ins.close()
