"""USE_BF's filter chain for batches of any size (rpt_bf_probe_chain_ws) vs the oracle: the rows passing every
filter of the chain, each probed on its own key column, i.e. the np.intersect1d of orc.probe_keys per filter (what
physical_use_bf.cpp:127-179 computes filter after filter over the previous survivors). Bit-exact.

The filters are built once per module (buf_util.FilterCache; two caches, so a chain can hold two filters of one
size with different strategies). Tests set the probe strategy of the shared filters freely and never insert."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import rpt_oracle as orc
from buf_util import (A5, CAPTURE_MODE_GLOBAL, FF, RAMP, FilterCache, GuardedBuffer, build_keys_for, graph_destroy,
                      graph_instantiate, graph_launch, hip_graph_api, int32_build_keys, stream_capture)

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED, BUCKETED = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def caches(rpt):
    a, b = FilterCache(), FilterCache()
    yield a, b
    a.close()
    b.close()


def dev(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def sel_of(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def rand_keys(dtype, n, seed):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)


def hits(rng, build, n, dtype, frac):
    """n keys of `dtype`: a fraction `frac` drawn from the filter's build keys, the rest random."""
    pool = build if dtype == np.int64 else int32_build_keys(build)
    miss = rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, size=n, dtype=dtype, endpoint=True)
    return np.where(rng.random(n) < frac, pool[rng.integers(0, pool.size, n)], miss).astype(dtype)


def force(bf, strategy, n):
    bf.probe_strategy = strategy
    if strategy != AUTO:
        assert bf.probe_strategy_for(n) == strategy
    return bf


def intersect(refs):
    return functools.reduce(np.intersect1d, refs).astype(np.uint32)


# ---- 1. mixed columns ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16385, 16896, 65537, 131073, 300001])
@pytest.mark.parametrize("use_row_sel", [False, True])
def test_chain_ws_mixed_columns_vs_oracle(rpt, caches, n, use_row_sel):
    """Three filters (16 KiB, 256 KiB, 16 MiB) on an int64 FLAT column, an int32 column with 10 % NULLs and an
    int64 DICTIONARY column, with and without a row selection of exactly n rows: the first size past the fused
    kernel, an exact number of segments, ragged tails, the first size past one 256-segment scan group."""
    rng = np.random.default_rng(n + use_row_sel)
    (f0, w0, b0), (f1, w1, b1), (f2, w2, b2) = (caches[0].get(L) for L in (11, 15, 21))
    for f in (f0, f1, f2):
        force(f, AUTO, n)
    rows = n + n // 2 if use_row_sel else n  # rows of the columns; n of them are probed
    c0 = hits(rng, b0, rows, np.int64, 0.8)
    c1 = hits(rng, b1, rows, np.int32, 0.8)
    vw1 = gu.validity_words(rng.random(rows) < 0.9)
    dict2 = hits(rng, b2, rows // 2 + 1, np.int64, 0.8)
    ksel2 = rng.integers(0, dict2.size, rows).astype(np.uint32)
    refs = [orc.probe_keys(w0, 11, c0), orc.probe_keys(w1, 15, c1, validity=vw1),
            orc.probe_keys(w2, 21, dict2, key_sel=ksel2)]
    row_sel = None
    if use_row_sel:
        row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32)
        refs = [np.intersect1d(r, row_sel) for r in refs]
    exp = intersect(refs)
    cols = [dev(c0), {"keys": dev(c1), "validity": dev(vw1)}, {"keys": dev(dict2), "key_sel": dev(ksel2)}]
    got = rpt.probe_chain_ws([f0, f1, f2], cols, row_sel=dev(row_sel) if row_sel is not None else None, n=n)
    assert np.array_equal(sel_of(got), exp)
    if n >= 65537:
        assert 0 < exp.size < n
        assert all(r.size < n for r in refs) and exp.size < min(r.size for r in refs)  # every filter removes rows
    # the order of the filters does not change the result
    got = rpt.probe_chain_ws([f2, f0, f1], [cols[2], cols[0], cols[1]],
                             row_sel=dev(row_sel) if row_sel is not None else None, n=n)
    assert np.array_equal(sel_of(got), exp)


# ---- 2. every stage kind in both positions ---------------------------------------------------------------
STAGES = {"gather": (GATHER, 16), "lds": (LDS, 13), "hybrid": (LDS, 16), "partitioned": (PARTITIONED, 18),
          "bucketed": (BUCKETED, 22)}
N_STAGES = 70001


@functools.lru_cache(maxsize=None)
def stage_column(kind: str, slot: int):
    """The key column (and validity words) stage `slot` probes, per column kind; shared by the 25 pairs."""
    rng = np.random.default_rng(100 + slot + (10 if kind == "i32" else 0))
    dtype = np.int64 if kind == "i64" else np.int32
    # one part in six hits each stage filter's build keys, one part is random misses: whichever filter probes the
    # column passes about a sixth of its rows
    keys = rand_keys(dtype, N_STAGES, 200 + slot)
    which = rng.integers(0, len(STAGES) + 1, N_STAGES)
    for i, (_st, L) in enumerate(STAGES.values()):
        b = build_keys_for(L)
        pool = b if dtype == np.int64 else int32_build_keys(b)
        m = which == i
        keys[m] = pool[rng.integers(0, pool.size, int(m.sum()))]
    validity = gu.validity_words(rng.random(N_STAGES) < 0.9) if kind == "i32" else None
    return keys, validity


_stage_refs = {}


def stage_ref(kind, slot, L, words):
    key = (kind, slot, L)
    if key not in _stage_refs:
        keys, validity = stage_column(kind, slot)
        _stage_refs[key] = orc.probe_keys(words, L, keys, validity=validity)
    return _stage_refs[key]


@pytest.mark.parametrize("kind", ["i64", "i32"])  # dense NULL-free int64 (pipelined loop); int32 with NULLs (general loop)
@pytest.mark.parametrize("second", list(STAGES))
@pytest.mark.parametrize("first", list(STAGES))
def test_chain_ws_every_stage_kind_in_both_positions(rpt, caches, first, second, kind):
    n = N_STAGES
    (s0, L0), (s1, L1) = STAGES[first], STAGES[second]
    f0, w0, _ = caches[0].get(L0)
    f1, w1, _ = caches[1].get(L1)
    force(f0, s0, n)
    force(f1, s1, n)
    cols, refs = [], []
    for slot, (L, w) in enumerate(((L0, w0), (L1, w1))):
        keys, validity = stage_column(kind, slot)
        cols.append({"keys": dev(keys), "validity": dev(validity) if validity is not None else None})
        refs.append(stage_ref(kind, slot, L, w))
    exp = intersect(refs)
    assert 0 < exp.size < min(r.size for r in refs)
    assert np.array_equal(sel_of(rpt.probe_chain_ws([f0, f1], cols)), exp)


# ---- 3. forced strategies at tiny n: the large path below the fused size ----------------------------------
@pytest.mark.parametrize("n", [1, 63, 511, 513])
@pytest.mark.parametrize("second", ["gather", "lds", "hybrid"])
def test_chain_ws_forced_strategies_at_tiny_n(rpt, caches, second, n):
    rng = np.random.default_rng(n)
    f0, w0, b0 = caches[0].get(16)
    s1, L1 = STAGES[second]
    f1, w1, b1 = caches[1].get(L1)
    force(f0, GATHER, n)
    force(f1, s1, n)
    c0, c1 = hits(rng, b0, n, np.int64, 0.7), hits(rng, b1, n, np.int64, 0.7)
    exp = intersect([orc.probe_keys(w0, 16, c0), orc.probe_keys(w1, L1, c1)])
    ws = GuardedBuffer(rpt.probe_chain_workspace_bytes([f0, f1], n)).poison(A5)
    got = rpt.probe_chain_ws([f0, f1], [dev(c0), dev(c1)], workspace=ws.bytes())
    assert np.array_equal(sel_of(got), exp)
    assert not torch.all(ws.bytes() == 0xA5), "the large path was not taken: the workspace is untouched"
    ws.assert_guards_intact("workspace")
    # ... and with every filter on AUTO the one-launch kernel takes over and leaves the workspace alone
    force(f0, AUTO, n)
    force(f1, AUTO, n)
    ws.poison(A5)
    got = rpt.probe_chain_ws([f0, f1], [dev(c0), dev(c1)], workspace=ws.bytes())
    assert np.array_equal(sel_of(got), exp)
    assert torch.all(ws.bytes() == 0xA5)


# ---- 4. dead rows ------------------------------------------------------------------------------------------
N_DEAD = 131072 + 4096 + 1  # 264 full segments and a one-row tail segment


@functools.lru_cache(maxsize=None)
def dead_rows():
    dead = np.zeros(N_DEAD, dtype=bool)
    dead[:4096] = True
    dead[131072 - 300: 131072 + 300] = True  # straddles the scan-group boundary (256 segments)
    dead[N_DEAD - 1 - 512: N_DEAD - 1] = True  # every row of the last full segment; row N_DEAD - 1 stays alive
    return dead


@pytest.mark.parametrize("kind", ["i64", "i32"])
@pytest.mark.parametrize("second", ["gather", "lds", "hybrid", "partitioned"])
def test_chain_ws_dead_rows(rpt, caches, second, kind):
    """The first filter rejects rows [0, 4096), a run across row 131072 and the whole last full segment, and lets
    the single row of the one-row tail segment through; the second filter's column would pass every row. A masked
    stage that ignores the mask, or a skipped segment that leaves a stale count, fails here."""
    n = N_DEAD
    assert n % 512 == 1
    dtype = np.int64 if kind == "i64" else np.int32
    rng = np.random.default_rng(7)
    f0, w0, b0 = caches[0].get(21)
    s1, L1 = STAGES[second]
    f1, w1, b1 = caches[1].get(L1)
    force(f0, GATHER, n)
    force(f1, s1, n)
    dead = dead_rows()
    c0 = hits(rng, b0, n, dtype, 1.0)
    miss = rand_keys(dtype, n, 8)
    for _ in range(8):  # keys the first filter certainly rejects (re-drawn while the oracle lets one through)
        bad = orc.probe_keys(w0, 21, miss)
        if bad.size == 0:
            break
        miss[bad] = rand_keys(dtype, bad.size, 9 + _)
    assert orc.probe_keys(w0, 21, miss).size == 0
    c0[dead] = miss[dead]
    c1 = hits(rng, b1, n, dtype, 1.0)
    validity = gu.validity_words(np.ones(n, dtype=bool)) if kind == "i32" else None  # general loop, nothing NULL
    r0, r1 = orc.probe_keys(w0, 21, c0, validity=validity), orc.probe_keys(w1, L1, c1, validity=validity)
    assert np.array_equal(r0, np.flatnonzero(~dead)) and r0[-1] == n - 1
    assert r1.size == n
    cols = [{"keys": dev(c), "validity": dev(validity) if validity is not None else None} for c in (c0, c1)]
    got = sel_of(rpt.probe_chain_ws([f0, f1], cols))
    assert np.array_equal(got, r0.astype(np.uint32))


# ---- 5. chain shapes -----------------------------------------------------------------------------------------
def test_chain_ws_of_one_equals_lookup_sel(rpt, caches):
    n = 40000
    f, _w, b = caches[0].get(17)
    force(f, AUTO, n)
    p = dev(hits(np.random.default_rng(8), b, n, np.int64, 0.5))
    got = sel_of(rpt.probe_chain_ws([f], [p]))
    assert 0 < got.size < n
    assert np.array_equal(got, sel_of(f.lookup_sel(p)))


def test_chain_ws_of_eight_with_hash_column(rpt, caches):
    """RPT_MAX_CHAIN filters; one column given as precomputed hashes (RPT_KEY_HASH); the same filter twice."""
    rng = np.random.default_rng(10)
    n = 40000
    sizes = [11, 13, 15, 16, 17, 18, 21]
    trip = [caches[0].get(L) for L in sizes]
    for f, _w, _b in trip:
        force(f, AUTO, n)
    cols_np = [hits(rng, b, n, np.int64, 0.97) for _f, _w, b in trip]
    refs = [orc.probe_keys(w, L, c) for L, (_f, w, _b), c in zip(sizes, trip, cols_np)]
    exp = intersect(refs + [refs[0]])
    cols = [dev(c) for c in cols_np]
    cols[3] = {"keys": rpt.hash_keys(cols[3]), "key_type": rpt.RPT_KEY_HASH}
    filters = [f for f, _w, _b in trip] + [trip[0][0]]
    assert len(filters) == 8
    got = rpt.probe_chain_ws(filters, cols + [cols[0]])
    assert np.array_equal(sel_of(got), exp)
    assert 0 < exp.size < n


# ---- 6. buffer hygiene -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["direct_first", "partitioned_first"])
def test_chain_ws_buffer_hygiene(rpt, caches, order):
    """Exactly sized workspace, out_sel and out_count between guard bands, poisoned with FF, A5 and a ramp in
    turn: the oracle's result every time, guards intact."""
    n = 70001
    rng = np.random.default_rng(11)
    fd, wd, bd = caches[0].get(16)
    fp, wp, bp = caches[1].get(18)
    force(fd, GATHER, n)
    force(fp, PARTITIONED, n)
    cd, cp = hits(rng, bd, n, np.int64, 0.7), hits(rng, bp, n, np.int64, 0.7)
    exp = intersect([orc.probe_keys(wd, 16, cd), orc.probe_keys(wp, 18, cp)])
    assert 0 < exp.size < n
    filters, cols = ([fd, fp], [dev(cd), dev(cp)]) if order == "direct_first" else ([fp, fd], [dev(cp), dev(cd)])
    need = rpt.probe_chain_workspace_bytes(filters, n)
    assert need > 0 and need % 256 == 0
    ws, sel, cnt = GuardedBuffer(need), GuardedBuffer(4 * n), GuardedBuffer(8)
    for pattern in (FF, A5, RAMP):
        for g in (ws, sel, cnt):
            g.poison(pattern)
        got = rpt.probe_chain_ws(filters, cols, n=n, out_sel=sel.view(torch.int32), out_count=cnt.view(torch.int64),
                                 workspace=ws.bytes())
        assert np.array_equal(sel_of(got), exp), pattern
        for name, g in (("workspace", ws), ("out_sel", sel), ("out_count", cnt)):
            g.assert_guards_intact(f"{order}, {pattern}: {name}")


# ---- 7. graph capture ------------------------------------------------------------------------------------------
def chain_call(rpt, filters, cols, n, out_sel, out_count, ws, stream_handle, row_sel=None):
    """rpt_bf_probe_chain_ws through ctypes: nothing but the call (the Python wrapper reads the count back)."""
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * len(filters))(*[f.handle for f in filters])
    arr = (KeyColumn * len(cols))(*cols)
    return rpt.load().rpt_bf_probe_chain_ws(handles, arr, len(filters), row_sel, n, out_sel.data_ptr(),
                                            out_count.data_ptr(), ws.data_ptr(), ws.numel(), stream_handle)


def test_chain_ws_graph_capture(rpt, caches):
    """One chain call captured on a side stream (linear, one stream; global mode), replayed, the key tensors
    overwritten in place, replayed again: the oracle's result for the keys in place at each replay. A filter with a
    pending clear is refused inside the capture, which stays valid."""
    hip = hip_graph_api()
    n = 70001
    rng = np.random.default_rng(12)
    f0, w0, b0 = caches[0].get(13)
    f1, w1, b1 = caches[1].get(16)
    force(f0, AUTO, n)  # LDS
    force(f1, GATHER, n)
    k0, k1 = dev(hits(rng, b0, n, np.int64, 0.7)), dev(hits(rng, b1, n, np.int64, 0.7))
    cols = [rpt.make_column(k0), rpt.make_column(k1)]
    out_sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(rpt.probe_chain_workspace_bytes([f0, f1], n), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)

    def expected():
        return intersect([orc.probe_keys(w0, 13, k0.cpu().numpy()), orc.probe_keys(w1, 16, k1.cpu().numpy())])

    # once outside any capture (the kernels' first launch sets their LDS allowance)
    assert chain_call(rpt, [f0, f1], cols, n, out_sel, out_count, ws, sh) == 0
    s.synchronize()
    assert np.array_equal(sel_of(out_sel[: int(out_count.item())]), expected())

    # a pending clear is refused inside the capture; the capture itself stays valid
    cleared = rpt.BloomFilter(log_num_blocks=13)
    cleared.insert(dev(b0[:1000]))
    cleared.clear()
    torch.cuda.synchronize()
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph,
                             lambda: chain_call(rpt, [f0, cleared], cols, n, out_sel, out_count, ws, sh))
    assert end == 0
    assert st == 1 and b"rpt_bf_settle" in rpt.load().rpt_last_error()
    assert hip.hipGraphDestroy(graph) == 0

    graph = ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph,
                             lambda: chain_call(rpt, [f0, f1], cols, n, out_sel, out_count, ws, sh))
    assert end == 0 and st == 0, rpt.load().rpt_last_error()
    assert graph_instantiate(graph, exe) == 0
    for replay in range(2):
        if replay == 1:  # other keys in the same tensors
            k0.copy_(dev(hits(rng, b0, n, np.int64, 0.4)))
            k1.copy_(dev(hits(rng, b1, n, np.int64, 0.9)))
        out_sel.fill_(-1)
        out_count.fill_(-1)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        exp = expected()
        assert 0 < exp.size < n
        assert int(out_count.item()) == exp.size
        assert np.array_equal(sel_of(out_sel[: exp.size]), exp), replay
    assert graph_destroy(exe, graph)
    cleared.close()


# ---- 8. empty and cleared filters, n = 0 ------------------------------------------------------------------------
def test_chain_ws_empty_and_cleared_filters(rpt):
    n = 20000
    b = rand_keys(np.int64, 3000, 17)
    f = rpt.BloomFilter(log_num_blocks=13)
    f.insert(dev(b))
    w = orc.new_words(13)
    orc.insert_keys(w, 13, b)
    empty = rpt.BloomFilter(log_num_blocks=13)
    pk = hits(np.random.default_rng(18), b, n, np.int64, 0.5)
    p = dev(pk)
    assert sel_of(rpt.probe_chain_ws([f, empty], [p, p])).size == 0  # an empty filter passes nothing
    assert sel_of(rpt.probe_chain_ws([empty, f], [p, p])).size == 0
    f.clear()  # deferred clear: the chain settles it before reading
    assert sel_of(rpt.probe_chain_ws([f], [p])).size == 0
    f.insert(dev(b))
    exp = orc.probe_keys(w, 13, pk)
    assert 0 < exp.size < n
    assert np.array_equal(sel_of(rpt.probe_chain_ws([f, f], [p, p])), exp)
    out = torch.empty(1, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda:0")
    assert rpt.probe_chain_ws([f], [p], n=0, out_sel=out, out_count=cnt).numel() == 0
    assert int(cnt.item()) == 0
    f.close()
    empty.close()


# ---- 9. argument errors -----------------------------------------------------------------------------------------
def test_chain_ws_argument_errors(rpt, caches):
    from rpt_amd._lib import RPT_ERR_INVALID_ARGUMENT, RPT_ERR_WORKSPACE

    n = 20000
    f, _w, b = caches[0].get(13)
    force(f, AUTO, n)
    p = dev(b[:n])
    with pytest.raises(rpt.RptError):
        rpt.probe_chain_ws([], [])
    with pytest.raises(rpt.RptError) as e:
        rpt.probe_chain_ws([f] * 9, [p] * 9)  # more than RPT_MAX_CHAIN
    assert e.value.status == RPT_ERR_INVALID_ARGUMENT
    with pytest.raises(rpt.RptError):
        rpt.probe_chain_ws([f, f], [p])  # one column per filter
    assert rpt.probe_chain_workspace_bytes([f] * 9, n) == 0
    lib = rpt.load()
    handles = (ctypes.c_void_p * 9)(*[f.handle] * 9)
    cols9 = (type(rpt.make_column(p)) * 9)(*[rpt.make_column(p)] * 9)
    need = rpt.probe_chain_workspace_bytes([f], n)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    out_sel = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_count = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def call(k, rows, ws_ptr, ws_bytes):
        return lib.rpt_bf_probe_chain_ws(handles, cols9, k, None, rows, out_sel.data_ptr(), out_count.data_ptr(),
                                         ws_ptr, ws_bytes, stream)

    assert call(0, n, ws.data_ptr(), need) == RPT_ERR_INVALID_ARGUMENT
    assert call(9, n, ws.data_ptr(), need) == RPT_ERR_INVALID_ARGUMENT
    assert call(1, n, ws.data_ptr(), need - 1) == RPT_ERR_WORKSPACE  # one byte short
    assert b"workspace" in lib.rpt_last_error()
    assert call(1, n, ws.data_ptr() + 8, need) == RPT_ERR_INVALID_ARGUMENT  # base offset by 8
    assert b"aligned" in lib.rpt_last_error()
    assert call(1, 2**32, ws.data_ptr(), need) == RPT_ERR_INVALID_ARGUMENT
    assert lib.rpt_bf_probe_chain_workspace_bytes(handles, 1, 2**32) == 0
    torch.cuda.synchronize()
    assert int(out_count.item()) == -1 and bool((out_sel == -1).all())  # every refusal came before any launch
    assert call(1, n, ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert int(out_count.item()) == n


# ---- 10. a seeded sweep ------------------------------------------------------------------------------------------
SWEEP_SIZES = [4, 10, 13, 14, 16, 17, 18, 21, 22, 23]


# RPT_FUZZ_SEEDS seeds from RPT_FUZZ_SEED_BASE (tools/gpu_soak.sh sweeps more of them)
@pytest.mark.parametrize("seed", range(int(os.environ.get("RPT_FUZZ_SEED_BASE", "0")),
                                       int(os.environ.get("RPT_FUZZ_SEED_BASE", "0")) + int(os.environ.get("RPT_FUZZ_SEEDS", "16"))))
def test_chain_ws_random(rpt, caches, seed):
    """Seeded sweep: 1..8 filters of 2^4..2^23 blocks, each with a random supported strategy forced and its own
    column with a random key type (int64 / int32 / precomputed hashes), NULL rate and dictionary; random row counts
    up to 200000 and row selections. The AND of the oracle's per-filter results, bit-exact."""
    rng = np.random.default_rng(5000 + seed)
    lib = rpt.load()
    k = int(rng.integers(1, 9))
    n = int(rng.choice([1, 513, 16385, int(rng.integers(1, 200001)), int(rng.integers(1, 200001))]))
    filters, cols, refs = [], [], []
    for log_nb in rng.choice(SWEEP_SIZES, size=k, replace=False):
        log_nb = int(log_nb)
        bf, w, build = caches[0].get(log_nb)
        supported = [st for st in (GATHER, LDS, PARTITIONED, BUCKETED) if lib.rpt_probe_strategy_supported(st, log_nb)]
        force(bf, int(rng.choice(supported)), n)
        filters.append(bf)
        dtype = np.int64 if rng.random() < 0.6 else np.int32
        m = int(rng.integers(1, 2 * n + 1)) if rng.random() < 0.4 else n  # dictionary size (if used)
        vals = hits(rng, build, m, dtype, float(rng.choice([0.5, 0.9, 1.0])))
        ksel = rng.integers(0, m, n).astype(np.uint32) if m != n else None
        valid = gu.validity_words(rng.random(m) >= 0.1) if rng.random() < 0.4 else None
        if rng.random() < 0.2 and dtype == np.int64:  # the column as precomputed hashes (NULLs not applied)
            col = {"keys": rpt.hash_keys(dev(vals)), "key_type": rpt.RPT_KEY_HASH}
            ref = orc.probe_keys(w, log_nb, vals, key_sel=ksel)
        else:
            col = {"keys": dev(vals), "validity": dev(valid) if valid is not None else None}
            ref = orc.probe_keys(w, log_nb, vals, key_sel=ksel, validity=valid)
        if ksel is not None:
            col["key_sel"] = dev(ksel)
        cols.append(col)
        refs.append(ref)
    exp = intersect(refs)
    row_sel = None
    if rng.random() < 0.3:
        row_sel = np.sort(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False)).astype(np.uint32)
        exp = np.intersect1d(exp, row_sel).astype(np.uint32)
    got = rpt.probe_chain_ws(filters, cols, row_sel=dev(row_sel) if row_sel is not None else None,
                             n=row_sel.size if row_sel is not None else n)
    assert np.array_equal(sel_of(got), exp)
