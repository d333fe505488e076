"""Routed device-side inserts (rpt_bf_insert_bits_ws, rpt_bf_insert_sel_ws, rpt_bf_transfer_insert_ws) vs the oracle,
bit-exact: after a call the filter's words are its words before the call plus orc.insert_keys of exactly the selected
rows, and its min/max is orc.minmax over the selected valid rows (test_gpu_transfer's Col.expect / check).

The destination's insert strategy is forced to PARTITIONED (AUTO's thresholds of 2-4 Mi rows are far above these
sizes) and checked to resolve to it. Shapes: n = 3 * 16384 + 5 (three full 16 Ki-row tiles and a tail; a full and a
part tile at tile multiple 2) plus 1, 513 and 16385; filters of 2^16 blocks (4 slices: the wave-aggregated counters),
2^18 (16 Ki-row tiles) and 2^22 (32 Ki-row tiles). Workspaces are exactly sized between guard bands and poisoned."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kernel_ledger as kl
import rpt_oracle as orc
from buf_util import (A5, CAPTURE_MODE_GLOBAL, FF, FilterCache, GuardedBuffer, graph_destroy, graph_instantiate,
                      graph_launch, hip_graph_api, stream_capture)
from test_gpu_kernel_ledger import make_col, row_ids_of
from test_gpu_transfer import (AUTO, DTYPES, GATHER, Col, Targets, bits_words, check, dev, graph_node_count, hits,
                               probed_column, rand_keys, sel_of)

pytestmark = pytest.mark.gpu

N = kl.N_TILES
LOGS = sorted(kl.PARTITION_SHAPES)  # 16, 18, 22
KINDS = [kl.DENSE, kl.DICT, kl.ROW_SEL, kl.MISALIGNED]
ATOMIC, PARTITIONED = kl.INS_ATOMIC, kl.INS_PARTITIONED
RPT_ERR_INVALID_ARGUMENT, RPT_ERR_WORKSPACE = 1, 4


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def targets(rpt):
    t = Targets(rpt)
    yield t
    t.close()


@pytest.fixture(scope="module")
def caches(rpt):
    a = FilterCache()
    yield a
    a.close()


def force(rpt, bf, strategy, n):
    from rpt_amd import _lib

    _lib.check(rpt.load().rpt_bf_set_insert_strategy(bf.handle, strategy))
    assert bf.insert_strategy_for(n) == strategy
    return bf


def target_in_state(rpt, targets, log_nb, state, n, rng):
    """(filter forced PARTITIONED, the words it holds, close it afterwards?) in one of the three states a slice merge
    tells apart: "pristine" (a fresh filter: plain stores), "prefilled" (words imported: adaptive), "cleared" (right
    after rpt_bf_clear, the zeroing still deferred: every slice stored whole)."""
    if state == "pristine":
        return force(rpt, rpt.BloomFilter(log_num_blocks=log_nb), PARTITIONED, n), orc.new_words(log_nb), True
    bf, base = targets.reset(log_nb, True)
    force(rpt, bf, PARTITIONED, n)
    if state == "cleared":
        bf.clear()
        base = orc.new_words(log_nb)
    return bf, base, False


STATES = ["pristine", "prefilled", "cleared"]


def guarded_ws(bf, n, pattern):
    return GuardedBuffer(int(bf._lib.rpt_bf_insert_workspace_bytes(bf.handle, n))).poison(pattern)


# ---- rows given as result bits -------------------------------------------------------------------------------------
PATTERNS = ["half", "none", "all", "dead_tile", "dead_first_32k", "dead_segments", "last", "half_ones_past_n"]


def pattern_mask(name, n, rng):
    m = rng.random(n) < 0.5
    if name == "none":
        m[:] = False
    elif name == "all":
        m[:] = True
    elif name == "dead_tile":  # the second 16 Ki-row tile, between two live ones
        m[16384:32768] = False
    elif name == "dead_first_32k":  # the whole first 32 Ki-row tile (two 16 Ki-row tiles), then live rows
        m[:32768] = False
    elif name == "dead_segments":  # every other 512-row segment of every tile
        for s in range(1, (n + 511) // 512, 2):
            m[s * 512: (s + 1) * 512] = False
    elif name == "last":
        m[:] = False
        m[n - 1] = True
    return m


@pytest.mark.parametrize("log_nb", LOGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kt", list(DTYPES))
def test_insert_bits_ws_patterns(rpt, targets, kt, kind, log_nb):
    """Every mask pattern on one column per (key type, row mapping, filter size); the target state rotates over the
    patterns so each pairing occurs across the cases. The column has 15 % NULL rows, selected ones among them."""
    seed = LOGS.index(log_nb) * 100 + KINDS.index(kind) * 10 + list(DTYPES).index(kt)
    rng = np.random.default_rng(seed)
    col, row_sel, d_row_sel = make_col(rng, kt, kind, N, rand_keys(np.int64, 4096, rng))
    ids = row_ids_of(row_sel, N)
    for idx, pattern in enumerate(PATTERNS):
        state = STATES[(idx + seed) % 3]
        bf, base, owned = target_in_state(rpt, targets, log_nb, state, N, rng)
        mask = pattern_mask(pattern.replace("_ones_past_n", ""), N, rng)
        bits = dev(bits_words(mask, ones_past_n=pattern.endswith("ones_past_n")))
        ws = guarded_ws(bf, N, A5 if idx % 2 else FF)
        bf.insert_bits_ws(col.d_keys, bits, n=N, row_sel=d_row_sel, workspace=ws.bytes(), **col.kwargs(rpt))
        exp = col.expect(base, log_nb, ids[mask])
        what = f"{pattern}, {state}"
        if pattern == "none":
            got = bf.export_words()
            assert np.array_equal(got, base), what
            assert bf.minmax() is None and not bf.is_empty(), what
        else:
            check(bf, exp, what)
        ws.assert_guards_intact(what)
        if pattern == "half" and kt != "hash":
            p = col.phys(ids[mask]).astype(np.int64)
            null = ((col.validity[p >> 6] >> (p & 63).astype(np.uint64)) & np.uint64(1)) == 0
            assert null.any() and not null.all(), "selected rows: some NULL, some not"
        if pattern == "all":  # ... equals rpt_bf_insert_ws of the same rows
            other = force(rpt, rpt.BloomFilter(log_num_blocks=log_nb), PARTITIONED, N)
            other.import_words(base)
            if row_sel is None:
                other.insert(col.d_keys, n=N, **col.kwargs(rpt))
                assert bf.is_same_as(other) and bf.minmax() == other.minmax()
            other.close()
        if owned:
            bf.close()


@pytest.mark.parametrize("log_nb", LOGS)
@pytest.mark.parametrize("n", [1, 513, 16385])
def test_insert_bits_ws_small_shapes(rpt, targets, n, log_nb):
    """One row, one segment and a row, one tile and a row: key type, row mapping and target state rotate."""
    i = [1, 513, 16385].index(n) + LOGS.index(log_nb)
    rng = np.random.default_rng(7000 + n + log_nb)
    for j, pattern in enumerate(["half", "all", "last", "none"]):
        kt, kind = list(DTYPES)[(i + j) % 3], KINDS[(i + j) % 4]
        col, row_sel, d_row_sel = make_col(rng, kt, kind, n, rand_keys(np.int64, 4096, rng))
        bf, base, owned = target_in_state(rpt, targets, log_nb, STATES[(i + j) % 3], n, rng)
        mask = pattern_mask(pattern, n, rng)
        ws = guarded_ws(bf, n, A5)
        bf.insert_bits_ws(col.d_keys, dev(bits_words(mask, ones_past_n=bool(j % 2))), n=n, row_sel=d_row_sel,
                          workspace=ws.bytes(), **col.kwargs(rpt))
        exp = col.expect(base, log_nb, row_ids_of(row_sel, n)[mask])
        assert np.array_equal(bf.export_words(), exp[0]), (pattern, kt, kind)
        assert bf.minmax() == exp[1] and not bf.is_empty(), (pattern, kt, kind)
        ws.assert_guards_intact(pattern)
        if owned:
            bf.close()


@pytest.mark.parametrize("log_nb", LOGS)
@pytest.mark.parametrize("kind", ["valid", "dict", "row_sel"])
@pytest.mark.parametrize("kt", ["i64", "i32"])
def test_insert_bits_ws_dead_and_null_rows_do_not_move_minmax(rpt, targets, kt, kind, log_nb):
    """Keys of the selected valid rows lie in [-1000, 1000]; the dead rows and the NULL rows hold the type's
    minimum and maximum."""
    rng = np.random.default_rng(37 + log_nb)
    n = N
    dtype = DTYPES[kt]
    rows = n + 1000 if kind == "row_sel" else n
    col = Col(rng, kt, "valid" if kind == "row_sel" else kind, rows)
    m = col.keys.size
    valid = ((col.validity[np.arange(m) >> 6] >> (np.arange(m) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if kind == "row_sel" else None
    mask = rng.random(n) < 0.5
    pos = np.flatnonzero(mask)
    sel_rows = row_sel[pos] if row_sel is not None else pos
    keep = np.zeros(m, dtype=bool)
    keep[col.phys(sel_rows)] = True
    keep &= valid
    extremes = np.where(rng.random(m) < 0.5, np.iinfo(dtype).min, np.iinfo(dtype).max).astype(dtype)
    col.keys = np.where(keep, rng.integers(-1000, 1001, m).astype(dtype), extremes)
    col.d_keys = dev(col.keys)
    bf, base = targets.reset(log_nb, False)
    force(rpt, bf, PARTITIONED, n)
    bf.insert_bits_ws(col.d_keys, dev(bits_words(mask)), n=n, row_sel=dev(row_sel), **col.kwargs(rpt))
    exp = col.expect(base, log_nb, sel_rows)
    assert exp[1] is not None and -1000 <= exp[1][0] <= exp[1][1] <= 1000
    check(bf, exp)


# ---- rows given as a selection vector with a device-side count ------------------------------------------------------
COUNTS = {"zero": lambda n: 0, "one": lambda n: 1, "inside_second_tile": lambda n: 16384 + 100,
          "max_rows": lambda n: n, "past_max_rows": lambda n: n + 100}


@pytest.mark.parametrize("log_nb", LOGS)
@pytest.mark.parametrize("count_kind", list(COUNTS))
def test_insert_sel_ws_counts(rpt, targets, count_kind, log_nb):
    """max_rows = n; the device count is 0, 1, a count that ends inside the second 16 Ki-row tile (the later tiles are
    wholly past it), max_rows, or max_rows + 100 (clamped). The entries of sel at and past the clamped count hold ids
    far outside the column: none of them may be read. Key type, column kind and target state rotate."""
    ci = list(COUNTS).index(count_kind)
    i = ci + LOGS.index(log_nb)
    rng = np.random.default_rng(9000 + 10 * log_nb + ci)
    n = N
    kt, kind = list(DTYPES)[i % 3], ["flat", "valid", "dict"][(i // 3 + ci) % 3]
    count = COUNTS[count_kind](n)
    used = min(count, n)
    rows = n + 100
    col = Col(rng, kt, kind, rows)
    sel = np.full(n, 0xFFFFFFF0, dtype=np.uint32)
    sel[:used] = rng.integers(0, rows, used)  # any order, repeats allowed
    g_sel = GuardedBuffer(4 * n)
    g_sel.view(torch.int32).copy_(dev(sel))
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda:0")
    results = []
    for pattern in (A5, FF):
        bf, base, owned = target_in_state(rpt, targets, log_nb, STATES[i % 3], n, rng)
        ws = guarded_ws(bf, n, pattern)
        bf.insert_sel_ws(col.d_keys, g_sel.view(torch.int32), d_count, max_rows=n, workspace=ws.bytes(), **col.kwargs(rpt))
        exp = col.expect(base, log_nb, sel[:used])
        got = bf.export_words()
        assert np.array_equal(got, exp[0]), f"{kt} {kind}, workspace {pattern}"
        assert bf.minmax() == exp[1] and not bf.is_empty()
        ws.assert_guards_intact("workspace")
        results.append(got)
        if owned:
            bf.close()
    assert np.array_equal(results[0], results[1])
    assert int(d_count.item()) == count
    g_sel.assert_guards_intact("sel")


# ---- workspace and strategy rules ------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_nb", LOGS)
def test_workspace_contents_do_not_matter_and_bad_workspaces_are_refused(rpt, targets, log_nb):
    from rpt_amd import RptError

    rng = np.random.default_rng(11 + log_nb)
    n = N
    col = Col(rng, "i64", "valid", n)
    mask = rng.random(n) < 0.5
    mask[16384:32768] = False  # a tile whose run-table row must be written as zeros over the poison
    bits = dev(bits_words(mask))
    bf, base = targets.reset(log_nb, True)
    force(rpt, bf, PARTITIONED, n)
    need = int(bf._lib.rpt_bf_insert_workspace_bytes(bf.handle, n))
    assert need > 0 and need % 256 == 0
    exp = col.expect(base, log_nb, np.flatnonzero(mask))
    for pattern in (A5, FF):
        bf, base = targets.reset(log_nb, True)
        ws = GuardedBuffer(need).poison(pattern)
        bf.insert_bits_ws(col.d_keys, bits, workspace=ws.bytes(), **col.kwargs(rpt))
        check(bf, exp, pattern)
        ws.assert_guards_intact(pattern)
    bf, base = targets.reset(log_nb, True)
    ws = GuardedBuffer(need + 256)
    count = torch.tensor([n], dtype=torch.int64, device="cuda:0")
    sel = dev(np.arange(n, dtype=np.uint32))
    calls = {
        "bits": lambda w: bf.insert_bits_ws(col.d_keys, bits, workspace=w, **col.kwargs(rpt)),
        "sel": lambda w: bf.insert_sel_ws(col.d_keys, sel, count, workspace=w, **col.kwargs(rpt)),
    }
    for name, call in calls.items():
        with pytest.raises(RptError) as e:
            call(ws.bytes()[: need - 1])
        assert e.value.status == RPT_ERR_WORKSPACE, name
        with pytest.raises(RptError) as e:
            call(ws.bytes()[8: 8 + need])
        assert e.value.status == RPT_ERR_INVALID_ARGUMENT and "aligned" in str(e.value), name
    torch.cuda.synchronize()
    assert bf.is_empty() and np.array_equal(bf.export_words(), base)  # a refused call has done nothing


def test_atomic_strategy_takes_todays_kernels_and_no_workspace(rpt, targets):
    """ATOMIC (and AUTO below the partitioned threshold) run insert_bits_kernel / insert_sel_kernel; a null workspace
    is fine then."""
    from rpt_amd import _lib

    rng = np.random.default_rng(13)
    n = N
    col = Col(rng, "i32", "valid", n)
    mask = rng.random(n) < 0.5
    lib = rpt.load()
    c = rpt.make_column(col.d_keys, **col.kwargs(rpt))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bits = dev(bits_words(mask))
    chosen = np.flatnonzero(mask).astype(np.uint32)
    d_chosen, d_count = dev(chosen), torch.tensor([chosen.size], dtype=torch.int64, device="cuda:0")
    for strategy in (ATOMIC, kl.AUTO):
        bf, base = targets.reset(18, True)
        _lib.check(lib.rpt_bf_set_insert_strategy(bf.handle, strategy))
        assert bf.insert_strategy_for(n) == ATOMIC
        assert lib.rpt_bf_insert_workspace_bytes(bf.handle, n) == 0
        torch.cuda.synchronize()
        _lib.profiling_reset()
        _lib.profiling(True)
        try:
            _lib.check(lib.rpt_bf_insert_bits_ws(bf.handle, ctypes.byref(c), None, n, bits.data_ptr(), None, 0, stream),
                       lib)
            torch.cuda.synchronize()
        finally:
            _lib.profiling(False)
        ran = _lib.kernel_times()
        _lib.profiling_reset()
        assert set(ran) == {"insert_bits_kernel<1,true>"}, ran
        check(bf, col.expect(base, 18, np.flatnonzero(mask)))
        bf, base = targets.reset(18, True)
        _lib.check(lib.rpt_bf_insert_sel_ws(bf.handle, ctypes.byref(c), d_chosen.data_ptr(), d_count.data_ptr(),
                                            chosen.size, None, 0, stream), lib)
        check(bf, col.expect(base, 18, chosen))


# ---- the fused call ----------------------------------------------------------------------------------------------------
def recorded(fn):
    """fn() with kernel profiling around it: {name: (launches, ms)}."""
    from rpt_amd import _lib

    torch.cuda.synchronize()
    _lib.profiling_reset()
    _lib.profiling(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.profiling(False)
    rec = _lib.kernel_times()
    _lib.profiling_reset()
    return rec


@pytest.mark.parametrize("use_row_sel", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2)])
@pytest.mark.parametrize("n", [16385, 40003])
def test_transfer_insert_ws_vs_oracle(rpt, caches, targets, n, shape, use_row_sel):
    """1-2 probed filters (the first forced to GATHER, so the workspace path runs) and 1-2 destinations: the first
    forced PARTITIONED (routed, from the accumulated bits), the second ATOMIC (insert_bits_kernel). Every destination
    equals the oracle's filter over the oracle's survivors; out_sel and the count equal rpt_bf_transfer_ws's."""
    k, n_dst = shape
    rng = np.random.default_rng(n * 3 + k + 10 * use_row_sel)
    order = [16, 13][:k]
    for L in order:
        caches.get(L)[0].probe_strategy = AUTO
    caches.get(16)[0].probe_strategy = GATHER
    filters = [caches.get(L)[0] for L in order]
    rows = n + n // 2 + 1 if use_row_sel else n
    cols, refs = zip(*[probed_column(rng, caches, L, rows) for L in order])
    exp = functools.reduce(np.intersect1d, refs)
    row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if use_row_sel else None
    if row_sel is not None:
        exp = np.intersect1d(exp, row_sel)
    exp = exp.astype(np.uint32)
    assert 0 < exp.size < n
    routed_log = LOGS[(n + k + use_row_sel) % 3]
    dst_specs = [("i64", "valid", routed_log, True, PARTITIONED), ("i32", "dict", 14, True, ATOMIC)][:n_dst]
    dst_cols = [Col(rng, kt, kind, rows) for kt, kind, _L, _p, _s in dst_specs]
    dst = [targets.reset(L, p, tag=j) for j, (_kt, _kind, L, p, _s) in enumerate(dst_specs)]
    for (bf, _b), spec in zip(dst, dst_specs):
        force(rpt, bf, spec[4], n)
    dst_filters = [bf for bf, _b in dst]
    need = rpt.probe_chain_workspace_bytes(filters, n)
    ineed = rpt.transfer_insert_workspace_bytes(dst_filters, n)
    assert ineed == int(dst_filters[0]._lib.rpt_bf_insert_workspace_bytes(dst_filters[0].handle, n)) > 0
    ws, iws = GuardedBuffer(need).poison(A5), GuardedBuffer(ineed).poison(FF)
    sel, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    col_args = [c.as_dict(rpt) for c in cols]
    dcol_args = [c.as_dict(rpt) for c in dst_cols]
    out = {}

    def call():
        out["r"] = rpt.transfer_insert_ws(filters, col_args, dst_filters, dcol_args, row_sel=dev(row_sel), n=n,
                                          out_sel=sel.view(torch.int32), out_count=cnt.view(torch.int64),
                                          workspace=ws.bytes(), insert_workspace=iws.bytes())

    ran = recorded(call)
    out_sel, out_count = out["r"]
    for (bf, base), c, spec in zip(dst, dst_cols, dst_specs):
        check(bf, c.expect(base, spec[2], exp), f"destination {spec}")
    assert int(out_count.item()) == exp.size
    assert np.array_equal(sel_of(out_sel[: exp.size]), exp)
    masked = [name for name in ran if name.startswith("partition_masked_kernel<0,%s,false," % kl.targ(not use_row_sel))]
    assert len(masked) == 1 and ran[masked[0]][0] == 1, ran
    assert ran["slice_insert_kernel"][0] == 1
    assert ("insert_bits_kernel<1,false>" in ran) == (n_dst == 2), ran
    for name, g in (("workspace", ws), ("insert workspace", iws), ("out_sel", sel), ("out_count", cnt)):
        g.assert_guards_intact(name)
    # rpt_bf_transfer_ws on the same inputs: the same selection vector and count, the same filters
    twins = [targets.reset(L, p, tag=10 + j) for j, (_kt, _kind, L, p, _s) in enumerate(dst_specs)]
    sel2, cnt2 = rpt.transfer_ws(filters, col_args, [bf for bf, _b in twins], dcol_args, row_sel=dev(row_sel), n=n)
    assert int(cnt2.item()) == exp.size and torch.equal(sel2[: exp.size], out_sel[: exp.size])
    for (bf, _b), (twin, _b2) in zip(dst, twins):
        assert bf.is_same_as(twin) and bf.minmax() == twin.minmax()
    caches.get(16)[0].probe_strategy = AUTO


def test_transfer_insert_ws_small_batch_hand_over_is_unchanged(rpt, caches, targets):
    """n = 2048 with every probed filter on AUTO: the one-launch chain, then insert_sel_kernel from out_sel for every
    destination, whatever its insert strategy; neither workspace is touched."""
    n = 2048
    rng = np.random.default_rng(2048)
    for L in (13, 16):
        caches.get(L)[0].probe_strategy = AUTO
    filters = [caches.get(13)[0], caches.get(16)[0]]
    cols, refs = zip(*[probed_column(rng, caches, L, n) for L in (13, 16)])
    exp = functools.reduce(np.intersect1d, refs).astype(np.uint32)
    assert 0 < exp.size < n
    specs = [("i64", "valid", 18, PARTITIONED), ("i32", "dict", 14, kl.AUTO)]
    dst_cols = [Col(rng, kt, kind, n) for kt, kind, _L, _s in specs]
    dst = [targets.reset(L, True, tag=j) for j, (_kt, _kind, L, _s) in enumerate(specs)]
    force(rpt, dst[0][0], PARTITIONED, n)
    dst[1][0]._lib.rpt_bf_set_insert_strategy(dst[1][0].handle, kl.AUTO)
    dst_filters = [bf for bf, _b in dst]
    ws = GuardedBuffer(rpt.probe_chain_workspace_bytes(filters, n)).poison(A5)
    iws = GuardedBuffer(rpt.transfer_insert_workspace_bytes(dst_filters, n)).poison(A5)
    out = {}
    ran = recorded(lambda: out.update(r=rpt.transfer_insert_ws(
        filters, [c.as_dict(rpt) for c in cols], dst_filters, [c.as_dict(rpt) for c in dst_cols], n=n,
        workspace=ws.bytes(), insert_workspace=iws.bytes())))
    assert set(ran) == {"probe_chain_small_kernel", "insert_sel_kernel<0>", "insert_sel_kernel<1>"}, ran
    assert all(ran[name][0] == 1 for name in ran), ran
    out_sel, out_count = out["r"]
    assert int(out_count.item()) == exp.size and np.array_equal(sel_of(out_sel[: exp.size]), exp)
    for (bf, base), c, spec in zip(dst, dst_cols, specs):
        check(bf, c.expect(base, spec[2], exp), f"destination {spec}")
    assert bool(torch.all(ws.bytes() == 0xA5)) and bool(torch.all(iws.bytes() == 0xA5))


# ---- capture ---------------------------------------------------------------------------------------------------------
def raw_transfer_insert(rpt, filters, cols, dst, dst_cols, n, out_sel, out_count, ws, iws, stream_handle):
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * len(filters))(*[f.handle for f in filters])
    dst_handles = (ctypes.c_void_p * len(dst))(*[f.handle for f in dst])
    return rpt.load().rpt_bf_transfer_insert_ws(handles, (KeyColumn * len(cols))(*cols), len(filters), dst_handles,
                                                (KeyColumn * len(dst_cols))(*dst_cols), len(dst), None, n,
                                                out_sel.data_ptr(), out_count.data_ptr(), ws.data_ptr(), ws.numel(),
                                                iws.data_ptr(), iws.numel(), stream_handle)


def test_transfer_insert_ws_graph_capture(rpt, caches):
    """One rpt_bf_transfer_insert_ws (20000 rows, the destination forced PARTITIONED) captured on a side stream under
    the global capture mode (torch's default) and replayed twice over new key contents in the same tensors: the
    destination ORs each replay's survivors (the slice merge uses atomics inside a capture) and folds their min/max.
    A destination with a clear pending is refused inside the capture before anything is enqueued."""
    n = 20000
    rng = np.random.default_rng(4700)
    f0, w0, b0 = caches.get(13)
    f1, w1, b1 = caches.get(16)
    f0.probe_strategy = AUTO
    f1.probe_strategy = AUTO
    k0, k1 = dev(hits(rng, b0, n, np.int64, 0.6)), dev(hits(rng, b1, n, np.int64, 0.6))
    dk = dev(rand_keys(np.int64, n, rng))
    cols = [rpt.make_column(k0), rpt.make_column(k1)]
    dcols = [rpt.make_column(dk)]
    out_sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(rpt.probe_chain_workspace_bytes([f0, f1], n), dtype=torch.uint8, device="cuda:0")
    log_nb = 18
    bf = force(rpt, rpt.BloomFilter(log_num_blocks=log_nb), PARTITIONED, n)
    iws = torch.empty(rpt.transfer_insert_workspace_bytes([bf], n), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    words, lo, hi = orc.new_words(log_nb), None, None

    def expect_one_more():
        nonlocal lo, hi
        surv = np.intersect1d(orc.probe_keys(w0, 13, k0.cpu().numpy()), orc.probe_keys(w1, 16, k1.cpu().numpy()))
        assert 0 < surv.size < n
        keys = dk.cpu().numpy()
        orc.insert_keys(words, log_nb, keys, key_sel=surv.astype(np.uint32))
        mn, mx = orc.minmax(keys, key_sel=surv.astype(np.uint32))
        lo, hi = (mn if lo is None else min(lo, mn)), (mx if hi is None else max(hi, mx))
        return surv

    # once outside any capture (a kernel's first launch sets its LDS allowance), on another stream than the captured one
    assert raw_transfer_insert(rpt, [f0, f1], cols, [bf], dcols, n, out_sel, out_count, ws, iws,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    expect_one_more()
    check(bf, (words, (lo, hi)), "before the capture")
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph,
                             lambda: raw_transfer_insert(rpt, [f0, f1], cols, [bf], dcols, n, out_sel, out_count, ws, iws, sh))
    assert end == 0 and st == 0, rpt.load().rpt_last_error()
    assert graph_instantiate(graph, exe) == 0
    for replay in range(2):
        k0.copy_(dev(hits(rng, b0, n, np.int64, 0.4 + 0.3 * replay)))
        k1.copy_(dev(hits(rng, b1, n, np.int64, 0.8 - 0.3 * replay)))
        dk.copy_(dev(rand_keys(np.int64, n, rng)))
        out_count.fill_(-1)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        surv = expect_one_more()
        assert int(out_count.item()) == surv.size
        assert np.array_equal(sel_of(out_sel[: surv.size]), surv.astype(np.uint32))
        check(bf, (words, (lo, hi)), f"replay {replay}")
    assert graph_destroy(exe, graph)
    # a deferred clear cannot be settled inside a capture: refused there, nothing enqueued, the filter not marked
    bf.clear()
    torch.cuda.synchronize()
    hip = hip_graph_api()
    graph = ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph,
                             lambda: raw_transfer_insert(rpt, [f0, f1], cols, [bf], dcols, n, out_sel, out_count, ws, iws, sh))
    assert end == 0
    assert st == RPT_ERR_INVALID_ARGUMENT and b"rpt_bf_settle" in rpt.load().rpt_last_error()
    assert graph_node_count(graph) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert bf.is_empty()
    bf.close()
