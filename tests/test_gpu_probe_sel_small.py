"""The one-launch device-counted probes (rpt_bf_probe_chain_sel, rpt_bf_transfer_sel) vs the oracle, bit-exact, and vs
the workspace calls they twin (rpt_bf_probe_chain_sel_ws, rpt_bf_transfer_sel_ws) on the same inputs: the rows probed
are sel[0 .. min(count, max_rows)), the count living on the device, max_rows at most RPT_SMALL_PROBE_ROWS.

The shapes are the smallest at which the single-workgroup kernel can go wrong: max_rows around one 512-position segment,
around 8192 (where its 16 waves go from one segment each to two) and the limit 16384; device counts around a segment,
around max_rows and far past it (clamped). Poison as in tests/test_gpu_probe_sel.py, whose helpers this file reuses:
sel[used:] holds in-range ids of rows that pass every filter (for the transfers: rows whose destination keys occur
nowhere else), so an entry read past the count shows up as extra survivors or extra filter bits, never as a fault."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import rpt_oracle as orc
from buf_util import (CAPTURE_MODE_GLOBAL, FF, FilterCache, GuardedBuffer, graph_destroy, graph_instantiate, graph_launch,
                      hip_graph_api, stream_capture)
from test_gpu_probe_sel import (build_chain, count_of, device_count, dst_col, expected, poisoned_sel, probed_col,
                                row_pass_mask)
from test_gpu_transfer import Col, Targets, check, dev, graph_node_count, hits, rand_keys, sel_of

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED = 0, 1, 2, 3
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
MAX_ROWS = [1, 511, 512, 513, 8191, 8192, 8193, 16384]
COUNTS = ["0", "1", "511", "512", "513", "max_rows-1", "max_rows", "max_rows+100", str(2**40)]
# Chains of 1, 2, 3 and 8 filters of 2^11 .. 2^18 blocks: (log2 blocks, forced probe strategy, which the one-launch
# kernel ignores: it gathers every filter), and the fraction of each column's keys drawn from the filter's build keys
# (the 8-filter chain needs more hits per filter to leave survivors).
CHAINS = [
    ([(16, AUTO)], 0.8),
    ([(11, AUTO), (18, PARTITIONED)], 0.8),
    ([(13, LDS), (16, GATHER), (12, AUTO)], 0.8),
    ([(16, AUTO), (13, AUTO), (15, LDS), (18, AUTO), (11, AUTO), (14, AUTO), (17, LDS), (12, GATHER)], 0.97),
]


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def pools(rpt):
    made = (FilterCache(), FilterCache())
    yield made
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def targets(rpt):
    t = Targets(rpt)
    yield t
    t.close()


@pytest.fixture(autouse=True)
def strategies_back_to_auto(pools):
    yield
    for c in pools:
        for bf, _w, _k in c._made.values():
            bf.probe_strategy = AUTO


def rows_for(max_rows):
    return max(max_rows + 1000, 4096)


class Out:
    """out_sel of exactly max_rows entries and the 8-byte count, between guard bands and holding garbage."""

    def __init__(self, max_rows):
        self.sel = GuardedBuffer(4 * max_rows).poison(FF)
        self.cnt = GuardedBuffer(8).poison(FF)

    def outputs(self):
        return dict(out_sel=self.sel.view(torch.int32), out_count=self.cnt.view(torch.int64))

    def count(self):
        return int(self.cnt.view(torch.int64).item())

    def assert_intact(self, count, count_guarded=True):
        self.sel.assert_guards_intact("out_sel")
        if count_guarded:
            self.cnt.assert_guards_intact("out_count")
        assert bool(torch.all(self.sel.view(torch.int32)[count:] == -1)), "out_sel written past the returned count"


def ws_for(rpt, filters, max_rows):
    return torch.empty(rpt.probe_chain_sel_workspace_bytes(filters, max_rows), dtype=torch.uint8, device="cuda:0")


# ---- the chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_name", COUNTS)
@pytest.mark.parametrize("max_rows", MAX_ROWS)
def test_probe_chain_sel_vs_oracle_and_the_workspace_call(rpt, pools, max_rows, count_name):
    """Every (max_rows, device count) pair; the chain (1, 2, 3 or 8 filters), the key types, the column kinds and the
    order of sel (ascending, or any order with repeats) rotate over the pairs so that each occurs."""
    mi, ci = MAX_ROWS.index(max_rows), COUNTS.index(count_name)
    case = mi * len(COUNTS) + ci
    rng = np.random.default_rng(9000 + case)
    spec, frac = CHAINS[(ci + mi) % len(CHAINS)]
    chain = build_chain(rpt, rng, pools, spec, rows_for(max_rows), rot=case, frac=frac)
    count = count_of(count_name, max_rows)
    used = min(count, max_rows)
    sel = poisoned_sel(rng, max_rows, used, chain.alive, ascending=case % 2 == 0)
    exp = expected(sel, used, chain.alive)
    out = Out(max_rows)
    d_sel, d_count = dev(sel), device_count(count)
    out_sel, out_count = rpt.probe_chain_sel(chain.filters, chain.args, d_sel, d_count, max_rows=max_rows, **out.outputs())
    got = int(out_count.item())
    print(f"max_rows {max_rows} count {count} chain {spec}: {got} of {used} survive (oracle {exp.size})")
    assert got == exp.size
    assert np.array_equal(sel_of(out_sel[:got]), exp)
    out.assert_intact(got)
    assert int(d_count.item()) == count and np.array_equal(sel_of(d_sel), sel)  # the inputs are only read
    if used >= 512:
        assert 0 < exp.size < used  # the filters discriminate
    # ... and the workspace call returns the same on the same inputs
    twin = Out(max_rows)
    rpt.probe_chain_sel_ws(chain.filters, chain.args, d_sel, d_count, max_rows=max_rows,
                           workspace=ws_for(rpt, chain.filters, max_rows), **twin.outputs())
    assert twin.count() == got
    assert np.array_equal(sel_of(twin.sel.view(torch.int32)[:got]), sel_of(out_sel[:got]))


def test_eight_filter_chain_leaves_survivors_at_every_size(rpt, pools):
    """The 8-filter chain's hit fraction is chosen so that the oracle leaves survivors: checked here for the shapes of
    the parametrised test that use it, so a 0 there is never an empty chain."""
    spec, frac = CHAINS[3]
    for max_rows in (512, 8192, 16384):
        rng = np.random.default_rng(max_rows)
        chain = build_chain(rpt, rng, pools, spec, rows_for(max_rows), rot=max_rows, frac=frac)
        share = chain.alive.mean()
        assert 0.05 < share < 0.95, share


def test_count_may_be_overwritten_in_place(rpt, pools):
    """out_count is count itself, at max_rows = count = 16384: every wave holds two segments and is busy when thread 0
    writes the survivors' count. Every thread has read the count before the kernel's first barrier."""
    rng = np.random.default_rng(101)
    max_rows = SMALL_ROWS
    spec, frac = CHAINS[2]
    chain = build_chain(rpt, rng, pools, spec, rows_for(max_rows), rot=4, frac=frac)
    sel = poisoned_sel(rng, max_rows, max_rows, chain.alive)
    exp = expected(sel, max_rows, chain.alive)
    assert 0 < exp.size < max_rows
    for _ in range(3):
        out = Out(max_rows)
        d_count = device_count(max_rows)
        out_sel, out_count = rpt.probe_chain_sel(chain.filters, chain.args, dev(sel), d_count, max_rows=max_rows,
                                                 out_sel=out.sel.view(torch.int32), out_count=d_count)
        assert out_count.data_ptr() == d_count.data_ptr()
        assert int(d_count.item()) == exp.size
        assert np.array_equal(sel_of(out_sel[: exp.size]), exp)
        out.assert_intact(exp.size, count_guarded=False)
    # ... and with a count of 0 stored over itself
    d_count = device_count(0)
    out = Out(max_rows)
    rpt.probe_chain_sel(chain.filters, chain.args, dev(sel), d_count, max_rows=max_rows, out_sel=out.sel.view(torch.int32),
                        out_count=d_count)
    assert int(d_count.item()) == 0
    out.assert_intact(0, count_guarded=False)


def test_result_does_not_depend_on_filter_order(rpt, pools):
    rng = np.random.default_rng(11)
    max_rows, used = 8193, 8000
    spec, frac = CHAINS[2]
    chain = build_chain(rpt, rng, pools, spec, rows_for(max_rows), rot=1, frac=frac)
    sel = poisoned_sel(rng, max_rows, used, chain.alive)
    exp = expected(sel, used, chain.alive)
    assert 0 < exp.size < used
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        out = Out(max_rows)
        out_sel, out_count = rpt.probe_chain_sel([chain.filters[i] for i in order], [chain.args[i] for i in order],
                                                 dev(sel), device_count(used), max_rows=max_rows, **out.outputs())
        assert int(out_count.item()) == exp.size and np.array_equal(sel_of(out_sel[: exp.size]), exp), order
        out.assert_intact(exp.size)


def test_zero_max_rows_only_sets_the_count(rpt, pools, targets):
    from rpt_amd._lib import KeyColumn

    rng = np.random.default_rng(19)
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    lib = rpt.load()
    handles = (ctypes.c_void_p * 1)(chain.filters[0].handle)
    arr = (KeyColumn * 1)(rpt.make_column(**chain.args[0]))
    cnt = GuardedBuffer(8).poison(FF)
    stream = torch.cuda.current_stream().cuda_stream
    d_count = device_count(5)
    assert lib.rpt_bf_probe_chain_sel(handles, arr, 1, None, d_count.data_ptr(), 0, None, cnt.ptr, stream) == 0
    assert int(cnt.view(torch.int64).item()) == 0
    cnt.assert_guards_intact("out_count")
    bf, base = targets.reset(14, True)
    dst = (ctypes.c_void_p * 1)(bf.handle)
    cnt.poison(FF)
    st = lib.rpt_bf_transfer_sel(handles, arr, 1, dst, arr, 1, None, d_count.data_ptr(), 0, None, cnt.ptr, stream)
    assert st == 0, lib.rpt_last_error()
    assert int(cnt.view(torch.int64).item()) == 0
    assert bf.is_empty() and np.array_equal(bf.export_words(), base)  # no destination is touched


def test_max_rows_past_the_limit_is_refused(rpt, pools):
    rng = np.random.default_rng(23)
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    n = SMALL_ROWS + 1
    sel, out_sel = torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_count = device_count(-1)
    with pytest.raises(rpt.RptError) as e:
        rpt.probe_chain_sel(chain.filters, chain.args, sel, device_count(10), out_sel=out_sel, out_count=out_count)
    assert e.value.status == 1 and "exceeds RPT_SMALL_PROBE_ROWS" in str(e.value)
    torch.cuda.synchronize()
    assert int(out_count.item()) == -1 and bool(torch.all(out_sel == -1))


# ---- the transfer ---------------------------------------------------------------------------------------------------
def combine_minmax(a, b):
    if a is None or b is None:
        return a if b is None else b
    return min(a[0], b[0]), max(a[1], b[1])


def all_null_except(col, keep_rows):
    """Every row of the column NULL except keep_rows (the poison rows, which must stay valid to be seen)."""
    assert col.validity is not None
    col.validity[:] = 0
    phys = col.phys(keep_rows)
    np.bitwise_or.at(col.validity, phys >> 6, np.uint64(1) << (phys & 63).astype(np.uint64))
    col.d_validity = dev(col.validity)


def transfer_case(rpt, rng, pools, targets, spec, frac, max_rows, count, dst_specs, null_dst=None, no_survivor=False):
    """One rpt_bf_transfer_sel against the oracle and against rpt_bf_transfer_sel_ws into twin filters. dst_specs:
    (key type, column kind, log2 blocks, pre-filled, slot) per destination; two entries with one slot are the same
    filter listed twice. Returns the survivors."""
    rows = rows_for(max_rows)
    used = min(count, max_rows)
    chain = build_chain(rpt, rng, pools, spec, rows, rot=len(dst_specs), frac=frac)
    passing = np.flatnonzero(chain.alive)
    poison_rows = np.sort(rng.choice(passing, size=min(32, passing.size), replace=False))
    sel = poisoned_sel(rng, max_rows, used, chain.alive, avoid=poison_rows)
    if no_survivor:  # positions below the count hold only rows that some filter rejects
        dead = np.flatnonzero(~chain.alive)
        sel[:used] = dead[rng.integers(0, dead.size, used)]
    exp = expected(sel, used, chain.alive)
    dst_cols = [dst_col(rng, kt, kind, rows, poison_rows) for kt, kind, _L, _p, _s in dst_specs]
    if null_dst is not None:
        all_null_except(dst_cols[null_dst], poison_rows)
    slots = {}
    for _kt, _kind, L, p, slot in dst_specs:
        if slot not in slots:
            slots[slot] = (L, targets.reset(L, p, tag=slot), targets.reset(L, p, tag=100 + slot))
    dst = [slots[s[4]][1][0] for s in dst_specs]
    twins = [slots[s[4]][2][0] for s in dst_specs]
    dargs = [c.as_dict(rpt) for c in dst_cols]
    out = Out(max_rows)
    d_sel, d_count = dev(sel), device_count(count)
    out_sel, out_count = rpt.transfer_sel(chain.filters, chain.args, dst, dargs, d_sel, d_count, max_rows=max_rows,
                                          **out.outputs())
    got = int(out_count.item())
    assert got == exp.size
    assert np.array_equal(sel_of(out_sel[:got]), exp)
    out.assert_intact(got)
    assert int(d_count.item()) == count and np.array_equal(sel_of(d_sel), sel)
    twin_out = Out(max_rows)
    rpt.transfer_sel_ws(chain.filters, chain.args, twins, dargs, d_sel, d_count, max_rows=max_rows,
                        workspace=ws_for(rpt, chain.filters, max_rows), **twin_out.outputs())
    assert twin_out.count() == got
    for slot, (L, (bf, base), (twin, _base)) in slots.items():
        words, mm = base, None
        for c, s in zip(dst_cols, dst_specs):
            if s[4] == slot:
                words, m = c.expect(words, L, exp)
                mm = combine_minmax(mm, m)
        check(bf, (words, mm), f"destination slot {slot}")  # words, min/max, has_data
        assert np.array_equal(twin.export_words(), bf.export_words()), slot
        assert twin.minmax() == bf.minmax() and not twin.is_empty(), slot
    return exp


EIGHT_DST = [("i64", "flat", 17, False, 0), ("i32", "dict", 14, True, 1), ("hash", "valid", 12, True, 2),
             ("i64", "valid", 11, False, 3), ("i32", "flat", 16, True, 4), ("hash", "dict", 13, False, 5),
             ("i64", "dict", 15, True, 6), ("i32", "valid", 10, False, 7)]


@pytest.mark.parametrize("n_dst", [1, 2, 8])
@pytest.mark.parametrize("max_rows,count", [(513, 512), (8193, 8193 + 100), (16384, 16383)])
def test_transfer_sel_vs_oracle_and_the_workspace_call(rpt, pools, targets, max_rows, count, n_dst):
    """1, 2 and 8 destinations of every key type and column kind, pre-filled (the earlier bits survive) and empty: the
    words and the min/max equal the oracle's over the oracle's survivors and the workspace call's; out_sel and the
    count as for the chain alone."""
    rng = np.random.default_rng(max_rows * 8 + n_dst)
    spec, frac = CHAINS[(max_rows + n_dst) % 3]
    dst_specs = EIGHT_DST[:n_dst] if n_dst != 2 else EIGHT_DST[1:3]  # 2: an int32 dictionary and a HASH destination
    exp = transfer_case(rpt, rng, pools, targets, spec, frac, max_rows, count, dst_specs)
    assert 0 < exp.size < min(count, max_rows)


def test_transfer_sel_through_the_eight_filter_chain(rpt, pools, targets):
    rng = np.random.default_rng(53)
    spec, frac = CHAINS[3]
    exp = transfer_case(rpt, rng, pools, targets, spec, frac, 8192, 8000, EIGHT_DST[2:4])
    assert 0 < exp.size < 8000


def test_one_destination_listed_twice_with_two_columns(rpt, pools, targets):
    """The same filter as destination 0 and 2, on an int64 and an int32 column: it receives both columns' keys (and
    both min/max), locked, waited for and recorded once."""
    rng = np.random.default_rng(59)
    spec, frac = CHAINS[1]
    dst_specs = [("i64", "valid", 14, True, 0), ("hash", "flat", 12, False, 1), ("i32", "dict", 14, True, 0)]
    exp = transfer_case(rpt, rng, pools, targets, spec, frac, 8192, 7000, dst_specs)
    assert 0 < exp.size < 7000


def test_selected_null_rows_insert_null_hash_and_leave_no_minmax(rpt, pools, targets):
    """A destination whose selected rows are all NULL: NULL_HASH's bits and has_value == 0; a second destination on the
    same call keeps its min/max."""
    rng = np.random.default_rng(61)
    spec, frac = CHAINS[0]
    dst_specs = [("i64", "valid", 13, False, 0), ("i32", "valid", 13, True, 1)]
    exp = transfer_case(rpt, rng, pools, targets, spec, frac, 1543, 1500, dst_specs, null_dst=0)
    assert exp.size > 0
    bf = targets._made[(13, False, 0)][0]
    null_only = orc.new_words(13)
    orc.insert_hashes(null_only, 13, np.array([0xBF58476D1CE4E5B9], dtype=np.uint64))  # NULL_HASH
    assert np.array_equal(bf.export_words(), null_only) and bf.minmax() is None
    assert targets._made[(13, True, 1)][0].minmax() is not None


@pytest.mark.parametrize("how", ["count_zero", "nothing_passes"])
def test_an_empty_selection_leaves_has_data_set_and_the_words_unchanged(rpt, pools, targets, how):
    rng = np.random.default_rng(67 + len(how))
    spec, frac = CHAINS[1]
    dst_specs = [("i64", "flat", 16, True, 0), ("i32", "dict", 12, False, 1)]
    exp = transfer_case(rpt, rng, pools, targets, spec, frac, 2048, 0 if how == "count_zero" else 2000, dst_specs,
                        no_survivor=how == "nothing_passes")
    assert exp.size == 0  # transfer_case's check(): words = base, no min/max, is_empty() False


# ---- capture --------------------------------------------------------------------------------------------------------
def raw_probe_chain(rpt, bf, col, n, out_sel, out_count, stream_handle):
    """rpt_bf_probe_chain through ctypes: nothing but the call (the Python wrapper reads the count back)."""
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * 1)(bf.handle)
    arr = (KeyColumn * 1)(col)
    st = rpt.load().rpt_bf_probe_chain(handles, arr, 1, None, n, out_sel.data_ptr(), out_count.data_ptr(), stream_handle)
    assert st == 0, rpt.load().rpt_last_error()


def test_backward_step_of_one_vector_is_one_graph(rpt, pools):
    """probe -> rpt_bf_transfer_sel -> rpt_bf_probe_chain_sel for one 2048-row vector, captured under
    hipStreamCaptureModeGlobal (a synchronize, an allocation or a copy to the host would invalidate the capture) and
    replayed twice over other keys, i.e. other device counts and other sel contents: three kernels, the counts never
    on the host. The destination ORs every run's survivors."""
    n = 2048
    rng = np.random.default_rng(71)
    (f1, w1, b1), (f2, w2, b2), (f3, w3, b3) = pools[0].get(13), pools[0].get(16), pools[1].get(11)
    k1, k2, k3 = (dev(hits(rng, b, n, np.int64, 0.7)) for b in (b1, b2, b3))
    dk = dev(rand_keys(np.int64, n, rng))
    i32, i64 = torch.int32, torch.int64
    sel1, cnt1, sel2, cnt2, sel3, cnt3 = (GuardedBuffer(nb).poison(FF) for nb in (4 * n, 8, 4 * n, 8, 4 * n, 8))
    dst = rpt.BloomFilter(log_num_blocks=13)
    words, mm = orc.new_words(13), None

    def step(stream):
        sh = ctypes.c_void_p(stream.cuda_stream)
        raw_probe_chain(rpt, f1, rpt.make_column(k1), n, sel1.view(i32), cnt1.view(i64), sh)
        rpt.transfer_sel([f2], [k2], [dst], [dk], sel1.view(i32), cnt1.view(i64), out_sel=sel2.view(i32),
                         out_count=cnt2.view(i64), stream=stream)
        rpt.probe_chain_sel([f3], [k3], sel2.view(i32), cnt2.view(i64), out_sel=sel3.view(i32), out_count=cnt3.view(i64),
                            stream=stream)

    def check_against_oracle(what):
        nonlocal mm
        e1 = orc.probe_keys(w1, 13, k1.cpu().numpy()).astype(np.uint32)
        e2 = e1[orc.probe_keys(w2, 16, k2.cpu().numpy(), key_sel=e1)]
        e3 = e2[orc.probe_keys(w3, 11, k3.cpu().numpy(), key_sel=e2)]
        assert 0 < e3.size < e2.size < e1.size < n, what
        orc.insert_keys(words, 13, dk.cpu().numpy(), key_sel=e2)
        mm = combine_minmax(mm, orc.minmax(dk.cpu().numpy(), key_sel=e2))
        for name, e, s, c in (("sel1", e1, sel1, cnt1), ("sel2", e2, sel2, cnt2), ("sel3", e3, sel3, cnt3)):
            got = int(c.view(i64).item())
            assert got == e.size, f"{what}: {name} count {got}, oracle {e.size}"
            assert np.array_equal(sel_of(s.view(i32)[:got]), e), f"{what}: {name}"
            assert bool(torch.all(s.view(i32)[got:] == -1)), f"{what}: {name} written past its count"
            s.assert_guards_intact(name)
            c.assert_guards_intact(name + " count")
        check(dst, (words, mm), what)
        return e1.size, e2.size, e3.size

    # eagerly on the current stream first, not the one captured below: the capture asks whether the destination's
    # previous write has completed by querying the event recorded on that write's stream
    step(torch.cuda.current_stream())
    torch.cuda.synchronize()
    counts = [check_against_oracle("eager")]
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _none = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: step(s))
    assert end == 0, "the capture was invalidated: something in the step synchronized, allocated or copied back"
    assert graph_node_count(graph) == 3
    assert graph_instantiate(graph, exe) == 0
    for replay, frac in enumerate((0.9, 0.4)):
        k1.copy_(dev(hits(rng, b1, n, np.int64, frac)))
        k2.copy_(dev(hits(rng, b2, n, np.int64, 0.6)))
        dk.copy_(dev(rand_keys(np.int64, n, rng)))
        for g in (sel1, cnt1, sel2, cnt2, sel3, cnt3):
            g.poison(FF)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        counts.append(check_against_oracle(f"replay {replay}"))
    assert len(set(counts)) == 3  # other keys, other counts
    assert graph_destroy(exe, graph)
    dst.close()


@pytest.mark.parametrize("cleared", ["probed", "destination"])
def test_pending_clear_is_refused_inside_a_capture(rpt, pools, cleared):
    """A deferred clear cannot be settled inside a capture: a cleared probed filter refuses both calls and a cleared
    destination the transfer, before anything is enqueued (the captured graph has no node, the destination is not
    marked); outside a capture the same calls settle it."""
    rng = np.random.default_rng(73)
    max_rows, used = 2048, 1500
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    bf = rpt.BloomFilter(log_num_blocks=12)
    bf.insert(dev(np.arange(100, dtype=np.int64)))
    bf.clear()
    other = rpt.BloomFilter(log_num_blocks=12)
    torch.cuda.synchronize()
    col = probed_col(rng, "i64", "flat", 4096, pools[0].get(13)[2])
    if cleared == "probed":
        filters, args, dst = chain.filters + [bf], chain.args + [col.as_dict(rpt)], other
    else:
        filters, args, dst = chain.filters, chain.args, bf
    d_sel, d_count = dev(poisoned_sel(rng, max_rows, used, chain.alive)), device_count(used)
    out = Out(max_rows)
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)

    def call_chain():
        return rpt.probe_chain_sel(filters, args, d_sel, d_count, max_rows=max_rows, stream=s, **out.outputs())

    def call_transfer():
        return rpt.transfer_sel(filters, args, [dst], [col.as_dict(rpt)], d_sel, d_count, max_rows=max_rows, stream=s,
                                **out.outputs())

    def caught(call):
        try:
            call()
        except rpt.RptError as e:
            return e
        return None

    for call in ([call_chain, call_transfer] if cleared == "probed" else [call_transfer]):
        graph = ctypes.c_void_p()
        end, err = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: caught(call))
        assert end == 0
        assert err is not None and err.status == 1 and "rpt_bf_settle" in str(err)
        assert graph_node_count(graph) == 0
        assert hip_graph_api().hipGraphDestroy(graph) == 0
        assert dst.is_empty()  # a refused call has not marked the destination either
    s.synchronize()
    assert out.count() == -1 and bool(torch.all(out.sel.view(torch.int32) == -1))
    assert caught(call_transfer) is None
    s.synchronize()
    exp = expected(sel_of(d_sel), used, chain.alive) if cleared == "destination" else np.empty(0, dtype=np.uint32)
    assert out.count() == exp.size  # nothing passes the cleared (now settled, empty) probed filter
    out.assert_intact(exp.size)
    words, mm = col.expect(orc.new_words(12), 12, exp)
    check(dst, (words, mm), cleared)
    bf.close()
    other.close()


# ---- write order ----------------------------------------------------------------------------------------------------
def test_two_threads_listing_the_same_destinations_in_opposite_orders(rpt, pools):
    """Two host threads, each with a stream of its own, call rpt_bf_transfer_sel 50 times into the same two
    destinations, listed in opposite orders: the write scopes are taken in ascending handle address, so both finish
    (joined with a timeout: a lock-order inversion fails the test instead of hanging it), and the destinations hold the
    union of both threads' survivors."""
    rng = np.random.default_rng(79)
    max_rows, used, calls = 2048, 1800, 50
    rows = rows_for(max_rows)
    chain = build_chain(rpt, rng, pools, [(13, AUTO), (16, AUTO)], rows)
    d0, d1 = rpt.BloomFilter(log_num_blocks=12), rpt.BloomFilter(log_num_blocks=14)
    c0, c1 = Col(rng, "i64", "valid", rows), Col(rng, "i32", "dict", rows)
    work = []
    for t in range(2):
        sel = poisoned_sel(rng, max_rows, used, chain.alive)
        order = [(d0, c0), (d1, c1)] if t == 0 else [(d1, c1), (d0, c0)]
        work.append(dict(sel=sel, d_sel=dev(sel), d_count=device_count(used), out=Out(max_rows),
                         stream=torch.cuda.Stream(device="cuda:0"), dst=[d for d, _c in order],
                         dargs=[c.as_dict(rpt) for _d, c in order], error=None))
    torch.cuda.synchronize()

    def run(w):
        try:
            for _ in range(calls):
                rpt.transfer_sel(chain.filters, chain.args, w["dst"], w["dargs"], w["d_sel"], w["d_count"],
                                 max_rows=max_rows, stream=w["stream"], **w["out"].outputs())
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            w["error"] = e

    threads = [threading.Thread(target=run, args=(w,), daemon=True) for w in work]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads), "a thread is still inside rpt_bf_transfer_sel: lock-order deadlock"
    assert [w["error"] for w in work] == [None, None]
    torch.cuda.synchronize()
    w0, w1, mm0, mm1 = orc.new_words(12), orc.new_words(14), None, None
    for w in work:
        exp = expected(w["sel"], used, chain.alive)
        assert 0 < exp.size < used
        assert w["out"].count() == exp.size
        assert np.array_equal(sel_of(w["out"].sel.view(torch.int32)[: exp.size]), exp)
        w["out"].assert_intact(exp.size)
        w0, m = c0.expect(w0, 12, exp)
        mm0 = combine_minmax(mm0, m)
        w1, m = c1.expect(w1, 14, exp)
        mm1 = combine_minmax(mm1, m)
    check(d0, (w0, mm0), "destination 0")
    check(d1, (w1, mm1), "destination 1")
    d0.close()
    d1.close()
