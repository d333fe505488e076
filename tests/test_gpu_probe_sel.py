"""The device-counted probes (rpt_bf_probe_chain_sel_ws, rpt_bf_transfer_sel_ws, rpt_bf_transfer_insert_sel_ws) vs the
oracle, bit-exact: the rows probed are sel[0 .. min(count, max_rows)), the count living on the device. The expected
selection is orc.probe_keys per filter over the table's rows, intersected, taken at sel[:used] in position order; it
also equals what rpt_bf_probe_chain_ws(row_sel = sel, n = used) returns on the same buffers.

Poison: sel[used:] holds in-range ids of rows whose keys pass every filter of the chain (and, for the transfers, whose
destination keys occur nowhere else in the destination column), so an entry read past the count shows up as extra
survivors or extra filter bits, never as a fault. Outputs and workspaces are exactly sized GuardedBuffers holding
garbage on entry. The probed filters come from buf_util.FilterCache and are never inserted into."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import kernel_ledger as kl
import rpt_oracle as orc
from buf_util import (A5, CAPTURE_MODE_GLOBAL, FF, RAMP, FilterCache, GuardedBuffer, graph_destroy, graph_instantiate,
                      graph_launch, stream_capture)
from test_gpu_kernel_ledger import probe_ref
from test_gpu_transfer import Col, Targets, check, dev, hits, raw_chain_ws, sel_of

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED, BUCKETED = 0, 1, 2, 3, 4
INS_AUTO, INS_PARTITIONED = 0, 2
MAX_ROWS = [1, 513, 1543, 40003]
COUNTS = ["0", "1", "511", "512", "513", "max_rows-1", "max_rows", "max_rows+100"]
KTS = ["i64", "i32", "hash"]
KINDS = ["flat", "valid", "dict"]
# Chains, first stage first: (log2 blocks, forced strategy). 2^16 GATHER: the gather; 2^13: whole filter in LDS;
# 2^15 .. 2^17 LDS: the hybrid; 2^18 PARTITIONED: demoted to the gather.
CHAINS = [
    [(16, GATHER)],
    [(13, LDS)],
    [(16, LDS)],
    [(16, GATHER), (13, AUTO)],
    [(13, AUTO), (16, LDS)],
    [(16, LDS), (16, GATHER), (11, AUTO)],
    [(18, PARTITIONED), (13, AUTO), (18, PARTITIONED)],
    [(16, GATHER), (13, AUTO), (15, LDS), (18, PARTITIONED), (11, AUTO), (14, AUTO), (17, LDS), (12, GATHER)],
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
    """Two filters per size, so a chain can hold one size twice with different strategies."""
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


def probed_col(rng, kt, kind, rows, build, frac=0.8):
    """A column of `rows` rows of which about `frac` (less the NULLs) pass the filter built from `build`."""
    m = rows // 2 + 1 if kind == "dict" else rows
    keys = hits(rng, build, m, np.int32 if kt == "i32" else np.int64, frac)
    if kt == "hash":
        keys = orc.hash_keys(keys)
    return Col(rng, kt, kind, rows, keys=keys,
               key_sel=rng.integers(0, m, rows).astype(np.uint32) if kind == "dict" else None)


def row_pass_mask(col, words, log_nb):
    m = np.zeros(col.rows, dtype=bool)
    m[probe_ref(col, words, log_nb, np.arange(col.rows, dtype=np.uint32))] = True
    return m


Chain = collections.namedtuple("Chain", "filters cols args alive")


def build_chain(rpt, rng, pools, spec, rows, rot=0, frac=0.8):
    """The chain's filters with their strategies forced, one column of `rows` rows per filter (key types and column
    kinds rotate with rot), and alive[r]: row r passes every filter, by the oracle."""
    filters, cols = [], []
    alive = np.ones(rows, dtype=bool)
    seen = collections.Counter()
    for i, (log_nb, strategy) in enumerate(spec):
        bf, words, build = pools[seen[log_nb]].get(log_nb)
        seen[log_nb] += 1
        bf.probe_strategy = strategy
        col = probed_col(rng, KTS[(rot + i) % 3], KINDS[(rot // 3 + i) % 3], rows, build, frac)
        alive &= row_pass_mask(col, words, log_nb)
        filters.append(bf)
        cols.append(col)
    return Chain(filters, cols, [c.as_dict(rpt) for c in cols], alive)


def poisoned_sel(rng, max_rows, used, alive, ascending=False, avoid=None):
    """max_rows ids: sel[:used] any rows (ascending without repeats, or any order with repeats; never a row of
    `avoid`), sel[used:] rows that pass every filter (drawn from `avoid` when given: the poison rows)."""
    rows = alive.size
    poison = np.flatnonzero(alive) if avoid is None else np.asarray(avoid)
    assert poison.size, "no row passes the whole chain: nothing to poison with"
    pool = np.arange(rows) if avoid is None else np.setdiff1d(np.arange(rows), avoid)
    sel = np.empty(max_rows, dtype=np.uint32)
    sel[:used] = np.sort(rng.choice(pool, size=used, replace=False)) if ascending else pool[rng.integers(0, pool.size, used)]
    sel[used:] = poison[rng.integers(0, poison.size, max_rows - used)]
    return sel


def expected(sel, used, alive):
    s = sel[:used]
    return s[alive[s]]


def count_of(name, max_rows):
    named = {"max_rows-1": max_rows - 1, "max_rows": max_rows, "max_rows+100": max_rows + 100}
    return named[name] if name in named else int(name)


class Buffers:
    """out_sel of exactly max_rows entries, the count and the workspace of exactly the documented bytes, all between
    guard bands and holding garbage."""

    def __init__(self, rpt, filters, max_rows, ws_poison=A5):
        self.need = rpt.probe_chain_sel_workspace_bytes(filters, max_rows)
        assert self.need > 0 and self.need % 256 == 0
        self.ws = GuardedBuffer(self.need).poison(ws_poison)
        self.sel = GuardedBuffer(4 * max_rows).poison(FF)
        self.cnt = GuardedBuffer(8).poison(FF)

    def outputs(self):
        return dict(out_sel=self.sel.view(torch.int32), out_count=self.cnt.view(torch.int64), workspace=self.ws.bytes())

    def assert_intact(self, count):
        """Guards whole, and the garbage in out_sel past the returned count left alone."""
        for name, g in (("workspace", self.ws), ("out_sel", self.sel), ("out_count", self.cnt)):
            g.assert_guards_intact(name)
        assert bool(torch.all(self.sel.view(torch.int32)[count:] == -1)), "out_sel written past the returned count"


def device_count(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda:0")


# ---- the probe ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_name", COUNTS)
@pytest.mark.parametrize("max_rows", MAX_ROWS)
def test_probe_chain_sel_vs_oracle(rpt, pools, max_rows, count_name):
    """Every (max_rows, device count) pair; the chain (1, 2, 3 or 8 filters; first stage gather, whole-filter LDS or
    hybrid; later stages of each kind, and PARTITIONED demoted), the key types, the column kinds and the order of sel
    rotate over the pairs so that each occurs."""
    mi, ci = MAX_ROWS.index(max_rows), COUNTS.index(count_name)
    case = mi * len(COUNTS) + ci
    rng = np.random.default_rng(7000 + case)
    spec = CHAINS[(ci + 3 * mi) % len(CHAINS)]
    rows = max(2 * max_rows + 200, 4096)
    chain = build_chain(rpt, rng, pools, spec, rows, rot=case)
    count = count_of(count_name, max_rows)
    used = min(count, max_rows)
    sel = poisoned_sel(rng, max_rows, used, chain.alive, ascending=case % 2 == 0)
    exp = expected(sel, used, chain.alive)
    for bf in chain.filters:  # a routed strategy is demoted, the others stay
        st = bf.probe_strategy_for(max_rows)
        assert bf.probe_sel_strategy_for(max_rows) == (GATHER if st in (PARTITIONED, BUCKETED) else st)
    buf = Buffers(rpt, chain.filters, max_rows)
    d_sel, d_count = dev(sel), device_count(count)
    out_sel, out_count = rpt.probe_chain_sel_ws(chain.filters, chain.args, d_sel, d_count, max_rows=max_rows,
                                                **buf.outputs())
    got_count = int(out_count.item())
    print(f"max_rows {max_rows} count {count} chain {spec}: {got_count} of {used} survive (oracle {exp.size})")
    assert got_count == exp.size
    assert np.array_equal(sel_of(out_sel[:got_count]), exp)
    buf.assert_intact(got_count)
    assert int(d_count.item()) == count and np.array_equal(sel_of(d_sel), sel)  # the inputs are only read
    if used >= 512:
        assert 0 < exp.size < used
    # ... and rpt_bf_probe_chain_ws, told the count by the host, returns the same on the same buffers
    same = rpt.probe_chain_ws(chain.filters, chain.args, row_sel=d_sel, n=used)
    assert np.array_equal(sel_of(same), exp)


def test_result_does_not_depend_on_filter_order(rpt, pools):
    rng = np.random.default_rng(11)
    max_rows, used = 1543, 1400
    spec = [(16, GATHER), (13, AUTO), (16, LDS)]
    chain = build_chain(rpt, rng, pools, spec, 4096, rot=1)
    sel = poisoned_sel(rng, max_rows, used, chain.alive)
    exp = expected(sel, used, chain.alive)
    assert 0 < exp.size < used
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        buf = Buffers(rpt, chain.filters, max_rows)
        out_sel, out_count = rpt.probe_chain_sel_ws([chain.filters[i] for i in order], [chain.args[i] for i in order],
                                                    dev(sel), device_count(used), max_rows=max_rows, **buf.outputs())
        assert int(out_count.item()) == exp.size and np.array_equal(sel_of(out_sel[: exp.size]), exp), order
        buf.assert_intact(exp.size)


@pytest.mark.parametrize("stage", [0, 1])
def test_routed_strategies_are_demoted_to_the_gather(rpt, pools, stage):
    """A filter forced to PARTITIONED (2^18 blocks) and one forced to BUCKETED (2^22), as the first or as a later stage:
    both report GATHER from rpt_bf_probe_sel_strategy_for, the two results are equal, and both equal the oracle's and
    rpt_bf_probe_chain_ws's, which does run the routed probes."""
    rng = np.random.default_rng(13 + stage)
    max_rows, used = 40003, 33000
    results = []
    for log_nb, strategy in ((18, PARTITIONED), (22, BUCKETED)):
        # the same draws for both filters: only the demoted filter differs
        r = np.random.default_rng(1300 + stage)
        spec = [(log_nb, strategy), (13, AUTO)] if stage == 0 else [(13, AUTO), (log_nb, strategy)]
        chain = build_chain(rpt, r, pools, spec, 2 * max_rows, rot=stage)
        demoted = chain.filters[stage]
        assert demoted.probe_strategy_for(max_rows) == strategy
        assert demoted.probe_sel_strategy_for(max_rows) == GATHER
        sel = poisoned_sel(rng, max_rows, used, chain.alive)
        exp = expected(sel, used, chain.alive)
        assert 0 < exp.size < used
        buf = Buffers(rpt, chain.filters, max_rows)
        d_sel = dev(sel)
        out_sel, out_count = rpt.probe_chain_sel_ws(chain.filters, chain.args, d_sel, device_count(used),
                                                    max_rows=max_rows, **buf.outputs())
        assert int(out_count.item()) == exp.size and np.array_equal(sel_of(out_sel[: exp.size]), exp)
        buf.assert_intact(exp.size)
        routed = rpt.probe_chain_ws(chain.filters, chain.args, row_sel=d_sel, n=used)
        assert np.array_equal(sel_of(routed), exp)
        results.append((sel_of(out_sel[: exp.size]).copy(), sel_of(routed).copy()))
    for got, routed in results:
        assert np.array_equal(got, routed)


@pytest.mark.parametrize("source", ["probe", "chain_ws", "chain_ws_count_aliased"])
def test_straight_from_a_probe(rpt, pools, source):
    """out_sel and *out_count_dev of rpt_bf_probe and of rpt_bf_probe_chain_ws go into rpt_bf_probe_chain_sel_ws on
    other columns of the same rows with no host read in between; once with out_count_dev == count_dev."""
    rng = np.random.default_rng(17 + len(source))
    n = 40003
    f, w, b = pools[1].get(16)
    f.probe_strategy = AUTO
    pk = hits(rng, b, n, np.int64, 0.4)
    first = orc.probe_keys(w, 16, pk)
    assert 0 < first.size < n
    chain = build_chain(rpt, rng, pools, [(16, GATHER), (13, AUTO)], n, rot=2)
    exp = first[chain.alive[first]]
    assert 0 < exp.size < first.size
    # the first probe's output buffer doubles as the poison: past its count it holds rows that pass the second chain
    passing = np.flatnonzero(chain.alive)
    mid_sel = dev(passing[rng.integers(0, passing.size, n)].astype(np.uint32))
    mid_count = device_count(-1)
    d_pk = dev(pk)
    if source == "probe":
        f.probe_async(d_pk, out_sel=mid_sel, out_count=mid_count)
    else:
        ws = torch.empty(rpt.probe_chain_workspace_bytes([f], n), dtype=torch.uint8, device="cuda:0")
        assert raw_chain_ws(rpt, [f], [rpt.make_column(d_pk)], n, mid_sel, mid_count, ws) == 0
    buf = Buffers(rpt, chain.filters, n)
    outputs = buf.outputs()
    if source == "chain_ws_count_aliased":
        outputs["out_count"] = mid_count
    out_sel, out_count = rpt.probe_chain_sel_ws(chain.filters, chain.args, mid_sel, mid_count, **outputs)
    assert (out_count.data_ptr() == mid_count.data_ptr()) == (source == "chain_ws_count_aliased")
    assert int(out_count.item()) == exp.size
    assert np.array_equal(sel_of(out_sel[: exp.size]), exp.astype(np.uint32))
    buf.assert_intact(exp.size)
    assert np.array_equal(sel_of(mid_sel[: first.size]), first.astype(np.uint32))


def test_zero_max_rows_only_sets_the_count(rpt, pools, targets):
    rng = np.random.default_rng(19)
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    lib = rpt.load()
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * 1)(chain.filters[0].handle)
    arr = (KeyColumn * 1)(rpt.make_column(**chain.args[0]))
    cnt = GuardedBuffer(8).poison(FF)
    stream = torch.cuda.current_stream().cuda_stream
    d_count = device_count(5)
    assert lib.rpt_bf_probe_chain_sel_ws(handles, arr, 1, None, d_count.data_ptr(), 0, None, cnt.ptr, None, 0, stream) == 0
    assert int(cnt.view(torch.int64).item()) == 0
    cnt.assert_guards_intact("out_count")
    bf, base = targets.reset(14, True)
    dst = (ctypes.c_void_p * 1)(bf.handle)
    for routed in (False, True):
        cnt.poison(FF)
        if routed:
            st = lib.rpt_bf_transfer_insert_sel_ws(handles, arr, 1, dst, arr, 1, None, d_count.data_ptr(), 0, None, cnt.ptr,
                                                   None, 0, None, 0, stream)
        else:
            st = lib.rpt_bf_transfer_sel_ws(handles, arr, 1, dst, arr, 1, None, d_count.data_ptr(), 0, None, cnt.ptr, None, 0,
                                            stream)
        assert st == 0, lib.rpt_last_error()
        assert int(cnt.view(torch.int64).item()) == 0
        assert bf.is_empty() and np.array_equal(bf.export_words(), base)  # no destination is touched


def test_workspace_errors_come_before_any_launch(rpt, pools):
    rng = np.random.default_rng(23)
    max_rows = 1543
    chain = build_chain(rpt, rng, pools, [(16, GATHER), (13, AUTO)], 4096)
    sel = dev(poisoned_sel(rng, max_rows, 1000, chain.alive))
    buf = Buffers(rpt, chain.filters, max_rows)
    out = buf.outputs()
    short = dict(out, workspace=buf.ws.bytes()[: buf.need - 1])
    with pytest.raises(rpt.RptError) as e:
        rpt.probe_chain_sel_ws(chain.filters, chain.args, sel, device_count(1000), max_rows=max_rows, **short)
    assert e.value.status == 4  # RPT_ERR_WORKSPACE
    big = GuardedBuffer(buf.need + 256).poison(A5)
    with pytest.raises(rpt.RptError) as e:
        rpt.probe_chain_sel_ws(chain.filters, chain.args, sel, device_count(1000), max_rows=max_rows,
                               **dict(out, workspace=big.bytes()[8: 8 + buf.need]))
    assert e.value.status == 1 and "aligned" in str(e.value)
    torch.cuda.synchronize()
    assert bool(torch.all(buf.ws.bytes() == 0xA5)) and bool(torch.all(big.bytes() == 0xA5))
    assert bool(torch.all(buf.sel.view(torch.int32) == -1)) and int(buf.cnt.view(torch.int64).item()) == -1


# ---- the transfers --------------------------------------------------------------------------------------------------
def dst_col(rng, kt, kind, rows, poison_rows):
    """A destination column in which the keys of the poison rows are valid and occur nowhere else (a dictionary gives
    every poison row an entry of its own)."""
    key_sel = None
    if kind == "dict":
        m0 = rows // 2 + 1
        key_sel = rng.integers(0, m0, rows).astype(np.uint32)
        key_sel[poison_rows] = m0 + np.arange(len(poison_rows), dtype=np.uint32)
    col = Col(rng, kt, kind, rows, key_sel=key_sel)
    phys = col.phys(poison_rows)
    others = np.setdiff1d(np.arange(col.keys.size), phys)
    while np.isin(col.keys[phys], col.keys[others]).any() or np.unique(col.keys[phys]).size != phys.size:
        col.keys[phys] = Col(rng, kt, "flat", phys.size).keys
    col.d_keys = dev(col.keys)
    if col.validity is not None:
        np.bitwise_or.at(col.validity, phys >> 6, np.uint64(1) << (phys & 63).astype(np.uint64))
        col.d_validity = dev(col.validity)
    return col


def transfer_case(rpt, rng, pools, targets, spec, max_rows, used, dst_specs, routed, rows=None):
    """One transfer call against the oracle; dst_specs: (key type, column kind, log2 blocks, pre-filled, forced insert
    strategy or None) per destination. Returns the survivors."""
    rows = rows or max(2 * max_rows + 200, 4096)
    chain = build_chain(rpt, rng, pools, spec, rows, rot=len(dst_specs))
    passing = np.flatnonzero(chain.alive)
    poison_rows = np.sort(rng.choice(passing, size=min(32, passing.size), replace=False))
    sel = poisoned_sel(rng, max_rows, used, chain.alive, avoid=poison_rows)
    exp = expected(sel, used, chain.alive)
    dst_cols = [dst_col(rng, kt, kind, rows, poison_rows) for kt, kind, _L, _p, _s in dst_specs]
    dst = [targets.reset(L, p, tag=j) for j, (_kt, _kind, L, p, _s) in enumerate(dst_specs)]
    for (bf, _base), spec_j in zip(dst, dst_specs):
        bf._lib.rpt_bf_set_insert_strategy(bf.handle, INS_AUTO if spec_j[4] is None else spec_j[4])
        if spec_j[4] is not None:
            assert bf.insert_strategy_for(max_rows) == spec_j[4]
    buf = Buffers(rpt, chain.filters, max_rows)
    kwargs = buf.outputs()
    try:
        if routed:
            need = rpt.transfer_insert_workspace_bytes([bf for bf, _b in dst], max_rows)
            assert (need > 0) == any(s[4] == INS_PARTITIONED for s in dst_specs)
            iws = GuardedBuffer(need).poison(RAMP) if need else None
            out_sel, out_count = rpt.transfer_insert_sel_ws(
                chain.filters, chain.args, [bf for bf, _b in dst], [c.as_dict(rpt) for c in dst_cols], dev(sel),
                device_count(used), max_rows=max_rows, insert_workspace=iws.bytes() if iws else None, **kwargs)
        else:
            iws = None
            out_sel, out_count = rpt.transfer_sel_ws(
                chain.filters, chain.args, [bf for bf, _b in dst], [c.as_dict(rpt) for c in dst_cols], dev(sel),
                device_count(used), max_rows=max_rows, **kwargs)
        got = int(out_count.item())
        assert got == exp.size
        assert np.array_equal(sel_of(out_sel[:got]), exp)
        for (bf, base), c, spec_j in zip(dst, dst_cols, dst_specs):
            check(bf, c.expect(base, spec_j[2], exp), f"destination {spec_j}")
        buf.assert_intact(got)
        if iws is not None:
            iws.assert_guards_intact("insert workspace")
    finally:
        for bf, _b in dst:
            bf._lib.rpt_bf_set_insert_strategy(bf.handle, INS_AUTO)
    return exp


@pytest.mark.parametrize("n_dst", [1, 2])
@pytest.mark.parametrize("routed", [False, True], ids=["transfer_sel_ws", "transfer_insert_sel_ws"])
@pytest.mark.parametrize("max_rows,count", [(513, 512), (1543, 1543 + 100), (40003, 40002)])
def test_transfer_sel_vs_oracle(rpt, pools, targets, max_rows, count, routed, n_dst):
    """1-2 destinations, pre-filled and empty, on columns of their own, none of them routing: the words and the min/max
    equal the oracle's over the oracle's survivors, out_sel and the count as for the probe alone."""
    rng = np.random.default_rng(max_rows * 4 + 2 * routed + n_dst)
    spec = CHAINS[3 + (max_rows + n_dst) % 3]
    dst_specs = [("i64", "flat", 17, False, None), ("i32", "dict", 14, True, None)][:n_dst]
    if routed:
        dst_specs = [("i32", "valid", 14, True, None), ("hash", "dict", 15, False, None)][:n_dst]
    exp = transfer_case(rpt, rng, pools, targets, spec, max_rows, min(count, max_rows), dst_specs, routed)
    if max_rows > 1000:
        assert exp.size > 0


@pytest.mark.parametrize("log_nb", [16, 18])
def test_transfer_insert_sel_routes_a_partitioned_destination(rpt, pools, targets, log_nb):
    """max_rows = three 16 Ki-row tiles and a tail; one destination forced to PARTITIONED (the routed insert from the
    bits, with sel as the row mapping), a second one on atomics."""
    rng = np.random.default_rng(log_nb)
    max_rows = kl.N_TILES
    dst_specs = [("i64", "valid", log_nb, log_nb == 16, INS_PARTITIONED), ("i32", "flat", 14, log_nb != 16, None)]
    exp = transfer_case(rpt, rng, pools, targets, [(16, GATHER), (13, AUTO)], max_rows, max_rows - 4000, dst_specs, True,
                        rows=max_rows + 5000)
    assert 0 < exp.size < max_rows - 4000


@pytest.mark.parametrize("routed", [False, True])
def test_an_empty_selection_leaves_has_data_set_and_the_words_unchanged(rpt, pools, targets, routed):
    rng = np.random.default_rng(29 + routed)
    dst_specs = [("i64", "flat", 16, True, INS_PARTITIONED if routed else None)]
    exp = transfer_case(rpt, rng, pools, targets, [(13, AUTO)], 20000, 0, dst_specs, routed)
    assert exp.size == 0  # transfer_case's check(): words = base, no min/max, is_empty() False


# ---- workspace hygiene ----------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_what_the_workspace_held(rpt, pools):
    """The same call over a workspace left dirty by a larger call of another strategy (a partitioned
    rpt_bf_probe_chain_ws over more rows), over 0xFF and over 0xA5: identical results."""
    rng = np.random.default_rng(31)
    max_rows, used = 1543, 1100
    chain = build_chain(rpt, rng, pools, [(16, LDS), (13, AUTO), (16, GATHER)], 40003, rot=1)
    sel = poisoned_sel(rng, max_rows, used, chain.alive)
    exp = expected(sel, used, chain.alive)
    assert 0 < exp.size < used
    need = rpt.probe_chain_sel_workspace_bytes(chain.filters, max_rows)
    # the larger call: all 40003 rows through a forced-PARTITIONED chain, in a workspace of its own size
    big_f = pools[0].get(18)[0]
    big_f.probe_strategy = PARTITIONED
    big_col = probed_col(rng, "i64", "flat", 40003, pools[0].get(18)[2])
    big = torch.empty(rpt.probe_chain_workspace_bytes([big_f], 40003), dtype=torch.uint8, device="cuda:0")
    assert big.numel() > need
    rpt.probe_chain_ws([big_f], [big_col.as_dict(rpt)], workspace=big)
    torch.cuda.synchronize()
    results = []
    for dirt in ("larger call", FF, A5):
        buf = Buffers(rpt, chain.filters, max_rows, ws_poison=FF if dirt == "larger call" else dirt)
        if dirt == "larger call":
            buf.ws.bytes().copy_(big[:need])
        out_sel, out_count = rpt.probe_chain_sel_ws(chain.filters, chain.args, dev(sel), device_count(used),
                                                    max_rows=max_rows, **buf.outputs())
        got = int(out_count.item())
        buf.assert_intact(got)
        results.append(sel_of(out_sel[:got]).copy())
    for r in results:
        assert np.array_equal(r, exp)


def test_captured_call_replays_over_a_dirtied_workspace(rpt, pools):
    """The call captured into a graph and replayed three times, the workspace filled with other garbage and the device
    count changed between the replays."""
    rng = np.random.default_rng(37)
    max_rows = 1543
    chain = build_chain(rpt, rng, pools, [(16, GATHER), (13, AUTO)], 4096, rot=2)
    passing = np.flatnonzero(chain.alive)
    sel = poisoned_sel(rng, max_rows, max_rows, chain.alive)
    d_sel, d_count = dev(sel), device_count(max_rows)
    buf = Buffers(rpt, chain.filters, max_rows)
    s = torch.cuda.Stream(device="cuda:0")
    call = lambda stream: rpt.probe_chain_sel_ws(chain.filters, chain.args, d_sel, d_count, max_rows=max_rows,  # noqa: E731
                                                 stream=stream, **buf.outputs())
    call(None)  # once outside any capture: a kernel's first launch may set its LDS allowance
    torch.cuda.synchronize()
    sh = ctypes.c_void_p(s.cuda_stream)
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _res = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: call(s))
    assert end == 0
    assert graph_instantiate(graph, exe) == 0
    for replay, (used, dirt) in enumerate(((1543, FF), (700, RAMP), (0, A5), (1200, FF))):
        sel[used:] = passing[rng.integers(0, passing.size, max_rows - used)]
        d_sel.copy_(dev(sel))
        d_count.fill_(used)
        buf.ws.poison(dirt)
        buf.sel.poison(FF)
        buf.cnt.poison(FF)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        exp = expected(sel, used, chain.alive)
        got = int(buf.cnt.view(torch.int64).item())
        assert got == exp.size, replay
        assert np.array_equal(sel_of(buf.sel.view(torch.int32)[:got]), exp), replay
        buf.assert_intact(got)
    assert graph_destroy(exe, graph)


def test_pending_clear_of_a_probed_filter_is_refused_inside_a_capture(rpt, pools):
    """rpt_bf_probe_chain_ws's rule: a cleared filter cannot be settled inside a capture, and the refusal comes before
    anything is enqueued; outside a capture the same call settles it (and nothing passes an empty filter)."""
    from test_gpu_transfer import graph_node_count
    from buf_util import hip_graph_api

    rng = np.random.default_rng(41)
    max_rows = 1543
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    cleared = rpt.BloomFilter(log_num_blocks=12)
    cleared.insert(dev(np.arange(100, dtype=np.int64)))
    cleared.clear()
    torch.cuda.synchronize()
    col = probed_col(rng, "i64", "flat", 4096, pools[0].get(13)[2])
    filters, args = chain.filters + [cleared], chain.args + [col.as_dict(rpt)]
    d_sel, d_count = dev(poisoned_sel(rng, max_rows, 1000, chain.alive)), device_count(1000)
    buf = Buffers(rpt, filters, max_rows)
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)

    def call():
        try:
            rpt.probe_chain_sel_ws(filters, args, d_sel, d_count, max_rows=max_rows, stream=s, **buf.outputs())
        except rpt.RptError as e:
            return e
        return None

    graph = ctypes.c_void_p()
    end, err = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, call)
    assert end == 0
    assert err is not None and err.status == 1 and "rpt_bf_settle" in str(err)
    assert graph_node_count(graph) == 0
    assert hip_graph_api().hipGraphDestroy(graph) == 0
    assert call() is None
    s.synchronize()
    assert int(buf.cnt.view(torch.int64).item()) == 0
    buf.assert_intact(0)
    cleared.close()
