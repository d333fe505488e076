"""The one-launch row-list transfer and the multi-filter sink (rpt_bf_transfer, rpt_bf_transfer_range,
rpt_bf_insert_multi) vs the oracle, bit-exact, and vs the calls they twin on the same inputs (rpt_bf_transfer_ws,
rpt_bf_transfer_range_ws; one rpt_bf_insert per destination): the rows probed are 0 .. n or row_sel[0 .. n), n at most
RPT_SMALL_PROBE_ROWS and known to the host.

The shapes are the smallest at which the single-workgroup kernel can go wrong: n around one 512-position segment, around
8192 (where its 16 waves go from one segment each to two) and the limit 16384. Poison as in tests/test_gpu_probe_sel.py,
whose helpers this file reuses: a given row_sel is 64 entries longer than n, and the entries past n hold rows that pass
every filter and whose destination keys occur nowhere else, so an entry read past n shows up as extra survivors or
extra filter bits, never as a fault. Outputs are exactly sized GuardedBuffers holding garbage on entry. The probed
filters come from buf_util.FilterCache and are never inserted into."""
import ctypes
import gc
import threading

import numpy as np
import pytest
import torch

import golden_util as gu
import rpt_oracle as orc
from buf_util import (CAPTURE_MODE_GLOBAL, FF, FilterCache, GuardedBuffer, graph_destroy, graph_instantiate, graph_launch,
                      hip_graph_api, stream_capture)
from test_gpu_probe_sel import build_chain, dst_col, poisoned_sel, probed_col
from test_gpu_probe_sel_range import (EIGHT, I64_MAX, I64_MIN, THREE, host_range_pass, ranged_chain, recording)
from test_gpu_probe_sel_small import CHAINS, EIGHT_DST, Out, all_null_except, combine_minmax, rows_for
from test_gpu_transfer import Col, Targets, check, dev, graph_node_count, hits, rand_keys, sel_of

pytestmark = pytest.mark.gpu

AUTO = 0
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
SIZES = [1, 511, 512, 513, 8191, 8192, 8193, 16384]
ROW_SELS = ["null", "ascending", "any"]
SLACK = 64  # entries of a given row_sel past n: the poison
TWICE = [("i64", "valid", 14, True, 0), ("hash", "flat", 12, True, 1), ("i32", "dict", 14, True, 0)]
DSTS = {"1": EIGHT_DST[:1], "2": EIGHT_DST[1:3], "8": EIGHT_DST, "twice": TWICE}
SEED = 7700  # of this file's ranged chains: no key of test_gpu_probe_sel_range's cache is shared


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
    import test_gpu_probe_sel_range as tr

    made = (FilterCache(), FilterCache())
    yield made
    for key in [k for k in tr._CHAINS if k[2] == SEED]:  # the ranged chains hold this module's filters
        del tr._CHAINS[key]
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def targets(rpt):
    t = Targets(rpt)
    yield t
    t.close()


@pytest.fixture(scope="module", autouse=True)
def profiling_off_afterwards(rpt):
    from rpt_amd import _lib

    yield
    _lib.profiling(False)
    _lib.profiling_reset()


def all_auto(filters):
    """The one-launch kernel ignores the strategies; AUTO lets rpt_bf_transfer_ws take today's small-batch hand-over."""
    for bf in filters:
        bf.probe_strategy = AUTO


def row_list(rng, kind, n, alive, poison_rows, only=None):
    """(the listed row ids, the device row_sel or None). null: rows 0 .. n. Otherwise n ids of the table (ascending without
    repeats, or any order with repeats; `only`: drawn from these rows alone) followed by SLACK poison entries."""
    if kind == "null":
        return np.arange(n, dtype=np.uint32), None
    sel = poisoned_sel(rng, n + SLACK, n, alive, ascending=kind == "ascending", avoid=poison_rows)
    if only is not None:
        sel[:n] = np.sort(only[rng.integers(0, only.size, n)]) if kind == "ascending" else only[rng.integers(0, only.size, n)]
    return sel[:n].copy(), dev(sel)


def unchanged(cols):
    for c in cols:
        assert np.array_equal(c.d_keys.cpu().numpy().view(c.keys.dtype), c.keys)
        if c.key_sel is not None:
            assert np.array_equal(sel_of(c.d_key_sel), c.key_sel)
        if c.validity is not None:
            assert np.array_equal(c.d_validity.cpu().numpy().view(np.uint64), c.validity)


def run_transfer(rpt, rng, targets, filters, cols, args, alive, n, ids, d_row_sel, dst_specs, poison_rows, mask=None,
                 null_dst=None):
    """One rpt_bf_transfer (mask None) or rpt_bf_transfer_range against the expectation exp = ids[alive[ids]] and against
    the _ws twin into twin filters. dst_specs: (key type, column kind, log2 blocks, _, slot) per destination, every
    filter pre-filled; two entries with one slot are the same filter listed twice."""
    rows = alive.size
    exp = ids[alive[ids]]
    dst_cols = [dst_col(rng, kt, kind, rows, poison_rows) for kt, kind, _L, _p, _s in dst_specs]
    if null_dst is not None:
        all_null_except(dst_cols[null_dst], poison_rows)
    slots = {}
    for _kt, _kind, L, _p, slot in dst_specs:
        if slot not in slots:
            slots[slot] = (L, targets.reset(L, True, tag=slot), targets.reset(L, True, tag=100 + slot))
    dst = [slots[s[4]][1][0] for s in dst_specs]
    twins = [slots[s[4]][2][0] for s in dst_specs]
    dargs = [c.as_dict(rpt) for c in dst_cols]
    before = None if d_row_sel is None else sel_of(d_row_sel).copy()
    out, twin_out = Out(n), Out(n)
    if mask is None:
        rpt.transfer(filters, args, dst, dargs, row_sel=d_row_sel, n=n, **out.outputs())
        rpt.transfer_ws(filters, args, twins, dargs, row_sel=d_row_sel, n=n, **twin_out.outputs())
    else:
        rpt.transfer_range(filters, args, dst, dargs, range_mask=mask, row_sel=d_row_sel, n=n, **out.outputs())
        rpt.transfer_range_ws(filters, args, twins, dargs, range_mask=mask, row_sel=d_row_sel, n=n, **twin_out.outputs())
    got = out.count()
    print(f"n {n}, {len(filters)} filters, {len(dst_specs)} destinations, mask {mask}: {got} of {n} survive "
          f"(oracle {exp.size})")
    assert got == exp.size
    assert np.array_equal(sel_of(out.sel.view(torch.int32)[:got]), exp)
    out.assert_intact(got)
    if before is not None:
        assert np.array_equal(sel_of(d_row_sel), before)  # the inputs are only read
    unchanged(cols + dst_cols)
    assert twin_out.count() == got
    assert np.array_equal(sel_of(twin_out.sel.view(torch.int32)[:got]), exp)
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


def poison_of(rng, alive):
    passing = np.flatnonzero(alive)
    return np.sort(rng.choice(passing, size=min(32, passing.size), replace=False))


# ---- the matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_sel", ROW_SELS)
@pytest.mark.parametrize("n", SIZES)
def test_transfer_vs_oracle_and_the_workspace_call(rpt, pools, targets, n, row_sel):
    """Every (n, row mapping) pair; the chain (1, 2, 3 or 8 filters), the key types, the column kinds (flat, with NULLs,
    dictionary) and the destinations (1, 2, 8, and one filter listed twice with two columns) rotate over the pairs so
    that each occurs."""
    ni, ri = SIZES.index(n), ROW_SELS.index(row_sel)
    case = ni * len(ROW_SELS) + ri
    rng = np.random.default_rng(12000 + case)
    spec, frac = CHAINS[(ni + ri) % len(CHAINS)]
    chain = build_chain(rpt, rng, pools, spec, rows_for(n), rot=case, frac=frac)
    all_auto(chain.filters)
    poison_rows = poison_of(rng, chain.alive)
    ids, d_row_sel = row_list(rng, row_sel, n, chain.alive, poison_rows)
    dst_specs = DSTS[list(DSTS)[(case + ni // 4) % len(DSTS)]]
    exp = run_transfer(rpt, rng, targets, chain.filters, chain.cols, chain.args, chain.alive, n, ids, d_row_sel, dst_specs,
                       poison_rows)
    if n >= 512:
        assert 0 < exp.size < n  # the filters discriminate


def test_the_matrix_rotates_over_every_chain_and_destination_list():
    seen = set()
    for ni in range(len(SIZES)):
        for ri in range(len(ROW_SELS)):
            case = ni * len(ROW_SELS) + ri
            seen.add(("chain", (ni + ri) % len(CHAINS)))
            seen.add(("dst", list(DSTS)[(case + ni // 4) % len(DSTS)]))
    assert seen == {("chain", i) for i in range(len(CHAINS))} | {("dst", k) for k in DSTS}


@pytest.mark.parametrize("row_sel", ["null", "any"])
@pytest.mark.parametrize("how", ["none", "all"])
def test_no_survivor_and_every_row_surviving(rpt, pools, targets, how, row_sel):
    """No survivor: the count is 0, out_sel and the destinations' words and min/max are untouched, has_data is 1. Every
    row surviving: the whole list comes back and is inserted."""
    rng = np.random.default_rng(131 + len(how) + len(row_sel))
    n = 1024
    spec, frac = CHAINS[1]
    rows = rows_for(n)
    chain = build_chain(rpt, rng, pools, spec, rows, rot=2, frac=frac)
    all_auto(chain.filters)
    wanted = np.flatnonzero(chain.alive if how == "all" else ~chain.alive)
    assert wanted.size >= n + 64
    if row_sel == "null":  # rows 0 .. n are the list: the table reordered so that its first n rows are wanted ones
        order = np.concatenate([wanted[:n], np.setdiff1d(np.arange(rows), wanted[:n])])
        for c in chain.cols:
            if c.key_sel is not None:
                c.key_sel = c.key_sel[order]
                c.d_key_sel = dev(c.key_sel)
                continue
            c.keys = c.keys[order]
            c.d_keys = dev(c.keys)
            if c.validity is not None:
                c.validity = gu.validity_words(((c.validity[order >> 6] >> (order & 63).astype(np.uint64)) & np.uint64(1)).astype(bool))
                c.d_validity = dev(c.validity)
        alive = chain.alive[order]
        assert alive[:n].all() if how == "all" else not alive[:n].any()
        args = [c.as_dict(rpt) for c in chain.cols]
        poison_rows = np.flatnonzero(alive)[-32:]
        ids, d_row_sel = np.arange(n, dtype=np.uint32), None
    else:
        alive, args = chain.alive, chain.args
        poison_rows = poison_of(rng, alive)
        ids, d_row_sel = row_list(rng, "any", n, alive, poison_rows, only=np.setdiff1d(wanted, poison_rows))
    exp = run_transfer(rpt, rng, targets, chain.filters, chain.cols, args, alive, n, ids, d_row_sel, EIGHT_DST[1:3],
                       poison_rows)
    assert exp.size == (n if how == "all" else 0)  # run_transfer's check(): words and min/max as the oracle's, has_data


def test_selected_null_rows_insert_null_hash_and_leave_no_minmax(rpt, pools, targets):
    rng = np.random.default_rng(137)
    n = 1543
    spec, frac = CHAINS[0]
    chain = build_chain(rpt, rng, pools, spec, rows_for(n), rot=0, frac=frac)
    all_auto(chain.filters)
    poison_rows = poison_of(rng, chain.alive)
    ids, d_row_sel = row_list(rng, "any", n, chain.alive, poison_rows)
    dst_specs = [("i64", "valid", 13, True, 0), ("i32", "valid", 13, True, 1)]
    exp = run_transfer(rpt, rng, targets, chain.filters, chain.cols, chain.args, chain.alive, n, ids, d_row_sel, dst_specs,
                       poison_rows, null_dst=0)
    assert exp.size > 0
    bf, base = targets._made[(13, True, 0)]
    null_only = base.copy()
    orc.insert_hashes(null_only, 13, np.array([0xBF58476D1CE4E5B9], dtype=np.uint64))  # NULL_HASH
    assert np.array_equal(bf.export_words(), null_only) and bf.minmax() is None
    assert targets._made[(13, True, 1)][0].minmax() is not None


def test_zero_rows_only_set_the_count(rpt, pools, targets):
    from rpt_amd._lib import KeyColumn

    rng = np.random.default_rng(139)
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    lib = rpt.load()
    handles = (ctypes.c_void_p * 1)(chain.filters[0].handle)
    arr = (KeyColumn * 1)(rpt.make_column(**chain.args[0]))
    bf, base = targets.reset(14, True)
    dst = (ctypes.c_void_p * 1)(bf.handle)
    stream = torch.cuda.current_stream().cuda_stream
    for mask in (None, 0, 1):
        cnt = GuardedBuffer(8).poison(FF)
        if mask is None:
            st = lib.rpt_bf_transfer(handles, arr, 1, dst, arr, 1, None, 0, None, cnt.ptr, stream)
        else:
            st = lib.rpt_bf_transfer_range(handles, arr, 1, mask, dst, arr, 1, None, 0, None, cnt.ptr, stream)
        assert st == 0, lib.rpt_last_error()
        assert int(cnt.view(torch.int64).item()) == 0
        cnt.assert_guards_intact("out_count")
    assert lib.rpt_bf_insert_multi(dst, arr, 1, None, 0, stream) == 0
    assert bf.is_empty() and np.array_equal(bf.export_words(), base)  # no destination is touched
    assert lib.rpt_bf_transfer(handles, arr, 1, dst, arr, 1, None, 100, None, cnt.ptr, stream) == 1
    assert b"null out_sel" in lib.rpt_last_error()
    assert bf.is_empty()


# ---- ranges -----------------------------------------------------------------------------------------------------------
RANGE_CASES = [(THREE, "all", "half"), (THREE, "first", "own"), (THREE, "last", "own"), (EIGHT, "middle", "own"), (EIGHT, "all", "own"),
               (THREE, "all", "everything"), (THREE, "first", "nothing"), (3, "all", "no_value"), (EIGHT, "all", "no_value")]


@pytest.mark.parametrize("which,mask_kind,variant", RANGE_CASES)
def test_transfer_range_vs_host_expectation_and_the_workspace_call(rpt, pools, targets, which, mask_kind, variant):
    """Masks that flag filter 0, a middle filter, the last and all (the HASH column never); ranges that cover about
    0.6-0.9 of the build keys, the middle half of the column's keys, every key and none; flagged filters without a
    value (they pass every row, NULL rows included). The chains hold int32 columns with negative keys (sign-extended)
    and unflagged filters with hostile ranges."""
    n = 2053
    rows = rows_for(n)
    chain = ranged_chain(rpt, pools, which, rows, seed=SEED)
    all_auto(chain.filters)
    flaggable = [f for f, s in enumerate(chain.spec) if s[2] != "hash"]
    mask = {"first": 1, "last": 1 << (len(chain.spec) - 1), "middle": 1 << flaggable[len(flaggable) // 2],
            "all": sum(1 << f for f in flaggable)}[mask_kind]
    alive = np.logical_and.reduce(chain.bloom)
    bloom = alive.copy()
    all_rows = np.arange(rows)
    for f, bf in enumerate(chain.filters):
        mm = (0, 0)  # hostile: applied to an unflagged filter, it would show
        if (mask >> f) & 1:
            ordered = np.sort(chain.cols[f].keys.astype(np.int64))  # "half": the column's own middle half
            mm = {"own": chain.mms[f], "half": (int(ordered[ordered.size // 4]), int(ordered[3 * ordered.size // 4])),
                  "everything": (I64_MIN, I64_MAX), "nothing": (2**40, 2**40 + 5),
                  "no_value": None if f % 2 == 0 else chain.mms[f]}[variant]
            alive &= host_range_pass(chain.cols[f], all_rows, mm)
        bf.set_minmax(mm)
    rng = np.random.default_rng(151 + which + len(mask_kind) + len(variant))
    poison_rows = poison_of(rng, bloom) if not alive.any() else poison_of(rng, alive)
    ids, d_row_sel = row_list(rng, "any", n, bloom if not alive.any() else alive, poison_rows)
    exp = run_transfer(rpt, rng, targets, chain.filters, chain.cols, chain.args, alive, n, ids, d_row_sel,
                       EIGHT_DST[:2] if which == THREE else EIGHT_DST[3:4], poison_rows, mask=mask)
    in_bloom = int(bloom[ids].sum())
    assert 0 < in_bloom < n
    if variant in ("own", "half"):
        assert 0 < exp.size < in_bloom  # the ranges remove rows the Bloom tests keep
    elif variant == "everything":
        valid = np.logical_and.reduce([host_range_pass(chain.cols[f], ids, (I64_MIN, I64_MAX)) for f in flaggable])
        assert exp.size == int((bloom[ids] & valid).sum()) > 0
    elif variant == "nothing":
        assert exp.size == 0
    else:
        assert 0 < exp.size <= in_bloom


def test_a_zero_mask_runs_the_plain_kernel(rpt, pools, targets):
    n = 2053
    chain = ranged_chain(rpt, pools, THREE, rows_for(n), seed=SEED)
    all_auto(chain.filters)
    for bf in chain.filters:
        bf.set_minmax((0, 0))  # hostile: applied anywhere, it would show
    alive = np.logical_and.reduce(chain.bloom)
    ids = np.arange(n, dtype=np.uint32)
    exp = ids[alive[ids]]
    assert 0 < exp.size < n
    col = Col(np.random.default_rng(157), "i64", "valid", alive.size)
    bf, base = targets.reset(12, True)
    out = Out(n)
    with recording() as rec:
        rpt.transfer_range(chain.filters, chain.args, [bf], [col.as_dict(rpt)], range_mask=0, n=n, **out.outputs())
    assert rec == {"transfer_small_kernel<false,true>": 1}
    assert out.count() == exp.size and np.array_equal(sel_of(out.sel.view(torch.int32)[: exp.size]), exp)
    check(bf, col.expect(base, 12, exp))
    bf, base = targets.reset(12, True)
    with recording() as rec:
        rpt.transfer_range(chain.filters, chain.args, [bf], [col.as_dict(rpt)], range_mask=0b101, n=n, **out.outputs())
    assert rec == {"transfer_small_kernel<true,true>": 1}
    assert out.count() == 0  # no key of filter 0's column is 0


# ---- the sink alone -------------------------------------------------------------------------------------------------
def gathered(rpt, col, ids):
    """make_column's arguments of the listed rows of a column as a column of its own: what rpt_bf_insert, which takes
    no row list, inserts for them."""
    kw = col.kwargs(rpt)
    kw["key_sel"] = dev(col.phys(ids))
    return dict(keys=col.d_keys, **kw)


def check_insert_multi(rpt, targets, cols, specs, n, ids, d_row_sel):
    pairs = [(targets.reset(L, True, tag=j), targets.reset(L, True, tag=100 + j)) for j, (_k, _c, L, _p, _s) in enumerate(specs)]
    rpt.insert_multi([p[0][0] for p in pairs], [c.as_dict(rpt) for c in cols], row_sel=d_row_sel, n=n)
    for j, (((bf, base), (twin, _b)), c, s) in enumerate(zip(pairs, cols, specs)):
        twin.insert(n=n, strategy=rpt.RPT_INSERT_ATOMIC, **gathered(rpt, c, ids))
        check(bf, c.expect(base, s[2], ids), f"destination {j}")
        assert np.array_equal(twin.export_words(), bf.export_words()), j
        assert twin.minmax() == bf.minmax() and not twin.is_empty(), j
    unchanged(cols)


@pytest.mark.parametrize("with_row_sel", [False, True])
@pytest.mark.parametrize("n", [1, 513, 8193, 16384])
@pytest.mark.parametrize("n_dst", [1, 2, 8])
def test_insert_multi_vs_one_insert_per_destination(rpt, targets, n, n_dst, with_row_sel):
    case = ([1, 2, 8].index(n_dst) * 4 + [1, 513, 8193, 16384].index(n)) * 2 + with_row_sel
    rng = np.random.default_rng(163 + case)
    specs = EIGHT_DST[:n_dst] if n_dst != 2 else EIGHT_DST[1:3]
    rows = n + 700
    cols = [Col(rng, kt, kind, rows) for kt, kind, _L, _p, _s in specs]
    if with_row_sel:  # any order, with repeats; the entries past n name a row no listed entry may name
        ids = rng.integers(0, rows - 1, n).astype(np.uint32)
        d_row_sel = dev(np.concatenate([ids, np.full(SLACK, rows - 1, dtype=np.uint32)]))
    else:
        ids, d_row_sel = np.arange(n, dtype=np.uint32), None
    check_insert_multi(rpt, targets, cols, specs, n, ids, d_row_sel)


@pytest.mark.parametrize("with_row_sel", [False, True])
def test_insert_multi_of_one_repeated_key_and_of_all_nulls(rpt, targets, with_row_sel):
    """A column of one key (every atomic after the first of a wave is a duplicate) and a column whose rows are all NULL
    (NULL_HASH, no min/max)."""
    rng = np.random.default_rng(167)
    n, rows = 8193, 9000
    specs = [("i64", "flat", 12, True, 0), ("i32", "valid", 13, True, 1)]
    same = Col(rng, "i64", "flat", rows, keys=np.repeat(rand_keys(np.int64, 1, rng), rows))
    nulls = Col(rng, "i32", "valid", rows)
    nulls.validity[:] = 0
    nulls.d_validity = dev(nulls.validity)
    ids = rng.integers(0, rows, n).astype(np.uint32) if with_row_sel else np.arange(n, dtype=np.uint32)
    check_insert_multi(rpt, targets, [same, nulls], specs, n, ids, dev(ids) if with_row_sel else None)
    assert targets._made[(13, True, 1)][0].minmax() is None


# ---- capture --------------------------------------------------------------------------------------------------------
def test_forward_step_of_one_vector_is_one_graph_node(rpt, pools):
    """rpt_bf_transfer_range over one 2048-row vector, captured under hipStreamCaptureModeGlobal (a synchronize, an
    allocation or a copy to the host would invalidate the capture): one kernel node. Replayed twice; between the replays
    rpt_bf_set_minmax narrows the probed filter's range, which the second replay reads from the device."""
    n = 2048
    rng = np.random.default_rng(173)
    f1, w1, b1 = pools[0].get(13)
    f1.probe_strategy = AUTO
    keys = hits(rng, b1, n, np.int64, 0.7)
    k1, dk = dev(keys), dev(rand_keys(np.int64, n, rng))
    i32, i64 = torch.int32, torch.int64
    sel, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    dst = rpt.BloomFilter(log_num_blocks=13)
    words, mm = orc.new_words(13), None
    wide, narrow = (I64_MIN, I64_MAX), (int(np.sort(b1)[b1.size // 4]), int(np.sort(b1)[3 * b1.size // 4]))
    f1.set_minmax(wide)

    def step(stream):
        rpt.transfer_range([f1], [k1], [dst], [dk], range_mask=1, n=n, out_sel=sel.view(i32), out_count=cnt.view(i64),
                           stream=stream)

    def check_against_oracle(what, rng_mm):
        nonlocal mm
        e = orc.probe_keys(w1, 13, keys).astype(np.uint32)
        e = e[(keys[e] >= rng_mm[0]) & (keys[e] <= rng_mm[1])]
        orc.insert_keys(words, 13, dk.cpu().numpy(), key_sel=e)
        mm = combine_minmax(mm, orc.minmax(dk.cpu().numpy(), key_sel=e))
        got = int(cnt.view(i64).item())
        assert got == e.size, f"{what}: count {got}, oracle {e.size}"
        assert np.array_equal(sel_of(sel.view(i32)[:got]), e), what
        assert bool(torch.all(sel.view(i32)[got:] == -1)), what
        sel.assert_guards_intact("out_sel")
        cnt.assert_guards_intact("out_count")
        check(dst, (words, mm), what)
        return e.size

    step(torch.cuda.current_stream())
    torch.cuda.synchronize()
    counts = [check_against_oracle("eager", wide)]
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _none = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: step(s))
    assert end == 0, "the capture was invalidated: something in the step synchronized, allocated or copied back"
    assert graph_node_count(graph) == 1
    assert graph_instantiate(graph, exe) == 0
    for replay, rng_mm in enumerate((wide, narrow)):
        f1.set_minmax(rng_mm)
        dk.copy_(dev(rand_keys(np.int64, n, rng)))
        sel.poison(FF)
        cnt.poison(FF)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        counts.append(check_against_oracle(f"replay {replay}", rng_mm))
    assert 0 < counts[2] < counts[1] == counts[0] < n
    assert graph_destroy(exe, graph)
    f1.set_minmax(None)
    dst.close()


@pytest.mark.parametrize("what", ["probed_cleared", "destination_in_flight"])
def test_refusals_inside_a_capture_come_before_anything_is_enqueued(rpt, pools, what):
    """A pending clear of a probed filter, and a destination whose earlier write (on another stream, queued behind a spin
    kernel) is still in flight: both refuse the captured call; the graph has no node and the
    outputs are untouched. Outside a capture the same call settles, waits and runs."""
    rng = np.random.default_rng(179)
    n = 2048
    chain = build_chain(rpt, rng, pools, [(13, AUTO)], 4096)
    col = probed_col(rng, "i64", "flat", 4096, pools[0].get(13)[2])
    dst = rpt.BloomFilter(log_num_blocks=12)
    filters, args = list(chain.filters), list(chain.args)
    s, other = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    out = Out(n)
    words, mm = orc.new_words(12), None
    if what == "probed_cleared":
        cleared = rpt.BloomFilter(log_num_blocks=12)
        cleared.insert(dev(np.arange(100, dtype=np.int64)))
        cleared.clear()
        filters.append(cleared)
        args.append(col.as_dict(rpt))
        torch.cuda.synchronize()
    else:
        # as tests/test_gpu_deferred_clear.py holds a stream back: a spin kernel in front of the write. Nothing between
        # here and the captured call below synchronizes, allocates or collects garbage
        gc.collect()
        torch.cuda.synchronize()
        with torch.cuda.stream(other):
            torch.cuda._sleep(100_000_000)
        dst.insert(col.d_keys, n=64, stream=other)
        words, mm = col.expect(words, 12, np.arange(64))

    def call():
        try:
            rpt.transfer(filters, args, [dst], [col.as_dict(rpt)], n=n, stream=s, **out.outputs())
        except rpt.RptError as e:
            return e
        return None

    graph = ctypes.c_void_p()
    if what == "probed_cleared":
        end, err = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, call)
    else:  # stream_capture() synchronizes the device first, which would let the write complete: the same without it
        hip = hip_graph_api()
        gc.disable()
        try:
            assert hip.hipStreamBeginCapture(sh, CAPTURE_MODE_GLOBAL) == 0
            err = call()
            end = hip.hipStreamEndCapture(sh, ctypes.byref(graph))
        finally:
            gc.enable()
    still_running = not other.query()
    assert end == 0
    assert what == "probed_cleared" or still_running, "the spin kernel ended before the captured call looked at the destination"
    assert err is not None and err.status == 1 and "rpt_bf_settle" in str(err)
    assert ("in flight" in str(err)) == (what == "destination_in_flight")
    assert graph_node_count(graph) == 0
    assert hip_graph_api().hipGraphDestroy(graph) == 0
    torch.cuda.synchronize()
    if what == "probed_cleared":
        assert dst.is_empty()  # a refused call has not marked the destination either
    assert out.count() == -1 and bool(torch.all(out.sel.view(torch.int32) == -1))
    assert call() is None
    s.synchronize()
    exp = np.flatnonzero(chain.alive[:n]).astype(np.uint32) if what != "probed_cleared" else np.empty(0, dtype=np.uint32)
    assert out.count() == exp.size  # nothing passes the cleared (now settled, empty) probed filter
    out.assert_intact(exp.size)
    w2, m2 = col.expect(words, 12, exp)
    check(dst, (w2, combine_minmax(mm, m2)), what)
    for bf in filters[1:] + [dst]:
        bf.close()


# ---- write order ----------------------------------------------------------------------------------------------------
def test_two_threads_listing_the_same_destinations_in_opposite_orders(rpt, pools):
    """Two host threads, each with a stream of its own, call rpt_bf_transfer and rpt_bf_insert_multi 40 times into the
    same two destinations, listed in opposite orders: the write scopes are taken in ascending handle address, so both
    finish (joined with a timeout: a lock-order inversion fails the test instead of hanging it)."""
    rng = np.random.default_rng(181)
    n, calls = 2048, 40
    rows = rows_for(n)
    chain = build_chain(rpt, rng, pools, [(13, AUTO), (16, AUTO)], rows)
    d0, d1 = rpt.BloomFilter(log_num_blocks=12), rpt.BloomFilter(log_num_blocks=14)
    c0, c1 = Col(rng, "i64", "valid", rows), Col(rng, "i32", "dict", rows)
    work = []
    for t in range(2):
        ids = rng.integers(0, rows, n).astype(np.uint32)
        order = [(d0, c0), (d1, c1)] if t == 0 else [(d1, c1), (d0, c0)]
        work.append(dict(ids=ids, d_sel=dev(ids), out=Out(n), stream=torch.cuda.Stream(device="cuda:0"),
                         dst=[d for d, _c in order], dargs=[c.as_dict(rpt) for _d, c in order], error=None))
    torch.cuda.synchronize()

    def run(w):
        try:
            for i in range(calls):
                if i % 4 == 3:
                    rpt.insert_multi(w["dst"], w["dargs"], row_sel=w["d_sel"], n=64, stream=w["stream"])
                else:
                    rpt.transfer(chain.filters, chain.args, w["dst"], w["dargs"], row_sel=w["d_sel"], n=n,
                                 stream=w["stream"], **w["out"].outputs())
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            w["error"] = e

    threads = [threading.Thread(target=run, args=(w,), daemon=True) for w in work]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads), "a thread is still inside a call: lock-order deadlock"
    assert [w["error"] for w in work] == [None, None]
    torch.cuda.synchronize()
    w0, w1, mm0, mm1 = orc.new_words(12), orc.new_words(14), None, None
    for w in work:
        exp = w["ids"][chain.alive[w["ids"]]]
        assert 0 < exp.size < n
        assert w["out"].count() == exp.size
        assert np.array_equal(sel_of(w["out"].sel.view(torch.int32)[: exp.size]), exp)
        w["out"].assert_intact(exp.size)
        for rows_in in (exp, w["ids"][:64]):
            w0, m = c0.expect(w0, 12, rows_in)
            mm0 = combine_minmax(mm0, m)
            w1, m = c1.expect(w1, 14, rows_in)
            mm1 = combine_minmax(mm1, m)
    check(d0, (w0, mm0), "destination 0")
    check(d1, (w1, mm1), "destination 1")
    d0.close()
    d1.close()


# ---- mapped pinned host memory --------------------------------------------------------------------------------------
HOST_MALLOC_MAPPED = 0x2  # hipHostMallocMapped


class Mapped:
    """`nbytes` of pinned host memory mapped into the device's address space: .host for numpy, .dev for the kernel."""

    def __init__(self, nbytes, dtype):
        self.hip = hip_graph_api()
        self.host_ptr, self.dev_ptr = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.hip.hipHostMalloc(ctypes.byref(self.host_ptr), ctypes.c_size_t(nbytes), ctypes.c_uint(HOST_MALLOC_MAPPED)) == 0
        assert self.hip.hipHostGetDevicePointer(ctypes.byref(self.dev_ptr), self.host_ptr, ctypes.c_uint(0)) == 0
        raw = (ctypes.c_uint8 * nbytes).from_address(self.host_ptr.value)
        self.host = np.frombuffer(raw, dtype=dtype)
        self.dev = self.dev_ptr.value

    def free(self):
        self.host = None
        assert self.hip.hipHostFree(self.host_ptr) == 0


def test_buffers_in_mapped_pinned_host_memory(rpt, pools, targets):
    """The key column, row_sel, out_sel and the count in hipHostMalloc'ed mapped memory, reached by the kernel through
    hipHostGetDevicePointer; the host reads the result after a synchronize. The filters' words stay on the device."""
    from rpt_amd._lib import KeyColumn

    n, rows = 2048, 4096
    rng = np.random.default_rng(191)
    f, w, b = pools[0].get(16)
    f.probe_strategy = AUTO
    keys, row_sel = Mapped(8 * rows, np.int64), Mapped(4 * n, np.uint32)
    out_sel, count = Mapped(4 * n, np.uint32), Mapped(8, np.uint64)
    try:
        keys.host[:] = hits(rng, b, rows, np.int64, 0.6)
        row_sel.host[:] = rng.integers(0, rows, n)
        out_sel.host[:] = 0xFFFFFFFF
        count.host[:] = 0xFFFFFFFFFFFFFFFF
        alive = np.zeros(rows, dtype=bool)
        alive[orc.probe_keys(w, 16, keys.host)] = True
        exp = row_sel.host[alive[row_sel.host]]
        assert 0 < exp.size < n
        bf, base = targets.reset(12, True)
        lib = rpt.load()
        col = (KeyColumn * 1)(KeyColumn(rpt.RPT_KEY_I64, keys.dev, None, None))
        st = lib.rpt_bf_transfer((ctypes.c_void_p * 1)(f.handle), col, 1, (ctypes.c_void_p * 1)(bf.handle), col, 1,
                                 row_sel.dev, n, out_sel.dev, count.dev, torch.cuda.current_stream().cuda_stream)
        assert st == 0, lib.rpt_last_error()
        torch.cuda.synchronize()
        assert int(count.host[0]) == exp.size
        assert np.array_equal(out_sel.host[: exp.size], exp)
        assert bool(np.all(out_sel.host[exp.size:] == 0xFFFFFFFF))
        words = base.copy()
        orc.insert_keys(words, 12, keys.host.copy(), key_sel=exp)
        check(bf, (words, orc.minmax(keys.host.copy(), key_sel=exp)))
    finally:
        torch.cuda.synchronize()
        for m in (keys, row_sel, out_sel, count):
            m.free()
