"""The min/max range in the device-counted probes and in the one-launch chains (rpt_bf_probe_chain_sel_range_ws,
rpt_bf_transfer_sel_range_ws, rpt_bf_transfer_insert_sel_range_ws, rpt_bf_probe_chain_sel_range,
rpt_bf_transfer_sel_range, rpt_bf_probe_chain_range), bit-exact against a host expectation: a numpy range test written
here (host_range_pass), the oracle's probe per filter, and the oracle's insert of exactly the survivors for the
destinations. What the GPU's own twin calls return is a secondary cross-check only.

"ws" is the workspace form, "one" the one-launch form. sel[used:] holds in-range ids of rows that pass every test of
the call (and, for the transfers, whose destination keys occur nowhere else), so an entry read past the count shows up
as a wrong result, never as a fault. Outputs and workspaces are exactly sized GuardedBuffers holding garbage on entry.
The probed pool filters are never inserted into; their ranges are pinned with set_minmax before every call: a flagged
filter's to the case's range, an unflagged filter's to (0, 0), which would remove nearly every row if it were applied.

A parity case asserts that its expectation is non-degenerate: the expected selection is neither empty nor everything,
and the range tests alone and the Bloom tests alone each remove a position the other keeps. That needs more than one
position: the cases with a count of 0 or 1 (and the named degenerate cases: count 0, nothing passes) are exempt."""
import collections
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import kernel_ledger as kl
import rpt_oracle as orc
from buf_util import A5, FF, RAMP, FilterCache, GuardedBuffer, int32_build_keys
from test_gpu_probe_sel import count_of, device_count, dst_col, expected, poisoned_sel, probed_col, row_pass_mask
from test_gpu_probe_sel_small import EIGHT_DST, all_null_except, combine_minmax
from test_gpu_transfer import Col, Targets, check, dev, sel_of

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED = 0, 1, 2, 3
INS_AUTO, INS_PARTITIONED = 0, 2
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
NULL_HASH = 0xBF58476D1CE4E5B9
MAX_ROWS = {"one": [1, 511, 512, 513, 2053, 8193, 16384], "ws": [1, 511, 512, 513, 2053, 8193, 16384, 40000]}
COUNTS = ["0", "1", "511", "512", "513", "max_rows-1", "max_rows", "max_rows+100", str(2**40)]
MASKS = ["none", "all", "first", "last"]
NEW_BASES = ("range_bits_sel_kernel", "probe_chain_range_small_kernel")
# Chains: ((log2 blocks, forced strategy, key type, column kind) per filter, hit fraction, share of the build keys each
# range covers). int64 build keys are drawn from +-2^62 and int32 keys are uniform over int32: negative keys throughout.
# The HASH column is never first or last and never flagged.
SPECS = [
    ([(16, GATHER, "i64", "flat")], 0.8, 0.6),
    ([(13, AUTO, "i32", "valid"), (16, GATHER, "hash", "flat"), (11, AUTO, "i64", "dict")], 0.9, 0.6),
    ([(14, LDS, "i64", "dict"), (15, LDS, "i32", "flat")], 0.9, 0.6),
    ([(18, PARTITIONED, "i64", "valid"), (13, AUTO, "i32", "dict")], 0.9, 0.6),
    ([(16, AUTO, "i64", "flat"), (13, AUTO, "i32", "flat"), (15, LDS, "hash", "flat"), (18, AUTO, "i64", "valid"),
      (11, AUTO, "i32", "flat"), (14, AUTO, "i64", "flat"), (17, LDS, "i32", "dict"), (12, GATHER, "i64", "flat")],
     0.97, 0.9),
]
THREE, EIGHT = 1, 4


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
    """Two filters per size, so a chain can hold one size twice."""
    made = (FilterCache(), FilterCache())
    yield made
    _CHAINS.clear()
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


@pytest.fixture(scope="module", autouse=True)
def profiling_off_afterwards(rpt):
    from rpt_amd import _lib

    yield
    _lib.profiling(False)
    _lib.profiling_reset()


# ---- the host expectation ---------------------------------------------------------------------------------------------
def host_range_pass(col, row_ids, mm):
    """The header's range test of the given rows of a column: without a value (mm None) every row passes, NULL rows
    included; with one a row passes iff its key is not NULL and min <= key <= max (int32 keys sign-extended)."""
    phys = col.phys(row_ids).astype(np.int64)
    if mm is None:
        return np.ones(phys.size, dtype=bool)
    v = col.keys[phys].astype(np.int64)
    valid = np.ones(phys.size, dtype=bool)
    if col.validity is not None:
        p = phys.astype(np.uint64)
        valid = ((col.validity[p >> np.uint64(6)] >> (p & np.uint64(63))) & np.uint64(1)).astype(bool)
    return valid & (v >= mm[0]) & (v <= mm[1])


def covering_range(kt, build, cover):
    """(min, max), two of the filter's build keys, with about `cover` of the build keys between them."""
    pool = np.sort(build if kt == "i64" else int32_build_keys(build))
    cut = int(pool.size * (1 - cover) / 2)
    return int(pool[cut]), int(pool[pool.size - 1 - cut])


Ranged = collections.namedtuple("Ranged", "spec filters cols args bloom in_range mms")
_CHAINS = {}


def ranged_chain(rpt, pools, which, rows, seed=0):
    """SPECS[which] over a table of `rows` rows, computed once and left unchanged: per filter its column, bloom[f][r]
    (row r passes filter f, by the oracle), mms[f] (its range) and in_range[f][r] (None for the HASH column)."""
    key = (which, rows, seed)
    if key not in _CHAINS:
        spec, frac, cover = SPECS[which]
        rng = np.random.default_rng(3000 + 97 * which + rows + seed)
        filters, cols, bloom, in_range, mms = [], [], [], [], []
        seen = collections.Counter()
        all_rows = np.arange(rows)
        for log_nb, _strategy, kt, kind in spec:
            bf, words, build = pools[seen[log_nb]].get(log_nb)
            seen[log_nb] += 1
            col = probed_col(rng, kt, kind, rows, build, frac)
            mm = None if kt == "hash" else covering_range(kt, build, cover)
            filters.append(bf)
            cols.append(col)
            bloom.append(row_pass_mask(col, words, log_nb))
            in_range.append(None if kt == "hash" else host_range_pass(col, all_rows, mm))
            mms.append(mm)
        _CHAINS[key] = Ranged(spec, filters, cols, [c.as_dict(rpt) for c in cols], bloom, in_range, mms)
    return _CHAINS[key]


def mask_of(kind, spec):
    flaggable = [f for f, s in enumerate(spec) if s[2] != "hash"]
    assert flaggable[0] == 0 and flaggable[-1] == len(spec) - 1
    return {"none": 0, "all": sum(1 << f for f in flaggable), "first": 1, "last": 1 << (len(spec) - 1)}[kind]


def arm(chain, mask, order=None):
    """Force the strategies, pin the ranges (a flagged filter's own, an unflagged filter's hostile), and return per row:
    passes every Bloom test; passes every flagged filter's range test."""
    bloom = np.logical_and.reduce(chain.bloom)
    ranged = np.ones(bloom.size, dtype=bool)
    for f, (bf, s) in enumerate(zip(chain.filters, chain.spec)):
        bf.probe_strategy = s[1]
        if (mask >> f) & 1:
            bf.set_minmax(chain.mms[f])
            ranged &= chain.in_range[f]
        else:
            bf.set_minmax((0, 0))
    return bloom, ranged


def assert_non_degenerate(sel, used, bloom, ranged, mask, exp):
    if used < 2:
        return
    s = sel[:used]
    assert 0 < exp.size < used, "the expected selection is empty or everything"
    if mask:
        assert (bloom[s] & ~ranged[s]).any(), "the range tests remove nothing the Bloom tests keep"
        assert (ranged[s] & ~bloom[s]).any(), "the Bloom tests remove nothing the range tests keep"


class Bufs:
    """out_sel of exactly max_rows entries, the count and (ws form) the workspace of exactly the reported bytes, all
    between guard bands and holding garbage."""

    def __init__(self, rpt, form, filters, max_rows, ws_poison=A5):
        self.ws = None
        if form == "ws":
            need = rpt.probe_chain_sel_workspace_bytes(filters, max_rows)
            assert need > 0 and need % 256 == 0
            self.ws = GuardedBuffer(need).poison(ws_poison)
        self.sel = GuardedBuffer(4 * max_rows).poison(FF)
        self.cnt = GuardedBuffer(8).poison(FF)

    def outputs(self):
        out = dict(out_sel=self.sel.view(torch.int32), out_count=self.cnt.view(torch.int64))
        if self.ws is not None:
            out["workspace"] = self.ws.bytes()
        return out

    def count(self):
        return int(self.cnt.view(torch.int64).item())

    def got(self):
        return sel_of(self.sel.view(torch.int32)[: self.count()])

    def assert_intact(self, count, count_guarded=True):
        for name, g in (("workspace", self.ws), ("out_sel", self.sel), ("out_count", self.cnt if count_guarded else None)):
            if g is not None:
                g.assert_guards_intact(name)
        assert bool(torch.all(self.sel.view(torch.int32)[count:] == -1)), "out_sel written past the returned count"


def chain_call(rpt, form):
    return rpt.probe_chain_sel_range_ws if form == "ws" else rpt.probe_chain_sel_range


def run_chain(rpt, form, filters, args, mask, sel, count, max_rows, ws_poison=A5, **over):
    buf = Bufs(rpt, form, filters, max_rows, ws_poison)
    d_sel, d_count = dev(sel), device_count(count)
    chain_call(rpt, form)(filters, args, d_sel, d_count, range_mask=mask, max_rows=max_rows, **dict(buf.outputs(), **over))
    assert int(d_count.item()) == count and np.array_equal(sel_of(d_sel), sel)  # the inputs are only read
    return buf


# ---- 1. parity at every size and count --------------------------------------------------------------------------------
CASES = [(form, m, c) for form in ("one", "ws") for m in MAX_ROWS[form] for c in COUNTS]


@pytest.mark.parametrize("form,max_rows,count_name", CASES, ids=["%s-%d-%s" % c for c in CASES])
def test_chain_vs_host_expectation(rpt, pools, form, max_rows, count_name):
    """Every (max_rows, device count) pair in both forms; the chain (1, 2, 3 or 8 filters of mixed key types and column
    kinds, an unflagged HASH column among them; GATHER, LDS, hybrid and a demoted PARTITIONED stage), the mask (none,
    all, only filter 0, only the last filter) and the order of sel (ascending, or any order with repeats) rotate over
    the pairs so that each occurs at every size."""
    mi, ci = MAX_ROWS[form].index(max_rows), COUNTS.index(count_name)
    case = mi * len(COUNTS) + ci
    which = (mi + ci) % len(SPECS)
    chain = ranged_chain(rpt, pools, which, max(max_rows + 1000, 4096))
    mask = mask_of(MASKS[(ci + mi // 2) % len(MASKS)], chain.spec)
    bloom, ranged = arm(chain, mask)
    alive = bloom & ranged
    count = count_of(count_name, max_rows)
    used = min(count, max_rows)
    rng = np.random.default_rng(5000 + case)
    sel = poisoned_sel(rng, max_rows, used, alive, ascending=case % 2 == 0)
    exp = expected(sel, used, alive)
    assert_non_degenerate(sel, used, bloom, ranged, mask, exp)
    buf = run_chain(rpt, form, chain.filters, chain.args, mask, sel, count, max_rows)
    print(f"{form} max_rows {max_rows} count {count} chain {which} mask {mask:#x}: {buf.count()} of {used} survive "
          f"(host {exp.size}, Bloom alone {int(bloom[sel[:used]].sum())})")
    assert buf.count() == exp.size
    assert np.array_equal(buf.got(), exp)
    buf.assert_intact(exp.size)
    # secondary: the row-list range call, told the count by the host, returns the same
    if used:
        same = rpt.probe_chain_range_ws(chain.filters, chain.args, range_mask=mask, row_sel=dev(sel), n=used)
        assert np.array_equal(sel_of(same), exp)


@pytest.mark.parametrize("which,max_rows,used", [(THREE, 4096, 4096), (EIGHT, 16384, 16384), (EIGHT, 16384, 9000)],
                         ids=["3x8", "8x32", "8x18"])
def test_every_wave_of_the_one_launch_kernel_takes_more_than_one_item(rpt, pools, which, max_rows, used):
    """3 filters x 8 segments = 24 items and 8 filters x 32 (18) segments over the 16 waves, every value filter flagged,
    with survivors left."""
    chain = ranged_chain(rpt, pools, which, max_rows + 1000)
    mask = mask_of("all", chain.spec)
    bloom, ranged = arm(chain, mask)
    alive = bloom & ranged
    rng = np.random.default_rng(which + used)
    sel = poisoned_sel(rng, max_rows, used, alive)
    exp = expected(sel, used, alive)
    assert_non_degenerate(sel, used, bloom, ranged, mask, exp)
    for form in ("one", "ws"):
        buf = run_chain(rpt, form, chain.filters, chain.args, mask, sel, used, max_rows)
        assert buf.count() == exp.size and np.array_equal(buf.got(), exp), form
        buf.assert_intact(exp.size)


# ---- 2. every strategy kind as filter 0's later stage (ws form) ---------------------------------------------------------
KINDS0 = {"gather": (16, GATHER, GATHER), "lds": (14, LDS, LDS), "hybrid": (15, LDS, LDS), "demoted": (18, PARTITIONED, GATHER)}


@pytest.mark.parametrize("flag", ["first", "last"])
@pytest.mark.parametrize("kind", list(KINDS0))
def test_every_strategy_kind_as_filter_0s_later_stage(rpt, pools, kind, flag):
    """Filter 0 runs as a masked later stage behind the range stages: the gather, the whole filter in LDS (2^14
    blocks), the hybrid (LDS forced on 2^15 blocks) and a filter forced to PARTITIONED, which is demoted to the gather.
    With only the last filter flagged, stage 0 is that filter's range stage."""
    log_nb, strategy, want = KINDS0[kind]
    max_rows, used = 2053, 1900
    rng = np.random.default_rng(700 + log_nb)
    f0, w0, b0 = pools[0].get(log_nb)
    f1, w1, b1 = pools[1].get(13)
    c0 = probed_col(rng, "i64", "dict", 4096, b0, 0.9)
    c1 = probed_col(rng, "i32", "valid", 4096, b1, 0.9)
    f0.probe_strategy, f1.probe_strategy = strategy, AUTO
    assert f0.probe_strategy_for(max_rows) == strategy and f0.probe_sel_strategy_for(max_rows) == want
    flagged, col, kt, build = (f0, c0, "i64", b0) if flag == "first" else (f1, c1, "i32", b1)
    mm = covering_range(kt, build, 0.6)
    (f1 if flag == "first" else f0).set_minmax((0, 0))
    flagged.set_minmax(mm)
    bloom = row_pass_mask(c0, w0, log_nb) & row_pass_mask(c1, w1, 13)
    ranged = host_range_pass(col, np.arange(4096), mm)
    mask = 1 if flag == "first" else 2
    sel = poisoned_sel(rng, max_rows, used, bloom & ranged)
    exp = expected(sel, used, bloom & ranged)
    assert_non_degenerate(sel, used, bloom, ranged, mask, exp)
    buf = run_chain(rpt, "ws", [f0, f1], [c0.as_dict(rpt), c1.as_dict(rpt)], mask, sel, used, max_rows, ws_poison=FF)
    assert buf.count() == exp.size and np.array_equal(buf.got(), exp)
    buf.assert_intact(exp.size)


# ---- 3. range boundaries and NULL rows ----------------------------------------------------------------------------------
def own_filter(rpt, keys, validity=None, log_nb=10):
    """A filter holding exactly these keys (NULL rows insert NULL_HASH), and the oracle's words of it."""
    bf = rpt.BloomFilter(log_num_blocks=log_nb)
    bf.insert(dev(keys), validity=dev(validity), strategy=1)
    words = orc.new_words(log_nb)
    orc.insert_keys(words, log_nb, keys, validity=validity)
    assert np.array_equal(bf.export_words(), words)
    return bf, words


def all_forms(rpt, filters, cols, mask, alive, rng, max_rows=1543, used=1400):
    """The device-counted chain in both forms over a poisoned selection, and the row-list one-launch chain over all
    rows: each against the host expectation. Returns the row-list survivors."""
    args = [c.as_dict(rpt) for c in cols]
    sel = poisoned_sel(rng, max_rows, used, alive)
    exp = expected(sel, used, alive)
    for form in ("one", "ws"):
        buf = run_chain(rpt, form, filters, args, mask, sel, used, max_rows)
        assert buf.count() == exp.size and np.array_equal(buf.got(), exp), form
        buf.assert_intact(exp.size)
    got = rpt.probe_chain_range(filters, args, range_mask=mask, n=alive.size)
    assert np.array_equal(sel_of(got), np.flatnonzero(alive).astype(np.uint32))
    return exp


@pytest.mark.parametrize("kt", ["i64", "i32"])
def test_range_boundaries_are_inclusive(rpt, kt):
    """The filter holds min - 1, min, max and max + 1 (and more), so all four pass its Bloom test and the range decides:
    min and max stay, min - 1 and max + 1 go. Negative min; int32 keys sign-extended."""
    rng = np.random.default_rng(31 + len(kt))
    dtype = np.int64 if kt == "i64" else np.int32
    mn, mx = -1000, 1000
    edge = np.array([mn - 1, mn, mx, mx + 1, -1, 0, 1], dtype=dtype)
    inserted = np.concatenate([edge, rng.integers(-3000, 3000, 200).astype(dtype)])
    bf, words = own_filter(rpt, inserted)
    rows = 4096
    keys = np.where(rng.random(rows) < 0.7, inserted[rng.integers(0, inserted.size, rows)],
                    rng.integers(-5000, 5000, rows)).astype(dtype)
    keys[: 4 * edge.size] = np.tile(edge, 4)
    col = Col(rng, kt, "flat", rows, keys=keys)
    bloom = row_pass_mask(col, words, 10)
    try:
        for mm in ((mn, mx), (I64_MIN, I64_MAX), (mx, mx), (I64_MIN, mn - 1)):
            bf.set_minmax(mm)
            ranged = host_range_pass(col, np.arange(rows), mm)
            alive = bloom & ranged
            assert bloom[:4].all()  # min - 1, min, max, max + 1 pass the Bloom test
            if mm == (mn, mx):
                assert list(alive[:4]) == [False, True, True, False]
                assert (bloom & ~ranged).any() and (ranged & ~bloom).any() and 0 < alive.sum() < rows
            if mm == (I64_MIN, I64_MAX):
                assert np.array_equal(alive, bloom)  # no NULLs here: the range removes nothing
            all_forms(rpt, [bf], [col], 1, alive, rng)
    finally:
        bf.close()


def test_null_rows_fail_a_range_with_a_value_and_pass_one_without(rpt):
    """A NULL row was inserted into the filter, so NULL rows pass its Bloom test. Flagged with a value (even
    INT64_MIN..INT64_MAX) the NULL rows fail; flagged without a value they pass."""
    rng = np.random.default_rng(37)
    import golden_util as gu

    built = rng.integers(-(2**40), 2**40, 300).astype(np.int64)
    bvalid = np.ones(300, dtype=bool)
    bvalid[::10] = False
    bf, words = own_filter(rpt, built, validity=gu.validity_words(bvalid))
    rows = 4096
    keys = np.where(rng.random(rows) < 0.7, built[rng.integers(0, 300, rows)], rng.integers(-(2**41), 2**41, rows))
    col = Col(rng, "i64", "valid", rows, keys=keys.astype(np.int64))
    ids = np.arange(rows)
    is_null = ~host_range_pass(col, ids, (I64_MIN, I64_MAX))
    bloom = row_pass_mask(col, words, 10)
    assert is_null.any() and bloom[is_null].all()  # NULL_HASH is in the filter
    try:
        for mm in ((-(2**39), 2**39), (I64_MIN, I64_MAX), None):
            bf.set_minmax(mm)
            assert bf.minmax() == mm
            alive = bloom & host_range_pass(col, ids, mm)
            assert alive[is_null].all() if mm is None else not alive[is_null].any()
            assert 0 < alive.sum() < rows
            exp = all_forms(rpt, [bf], [col], 1, alive, rng)
            assert is_null[exp].any() == (mm is None)
    finally:
        bf.close()


# ---- 4. other contracts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "ws"])
def test_result_does_not_depend_on_filter_order(rpt, pools, form):
    max_rows, used = 2053, 2000
    chain = ranged_chain(rpt, pools, THREE, 4096)
    mask = 0b101
    bloom, ranged = arm(chain, mask)
    rng = np.random.default_rng(41)
    sel = poisoned_sel(rng, max_rows, used, bloom & ranged)
    exp = expected(sel, used, bloom & ranged)
    assert_non_degenerate(sel, used, bloom, ranged, mask, exp)
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        flags = [bool((mask >> old) & 1) for old in order]
        buf = run_chain(rpt, form, [chain.filters[i] for i in order], [chain.args[i] for i in order], flags, sel, used,
                        max_rows)
        assert buf.count() == exp.size and np.array_equal(buf.got(), exp), order
        buf.assert_intact(exp.size)


@pytest.mark.parametrize("form,max_rows", [("one", SMALL_ROWS), ("ws", 40000)])
def test_count_may_be_overwritten_in_place(rpt, pools, form, max_rows):
    """out_count_dev == count_dev: only the call's first kernel (one launch: every thread before the first barrier)
    reads the count. Also with a count of 0 stored over itself."""
    chain = ranged_chain(rpt, pools, THREE, max_rows + 1000)
    mask = mask_of("all", chain.spec)
    bloom, ranged = arm(chain, mask)
    rng = np.random.default_rng(43)
    sel = poisoned_sel(rng, max_rows, max_rows, bloom & ranged)
    exp = expected(sel, max_rows, bloom & ranged)
    assert_non_degenerate(sel, max_rows, bloom, ranged, mask, exp)
    for count, want in ((max_rows, exp), (0, exp[:0])):
        buf = Bufs(rpt, form, chain.filters, max_rows)
        d_count = device_count(count)
        _o, out_count = chain_call(rpt, form)(chain.filters, chain.args, dev(sel), d_count, range_mask=mask,
                                              max_rows=max_rows, **dict(buf.outputs(), out_count=d_count))
        assert out_count.data_ptr() == d_count.data_ptr()
        assert int(d_count.item()) == want.size
        assert np.array_equal(sel_of(buf.sel.view(torch.int32)[: want.size]), want)
        buf.assert_intact(want.size, count_guarded=False)


def test_result_does_not_depend_on_what_the_workspace_held(rpt, pools):
    """The ws form over a workspace of exactly the reported size pre-filled with 0xFF, 0xA5 and a ramp, out_sel between
    guards: identical results. The size does not depend on the mask."""
    max_rows, used = 8193, 7000
    chain = ranged_chain(rpt, pools, 2, max_rows + 1000)
    mask = mask_of("last", chain.spec)
    bloom, ranged = arm(chain, mask)
    rng = np.random.default_rng(47)
    sel = poisoned_sel(rng, max_rows, used, bloom & ranged)
    exp = expected(sel, used, bloom & ranged)
    assert_non_degenerate(sel, used, bloom, ranged, mask, exp)
    for dirt in (FF, A5, RAMP):
        buf = run_chain(rpt, "ws", chain.filters, chain.args, mask, sel, used, max_rows, ws_poison=dirt)
        assert buf.count() == exp.size and np.array_equal(buf.got(), exp)
        buf.assert_intact(exp.size)


def test_zero_rows_set_the_count_and_a_bad_mask_is_still_refused(rpt, pools, targets):
    from rpt_amd._lib import KeyColumn

    chain = ranged_chain(rpt, pools, 0, 4096)
    arm(chain, 1)
    lib = rpt.load()
    handles = (ctypes.c_void_p * 1)(chain.filters[0].handle)
    arr = (KeyColumn * 1)(rpt.make_column(**chain.args[0]))
    cnt = GuardedBuffer(8).poison(FF)
    stream = torch.cuda.current_stream().cuda_stream
    d_count = device_count(5)
    bf, base = targets.reset(14, True)
    dst = (ctypes.c_void_p * 1)(bf.handle)
    calls = {
        "chain_ws": lambda m: lib.rpt_bf_probe_chain_sel_range_ws(handles, arr, 1, m, None, d_count.data_ptr(), 0, None,
                                                                  cnt.ptr, None, 0, stream),
        "transfer_ws": lambda m: lib.rpt_bf_transfer_sel_range_ws(handles, arr, 1, m, dst, arr, 1, None, d_count.data_ptr(),
                                                                  0, None, cnt.ptr, None, 0, stream),
        "transfer_insert_ws": lambda m: lib.rpt_bf_transfer_insert_sel_range_ws(
            handles, arr, 1, m, dst, arr, 1, None, d_count.data_ptr(), 0, None, cnt.ptr, None, 0, None, 0, stream),
        "chain_one": lambda m: lib.rpt_bf_probe_chain_sel_range(handles, arr, 1, m, None, d_count.data_ptr(), 0, None,
                                                                cnt.ptr, stream),
        "transfer_one": lambda m: lib.rpt_bf_transfer_sel_range(handles, arr, 1, m, dst, arr, 1, None, d_count.data_ptr(),
                                                                0, None, cnt.ptr, stream),
        "chain_rows": lambda m: lib.rpt_bf_probe_chain_range(handles, arr, 1, m, None, 0, None, cnt.ptr, stream),
    }
    for name, call in calls.items():
        cnt.poison(FF)
        assert call(1) == 0, (name, lib.rpt_last_error())
        assert int(cnt.view(torch.int64).item()) == 0, name
        cnt.assert_guards_intact("out_count")
        cnt.poison(FF)
        assert call(0b10) == 1 and b"at or above n_filters=1" in lib.rpt_last_error(), name
        torch.cuda.synchronize()
        assert int(cnt.view(torch.int64).item()) == -1, name
    assert bf.is_empty() and np.array_equal(bf.export_words(), base)  # no destination is touched


# ---- 5. transfers -------------------------------------------------------------------------------------------------------
def transfer_case(rpt, pools, targets, call, which, mask_kind, max_rows, count, dst_specs, seed, null_dst=None,
                  no_survivor=False, rows=None):
    """One ranged transfer against the host expectation. dst_specs: (key type, column kind, log2 blocks, pre-filled,
    slot[, forced insert strategy]) per destination; two entries with one slot are the same filter listed twice.
    Returns the survivors."""
    rows = rows or max(max_rows + 1000, 4096)
    used = min(count, max_rows)
    chain = ranged_chain(rpt, pools, which, rows)
    mask = mask_of(mask_kind, chain.spec)
    bloom, ranged = arm(chain, mask)
    alive = bloom & ranged
    rng = np.random.default_rng(seed)
    passing = np.flatnonzero(alive)
    poison_rows = np.sort(rng.choice(passing, size=min(32, passing.size), replace=False))
    sel = poisoned_sel(rng, max_rows, used, alive, avoid=poison_rows)
    if no_survivor:  # positions below the count hold only rows that some test rejects
        dead = np.flatnonzero(~alive)
        sel[:used] = dead[rng.integers(0, dead.size, used)]
    exp = expected(sel, used, alive)
    if not no_survivor:
        assert_non_degenerate(sel, used, bloom, ranged, mask, exp)
    dst_cols = [dst_col(rng, s[0], s[1], rows, poison_rows) for s in dst_specs]
    if null_dst is not None:
        all_null_except(dst_cols[null_dst], poison_rows)
    slots = {}
    for s in dst_specs:
        if s[4] not in slots:
            slots[s[4]] = (s[2], targets.reset(s[2], s[3], tag=s[4]))
            forced = s[5] if len(s) > 5 else INS_AUTO
            bf = slots[s[4]][1][0]
            bf._lib.rpt_bf_set_insert_strategy(bf.handle, forced)
            if forced != INS_AUTO:
                assert bf.insert_strategy_for(max_rows) == forced
    dst = [slots[s[4]][1][0] for s in dst_specs]
    dargs = [c.as_dict(rpt) for c in dst_cols]
    form = "one" if call == "transfer_sel_range" else "ws"
    buf = Bufs(rpt, form, chain.filters, max_rows)
    kwargs = buf.outputs()
    iws = None
    try:
        if call == "transfer_insert_sel_range_ws":
            need = rpt.transfer_insert_workspace_bytes(list(dict.fromkeys(dst)), max_rows)
            assert (need > 0) == any(len(s) > 5 and s[5] == INS_PARTITIONED for s in dst_specs)
            iws = GuardedBuffer(need).poison(RAMP) if need else None
            kwargs["insert_workspace"] = iws.bytes() if iws else None
        d_sel, d_count = dev(sel), device_count(count)
        getattr(rpt, call)(chain.filters, chain.args, dst, dargs, d_sel, d_count, range_mask=mask, max_rows=max_rows,
                           **kwargs)
        assert buf.count() == exp.size
        assert np.array_equal(buf.got(), exp)
        buf.assert_intact(exp.size)
        assert int(d_count.item()) == count and np.array_equal(sel_of(d_sel), sel)
        if iws is not None:
            iws.assert_guards_intact("insert workspace")
        for slot, (L, (bf, base)) in slots.items():
            words, mm = base, None
            for c, s in zip(dst_cols, dst_specs):
                if s[4] == slot:
                    words, m = c.expect(words, L, exp)
                    mm = combine_minmax(mm, m)
            check(bf, (words, mm), f"{call}: destination slot {slot}")  # words, min/max, has_data
    finally:
        for _L, (bf, _b) in slots.values():
            bf._lib.rpt_bf_set_insert_strategy(bf.handle, INS_AUTO)
    return exp


TRANSFER_CALLS = {"transfer_sel_range": [(513, 512), (8193, 8193 + 100), (16384, 16383)],
                  "transfer_sel_range_ws": [(513, 512), (8193, 8193 + 100), (40000, 39999)],
                  "transfer_insert_sel_range_ws": [(2053, 2**40)]}
TRANSFER_CASES = [(call, m, c, n_dst) for call, shapes in TRANSFER_CALLS.items() for m, c in shapes for n_dst in (1, 2, 8)]


@pytest.mark.parametrize("call,max_rows,count,n_dst", TRANSFER_CASES, ids=["%s-%d-%d-%d" % c for c in TRANSFER_CASES])
def test_transfer_vs_host_expectation(rpt, pools, targets, call, max_rows, count, n_dst):
    """1, 2 and 8 destinations of every key type and column kind, pre-filled and empty: the words and the min/max equal
    the oracle's insert of exactly the expected survivors; out_sel and the count as for the chain alone."""
    which = (max_rows + n_dst) % 4
    dst_specs = EIGHT_DST[:n_dst] if n_dst != 2 else EIGHT_DST[1:3]  # 2: an int32 dictionary and a HASH destination
    mask_kind = MASKS[1 + (max_rows + n_dst) % 3]
    transfer_case(rpt, pools, targets, call, which, mask_kind, max_rows, count, dst_specs, seed=max_rows * 8 + n_dst)


def test_one_destination_listed_twice_in_the_one_launch_transfer(rpt, pools, targets):
    dst_specs = [("i64", "valid", 14, True, 0), ("hash", "flat", 12, False, 1), ("i32", "dict", 14, True, 0)]
    transfer_case(rpt, pools, targets, "transfer_sel_range", THREE, "all", 8192, 7000, dst_specs, seed=59)


@pytest.mark.parametrize("call", ["transfer_sel_range", "transfer_sel_range_ws"])
def test_selected_null_rows_insert_null_hash_and_move_no_minmax(rpt, pools, targets, call):
    dst_specs = [("i64", "valid", 13, False, 0), ("i32", "valid", 13, True, 1)]
    exp = transfer_case(rpt, pools, targets, call, 0, "all", 1543, 1500, dst_specs, seed=61, null_dst=0)
    assert exp.size > 0
    bf = targets._made[(13, False, 0)][0]
    null_only = orc.new_words(13)
    orc.insert_hashes(null_only, 13, np.array([NULL_HASH], dtype=np.uint64))
    assert np.array_equal(bf.export_words(), null_only) and bf.minmax() is None
    assert targets._made[(13, True, 1)][0].minmax() is not None


@pytest.mark.parametrize("how", ["count_zero", "nothing_passes"])
@pytest.mark.parametrize("call", list(TRANSFER_CALLS))
def test_an_empty_selection_leaves_has_data_set_and_the_words_unchanged(rpt, pools, targets, call, how):
    dst_specs = [("i64", "flat", 16, True, 0), ("i32", "dict", 12, False, 1)]
    exp = transfer_case(rpt, pools, targets, call, THREE, "all", 2048, 0 if how == "count_zero" else 2000, dst_specs,
                        seed=67 + len(how), no_survivor=how == "nothing_passes")
    assert exp.size == 0  # transfer_case's check(): words = base, no min/max, is_empty() False


def test_transfer_insert_routes_a_partitioned_destination(rpt, pools, targets):
    """max_rows = three 16 Ki-row tiles and a tail; one destination forced to PARTITIONED (the routed insert from the
    bits, with sel as the row mapping), a second one on atomics."""
    max_rows = kl.N_TILES
    dst_specs = [("i64", "valid", 16, True, 0, INS_PARTITIONED), ("i32", "flat", 14, False, 1)]
    exp = transfer_case(rpt, pools, targets, "transfer_insert_sel_range_ws", 2, "first", max_rows, max_rows - 4000, dst_specs,
                        seed=71, rows=max_rows + 5000)
    assert 0 < exp.size < max_rows - 4000


# ---- 6. range_mask == 0 runs the twin's kernels -------------------------------------------------------------------------
@contextlib.contextmanager
def recording():
    """{kernel name: launches} of exactly the launches made inside the block (rpt_profiling_*)."""
    from rpt_amd import _lib

    rec = {}
    torch.cuda.synchronize()
    _lib.profiling_reset()
    _lib.profiling(True)
    try:
        yield rec
        torch.cuda.synchronize()
    finally:
        _lib.profiling(False)
    rec.update({name: launches for name, (launches, _ms) in _lib.kernel_times().items()})
    _lib.profiling_reset()


def test_a_zero_mask_runs_exactly_the_twins_kernels(rpt, pools, targets):
    max_rows, used = 2053, 1800
    chain = ranged_chain(rpt, pools, THREE, 4096)
    bloom, _ranged = arm(chain, 0)  # every range hostile: applied anywhere, it would show
    rng = np.random.default_rng(73)
    sel = poisoned_sel(rng, max_rows, used, bloom)
    exp = expected(sel, used, bloom)
    assert 0 < exp.size < used
    d_sel = dev(sel)
    dcol = Col(rng, "i64", "valid", 4096)
    f, a = chain.filters, chain.args

    def counted(name, form, transfer, **extra):
        def call(masked):
            buf = Bufs(rpt, form, f, max_rows)
            kw = dict(buf.outputs(), max_rows=max_rows, **extra)
            if masked:
                name_, kw = name.replace("_sel", "_sel_range"), dict(kw, range_mask=0)
            else:
                name_ = name
            bf, base = targets.reset(12, True)
            lists = (f, a, [bf], [dcol.as_dict(rpt)]) if transfer else (f, a)
            with recording() as rec:
                getattr(rpt, name_)(*lists, d_sel, device_count(used), **kw)
            assert buf.count() == exp.size and np.array_equal(buf.got(), exp), name_
            if transfer:
                check(bf, dcol.expect(base, 12, exp), name_)
            return rec
        return call

    def row_list(masked):
        with recording() as rec:
            got = (rpt.probe_chain_range(f, a, range_mask=0, row_sel=d_sel, n=used) if masked else
                   rpt.probe_chain(f, a, row_sel=d_sel, n=used))
        assert np.array_equal(sel_of(got), exp)
        return rec

    calls = {"probe_chain_sel_ws": counted("probe_chain_sel_ws", "ws", False),
             "transfer_sel_ws": counted("transfer_sel_ws", "ws", True),
             "transfer_insert_sel_ws": counted("transfer_insert_sel_ws", "ws", True, insert_workspace=None),
             "probe_chain_sel": counted("probe_chain_sel", "one", False),
             "transfer_sel": counted("transfer_sel", "one", True),
             "probe_chain": row_list}
    for name, call in calls.items():
        twin, masked = call(False), call(True)
        assert twin and masked == twin, (name, masked, twin)
        assert not {kl.base_name(k) for k in masked} & set(NEW_BASES), (name, masked)
    # ... and with a bit set the new kernels are what run
    arm(chain, 1)
    buf = Bufs(rpt, "ws", f, max_rows)
    with recording() as rec:
        rpt.probe_chain_sel_range_ws(f, a, d_sel, device_count(used), range_mask=1, max_rows=max_rows, **buf.outputs())
    assert "range_bits_sel_kernel" in {kl.base_name(k) for k in rec}
    assert "probe_bits_sel_kernel" not in {kl.base_name(k) for k in rec}
    buf = Bufs(rpt, "one", f, max_rows)
    with recording() as rec:
        rpt.probe_chain_sel_range(f, a, d_sel, device_count(used), range_mask=1, max_rows=max_rows, **buf.outputs())
    assert list(rec) == ["probe_chain_range_small_kernel<true,false>"] and rec[list(rec)[0]] == 1


# ---- 7. the row-list one-launch chain -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_row_sel", [False, True], ids=["rows", "row_sel"])
@pytest.mark.parametrize("n", [1, 513, SMALL_ROWS])
def test_probe_chain_range_vs_host_expectation(rpt, pools, n, with_row_sel):
    """rpt_bf_probe_chain_range with and without row_sel against the same host expectation, and against
    rpt_bf_probe_chain_range_ws for the same arguments."""
    rows = max(n + 1000, 4096)
    chain = ranged_chain(rpt, pools, THREE, rows)
    mask = mask_of("all", chain.spec)
    bloom, ranged = arm(chain, mask)
    alive = bloom & ranged
    rng = np.random.default_rng(79 + n)
    row_sel = rng.integers(0, rows, n).astype(np.uint32) if with_row_sel else None  # any order, with repeats
    ids = row_sel if with_row_sel else np.arange(n, dtype=np.uint32)
    exp = ids[alive[ids]]
    assert_non_degenerate(ids, n, bloom, ranged, mask, exp)
    out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    got = rpt.probe_chain_range(chain.filters, chain.args, range_mask=mask, row_sel=dev(row_sel), n=n,
                                out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64))
    assert int(cnt.view(torch.int64).item()) == exp.size and np.array_equal(sel_of(got), exp)
    assert bool(torch.all(out.view(torch.int32)[exp.size:] == -1)), "out_sel written past the returned count"
    for name, g in (("out_sel", out), ("out_count", cnt)):
        g.assert_guards_intact(name)
    same = rpt.probe_chain_range_ws(chain.filters, chain.args, range_mask=mask, row_sel=dev(row_sel), n=n)
    assert np.array_equal(sel_of(same), exp)


def test_probe_chain_range_past_the_limit_is_refused(rpt, pools):
    chain = ranged_chain(rpt, pools, 0, SMALL_ROWS + 1000)
    arm(chain, 1)
    n = SMALL_ROWS + 1
    out_sel = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_count = device_count(-1)
    with pytest.raises(rpt.RptError) as e:
        rpt.probe_chain_range(chain.filters, chain.args, range_mask=1, n=n, out_sel=out_sel, out_count=out_count)
    assert e.value.status == 1 and "exceeds RPT_SMALL_PROBE_ROWS" in str(e.value)
    torch.cuda.synchronize()
    assert int(out_count.item()) == -1 and bool(torch.all(out_sel == -1))
