"""The min/max range stage (rpt_bf_range_bits, rpt_bf_probe_chain_range_ws, rpt_bf_transfer_range_ws,
rpt_bf_transfer_insert_range_ws) on the GPU, bit-exact.

Expectation for a flagged column: (valid & (keys >= mn) & (keys <= mx)) in numpy, the keys gathered through key_sel /
row_sel as the call sees them and int32 compared as int64; a filter without a value passes every row. It is ANDed with
orc.probe_keys per filter. mn, mx come from orc.minmax of the build keys or from the values given to set_minmax.

The probed filters come from buf_util.FilterCache (two caches of this module's own, never inserted into; their min/max is
set freely, which no other module sees)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import rpt_oracle as orc
from buf_util import (A5, CAPTURE_MODE_GLOBAL, FF, RAMP, FilterCache, GuardedBuffer, graph_destroy, graph_instantiate,
                      graph_launch, int32_build_keys, stream_capture)
from test_gpu_transfer import Col, Targets, bits_words, check, dev, sel_of

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED, BUCKETED = 0, 1, 2, 3, 4
INS_ATOMIC, INS_PARTITIONED = 1, 2
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
DTYPES = {"i64": np.int64, "i32": np.int32}


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


@pytest.fixture(scope="module")
def targets(rpt):
    t = Targets(rpt)
    yield t
    t.close()


@pytest.fixture(scope="module")
def scratch_filter(rpt):
    """A small filter whose min/max the range_bits tests set; its words are never read by the range test."""
    bf = rpt.BloomFilter(log_num_blocks=10)
    yield bf
    bf.close()


# ---- the numpy expectation ---------------------------------------------------------------------------------------
def valid_bits(validity, phys):
    if validity is None:
        return np.ones(phys.size, dtype=bool)
    p = phys.astype(np.uint64)
    return ((validity[p >> np.uint64(6)] >> (p & np.uint64(63))) & np.uint64(1)).astype(bool)


def range_pass(keys, phys, validity, mm):
    """The range test of the rows whose physical key indices are `phys`: a bool per probed row."""
    if mm is None:
        return np.ones(phys.size, dtype=bool)
    v = keys[phys].astype(np.int64)
    return valid_bits(validity, phys) & (v >= mm[0]) & (v <= mm[1])


def misaligned(t: torch.Tensor) -> torch.Tensor:
    """The same values at a base that is 8-byte but not 16-byte aligned."""
    shift = 8 // t.element_size()
    raw = torch.empty(t.numel() + shift, dtype=t.dtype, device=t.device)
    raw[shift:].copy_(t)
    out = raw[shift:]
    assert out.data_ptr() % 16 == 8
    return out


# ---- 1. range_bits against numpy -----------------------------------------------------------------------------------
RANGES = {
    # pinned with set_minmax; the keys equal to min and max, and min - 1 and max + 1, are planted in the column
    "i64": [(-1000, 1000), (-(2**40), -(2**20)), (I64_MIN, I64_MAX), (7, 7), (I64_MIN, -1), (0, I64_MAX)],
    # negative min; wholly negative; everything; min == max; a range past int32 that a zero-extended -1 would enter
    "i32": [(-1000, 1000), (-(2**31), -(2**10)), (I64_MIN, I64_MAX), (7, 7), (2**31, 2**40), (-(2**40), -(2**31))],
}
KINDS = ["flat", "nulls", "dict", "row_sel", "misaligned"]


def boundary_keys(kt):
    info = np.iinfo(DTYPES[kt])
    vals = []
    for lo, hi in RANGES[kt]:
        vals += [lo, hi, lo - 1, hi + 1]
    return np.array(sorted({v for v in vals if info.min <= v <= info.max}), dtype=DTYPES[kt])


class RangeCase:
    """n probed rows of a column of kind `kind`: physical keys (small values, full-range values and every boundary
    value), validity, key_sel, row_sel, and phys = the physical key index of each probed row."""

    def __init__(self, kt, kind, n, seed):
        rng = np.random.default_rng(seed)
        dtype, info = DTYPES[kt], np.iinfo(DTYPES[kt])
        rows = n + n // 2 + 3 if kind == "row_sel" else n
        m = rows // 2 + 1 if kind == "dict" else rows
        keys = np.where(rng.random(m) < 0.5, rng.integers(-3000, 3000, m),
                        rng.integers(info.min, info.max, m, endpoint=True)).astype(dtype)
        planted = boundary_keys(kt)
        at = rng.choice(m, size=min(m, planted.size), replace=False)
        keys[at] = rng.permutation(planted)[: at.size]
        self.keys = keys
        self.validity = gu.validity_words(rng.random(m) < 0.9) if kind in ("nulls", "dict") else None
        self.key_sel = rng.integers(0, m, rows).astype(np.uint32) if kind == "dict" else None
        self.row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if kind == "row_sel" else None
        r = self.row_sel if self.row_sel is not None else np.arange(n, dtype=np.uint32)
        self.phys = (self.key_sel[r] if self.key_sel is not None else r).astype(np.int64)
        self.n = n
        self.d_keys = misaligned(dev(keys)) if kind == "misaligned" else dev(keys)
        assert self.d_keys.data_ptr() % 16 == (8 if kind == "misaligned" else 0)
        self.kw = dict(n=n, row_sel=dev(self.row_sel), key_sel=dev(self.key_sel), validity=dev(self.validity))

    def expect(self, mm):
        return range_pass(self.keys, self.phys, self.validity, mm)


def got_bits(bf, case):
    """range_bits into an exactly sized, FF-poisoned buffer between guards: the words written."""
    need = (case.n + 511) // 512 * 8
    out = GuardedBuffer(need * 8).poison(FF)
    bf.range_bits(case.d_keys, out=out.view(torch.int64), **case.kw)
    torch.cuda.synchronize()
    out.assert_guards_intact("out_bits")
    return out.view(torch.int64).cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kt", ["i64", "i32"])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 16385, 70001])
def test_range_bits_vs_numpy(rpt, scratch_filter, n, kt, kind):
    bf = scratch_filter
    case = RangeCase(kt, kind, n, seed=n * 7 + len(kind) + (kt == "i32"))
    for mm in RANGES[kt]:
        bf.set_minmax(mm)
        exp = case.expect(mm)
        assert np.array_equal(got_bits(bf, case), bits_words(exp)), (mm, int(exp.sum()))
        if n >= 16385 and mm == RANGES[kt][0]:
            assert 0 < exp.sum() < n  # the range matters
    # no value: every row i < n passes, NULL rows included, and the bits past n are 0
    bf.set_minmax(None)
    assert np.array_equal(got_bits(bf, case), bits_words(np.ones(n, dtype=bool)))


def test_range_bits_boundaries_are_inclusive(rpt, scratch_filter):
    """min, max, min - 1, max + 1 side by side, int64 and int32 (negative min), dense."""
    for kt, (lo, hi) in (("i64", (-5, 9)), ("i32", (-5, 9)), ("i64", (I64_MIN + 1, I64_MAX - 1))):
        keys = np.array([lo, hi, lo - 1, hi + 1, lo + 1, hi - 1], dtype=np.int64)
        scratch_filter.set_minmax((lo, hi))
        bits = scratch_filter.range_bits(dev(keys.astype(DTYPES[kt]) if kt == "i32" else keys)).cpu().numpy().view(np.uint64)
        assert int(bits[0]) == 0b110011 and not bits[1:].any(), (kt, lo, hi, bin(int(bits[0])))


def test_range_bits_of_a_fresh_and_a_cleared_filter_passes_every_row(rpt):
    n = 1500
    rng = np.random.default_rng(3)
    keys = rng.integers(-100, 100, n).astype(np.int64)
    validity = gu.validity_words(rng.random(n) < 0.5)
    bf = rpt.BloomFilter(log_num_blocks=10)
    everything = bits_words(np.ones(n, dtype=bool))
    assert bf.minmax() is None
    assert np.array_equal(bf.range_bits(dev(keys), validity=dev(validity)).cpu().numpy().view(np.uint64), everything)
    bf.insert(dev(keys), validity=dev(validity))
    mm = orc.minmax(keys, validity=validity)
    assert bf.minmax() == mm
    probe = rng.integers(-200, 200, n).astype(np.int64)
    exp = range_pass(probe, np.arange(n), validity, mm)
    assert 0 < exp.sum() < n
    assert np.array_equal(bf.range_bits(dev(probe), validity=dev(validity)).cpu().numpy().view(np.uint64), bits_words(exp))
    bf.clear()  # resets the min/max; the deferred clear of the words is settled by the call, as a probe settles it
    assert np.array_equal(bf.range_bits(dev(probe), validity=dev(validity)).cpu().numpy().view(np.uint64), everything)
    bf.close()


def test_range_bits_after_an_insert_of_clustered_keys(rpt):
    """The min/max a real insert folded: build ids 40000..59999; a probe column sorted by id, so whole segments die."""
    build = np.arange(40000, 60000, dtype=np.int64)
    bf = rpt.BloomFilter(len(build))
    bf.insert(dev(np.random.default_rng(4).permutation(build)))
    assert bf.minmax() == orc.minmax(build) == (40000, 59999)
    for kt in ("i64", "i32"):
        probe = np.arange(0, 100001, dtype=DTYPES[kt])
        bits = bf.range_bits(dev(probe)).cpu().numpy().view(np.uint64)
        exp = (probe >= 40000) & (probe <= 59999)
        assert np.array_equal(bits, bits_words(exp))
        assert not bits[: 40000 // 512 * 8].any() and not bits[(60000 + 511) // 512 * 8:].any()
    bf.close()


def test_range_bits_refusals(rpt, scratch_filter):
    from rpt_amd._lib import RPT_ERR_INVALID_ARGUMENT

    keys = dev(np.arange(100, dtype=np.int64))
    with pytest.raises(rpt.RptError) as e:
        scratch_filter.range_bits(keys, key_type=rpt.RPT_KEY_HASH)
    assert e.value.status == RPT_ERR_INVALID_ARGUMENT and "hashes" in str(e.value)
    out = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    scratch_filter.range_bits(keys, n=0, out=out)  # a no-op
    torch.cuda.synchronize()
    assert bool((out == -1).all())


def test_range_bits_where_a_wave_owns_three_full_segments(rpt, scratch_filter):
    """The grid is persistent: at most kBlocksPerCU = 8 workgroups of kWavesPerBlock = 4 waves per CU (persistent_grid
    in csrc/rpt_gpu.hip), so W = CUs * 8 * 4 waves at the most, wave w owning segments w, w + W, w + 2 W, ... With
    n = (3 W + 5) * 512 + 77 rows every wave owns at least three full 512-row segments, five own a fourth, and one more
    the 77-row tail: a software-pipelined full-segment loop would run its prologue, steady state and epilogue."""
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4
    n = (3 * waves + 5) * 512 + 77
    rng = np.random.default_rng(5)
    keys = rng.integers(-(2**40), 2**40, n, dtype=np.int64)
    mm = (-(2**39), 2**38)
    scratch_filter.set_minmax(mm)
    exp = (keys >= mm[0]) & (keys <= mm[1])
    bits = scratch_filter.range_bits(dev(keys)).cpu().numpy().view(np.uint64)
    assert n // 3 < exp.sum() < n // 2
    assert np.array_equal(bits, bits_words(exp))


# ---- 2. the chain against the oracle -----------------------------------------------------------------------------
SUB_I64 = (-(2**61), 2**61)  # a sub-interval of the int64 build keys (drawn from +-2^62)
SUB_I32 = (-(2**30), 2**30 - 1)  # ... and of the build keys an int32 column can hit (uniform over int32)


def split_pool(pool, sub):
    inside = (pool >= sub[0]) & (pool <= sub[1])
    assert inside.any() and (~inside).any()
    return pool[inside], pool[~inside]


def constructed_column(rng, build, dtype, sub, n, slot):
    """n keys, a third of them (rows i = 3 j) drawn from the filter's build pool, the rest random. Bit `slot` of j
    decides whether row 3 j's pool key lies inside the sub-interval `sub` (0) or outside it (1): inserted keys always
    pass the Bloom test, so the rows with the bit set pass the filter and fail its range, and the rows j = 0 mod 2^k
    lie inside every filter's sub-interval: whatever the mask, some rows survive and the range removes some."""
    pool = build if dtype == np.int64 else int32_build_keys(build)
    inside, outside = split_pool(pool, sub)
    info = np.iinfo(dtype)
    keys = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    j = np.arange(0, n, 3) // 3
    out_bit = ((j >> slot) & 1).astype(bool)
    hit = np.where(out_bit, outside[rng.integers(0, outside.size, j.size)], inside[rng.integers(0, inside.size, j.size)])
    keys[::3] = hit.astype(dtype)
    return keys


def chain_expectation(per_filter, mask):
    """per_filter: [(bloom ref ids, range pass bools)]; -> (expected ids, bloom-only ids)."""
    bloom = functools.reduce(np.intersect1d, [r for r, _p in per_filter])
    alive = np.ones(per_filter[0][1].size, dtype=bool)
    for f, (_r, p) in enumerate(per_filter):
        if (mask >> f) & 1:
            alive &= p
    exp = bloom[alive[bloom]]
    return exp.astype(np.uint32), bloom.astype(np.uint32)


def permuted_mask(mask, order):
    return sum(1 << new for new, old in enumerate(order) if (mask >> old) & 1)


@functools.lru_cache(maxsize=None)
def mixed_columns(n):
    """The three columns of test_chain_ws_mixed_columns_vs_oracle (int64 FLAT, int32 with 10 % NULLs, int64
    DICTIONARY), constructed so that the ranges matter; computed once per n and left unchanged."""
    rng = np.random.default_rng(n)
    from buf_util import build_keys_for

    b0, b1, b2 = (build_keys_for(L) for L in (11, 15, 21))
    c0 = constructed_column(rng, b0, np.int64, SUB_I64, n, 0)
    c1 = constructed_column(rng, b1, np.int32, SUB_I32, n, 1)
    valid1 = rng.random(n) < 0.9
    valid1[::24] = True  # the rows inside every sub-interval stay valid: survivors by construction
    vw1 = gu.validity_words(valid1)
    logical2 = constructed_column(rng, b2, np.int64, SUB_I64, n, 2)
    perm = rng.permutation(n)
    dict2 = logical2[perm]
    ksel2 = np.argsort(perm).astype(np.uint32)  # dict2[ksel2[i]] == logical2[i]
    assert np.array_equal(dict2[ksel2], logical2)
    return c0, c1, vw1, dict2, ksel2


@pytest.mark.parametrize("mask", [0b001, 0b010, 0b101, 0b111])
@pytest.mark.parametrize("n", [513, 16385, 70001])
def test_chain_range_mixed_columns_vs_oracle(rpt, caches, n, mask):
    (f0, w0, _b0), (f1, w1, _b1), (f2, w2, _b2) = (caches[0].get(L) for L in (11, 15, 21))
    for f in (f0, f1, f2):
        f.probe_strategy = AUTO
    c0, c1, vw1, dict2, ksel2 = mixed_columns(n)
    ident = np.arange(n, dtype=np.int64)
    subs = [SUB_I64, SUB_I32, SUB_I64]
    for f, sub in zip((f0, f1, f2), subs):
        f.set_minmax(sub)
    per_filter = [
        (orc.probe_keys(w0, 11, c0), range_pass(c0, ident, None, subs[0])),
        (orc.probe_keys(w1, 15, c1, validity=vw1), range_pass(c1, ident, vw1, subs[1])),
        (orc.probe_keys(w2, 21, dict2, key_sel=ksel2), range_pass(dict2, ksel2.astype(np.int64), None, subs[2])),
    ]
    exp, bloom_only = chain_expectation(per_filter, mask)
    assert 0 < len(exp) < len(bloom_only)
    filters = [f0, f1, f2]
    cols = [dev(c0), {"keys": dev(c1), "validity": dev(vw1)}, {"keys": dev(dict2), "key_sel": dev(ksel2)}]
    got = rpt.probe_chain_range_ws(filters, cols, range_mask=mask, n=n)
    assert np.array_equal(sel_of(got), exp)
    # the mask as a sequence of bools; and the order of the filters does not change the result
    order = (2, 0, 1)
    flags = [bool((mask >> old) & 1) for old in order]
    got = rpt.probe_chain_range_ws([filters[i] for i in order], [cols[i] for i in order], range_mask=flags, n=n)
    assert np.array_equal(sel_of(got), exp)
    assert permuted_mask(mask, order) == sum(1 << i for i, fl in enumerate(flags) if fl)


STAGES = {"gather": (GATHER, 16), "lds": (LDS, 13), "hybrid": (LDS, 16), "partitioned": (PARTITIONED, 18),
          "bucketed": (BUCKETED, 22)}  # the table of test_gpu_chain_ws.py
N_STAGES = 70001


@functools.lru_cache(maxsize=None)
def stage_pair(kind):
    """(column of the stage filter, column of the partner gather filter) and their oracle parts, once per kind."""
    from buf_util import build_keys_for

    rng = np.random.default_rng(50 + list(STAGES).index(kind))
    ck = constructed_column(rng, build_keys_for(STAGES[kind][1]), np.int64, SUB_I64, N_STAGES, 0)
    cp = constructed_column(rng, build_keys_for(16), np.int64, SUB_I64, N_STAGES, 1)
    return ck, cp


@pytest.mark.parametrize("position", ["filter0", "later"])
@pytest.mark.parametrize("kind", list(STAGES))
def test_chain_range_every_stage_kind_in_both_positions(rpt, caches, kind, position):
    """Every stage kind once as filter 0 (which runs as a masked or routed later stage behind its own range stage) and
    once as a later filter behind the partner's range stage."""
    n = N_STAGES
    strategy, L = STAGES[kind]
    fk, wk, _ = caches[0].get(L)
    fp, wp, _ = caches[1].get(16)
    fk.probe_strategy = strategy
    fp.probe_strategy = GATHER
    assert fk.probe_strategy_for(n) == strategy
    ck, cp = stage_pair(kind)
    ident = np.arange(n, dtype=np.int64)
    fk.set_minmax(SUB_I64)
    fp.set_minmax(SUB_I64)
    part_k = (orc.probe_keys(wk, L, ck), range_pass(ck, ident, None, SUB_I64))
    part_p = (orc.probe_keys(wp, 16, cp), range_pass(cp, ident, None, SUB_I64))
    if position == "filter0":
        filters, cols, parts = [fk, fp], [dev(ck), dev(cp)], [part_k, part_p]
    else:
        filters, cols, parts = [fp, fk], [dev(cp), dev(ck)], [part_p, part_k]
    exp, bloom_only = chain_expectation(parts, 0b01)
    assert 0 < len(exp) < len(bloom_only)
    need = rpt.probe_chain_range_workspace_bytes(filters, 0b01, n)
    plain = rpt.probe_chain_workspace_bytes(filters, n)
    # the temporary bits are present whenever any filter routes, filter 0 included
    routes0 = position == "filter0" and strategy in (PARTITIONED, BUCKETED)
    assert need == plain + (((n + 511) // 512 * 64 + 255) & ~255 if routes0 else 0)
    ws = GuardedBuffer(need).poison(A5)
    got = rpt.probe_chain_range_ws(filters, cols, range_mask=0b01, n=n, workspace=ws.bytes())
    assert np.array_equal(sel_of(got), exp)
    ws.assert_guards_intact("workspace")
    fk.probe_strategy = AUTO
    fp.probe_strategy = AUTO


# ---- 3. range_mask == 0 is the non-range call ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [513, 16385])
def test_range_mask_zero_is_the_plain_chain(rpt, caches, n):
    (f0, _w0, _), (f1, _w1, _) = caches[0].get(11), caches[0].get(15)
    for f in (f0, f1):
        f.probe_strategy = AUTO
        f.set_minmax((0, 0))  # would kill nearly every row if it were applied
    c0, c1, vw1, _d, _k = mixed_columns(n)
    filters, cols = [f0, f1], [dev(c0), {"keys": dev(c1), "validity": dev(vw1)}]
    need = rpt.probe_chain_range_workspace_bytes(filters, 0, n)
    assert need == rpt.probe_chain_workspace_bytes(filters, n) > 0
    assert need == rpt.probe_chain_range_workspace_bytes(filters, [False, False], n)
    plain = rpt.probe_chain_ws(filters, cols, n=n)
    assert 0 < plain.numel() < n
    ws = GuardedBuffer(need).poison(A5)
    out_count = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    got = rpt.probe_chain_range_ws(filters, cols, range_mask=0, n=n, workspace=ws.bytes(), out_count=out_count)
    assert torch.equal(got, plain) and int(out_count.item()) == plain.numel()
    # the small-batch hand-over is the plain call's: one launch, the workspace untouched
    assert bool(torch.all(ws.bytes() == 0xA5)) == (n == 513)
    ws.assert_guards_intact("workspace")
    # ... and with a bit set the same n takes the workspace path
    ws.poison(A5)
    f0.set_minmax(SUB_I64)
    ranged = rpt.probe_chain_range_ws(filters, cols, range_mask=1, n=n, workspace=ws.bytes())
    assert 0 < ranged.numel() < plain.numel()
    assert not bool(torch.all(ws.bytes() == 0xA5))


# ---- 4. transfers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["transfer_range_ws", "transfer_insert_range_ws"])
def test_transfer_range_vs_oracle(rpt, caches, targets, call):
    """Two probed filters (the first flagged), one atomic and one PARTITIONED destination at n = 70001: out_sel and the
    count are the range chain's, the destinations' words and min/max equal rpt_bf_insert of exactly those rows."""
    from rpt_amd import _lib

    n = 70001
    rng = np.random.default_rng(61)
    (f0, w0, _), (f1, w1, _) = caches[0].get(16), caches[1].get(13)
    f0.probe_strategy = GATHER
    f1.probe_strategy = AUTO
    f0.set_minmax(SUB_I64)
    ck, cp = stage_pair("lds")  # (2^13 build pool, 2^16 build pool)
    ident = np.arange(n, dtype=np.int64)
    parts = [(orc.probe_keys(w0, 16, cp), range_pass(cp, ident, None, SUB_I64)), (orc.probe_keys(w1, 13, ck), None)]
    exp, bloom_only = chain_expectation(parts, 0b01)
    assert 0 < len(exp) < len(bloom_only)
    specs = [("i64", "valid", 14, INS_ATOMIC), ("i32", "dict", 18, INS_PARTITIONED)]
    dcols = [Col(rng, kt, kind, n) for kt, kind, _L, _s in specs]
    dst = [targets.reset(L, True, tag=j) for j, (_kt, _kind, L, _s) in enumerate(specs)]
    for (bf, _b), spec in zip(dst, specs):
        _lib.check(rpt.load().rpt_bf_set_insert_strategy(bf.handle, spec[3]))
        assert bf.insert_strategy_for(n) == spec[3]
    dst_filters = [bf for bf, _b in dst]
    sel, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    kw = dict(range_mask=0b01, n=n, out_sel=sel.view(torch.int32), out_count=cnt.view(torch.int64))
    out_sel, out_count = getattr(rpt, call)([f0, f1], [dev(cp), dev(ck)], dst_filters, [c.as_dict(rpt) for c in dcols], **kw)
    assert int(out_count.item()) == len(exp)
    assert np.array_equal(sel_of(out_sel[: len(exp)]), exp)
    assert bool(torch.all(out_sel[len(exp):] == -1)), "out_sel written past the count"
    for (bf, base), c, spec in zip(dst, dcols, specs):
        check(bf, c.expect(base, spec[2], exp), f"{call}: destination {spec}")
    for name, g in (("out_sel", sel), ("out_count", cnt)):
        g.assert_guards_intact(name)
    # flagging a HASH column is refused before anything is written
    before = [bf.export_words() for bf in dst_filters]
    hashed = {"keys": rpt.hash_keys(dev(ck)), "key_type": rpt.RPT_KEY_HASH}
    cnt.poison(FF)
    with pytest.raises(rpt.RptError) as e:
        getattr(rpt, call)([f0, f1], [dev(cp), hashed], dst_filters, [c.as_dict(rpt) for c in dcols],
                           **dict(kw, range_mask=0b10))
    assert e.value.status == _lib.RPT_ERR_INVALID_ARGUMENT and "hashes" in str(e.value)
    torch.cuda.synchronize()
    assert int(cnt.view(torch.int64).item()) == -1
    for bf, b in zip(dst_filters, before):
        assert np.array_equal(bf.export_words(), b)
    for bf in dst_filters:
        _lib.check(rpt.load().rpt_bf_set_insert_strategy(bf.handle, 0))
    f0.probe_strategy = AUTO


# ---- 5. capture -----------------------------------------------------------------------------------------------------
def test_chain_range_graph_capture_reads_the_range_at_replay(rpt, caches):
    """probe_chain_range_ws captured at n = 16385 and replayed; then set_minmax to another range outside the capture
    and replayed again: each replay applies the min/max the filter holds by then."""
    from rpt_amd._lib import KeyColumn

    n = 16385
    (f0, w0, _), (f1, w1, _) = caches[0].get(13), caches[1].get(16)
    f0.probe_strategy = AUTO
    f1.probe_strategy = GATHER
    ck, cp = stage_pair("lds")
    ck, cp = ck[:n], cp[:n]
    k0, k1 = dev(ck), dev(cp)
    ident = np.arange(n, dtype=np.int64)
    blooms = [orc.probe_keys(w0, 13, ck), orc.probe_keys(w1, 16, cp)]
    ranges = [SUB_I64, (-(2**60), 2**62)]

    def expected(mm):
        return chain_expectation([(blooms[0], range_pass(ck, ident, None, mm)), (blooms[1], None)], 0b01)[0]

    filters = [f0, f1]
    handles = (ctypes.c_void_p * 2)(*[f.handle for f in filters])
    arr = (KeyColumn * 2)(rpt.make_column(k0), rpt.make_column(k1))
    out_sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(rpt.probe_chain_range_workspace_bytes(filters, 0b01, n), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)

    def call():
        return rpt.load().rpt_bf_probe_chain_range_ws(handles, arr, 2, 0b01, None, n, out_sel.data_ptr(),
                                                      out_count.data_ptr(), ws.data_ptr(), ws.numel(), sh)

    f0.set_minmax(ranges[0])
    assert call() == 0  # once outside any capture (the kernels' first launch sets their LDS allowance)
    s.synchronize()
    assert np.array_equal(sel_of(out_sel[: int(out_count.item())]), expected(ranges[0]))
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, call)
    assert end == 0 and st == 0, rpt.load().rpt_last_error()
    assert graph_instantiate(graph, exe) == 0
    results = []
    for mm in ranges:
        f0.set_minmax(mm)  # outside the capture
        out_sel.fill_(-1)
        out_count.fill_(-1)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        exp = expected(mm)
        assert 0 < len(exp) < len(np.intersect1d(*blooms))
        assert int(out_count.item()) == len(exp)
        assert np.array_equal(sel_of(out_sel[: len(exp)]), exp), mm
        results.append(exp)
    assert not np.array_equal(results[0], results[1])
    assert graph_destroy(exe, graph)
    f1.probe_strategy = AUTO


# ---- 6. workspace hygiene ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routed_first", [False, True])
def test_chain_range_buffer_hygiene(rpt, caches, routed_first):
    """Exactly the reported workspace and exactly n out_sel entries between guard bands, poisoned with A5, FF and a
    ramp in turn: the same (expected) result every time, guards intact. With the PARTITIONED filter first the
    temporary bits exist only in the range layout."""
    n = 70001
    fd, wd, _ = caches[0].get(16)
    fp, wp, _ = caches[1].get(18)
    fd.probe_strategy = GATHER
    fp.probe_strategy = PARTITIONED
    ck, cp = stage_pair("partitioned")  # (2^18 build pool, 2^16 build pool)
    ident = np.arange(n, dtype=np.int64)
    fd.set_minmax(SUB_I64)
    fp.set_minmax(SUB_I64)
    part_d = (orc.probe_keys(wd, 16, cp), range_pass(cp, ident, None, SUB_I64))
    part_p = (orc.probe_keys(wp, 18, ck), range_pass(ck, ident, None, SUB_I64))
    if routed_first:
        filters, cols, parts = [fp, fd], [dev(ck), dev(cp)], [part_p, part_d]
    else:
        filters, cols, parts = [fd, fp], [dev(cp), dev(ck)], [part_d, part_p]
    exp, bloom_only = chain_expectation(parts, 0b11)
    assert 0 < len(exp) < len(bloom_only)
    need = rpt.probe_chain_range_workspace_bytes(filters, 0b11, n)
    assert need > 0 and need % 256 == 0
    ws, sel, cnt = GuardedBuffer(need), GuardedBuffer(4 * n), GuardedBuffer(8)
    results = []
    for pattern in (A5, FF, RAMP):
        for g in (ws, sel, cnt):
            g.poison(pattern)
        got = rpt.probe_chain_range_ws(filters, cols, range_mask=0b11, n=n, out_sel=sel.view(torch.int32),
                                       out_count=cnt.view(torch.int64), workspace=ws.bytes())
        results.append(sel_of(got).copy())
        assert np.array_equal(results[-1], exp), pattern
        for name, g in (("workspace", ws), ("out_sel", sel), ("out_count", cnt)):
            g.assert_guards_intact(f"{pattern}: {name}")
    assert all(np.array_equal(r, results[0]) for r in results)
    # one byte short, and a base offset by 8: refused before any launch
    from rpt_amd._lib import RPT_ERR_INVALID_ARGUMENT, RPT_ERR_WORKSPACE

    cnt.poison(FF)
    shifted = GuardedBuffer(need + 16).bytes()[8: 8 + need]
    for workspace, status in ((ws.bytes()[: need - 1], RPT_ERR_WORKSPACE), (shifted, RPT_ERR_INVALID_ARGUMENT)):
        with pytest.raises(rpt.RptError) as e:
            rpt.probe_chain_range_ws(filters, cols, range_mask=0b11, n=n, out_sel=sel.view(torch.int32),
                                     out_count=cnt.view(torch.int64), workspace=workspace)
        assert e.value.status == status
    torch.cuda.synchronize()
    assert int(cnt.view(torch.int64).item()) == -1
    # n == 0 sets the count and nothing else
    assert rpt.probe_chain_range_ws(filters, cols, range_mask=0b11, n=0, out_count=cnt.view(torch.int64)).numel() == 0
    assert int(cnt.view(torch.int64).item()) == 0
    fd.probe_strategy = AUTO
    fp.probe_strategy = AUTO
