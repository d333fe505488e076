"""Every row of the sixth kernel ledger (tests/kernel_ledger_sel_range.py) on the GPU: one ranged device-counted or
one-launch call over two flagged filters, whose result equals the expectation (numpy's range test, ANDed with the
oracle's probe per filter; for the transfer the oracle's insert of the survivors) AND whose launches, read back with
rpt_profiling_read around that one call, are exactly the instantiations the row names (as
tests/test_gpu_kernel_ledger_range.py does for csrc/rpt_probe_range.hpp)."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_sel_range as klsr
from buf_util import A5, FF, GuardedBuffer
from test_gpu_kernel_ledger import Ctx, forced, make_col, rng_of
from test_gpu_kernel_ledger_sel import pass_mask
from test_gpu_transfer import Col, check, dev, sel_of

pytestmark = pytest.mark.gpu

# sub-intervals of the key domains make_col draws from (int64 build keys in +-2^62; int32 keys uniform over int32)
SUBS = {"i64": (-(2**61), 2**61), "i32": (-(2**30), 2**30 - 1)}
ROWS = 4096  # rows of the table under the selection vector


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module", autouse=True)
def profiling_off_afterwards(rpt):
    """Profiling is process-wide: whatever a row did, the module leaves it disabled and empty."""
    from rpt_amd import _lib

    yield
    _lib.profiling(False)
    _lib.profiling_reset()


@pytest.fixture(scope="module")
def ctx(rpt):
    c = Ctx(rpt)
    yield c
    c.close()


def in_range(col, rows, mm):
    """The range test of rows 0 .. rows of a column, written out here: not NULL and min <= key <= max."""
    phys = col.phys(np.arange(rows)).astype(np.int64)
    v = col.keys[phys].astype(np.int64)
    valid = np.ones(rows, dtype=bool)
    if col.validity is not None:
        p = phys.astype(np.uint64)
        valid = ((col.validity[p >> np.uint64(6)] >> (p & np.uint64(63))) & np.uint64(1)).astype(bool)
    return valid & (v >= mm[0]) & (v <= mm[1])


def two_flagged_filters(ctx, a, rng, rows):
    """Both filters with pinned ranges, one column of `rows` rows each, and per row: passes both Bloom tests, and
    passes those and both range tests."""
    f0, w0, b0 = ctx.caches[0].get(a["log_nb"])
    f1, w1, b1 = ctx.caches[1].get(a["later_log_nb"])
    c0, _r, _d = make_col(rng, a["kt"], a["dkind"], rows, b0)
    c1, _r, _d = make_col(rng, "i64", kl.DICT, rows, b1)
    f0.set_minmax(SUBS[a["kt"]])
    f1.set_minmax(SUBS["i64"])
    bloom = pass_mask(c0, w0, a["log_nb"], rows) & pass_mask(c1, w1, a["later_log_nb"], rows)
    ranged = in_range(c0, rows, SUBS[a["kt"]]) & in_range(c1, rows, SUBS["i64"])
    assert (bloom & ~ranged).any() and (ranged & ~bloom).any()
    return [f0, f1], [c0, c1], bloom, bloom & ranged


def counted_inputs(rng, max_rows, used, alive):
    """sel[:used] any rows, with repeats; sel[used:] rows that pass every test."""
    passing = np.flatnonzero(alive)
    assert passing.size
    sel = np.empty(max_rows, dtype=np.uint32)
    sel[:used] = rng.integers(0, alive.size, used)
    sel[used:] = passing[rng.integers(0, passing.size, max_rows - used)]
    return sel, sel[:used][alive[sel[:used]]]


def check_outputs(out, cnt, exp):
    assert int(cnt.view(torch.int64).item()) == exp.size
    assert np.array_equal(sel_of(out.view(torch.int32)[: exp.size]), exp)
    assert bool(torch.all(out.view(torch.int32)[exp.size:] == -1)), "out_sel written past the returned count"
    for name, g in (("out_sel", out), ("out_count", cnt)):
        g.assert_guards_intact(name)


def op_chain_sel_range_ws(ctx, a, rng):
    """max_rows = 2053 with 1800 on the device: three full segments, one probed up to the count, and the fifth wholly
    past it."""
    max_rows, used = a["n"], 1800
    filters, cols, bloom, alive = two_flagged_filters(ctx, a, rng, ROWS)
    sel, exp = counted_inputs(rng, max_rows, used, alive)
    assert 0 < exp.size < int(bloom[sel[:used]].sum())
    ws = GuardedBuffer(ctx.rpt.probe_chain_sel_workspace_bytes(filters, max_rows)).poison(A5)
    out, cnt = GuardedBuffer(4 * max_rows).poison(FF), GuardedBuffer(8).poison(FF)
    d_sel, d_count = dev(sel), torch.tensor([used], dtype=torch.int64, device="cuda:0")
    with forced(filters[0], kl.GATHER, max_rows), forced(filters[1], kl.GATHER, max_rows):
        with ctx.recording() as rec:
            ctx.rpt.probe_chain_sel_range_ws(filters, [c.as_dict(ctx.rpt) for c in cols], d_sel, d_count,
                                             range_mask=[True, True], max_rows=max_rows, out_sel=out.view(torch.int32),
                                             out_count=cnt.view(torch.int64), workspace=ws.bytes())
    check_outputs(out, cnt, exp)
    ws.assert_guards_intact("workspace")
    return rec


def op_small(ctx, a, rng):
    """The one-launch calls at 2053 positions: the row-list chain over rows 0 .. n of the columns, the device-counted
    ones over a selection with 1800 on the device."""
    n = a["n"]
    out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    outputs = dict(out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64))
    if not a["counted"]:
        filters, cols, bloom, alive = two_flagged_filters(ctx, a, rng, n)
        exp = np.flatnonzero(alive).astype(np.uint32)
        assert 0 < exp.size < int(bloom.sum())
        with ctx.recording() as rec:
            ctx.rpt.probe_chain_range(filters, [c.as_dict(ctx.rpt) for c in cols], range_mask=0b11, n=n, **outputs)
        check_outputs(out, cnt, exp)
        return rec
    used = 1800
    filters, cols, bloom, alive = two_flagged_filters(ctx, a, rng, ROWS)
    sel, exp = counted_inputs(rng, n, used, alive)
    assert 0 < exp.size < int(bloom[sel[:used]].sum())
    d_sel, d_count = dev(sel), torch.tensor([used], dtype=torch.int64, device="cuda:0")
    args = [c.as_dict(ctx.rpt) for c in cols]
    if a["transfer"]:
        dcol = Col(rng, a["kt"], "valid", ROWS)
        bf, base = ctx.targets.reset(12, True)
        with ctx.recording() as rec:
            ctx.rpt.transfer_sel_range(filters, args, [bf], [dcol.as_dict(ctx.rpt)], d_sel, d_count, range_mask=0b11,
                                       max_rows=n, **outputs)
        check(bf, dcol.expect(base, 12, exp), "destination")
    else:
        with ctx.recording() as rec:
            ctx.rpt.probe_chain_sel_range(filters, args, d_sel, d_count, range_mask=0b11, max_rows=n, **outputs)
    check_outputs(out, cnt, exp)
    return rec


OPS = {klsr.WS_OP: op_chain_sel_range_ws, **{op: op_small for op in klsr.SMALL_OPS.values()}}


def test_every_row_names_a_call():
    assert {r.op for r in klsr.ROWS} == set(OPS)


@pytest.mark.parametrize("row", klsr.ROWS, ids=[r.id for r in klsr.ROWS])
def test_sel_range_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
