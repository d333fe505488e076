"""Every row of the seventh kernel ledger (tests/kernel_ledger_transfer_small.py) on the GPU: one rpt_bf_transfer,
rpt_bf_transfer_range or rpt_bf_insert_multi whose selection and destinations equal the oracle's AND whose launches,
read back with rpt_profiling_read around that one call, are exactly one launch of the row's instantiation of
transfer_small_kernel: no probe_chain_small_kernel, no insert_sel_kernel or insert_kernel, no selection-vector tail (as
tests/test_gpu_kernel_ledger_sel_small.py does for csrc/rpt_probe_sel_small.hpp)."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_transfer_small as klts
from buf_util import FF, GuardedBuffer
from test_gpu_kernel_ledger import Ctx, make_col, rng_of
from test_gpu_kernel_ledger_sel import pass_mask
from test_gpu_kernel_ledger_sel_range import SUBS, check_outputs, in_range
from test_gpu_transfer import Col, check, dev

pytestmark = pytest.mark.gpu

TABLE = 2048  # rows of the table under a given row list


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


def row_list(rng, a):
    """(rows of the table, the listed row ids, the device row_sel or None): rows 0 .. n of an n-row table, or n row ids
    of a 2048-row table in any order, with repeats."""
    n = a["n"]
    if not a["row_sel"]:
        return n, np.arange(n, dtype=np.uint32), None
    ids = rng.integers(0, TABLE, n).astype(np.uint32)
    return TABLE, ids, dev(ids)


def op_transfer(ctx, a, rng):
    """Two probed filters (with a mask both flagged, their ranges pinned to half the key domain), one destination."""
    n = a["n"]
    rows, ids, d_row_sel = row_list(rng, a)
    f0, w0, b0 = ctx.caches[0].get(a["log_nb"])
    f1, w1, b1 = ctx.caches[1].get(a["later_log_nb"])
    c0, _r, _d = make_col(rng, a["kt"], a["dkind"], rows, b0)
    c1, _r, _d = make_col(rng, "i64", kl.DICT, rows, b1)
    bloom = pass_mask(c0, w0, a["log_nb"], rows) & pass_mask(c1, w1, a["later_log_nb"], rows)
    alive = bloom
    if a["ranged"]:
        f0.set_minmax(SUBS[a["kt"]])
        f1.set_minmax(SUBS["i64"])
        alive = bloom & in_range(c0, rows, SUBS[a["kt"]]) & in_range(c1, rows, SUBS["i64"])
        assert 0 < int(alive[ids].sum()) < int(bloom[ids].sum())
    exp = ids[alive[ids]]
    assert 0 < exp.size < n
    dcol = Col(rng, a["kt"], "valid", rows)
    bf, base = ctx.targets.reset(12, True)
    out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    kw = dict(row_sel=d_row_sel, n=n, out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64))
    cols = [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)]
    with ctx.recording() as rec:
        if a["ranged"]:
            ctx.rpt.transfer_range([f0, f1], cols, [bf], [dcol.as_dict(ctx.rpt)], range_mask=0b11, **kw)
        else:
            ctx.rpt.transfer([f0, f1], cols, [bf], [dcol.as_dict(ctx.rpt)], **kw)
    check_outputs(out, cnt, exp)
    check(bf, dcol.expect(base, 12, exp), "destination")
    return rec


def op_insert_multi(ctx, a, rng):
    """Two destinations of different sizes, one pre-filled, the row's column and an int64 dictionary."""
    rows, ids, d_row_sel = row_list(rng, a)
    _f, _w, build = ctx.caches[0].get(a["log_nb"])
    c0, _r, _d = make_col(rng, a["kt"], a["dkind"], rows, build)
    c1 = Col(rng, "i64", "dict", rows)
    (bf0, base0), (bf1, base1) = ctx.targets.reset(12, True), ctx.targets.reset(14, False)
    with ctx.recording() as rec:
        ctx.rpt.insert_multi([bf0, bf1], [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)], row_sel=d_row_sel, n=a["n"])
    check(bf0, c0.expect(base0, 12, ids), "destination 0")
    check(bf1, c1.expect(base1, 14, ids), "destination 1")
    return rec


OPS = {"transfer_small": op_transfer, "transfer_range_small": op_transfer, "insert_multi_small": op_insert_multi}


def test_every_row_names_a_call():
    assert {r.op for r in klts.ROWS} == set(OPS)


@pytest.mark.parametrize("row", klts.ROWS, ids=[r.id for r in klts.ROWS])
def test_transfer_small_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
