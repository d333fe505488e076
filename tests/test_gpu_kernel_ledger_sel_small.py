"""Every row of the one-launch device-counted probes' kernel ledger (tests/kernel_ledger_sel_small.py) on the GPU: one
rpt_bf_probe_chain_sel or rpt_bf_transfer_sel over two filters whose selection (and, for the transfer, destination)
equals the oracle's AND whose launches, read back with rpt_profiling_read around that one call, are exactly one launch
of the row's instantiation of probe_chain_sel_small_kernel: no masked stage, no selection-vector tail, no
insert_sel_kernel (as tests/test_gpu_kernel_ledger_sel.py does for csrc/rpt_probe_sel.hpp)."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_sel_small as klss
from buf_util import FF, GuardedBuffer
from test_gpu_kernel_ledger import Ctx, make_col, rng_of
from test_gpu_kernel_ledger_sel import pass_mask
from test_gpu_transfer import Col, check, dev, sel_of

pytestmark = pytest.mark.gpu


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


def small_call(ctx, a, rng):
    """max_rows = 513 with 400 on the device: the first segment is probed up to the count, the second is wholly past it.
    sel[400:] holds rows that pass both filters."""
    max_rows, used, rows = a["n"], 400, 2048
    f0, w0, b0 = ctx.caches[0].get(a["log_nb"])
    f1, w1, b1 = ctx.caches[1].get(a["later_log_nb"])
    c0, _r, _d = make_col(rng, a["kt"], a["dkind"], rows, b0)
    c1, _r, _d = make_col(rng, "i64", kl.DICT, rows, b1)
    alive = pass_mask(c0, w0, a["log_nb"], rows) & pass_mask(c1, w1, a["later_log_nb"], rows)
    passing = np.flatnonzero(alive)
    assert passing.size
    sel = np.empty(max_rows, dtype=np.uint32)
    sel[:used] = rng.integers(0, rows, used)
    sel[used:] = passing[rng.integers(0, passing.size, max_rows - used)]
    exp = sel[:used][alive[sel[:used]]]
    assert 0 < exp.size < used
    out, cnt = GuardedBuffer(4 * max_rows).poison(FF), GuardedBuffer(8).poison(FF)
    d_sel, d_count = dev(sel), torch.tensor([used], dtype=torch.int64, device="cuda:0")
    outputs = dict(max_rows=max_rows, out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64))
    filters, cols = [f0, f1], [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)]
    if a["transfer"]:
        dcol = Col(rng, a["kt"], "valid", rows)
        bf, base = ctx.targets.reset(12, True)
        with ctx.recording() as rec:
            ctx.rpt.transfer_sel(filters, cols, [bf], [dcol.as_dict(ctx.rpt)], d_sel, d_count, **outputs)
        check(bf, dcol.expect(base, 12, exp), "destination")
    else:
        with ctx.recording() as rec:
            ctx.rpt.probe_chain_sel(filters, cols, d_sel, d_count, **outputs)
    assert int(cnt.view(torch.int64).item()) == exp.size
    assert np.array_equal(sel_of(out.view(torch.int32)[: exp.size]), exp)
    assert bool(torch.all(out.view(torch.int32)[exp.size:] == -1)), "out_sel written past the returned count"
    for name, g in (("out_sel", out), ("out_count", cnt)):
        g.assert_guards_intact(name)
    return rec


OPS = {"chain_sel_small": small_call, "transfer_sel_small": small_call}


def test_every_row_names_a_call():
    assert {r.op for r in klss.ROWS} == set(OPS)


@pytest.mark.parametrize("row", klss.ROWS, ids=[r.id for r in klss.ROWS])
def test_sel_small_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
