"""Every row of the device-counted probes' kernel ledger (tests/kernel_ledger_sel.py) on the GPU: one
rpt_bf_probe_chain_sel_ws over two filters whose selection equals the oracle's AND whose launches, read back with
rpt_profiling_read around that one call, are exactly the row's instantiation of probe_bits_sel_kernel, one masked later
stage and the selection-vector tail (as tests/test_gpu_kernel_ledger.py does for csrc/rpt_gpu.hip). The demotion rows
force PARTITIONED on a stage: no partition or bucket kernel may run."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_sel as kls
from buf_util import A5, FF, GuardedBuffer
from test_gpu_kernel_ledger import Ctx, make_col, probe_ref, rng_of
from test_gpu_transfer import dev, sel_of

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


def pass_mask(col, words, log_nb, rows):
    m = np.zeros(rows, dtype=bool)
    m[probe_ref(col, words, log_nb, np.arange(rows, dtype=np.uint32))] = True
    return m


def op_chain_sel(ctx, a, rng):
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
    filters = [f0, f1]
    f0.probe_strategy, f1.probe_strategy = a["strategy"], a["later_strategy"]
    try:
        for bf, st in ((f0, a["strategy"]), (f1, a["later_strategy"])):
            if st != kl.AUTO:
                assert bf.probe_strategy_for(max_rows) == st
            want = kl.GATHER if st in (kl.PARTITIONED, kl.BUCKETED) else bf.probe_strategy_for(max_rows)
            assert bf.probe_sel_strategy_for(max_rows) == want
        ws = GuardedBuffer(ctx.rpt.probe_chain_sel_workspace_bytes(filters, max_rows)).poison(A5)
        out, cnt = GuardedBuffer(4 * max_rows).poison(FF), GuardedBuffer(8).poison(FF)
        d_sel, d_count = dev(sel), torch.tensor([used], dtype=torch.int64, device="cuda:0")
        with ctx.recording() as rec:
            ctx.rpt.probe_chain_sel_ws(filters, [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)], d_sel, d_count,
                                       max_rows=max_rows, out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64),
                                       workspace=ws.bytes())
    finally:
        f0.probe_strategy = f1.probe_strategy = kl.AUTO
    assert int(cnt.view(torch.int64).item()) == exp.size
    assert np.array_equal(sel_of(out.view(torch.int32)[: exp.size]), exp)
    for name, g in (("workspace", ws), ("out_sel", out), ("out_count", cnt)):
        g.assert_guards_intact(name)
    return rec


OPS = {name[3:]: fn for name, fn in list(globals().items()) if name.startswith("op_")}


def test_every_row_names_a_call():
    assert {r.op for r in kls.ROWS} == set(OPS)


@pytest.mark.parametrize("row", kls.ROWS, ids=[r.id for r in kls.ROWS])
def test_sel_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
    if row in kls.DEMOTION_ROWS:
        routed = [n for n in observed if kl.base_name(n) == "partition_kernel" or kl.base_name(n).startswith("bucket_")]
        assert not routed, routed
