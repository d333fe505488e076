"""Every row of the range stage's kernel ledger (tests/kernel_ledger_range.py) on the GPU: one rpt_bf_range_bits, or one
rpt_bf_probe_chain_range_ws over two flagged filters, whose result equals the expectation (numpy's range test, ANDed
with the oracle's probe per filter) AND whose launches, read back with rpt_profiling_read around that one call, are
exactly the instantiations the row names (as tests/test_gpu_kernel_ledger.py does for csrc/rpt_gpu.hip)."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_range as klg
from buf_util import FF, GuardedBuffer
from test_gpu_kernel_ledger import Ctx, forced, make_col, probe_ref, rng_of, row_ids_of
from test_gpu_range import range_pass
from test_gpu_transfer import bits_words, sel_of

pytestmark = pytest.mark.gpu

# sub-intervals of the key domains make_col draws from (int64 build keys in +-2^62; int32 keys uniform over int32)
SUBS = {"i64": (-(2**61), 2**61), "i32": (-(2**30), 2**30 - 1)}


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


def col_range_pass(col, row_ids, mm):
    return range_pass(col.keys, col.phys(row_ids).astype(np.int64), col.validity, mm)


def op_range_bits(ctx, a, rng):
    bf, _words, build = ctx.caches[0].get(a["log_nb"])
    n = a["n"]
    col, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, build)
    bf.set_minmax(SUBS[a["kt"]])
    out = GuardedBuffer((n + 511) // 512 * 64).poison(FF)
    with ctx.recording() as rec:
        bf.range_bits(col.d_keys, n=n, row_sel=d_row_sel, out=out.view(torch.int64), **col.kwargs(ctx.rpt))
    exp = col_range_pass(col, row_ids_of(row_sel, n), SUBS[a["kt"]])
    assert 0 < exp.sum() < n
    assert np.array_equal(out.view(torch.int64).cpu().numpy().view(np.uint64), bits_words(exp))
    out.assert_guards_intact("out_bits")
    return rec


def op_chain_range(ctx, a, rng):
    (f0, w0, b0), (f1, w1, b1) = ctx.caches[0].get(a["log_nb"]), ctx.caches[1].get(a["log_nb"])
    n = a["n"]
    c1, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, b1)
    c0, _r, _d = make_col(rng, "i64", kl.DENSE, c1.rows, b0)  # dense, unless the call has a row_sel
    rows = row_ids_of(row_sel, n)
    f0.set_minmax(SUBS["i64"])
    f1.set_minmax(SUBS[a["kt"]])
    alive = np.zeros(c1.rows, dtype=bool)
    alive[np.intersect1d(probe_ref(c0, w0, a["log_nb"], rows), probe_ref(c1, w1, a["log_nb"], rows))] = True
    bloom_only = int(alive.sum())
    alive[rows] &= col_range_pass(c0, rows, SUBS["i64"]) & col_range_pass(c1, rows, SUBS[a["kt"]])
    exp = np.flatnonzero(alive).astype(np.uint32)
    assert 0 < exp.size < bloom_only
    out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    with forced(f0, kl.GATHER, n), forced(f1, kl.GATHER, n):
        with ctx.recording() as rec:
            ctx.rpt.probe_chain_range_ws([f0, f1], [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)], range_mask=[True, True],
                                         row_sel=d_row_sel, n=n, out_sel=out.view(torch.int32),
                                         out_count=cnt.view(torch.int64))
    assert int(cnt.view(torch.int64).item()) == exp.size
    assert np.array_equal(sel_of(out.view(torch.int32)[: exp.size]), exp)
    assert bool(torch.all(out.view(torch.int32)[exp.size:] == -1)), "out_sel written past the returned count"
    for name, g in (("out_sel", out), ("out_count", cnt)):
        g.assert_guards_intact(name)
    return rec


OPS = {"range_bits": op_range_bits, "chain_range": op_chain_range}


def test_every_row_names_a_call():
    assert {r.op for r in klg.ROWS} == set(OPS)


@pytest.mark.parametrize("row", klg.ROWS, ids=[r.id for r in klg.ROWS])
def test_range_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
