"""Every row of the routed inserts' kernel ledger (tests/kernel_ledger_routed.py) on the GPU: one forced-PARTITIONED
rpt_bf_insert_bits_ws / rpt_bf_insert_sel_ws whose filter equals the oracle's insert of exactly the selected rows AND
whose launches, read back with rpt_profiling_read around that one call, are exactly the row's instantiation of
partition_masked_kernel, one runs_transpose_kernel and one slice_insert_kernel (as tests/test_gpu_kernel_ledger.py
does for csrc/rpt_gpu.hip)."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_routed as klr
from test_gpu_kernel_ledger import Ctx, make_col, rng_of, row_ids_of
from test_gpu_transfer import bits_words, check, dev, rand_keys

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


def forced_target(ctx, log_nb, prefilled, n):
    bf, base = ctx.targets.reset(log_nb, prefilled)
    ctx.plib.check(ctx.lib.rpt_bf_set_insert_strategy(bf.handle, kl.INS_PARTITIONED), ctx.lib)
    assert bf.insert_strategy_for(n) == kl.INS_PARTITIONED
    return bf, base


def op_insert_bits_ws(ctx, a, rng):
    log_nb, n = a["log_nb"], a["n"]
    bf, base = forced_target(ctx, log_nb, True, n)
    col, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, rand_keys(np.int64, 4096, rng))
    mask = rng.random(n) < 0.5
    bits = dev(bits_words(mask))
    with ctx.recording() as rec:
        bf.insert_bits_ws(col.d_keys, bits, n=n, row_sel=d_row_sel, **col.kwargs(ctx.rpt))
    check(bf, col.expect(base, log_nb, row_ids_of(row_sel, n)[mask]))
    return rec


def op_insert_sel_ws(ctx, a, rng):
    log_nb, n = a["log_nb"], a["n"]
    bf, base = forced_target(ctx, log_nb, False, n)
    col, _rs, _d = make_col(rng, a["kt"], a["dkind"], n, rand_keys(np.int64, 4096, rng))
    chosen = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.uint32)
    sel = np.full(n, np.setdiff1d(np.arange(n, dtype=np.uint32), chosen)[0], dtype=np.uint32)  # past the count: a dead row
    sel[: chosen.size] = chosen
    d_sel, d_count = dev(sel), torch.tensor([chosen.size], dtype=torch.int64, device="cuda:0")
    with ctx.recording() as rec:
        bf.insert_sel_ws(col.d_keys, d_sel, d_count, **col.kwargs(ctx.rpt))
    check(bf, col.expect(base, log_nb, chosen))
    return rec


OPS = {name[3:]: fn for name, fn in list(globals().items()) if name.startswith("op_")}


def test_every_row_names_a_call():
    assert {r.op for r in klr.ROWS} == set(OPS)


@pytest.mark.parametrize("row", klr.ROWS, ids=[r.id for r in klr.ROWS])
def test_routed_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
