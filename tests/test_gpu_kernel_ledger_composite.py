"""Every row of the eighth kernel ledger (tests/kernel_ledger_composite.py) on the GPU: one rpt_hash_keys_composite,
rpt_bf_insert_composite, rpt_bf_probe_chain_composite, rpt_bf_transfer_composite or rpt_bf_insert_multi_composite
whose hashes, selection and destinations equal the oracle's AND whose launches, read back with rpt_profiling_read
around that one call, are exactly one launch of the row's instantiation: no hash_kernel, insert_kernel,
insert_sel_kernel, probe_chain_small_kernel and no selection-vector tail (as the seven sibling files do for their
headers)."""
import numpy as np
import pytest
import torch

import kernel_ledger as kl
import kernel_ledger_composite as klc
from buf_util import FF, GuardedBuffer
from composite_util import DENSE, Key, member_filter, row_list
from test_gpu_kernel_ledger import Ctx, rng_of
from test_gpu_kernel_ledger_sel_range import check_outputs
from test_gpu_transfer import check

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


def key_of(rng, a, rows):
    """The row's key: NULLs in column 1, the last column the dictionary or the misaligned one."""
    prefix = None
    if a["kts"][0] == "hash":
        prefix = Key(rng, ("i64", "i32"), rows).hashes()
    return Key(rng, a["kts"], rows, layout=a.get("mix", DENSE), nulls=(1,), prefix=prefix)


def op_hash_composite(ctx, a, rng):
    n = a["n"]
    key = key_of(rng, a, n)
    out = GuardedBuffer(8 * n).poison(FF)
    with ctx.recording() as rec:
        ctx.rpt.hash_columns_fused(key.columns(ctx.rpt), out=out.view(torch.int64))
    assert np.array_equal(out.view(torch.int64).cpu().numpy().view(np.uint64), key.hashes())
    out.assert_guards_intact("out_hashes")
    return rec


def op_insert_composite(ctx, a, rng):
    n = a["n"]
    key = key_of(rng, a, n)
    bf, base = ctx.targets.reset(a["log_nb"], True)
    with ctx.recording() as rec:
        bf.insert_composite(key.columns(ctx.rpt))
    check(bf, key.expect(base, a["log_nb"], np.arange(n)), "filter")
    return rec


def op_small(ctx, a, rng):
    """Two keys a side where the side exists: the row's key and a one-column dictionary key beside it."""
    n = a["n"]
    rows = TABLE if a["row_sel"] else n
    ids, d_row_sel = row_list(rng, "shuffled" if a["row_sel"] else None, n, rows)
    alive = np.ones(rows, dtype=bool)
    filters, keys, made = [], [], []
    if a["probed"]:
        k0, k1 = key_of(rng, a, rows), Key(rng, ("i64",), rows, layout=kl.DICT)
        for k, log_nb in ((k0, a["log_nb"]), (k1, a["later_log_nb"])):
            bf, _w, passes = member_filter(ctx.rpt, rng, k, log_nb, share=0.7)
            made.append(bf)
            filters.append(bf)
            keys.append(k.columns(ctx.rpt))
            alive &= passes
    exp = ids[alive[ids]]
    dsts, dkeys, expect = [], [], []
    if a["transfer"]:
        d0, d1 = key_of(rng, a, rows), Key(rng, ("i32",), rows, nulls=(0,))
        for tag, (k, log_nb, prefilled) in enumerate(((d0, 12, True), (d1, 14, False))):
            bf, base = ctx.targets.reset(log_nb, prefilled)
            dsts.append(bf)
            dkeys.append(k.columns(ctx.rpt))
            expect.append(k.expect(base, log_nb, exp))
    out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    kw = dict(row_sel=d_row_sel, n=n)
    okw = dict(out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64), **kw)
    try:
        with ctx.recording() as rec:
            if not a["probed"]:
                ctx.rpt.insert_multi_composite(dsts, dkeys, **kw)
            elif a["transfer"]:
                ctx.rpt.transfer_composite(filters, keys, dsts, dkeys, **okw)
            else:
                ctx.rpt.probe_chain_composite(filters, keys, **okw)
        if a["probed"]:
            assert 0 < exp.size < n
            check_outputs(out, cnt, exp)
        for j, (bf, e) in enumerate(zip(dsts, expect)):
            check(bf, e, "destination %d" % j)
    finally:
        for bf in made:
            bf.close()
    return rec


OPS = {"hash_composite": op_hash_composite, "insert_composite": op_insert_composite, "chain_composite": op_small,
       "transfer_composite": op_small, "insert_multi_composite": op_small}


def test_every_row_names_a_call():
    assert {r.op for r in klc.ROWS} == set(OPS)


@pytest.mark.parametrize("row", klc.ROWS, ids=[r.id for r in klc.ROWS])
def test_composite_ledger_row(ctx, row):
    observed = OPS[row.op](ctx, dict(row.args), rng_of(row))
    problems = kl.kernel_set_problems(dict(row.kernels), observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
