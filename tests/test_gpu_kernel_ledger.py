"""Every row of the kernel ledger (tests/kernel_ledger.py) on the GPU: one small call through the C-ABI or the Python
wrapper whose result equals the oracle's exactly AND whose launches, read back with rpt_profiling_read around that one
call, are exactly the instantiations the row names. A parity test elsewhere says which kernel it means to test in its
docstring; here the library says which one ran, so a dispatch change that reroutes a shape fails the row instead of
quietly leaving the kernel it was written for without oracle coverage.

Filters are built once per size (buf_util.FilterCache, two of them so a chain can hold one size twice) and never
inserted into; the inserts go into test_gpu_transfer's Targets, put back to known words before every use."""
import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch

import kernel_ledger as kl
import rpt_oracle as orc
from buf_util import FilterCache, int32_build_keys
from test_gpu_transfer import Col, Targets, bits_words, check, dev, rand_keys, sel_of

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


class Ctx:
    def __init__(self, rpt):
        from rpt_amd import _lib

        self.rpt, self.plib, self.lib = rpt, _lib, _lib.load()
        self.caches = (FilterCache(), FilterCache())
        self.targets = Targets(rpt)

    def close(self):
        for c in self.caches:
            c.close()
        self.targets.close()

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @contextlib.contextmanager
    def recording(self):
        """Reset, enable, <the call>, synchronise, disable, read: the dictionary yielded holds {name: (launches, ms)}
        of exactly the launches made inside the block once the block has ended."""
        rec = {}
        torch.cuda.synchronize()
        self.plib.profiling_reset()
        self.plib.profiling(True)
        try:
            yield rec
            torch.cuda.synchronize()
        finally:
            self.plib.profiling(False)
        rec.update(self.plib.kernel_times())
        self.plib.profiling_reset()


# ---- columns --------------------------------------------------------------------------------------------------------
def hit_keys(rng, kt, m, build):
    """m keys of the column type, half of them drawn from the filter's build keys ("hash": their hashes)."""
    dtype = np.int32 if kt == "i32" else np.int64
    pool = int32_build_keys(build) if kt == "i32" else build
    keys = np.where(rng.random(m) < 0.5, pool[rng.integers(0, pool.size, m)], rand_keys(dtype, m, rng)).astype(dtype)
    return orc.hash_keys(keys) if kt == "hash" else keys


def make_col(rng, kt, dkind, n, build):
    """(column, row_sel, its device copy): n probed rows in the row mapping `dkind`. dense / misaligned / row_sel
    columns are flat with 15 % NULLs (row_sel: n of n + n/2 + 3 rows), dict is a dictionary with NULLs; misaligned
    keys start 8 bytes past a 16-byte boundary."""
    rows = n + n // 2 + 3 if dkind == kl.ROW_SEL else n
    if dkind == kl.DICT:
        col = Col(rng, kt, "dict", rows, keys=hit_keys(rng, kt, rows // 2 + 1, build))
    else:
        col = Col(rng, kt, "valid", rows, keys=hit_keys(rng, kt, rows, build))
    if dkind == kl.MISALIGNED:
        shift = 8 // col.d_keys.element_size()
        raw = torch.empty(col.d_keys.numel() + shift, dtype=col.d_keys.dtype, device="cuda:0")
        raw[shift:].copy_(col.d_keys)
        col.d_keys = raw[shift:]
    assert col.d_keys.data_ptr() % 16 == (8 if dkind == kl.MISALIGNED else 0)
    assert (col.d_key_sel is not None) == (dkind == kl.DICT)
    row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if dkind == kl.ROW_SEL else None
    return col, row_sel, dev(row_sel)


def row_ids_of(row_sel, n):
    return row_sel if row_sel is not None else np.arange(n, dtype=np.uint32)


def probe_ref(col, words, log_nb, row_ids):
    """The oracle's LookupSel of rows `row_ids` of the column: the ids that pass, ascending."""
    p = col.phys(row_ids)
    if col.kt == "hash":
        pos = orc.lookup_sel_hashes(words, log_nb, col.keys[p])
    else:
        pos = orc.probe_keys(words, log_nb, col.keys, key_sel=p, validity=col.validity)
    return np.asarray(row_ids, dtype=np.uint32)[pos]


def rng_of(row):
    return np.random.default_rng(zlib.crc32(row.id.encode()))


@contextlib.contextmanager
def forced(bf, strategy, n):
    """The shared filter with its probe strategy forced (and checked to resolve to it), AUTO again afterwards."""
    bf.probe_strategy = strategy
    try:
        if strategy != kl.AUTO:
            assert bf.probe_strategy_for(n) == strategy
        yield bf
    finally:
        bf.probe_strategy = kl.AUTO


# ---- the calls ------------------------------------------------------------------------------------------------------
def op_find_bits(ctx, a, rng):
    bf, words, build = ctx.caches[0].get(a["log_nb"])
    n = a["n"]
    col, _rs, _d = make_col(rng, a["kt"], a["dkind"], n, build)
    with ctx.recording() as rec:
        got = bf.find_bits(col.d_keys, n=n, **col.kwargs(ctx.rpt))
    mask = np.zeros(n, dtype=bool)
    mask[probe_ref(col, words, a["log_nb"], row_ids_of(None, n))] = True
    assert 0 < mask.sum() < n
    assert np.array_equal(got.cpu().numpy().view(np.uint64), bits_words(mask))
    return rec


def op_probe(ctx, a, rng):
    bf, words, build = ctx.caches[0].get(a["log_nb"])
    n = a["n"]
    col, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, build)
    out_sel = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_count = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    with forced(bf, a["strategy"], n):
        assert ctx.lib.rpt_bf_probe_is_fused(bf.handle, n) == int(a["what"] == "small")
        with ctx.recording() as rec:
            bf.probe_async(col.d_keys, n=n, row_sel=d_row_sel, out_sel=out_sel, out_count=out_count,
                           **col.kwargs(ctx.rpt))
    ref = probe_ref(col, words, a["log_nb"], row_ids_of(row_sel, n))
    assert 0 < ref.size < n
    assert int(out_count.item()) == ref.size
    assert np.array_equal(sel_of(out_sel[: ref.size]), ref)
    return rec


def op_probe_bits(ctx, a, rng):
    bf, words, build = ctx.caches[0].get(a["log_nb"])
    n = a["n"]
    col, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, build)
    out = torch.full(((n + 511) // 512 * 8,), -1, dtype=torch.int64, device="cuda:0")
    c = ctx.rpt.make_column(col.d_keys, **col.kwargs(ctx.rpt))
    with forced(bf, a["strategy"], n):
        ws = torch.empty(max(bf.workspace_bytes(n), 256), dtype=torch.uint8, device="cuda:0")
        with ctx.recording() as rec:
            ctx.plib.check(ctx.lib.rpt_bf_probe_bits(bf.handle, ctypes.byref(c), None, n, out.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), ctx.stream()), ctx.lib)
    mask = np.zeros(n, dtype=bool)
    mask[probe_ref(col, words, a["log_nb"], row_ids_of(row_sel, n))] = True
    assert 0 < mask.sum() < n
    assert np.array_equal(out.cpu().numpy().view(np.uint64), bits_words(mask))
    return rec


def op_chain_small(ctx, a, rng):
    n = a["n"]
    (f0, w0, b0), (f1, w1, b1) = ctx.caches[0].get(11), ctx.caches[1].get(16)
    c0, _r, _d = make_col(rng, "i64", kl.DENSE, n, b0)
    c1, _r, _d = make_col(rng, "i32", kl.DICT, n, b1)
    with ctx.recording() as rec:
        got = ctx.rpt.probe_chain([f0, f1], [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)], n=n)
    ids = row_ids_of(None, n)
    exp = np.intersect1d(probe_ref(c0, w0, 11, ids), probe_ref(c1, w1, 16, ids)).astype(np.uint32)
    assert 0 < exp.size < n
    assert np.array_equal(sel_of(got), exp)
    return rec


def op_chain_ws(ctx, a, rng):
    n, log0, log1 = a["n"], kl.LOG_GATHER, a["log_nb"]
    (f0, w0, b0), (f1, w1, b1) = ctx.caches[0].get(log0), ctx.caches[1].get(log1)
    c1, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, b1)
    c0 = Col(rng, "i64", "valid", c1.rows, keys=hit_keys(rng, "i64", c1.rows, b0))  # stage 0: dense unless row_sel
    assert c0.d_keys.data_ptr() % 16 == 0
    with forced(f0, kl.GATHER, n), forced(f1, a["strategy"], n):
        with ctx.recording() as rec:
            got = ctx.rpt.probe_chain_ws([f0, f1], [c0.as_dict(ctx.rpt), c1.as_dict(ctx.rpt)], row_sel=d_row_sel, n=n)
    ids = row_ids_of(row_sel, n)
    r0, r1 = probe_ref(c0, w0, log0, ids), probe_ref(c1, w1, log1, ids)
    exp = np.intersect1d(r0, r1).astype(np.uint32)
    assert 0 < exp.size < min(r0.size, r1.size)  # both stages remove rows
    assert np.array_equal(sel_of(got), exp)
    return rec


def op_insert(ctx, a, rng):
    log_nb, n = a["log_nb"], a["n"]
    bf, base = ctx.targets.reset(log_nb, False)
    col, _rs, _d = make_col(rng, a["kt"], a["dkind"], n, rand_keys(np.int64, 4096, rng))
    ctx.plib.check(ctx.lib.rpt_bf_set_insert_strategy(bf.handle, a["strategy"]), ctx.lib)
    assert bf.insert_strategy_for(n) == a["strategy"]
    with ctx.recording() as rec:
        bf.insert(col.d_keys, n=n, **col.kwargs(ctx.rpt))
    exp = col.expect(base, log_nb, row_ids_of(None, n))
    assert (exp[1] is None) == (a["kt"] == "hash")
    check(bf, exp, a["what"])
    return rec


def op_insert_bits(ctx, a, rng):
    log_nb, n = a["log_nb"], a["n"]
    bf, base = ctx.targets.reset(log_nb, True)
    col, row_sel, d_row_sel = make_col(rng, a["kt"], a["dkind"], n, rand_keys(np.int64, 4096, rng))
    mask = rng.random(n) < 0.5
    bits = dev(bits_words(mask))
    with ctx.recording() as rec:
        bf.insert_bits(col.d_keys, bits, n=n, row_sel=d_row_sel, **col.kwargs(ctx.rpt))
    check(bf, col.expect(base, log_nb, row_ids_of(row_sel, n)[mask]))
    return rec


def op_insert_sel(ctx, a, rng):
    log_nb, n = a["log_nb"], a["n"]
    bf, base = ctx.targets.reset(log_nb, True)
    col, _rs, _d = make_col(rng, a["kt"], a["dkind"], n, rand_keys(np.int64, 4096, rng))
    chosen = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.uint32)
    sel = np.full(n, np.setdiff1d(np.arange(n, dtype=np.uint32), chosen)[0], dtype=np.uint32)  # past the count: a dead row
    sel[: chosen.size] = chosen
    d_sel, d_count = dev(sel), torch.tensor([chosen.size], dtype=torch.int64, device="cuda:0")
    with ctx.recording() as rec:
        bf.insert_sel(col.d_keys, d_sel, d_count, **col.kwargs(ctx.rpt))
    check(bf, col.expect(base, log_nb, chosen))
    return rec


def op_hash(ctx, a, rng):
    n, kt = a["n"], a["kt"]
    if kt == "hash":  # precomputed hashes pass through as they are; NULLs do not apply
        source = rand_keys(np.int64, n, rng)
        col = Col(rng, kt, "flat", n, keys=orc.hash_keys(source))
        ref = col.keys
    else:
        col = Col(rng, kt, "valid", n)
        source = col.keys
        ref = orc.hash_keys(col.keys, validity=col.validity)
    if not a["combine"]:
        with ctx.recording() as rec:
            got = ctx.rpt.hash_keys(col.d_keys, **col.kwargs(ctx.rpt))
    else:
        first = rand_keys(np.uint64, n, rng)
        ref = orc.hash_combine(first, source, validity=col.validity)
        got = dev(first)
        c = ctx.rpt.make_column(col.d_keys, **col.kwargs(ctx.rpt))
        with ctx.recording() as rec:
            ctx.plib.check(ctx.lib.rpt_hash_combine(ctypes.byref(c), n, got.data_ptr(), ctx.stream()), ctx.lib)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), ref)
    return rec


def op_widen(ctx, a, rng):
    sizes = [0, 1, 2048, 3000, 7]
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(row0[-1])
    lo = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    hi = np.array([0, 5, 0xFFFFFFFF, 0x7FFFFFFF, 1], dtype=np.uint32)
    want = np.concatenate([(np.uint64(hi[c]) << np.uint64(32)) | lo[row0[c]:row0[c + 1]].astype(np.uint64)
                           for c in range(len(sizes))])
    d_lo, d_hi, d_row0 = dev(lo), dev(hi), dev(row0)
    out = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    with ctx.recording() as rec:
        ctx.plib.check(ctx.lib.rpt_keys_widen(d_lo.data_ptr(), d_hi.data_ptr(), d_row0.data_ptr(), len(sizes),
                                              out.data_ptr(), ctx.stream()), ctx.lib)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    return rec


def op_merge_or(ctx, a, rng):
    log_nb = a["log_nb"]
    src, w_src, build = ctx.caches[0].get(log_nb)
    dst, base = ctx.targets.reset(log_nb, True)
    with ctx.recording() as rec:
        dst.merge_or(src)
    check(dst, (base | w_src, orc.minmax(build)))
    assert not np.array_equal(base | w_src, base) and not np.array_equal(base | w_src, w_src)
    return rec


def op_words_or(ctx, a, rng):
    nw = a["n_words"]
    dst, src = rand_keys(np.uint64, nw, rng), rand_keys(np.uint64, nw, rng)
    d_dst, d_src = dev(dst), dev(src)
    with ctx.recording() as rec:
        ctx.plib.check(ctx.lib.rpt_words_or(d_dst.data_ptr(), d_src.data_ptr(), nw, ctx.stream()), ctx.lib)
    assert np.array_equal(d_dst.cpu().numpy().view(np.uint64), dst | src)
    return rec


def op_words_or_slices(ctx, a, rng):
    nw, k = a["n_words"], a["k"]
    srcs = rand_keys(np.uint64, nw * k, rng) & rand_keys(np.uint64, nw * k, rng)
    d_dst, d_srcs = dev(rand_keys(np.uint64, nw, rng)), dev(srcs)
    with ctx.recording() as rec:
        ctx.rpt.words_or_slices(d_dst, d_srcs, k, nw)
    assert np.array_equal(d_dst.cpu().numpy().view(np.uint64), np.bitwise_or.reduce(srcs.reshape(k, nw), axis=0))
    return rec


def fold_rounds(words, log_nb):
    """BlockedBloomFilter::Fold round by round on host words: (rounds, final log2 blocks). One OR launch per round."""
    rounds = 0
    while log_nb > 4:
        set_bits, num_bits = orc.count_bits(words), (1 << log_nb) * 64
        if 4 * set_bits >= num_bits:
            break
        folds = 1
        while log_nb - folds > 4 and 4 * set_bits < (num_bits >> folds):
            folds += 1
        words = np.bitwise_or.reduce(words.reshape(1 << folds, -1), axis=0)
        log_nb -= folds
        rounds += 1
    return rounds, log_nb


def op_fold(ctx, a, rng):
    log_nb = a["log_nb"]
    keys = rand_keys(np.int64, 300, rng)
    words = orc.new_words(log_nb)
    orc.insert_keys(words, log_nb, keys)
    rounds, final = fold_rounds(words, log_nb)
    assert rounds >= 1 and final < log_nb
    bf = ctx.rpt.BloomFilter(log_num_blocks=log_nb)
    try:
        bf.insert(dev(keys), strategy=kl.INS_ATOMIC)
        with ctx.recording() as rec:
            got_log = bf.fold()
        assert orc.fold(words, log_nb) == got_log == final
        assert np.array_equal(bf.export_words(), words[: 1 << final])
    finally:
        bf.close()
    a["_launches"] = {"or_slices_kernel(fold)": rounds}
    return rec


def op_synth_build(ctx, a, rng):
    with ctx.recording() as rec:
        got = ctx.rpt.synth_build_keys(a["n"], start=12345, device="cuda:0")
    assert np.array_equal(got.cpu().numpy(), orc.synth_build_keys(a["n"], start=12345))
    return rec


def op_synth_probe(ctx, a, rng):
    with ctx.recording() as rec:
        got = ctx.rpt.synth_probe_keys(a["n"], 1000, 100, start=77, device="cuda:0")
    assert np.array_equal(got.cpu().numpy(), orc.synth_probe_keys(a["n"], 1000, 100, start=77))
    return rec


OPS = {name[3:]: fn for name, fn in list(globals().items()) if name.startswith("op_")}


def test_every_row_names_a_call():
    assert {r.op for r in kl.ROWS} == set(OPS)


@pytest.mark.parametrize("row", kl.ROWS, ids=[r.id for r in kl.ROWS])
def test_ledger_row(ctx, row):
    args = dict(row.args)
    observed = OPS[row.op](ctx, args, rng_of(row))
    expected = dict(row.kernels, **args.get("_launches", {}))
    assert all(c is not None for c in expected.values()), "every launch count of this row is known by now"
    problems = kl.kernel_set_problems(expected, observed)
    assert not problems, "%s launched %s\n  %s" % (row.id, sorted(observed), "\n  ".join(problems))
    assert not set(observed) & set(kl.NEVER_LAUNCHED)
    assert not set(observed) & set(kl.EXEMPT)
    for name, (_launches, ms) in observed.items():
        assert np.isfinite(ms) and ms >= 0, name
