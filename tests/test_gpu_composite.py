"""Composite join keys hashed inside the kernels (rpt_hash_keys_composite, rpt_bf_insert_composite,
rpt_bf_probe_chain_composite, rpt_bf_transfer_composite, rpt_bf_insert_multi_composite) vs the oracle, bit-exact: the
hashes are orc.hash_columns (and the two-pass rpt.hash_columns), an inserted filter's words orc.insert_hashes of
exactly the inserted rows, a selection the AND of orc.lookup_sel_hashes over the listed positions. No tolerance
anywhere. Keys and probed filters come from tests/composite_util.py; destinations are test_gpu_transfer's Targets, put
back to known words before every use."""
import ctypes

import numpy as np
import pytest
import torch

import rpt_oracle as orc
from buf_util import (CAPTURE_MODE_GLOBAL, FF, GuardedBuffer, graph_destroy, graph_instantiate, stream_capture)
from composite_util import DENSE, DICT, LAYOUTS, MISALIGNED, Key, member_filter, row_list
from test_gpu_transfer import Col, Targets, check, dev, graph_node_count, sel_of

pytestmark = pytest.mark.gpu

SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS
I32, I64 = torch.int32, torch.int64
# (key types, the columns with NULLs): 2 columns; 3 with NULLs in the middle one; 4 with a HASH prefix
KEYSPECS = {"2": (("i64", "i32"), ()), "3nulls": (("i32", "i64", "i32"), (1,)), "4prefix": (("hash", "i32", "i64", "i32"), (2,))}
# a lone row, the segment edges, a second workgroup (4 waves of 512 rows), 257 segments
HASH_SIZES = [1, 511, 512, 513, 2567, 131075]


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def targets(rpt):
    t = Targets(rpt)
    yield t
    t.close()


def make_key(rng, spec, rows, layout=DENSE, special=None):
    kts, nulls = KEYSPECS[spec]
    prefix = Key(rng, ("i64", "i64"), rows).hashes() if kts[0] == "hash" else None
    return Key(rng, kts, rows, layout=layout, nulls=nulls, special=special, prefix=prefix)


# ---- hash and insert ------------------------------------------------------------------------------------------------
def check_hash_and_insert(rpt, targets, key, n, what):
    h = key.hashes()
    cols = key.columns(rpt)
    out = GuardedBuffer(8 * n).poison(FF)
    rpt.hash_columns_fused(cols, out=out.view(I64))
    got = out.view(I64).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, h), "%s: %d fused hashes differ from the oracle" % (what, int((got != h).sum()))
    out.assert_guards_intact("out_hashes")
    two_pass = rpt.hash_columns(cols).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, two_pass), "%s: fused and two-pass hashes differ" % what
    for log_nb in (10, 16):
        bf, base = targets.reset(log_nb, False)  # a fresh filter: zero words, no min/max
        assert not base.any()
        bf.insert_composite(cols)
        check(bf, key.expect(base, log_nb, np.arange(n)), "%s into 2^%d blocks" % (what, log_nb))
        assert bf.minmax() is None, "%s: a composite insert folded a min/max" % what


@pytest.mark.parametrize("spec", list(KEYSPECS))
@pytest.mark.parametrize("n", HASH_SIZES)
def test_hash_and_insert_vs_oracle(rpt, targets, n, spec):
    """All dense (hash_composite_kernel<true>, insert_composite_kernel<true>); one column behind a key_sel dictionary;
    one column's base off by one element (both <false>: not 16-byte aligned, the general mapping)."""
    rng = np.random.default_rng(1000 * n + len(spec))
    for layout in LAYOUTS:
        for special in ({None} if layout == DENSE else {1, len(KEYSPECS[spec][0]) - 1}):
            key = make_key(rng, spec, n, layout, special)
            check_hash_and_insert(rpt, targets, key, n, "%s %s n=%d" % (spec, layout, n))


def test_a_wave_takes_more_than_one_segment(rpt, targets):
    """The launchers' grid is insert_kernel's: up to 8 workgroups of 4 waves per CU, so at 131075 rows (257 segments) no
    wave takes a second segment on any device with more than 8 CUs. The smallest n at which one does is one row past
    CUs x 8 x 4 full segments; here three rows past, so the last segment is a tail."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 8 * 4 * 512 + 3
    rng = np.random.default_rng(77)
    for layout in (DENSE, MISALIGNED):
        key = make_key(rng, "2", n, layout)
        h = key.hashes()
        got = rpt.hash_columns_fused(key.columns(rpt)).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, h), layout
        bf, base = targets.reset(16, False)
        bf.insert_composite(key.columns(rpt))
        check(bf, key.expect(base, 16, np.arange(n)), layout)


@pytest.mark.parametrize("layout", [DENSE, DICT])
def test_one_repeated_pair_gives_the_same_words(rpt, targets, layout):
    """Every row holds the same pair: insert8 drops a row whose hash equals the previous row's before its atomic."""
    n = 2567
    rng = np.random.default_rng(5)
    key = make_key(rng, "2", n, layout)
    for c in key.cols:
        c.keys[:] = c.keys[0]
        c.d_keys.copy_(dev(c.keys))
        if c.validity is not None:
            c.validity[:] = ~np.uint64(0)
            c.d_validity.copy_(dev(c.validity))
    assert np.unique(key.hashes()).size == 1
    check_hash_and_insert(rpt, targets, key, n, "repeated pair %s" % layout)


# ---- the one-launch calls -------------------------------------------------------------------------------------------
# chains: the key types of each probed key
CHAINS = {
    "1": [("i32", "i64", "i32")],
    "3mixed": [("i64",), ("i64", "i32"), ("hash", "i32", "i64", "i32")],
    "8x2": [("i64", "i32"), ("i32", "i64"), ("i64", "i64"), ("i32", "i32"), ("hash", "i64"), ("i64", "i32"), ("i32", "i64"),
            ("hash", "i32")],
}
SMALL_SIZES = [1, 63, 64, 65, 512, 513, 1025, 2048, 16384]
ROW_SELS = [None, "ascending", "shuffled"]


def small_key(rng, kts, rows, j):
    """Key j of a list: NULLs in its last column, every third key with a dictionary column."""
    prefix = Key(rng, ("i64", "i32"), rows).hashes() if kts[0] == "hash" else None
    return Key(rng, kts, rows, layout=DICT if j % 3 == 1 else DENSE, nulls=(len(kts) - 1,), prefix=prefix)


class Chain:
    """The probed side of a call: one key and one member filter per entry of the chain."""

    def __init__(self, rpt, rng, chain, rows, share):
        self.keys = [small_key(rng, kts, rows, j) for j, kts in enumerate(chain)]
        self.filters, self.alive = [], np.ones(rows, dtype=bool)
        for j, k in enumerate(self.keys):
            bf, _w, passes = member_filter(rpt, rng, k, (10, 12, 16)[j % 3], share)
            self.filters.append(bf)
            self.alive &= passes

    def columns(self, rpt):
        return [k.columns(rpt) for k in self.keys]

    def close(self):
        for bf in self.filters:
            bf.close()


def check_sel(out, cnt, exp, what):
    got = int(cnt.view(I64).item())
    assert got == exp.size, "%s: count %d, oracle %d" % (what, got, exp.size)
    assert np.array_equal(sel_of(out.view(I32)[:got]), exp), what
    assert bool(torch.all(out.view(I32)[got:] == -1)), "%s: out_sel written past the returned count" % what
    out.assert_guards_intact("out_sel")
    cnt.assert_guards_intact("out_count")


def run_chain_and_transfer(rpt, targets, rng, chain_name, n, row_sel_kind, share=None):
    rows = max(n, 2048) if row_sel_kind else n
    # each filter keeps about share of the rows: the chain as a whole keeps a good tenth of them or more
    share = share if share is not None else 0.1 ** (1.0 / len(CHAINS[chain_name]))
    ids, d_row_sel = row_list(rng, row_sel_kind, n, rows)
    chain = Chain(rpt, rng, CHAINS[chain_name], rows, share)
    try:
        exp = ids[chain.alive[ids]]
        what = "%s n=%d %s" % (chain_name, n, row_sel_kind)
        out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
        kw = dict(row_sel=d_row_sel, n=n, out_sel=out.view(I32), out_count=cnt.view(I64))
        rpt.probe_chain_composite(chain.filters, chain.columns(rpt), **kw)
        check_sel(out, cnt, exp, "chain " + what)
        # the transfer: a two-column destination, a one-column one (min/max) and a HASH-prefixed three-column one
        dkeys = [small_key(rng, kts, rows, j) for j, kts in enumerate((("i32", "i64"), ("i64",), ("hash", "i64", "i32")))]
        dsts = [targets.reset(12, True), targets.reset(14, False), targets.reset(10, True)]
        out.poison(FF)
        cnt.poison(FF)
        rpt.transfer_composite(chain.filters, chain.columns(rpt), [bf for bf, _b in dsts], [k.columns(rpt) for k in dkeys], **kw)
        check_sel(out, cnt, exp, "transfer " + what)
        for j, (k, (bf, base)) in enumerate(zip(dkeys, dsts)):
            if exp.size:
                check(bf, k.expect(base, bf.log_num_blocks, exp), "destination %d of %s" % (j, what))
            else:  # an empty survivor set touches no destination word
                assert np.array_equal(bf.export_words(), base) and bf.minmax() is None, what
        return exp.size
    finally:
        chain.close()


@pytest.mark.parametrize("row_sel_kind", ROW_SELS, ids=["rows", "ascending", "shuffled"])
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_chain_and_transfer_vs_oracle(rpt, targets, n, row_sel_kind):
    """Chains of 1, 3 (one-, two- and four-column keys mixed) and 8 keys (two columns each: 16, the cap)."""
    rng = np.random.default_rng(31 * n + ROW_SELS.index(row_sel_kind))
    survivors = [run_chain_and_transfer(rpt, targets, rng, name, n, row_sel_kind) for name in CHAINS]
    if n >= 512:
        assert all(0 < s < n for s in survivors), survivors


def test_an_empty_survivor_set_touches_no_destination(rpt, targets):
    rng = np.random.default_rng(8)
    for row_sel_kind in ROW_SELS:
        assert run_chain_and_transfer(rpt, targets, rng, "3mixed", 1025, row_sel_kind, share=0.0) == 0


@pytest.mark.parametrize("with_row_sel", [False, True])
@pytest.mark.parametrize("n_dst", [1, 2, 8])
def test_insert_multi_vs_oracle(rpt, targets, n_dst, with_row_sel):
    """The sink of one vector into 1, 2 and 8 destinations (8 two-column keys: 16 columns, the cap; the eight are four
    filters, each listed twice)."""
    rng = np.random.default_rng(50 + n_dst + with_row_sel)
    for n in (1, 513, 2048, SMALL_ROWS):
        rows = max(n, 2048) if with_row_sel else n
        ids, d_row_sel = row_list(rng, "shuffled" if with_row_sel else None, n, rows)
        chain = ([("i64", "i32", "i64")], [("i32", "i64"), ("i64",)], CHAINS["8x2"])[(1, 2, 8).index(n_dst)]
        keys = [small_key(rng, kts, rows, j) for j, kts in enumerate(chain)]
        slots = [(10 + (j % 4), j % 2 == 0) for j in range(n_dst)]  # (log_nb, pre-filled); slots j and j + 4 are one filter
        distinct = {s: targets.reset(s[0], s[1]) for s in set(slots)}
        rpt.insert_multi_composite([distinct[s][0] for s in slots], [k.columns(rpt) for k in keys], row_sel=d_row_sel, n=n)
        for s, (bf, base) in distinct.items():
            words, mms = base.copy(), []
            for k, sk in zip(keys, slots):
                if sk == s:
                    words, mm = k.expect(words, s[0], ids)
                    mms.append(mm)
            mm = None if all(m is None for m in mms) else (min(m[0] for m in mms if m), max(m[1] for m in mms if m))
            check(bf, (words, mm), "n=%d destination %s" % (n, s))


# ---- one-column twins -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_sel_kind", [None, "shuffled"], ids=["rows", "shuffled"])
def test_one_column_keys_equal_the_single_column_calls(rpt, targets, row_sel_kind):
    """With every key one column, rpt_bf_transfer_composite / rpt_bf_probe_chain_composite / rpt_bf_insert_multi_composite
    leave what rpt_bf_transfer / rpt_bf_probe_chain / rpt_bf_insert_multi leave: out_sel, the count, the destinations'
    words and min/max."""
    n, rows = 2049, 4096 if row_sel_kind else 2049
    rng = np.random.default_rng(99)
    ids, d_row_sel = row_list(rng, row_sel_kind, n, rows)
    chain = Chain(rpt, rng, [("i64",), ("i32",), ("hash",)], rows, 0.7)
    dcols = [Col(rng, "i32", "valid", rows), Col(rng, "i64", "dict", rows), Col(rng, "hash", "flat", rows)]
    try:
        singles = [k.cols[0].as_dict(rpt) for k in chain.keys]
        dsingles = [c.as_dict(rpt) for c in dcols]

        def run(composite, call):
            dsts = [targets.reset(12, True), targets.reset(14, False), targets.reset(10, True)]
            bfs = [bf for bf, _b in dsts]
            out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
            kw = dict(row_sel=d_row_sel, n=n)
            okw = dict(out_sel=out.view(I32), out_count=cnt.view(I64), **kw)
            wrap = (lambda cs: [[c] for c in cs]) if composite else (lambda cs: cs)
            if call == "transfer":
                (rpt.transfer_composite if composite else rpt.transfer)(chain.filters, wrap(singles), bfs, wrap(dsingles), **okw)
            elif call == "chain":
                (rpt.probe_chain_composite if composite else rpt.probe_chain)(chain.filters, wrap(singles), **okw)
            else:
                (rpt.insert_multi_composite if composite else rpt.insert_multi)(bfs, wrap(dsingles), **kw)
            torch.cuda.synchronize()
            return (out.view(I32).cpu().numpy().copy(), int(cnt.view(I64).item()), [bf.export_words() for bf in bfs],
                    [bf.minmax() for bf in bfs])

        for call in ("transfer", "chain", "sink"):
            a, b = run(True, call), run(False, call)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], call
            assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and a[3] == b[3], call
            if call != "sink":
                assert np.array_equal(a[0][: a[1]].view(np.uint32), ids[chain.alive[ids]]), call
                assert 0 < a[1] < n
            if call != "chain":
                assert a[3][0] is not None and a[3][1] is not None and a[3][2] is None  # I32, I64, HASH
    finally:
        chain.close()


# ---- buffers --------------------------------------------------------------------------------------------------------
def test_a_row_sel_of_exactly_n_entries_is_never_read_past_n(rpt, targets):
    """row_sel holds n = 513 entries in an exactly sized buffer; a second run passes the same entries at the front of a
    longer buffer whose tail names rows that pass every filter: were an entry at or past n read, the count, the
    selection or a destination would differ between the runs and from the oracle."""
    n, rows = 513, 2048
    rng = np.random.default_rng(12)
    chain = Chain(rpt, rng, CHAINS["3mixed"], rows, 0.6)
    dkey = small_key(rng, ("i64", "i32"), rows, 0)
    try:
        passing = np.flatnonzero(chain.alive).astype(np.uint32)
        assert passing.size >= 64
        ids = rng.integers(0, rows, n).astype(np.uint32)
        exp = ids[chain.alive[ids]]
        exact = GuardedBuffer(4 * n)
        exact.view(I32).copy_(dev(ids))
        longer = dev(np.concatenate([ids, passing[rng.integers(0, passing.size, 1023)]]))
        for what, row_sel in (("exact", exact.view(I32)), ("poisoned tail", longer)):
            bf, base = targets.reset(12, True)
            out, cnt = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
            rpt.transfer_composite(chain.filters, chain.columns(rpt), [bf], [dkey.columns(rpt)], row_sel=row_sel, n=n,
                                   out_sel=out.view(I32), out_count=cnt.view(I64))
            check_sel(out, cnt, exp, what)
            check(bf, dkey.expect(base, 12, exp), what)
            bf, base = targets.reset(12, True)
            rpt.insert_multi_composite([bf], [dkey.columns(rpt)], row_sel=row_sel, n=n)
            check(bf, dkey.expect(base, 12, ids), what + " (sink)")
        exact.assert_guards_intact("row_sel")
    finally:
        chain.close()


def test_zero_rows_only_set_the_count(rpt, targets):
    rng = np.random.default_rng(3)
    chain = Chain(rpt, rng, CHAINS["3mixed"], 64, 0.5)
    dkey = small_key(rng, ("i64", "i32"), 64, 0)
    try:
        bf, base = targets.reset(12, True)
        cnt = GuardedBuffer(8).poison(FF)
        rpt.transfer_composite(chain.filters, chain.columns(rpt), [bf], [dkey.columns(rpt)], n=0, out_sel=torch.empty(1, dtype=I32, device="cuda:0"),
                               out_count=cnt.view(I64))
        assert int(cnt.view(I64).item()) == 0
        rpt.insert_multi_composite([bf], [dkey.columns(rpt)], n=0)
        assert np.array_equal(bf.export_words(), base) and bf.is_empty()
    finally:
        chain.close()


# ---- capture --------------------------------------------------------------------------------------------------------
def test_a_three_table_forward_step_is_one_graph_of_one_node_per_step(rpt):
    """Leaf table A sinks its two-column key into filter FA (rpt_bf_insert_multi_composite); table B probes FA on the
    two-column edge and sends its survivors' key on into FB (rpt_bf_transfer_composite); table C probes FB
    (rpt_bf_probe_chain_composite). Captured once, with torch.cuda.graph and under hipStreamCaptureModeGlobal (a
    synchronize, an allocation or a copy to the host would invalidate the capture): three kernel nodes. Replayed twice
    with the key tensors rewritten in between; FA and FB accumulate, as the oracle's words do."""
    n = 2048
    rng = np.random.default_rng(21)
    pool = [np.arange(4096, dtype=np.int64) * 7 + 3, (np.arange(4096) % 1000).astype(np.int32)]  # the tuples A can hold

    def draw(rows, hit):
        """Two-column rows: a share `hit` of them tuples of the pool, the rest random."""
        at = rng.integers(0, 4096, rows)
        miss = rng.random(rows) >= hit
        a = np.where(miss, rng.integers(-2**62, 2**62, rows), pool[0][at]).astype(np.int64)
        return a, pool[1][at].copy()

    host = {"a": draw(n, 1.0), "b": draw(n, 0.5), "b_out": (rng.integers(0, 3000, n).astype(np.int64),),
            "c": (rng.integers(0, 6000, n).astype(np.int64),)}
    d = {name: [dev(c) for c in cols] for name, cols in host.items()}
    fa, fb = rpt.BloomFilter(log_num_blocks=12), rpt.BloomFilter(log_num_blocks=12)
    wa, wb = orc.new_words(12), orc.new_words(12)
    mm_b = None
    for bf in (fa, fb):
        bf.settle()
    sel_b, cnt_b = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    sel_c, cnt_c = GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)

    def step(stream=None):
        rpt.insert_multi_composite([fa], [d["a"]], n=n, stream=stream)
        rpt.transfer_composite([fa], [d["b"]], [fb], [d["b_out"]], n=n, out_sel=sel_b.view(I32), out_count=cnt_b.view(I64),
                               stream=stream)
        rpt.probe_chain_composite([fb], [d["c"]], n=n, out_sel=sel_c.view(I32), out_count=cnt_c.view(I64), stream=stream)

    def rewrite():
        host.update(a=draw(n, 1.0), b=draw(n, 0.5), b_out=(rng.integers(0, 3000, n).astype(np.int64),),
                    c=(rng.integers(0, 6000, n).astype(np.int64),))
        for name, cols in host.items():
            for t, c in zip(d[name], cols):
                t.copy_(dev(c))
        for g in (sel_b, cnt_b, sel_c, cnt_c):
            g.poison(FF)
        torch.cuda.synchronize()

    def check_against_oracle(what):
        nonlocal mm_b
        orc.insert_hashes(wa, 12, orc.hash_columns(list(host["a"])))
        eb = orc.lookup_sel_hashes(wa, 12, orc.hash_columns(list(host["b"]))).astype(np.uint32)
        orc.insert_keys(wb, 12, host["b_out"][0], key_sel=eb)
        got = orc.minmax(host["b_out"][0], key_sel=eb)
        mm_b = got if mm_b is None else mm_b if got is None else (min(mm_b[0], got[0]), max(mm_b[1], got[1]))
        ec = orc.probe_keys(wb, 12, host["c"][0]).astype(np.uint32)
        check_sel(sel_b, cnt_b, eb, what + ": table B")
        check_sel(sel_c, cnt_c, ec, what + ": table C")
        check(fa, (wa, None), what + ": FA")  # a two-column key folds no min/max
        check(fb, (wb, mm_b), what + ": FB")
        return eb.size, ec.size

    step()
    torch.cuda.synchronize()
    counts = [check_against_oracle("eager")]
    # the raw capture, for its node count
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    raw, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _none = stream_capture(sh, CAPTURE_MODE_GLOBAL, raw, lambda: step(s))
    assert end == 0, "the capture was invalidated: something in the step synchronized, allocated or copied back"
    assert graph_node_count(raw) == 3
    assert graph_instantiate(raw, exe) == 0 and graph_destroy(exe, raw)
    # the same step under torch.cuda.graph, replayed
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for replay in range(2):
        rewrite()
        graph.replay()
        torch.cuda.synchronize()
        counts.append(check_against_oracle("replay %d" % replay))
    assert all(0 < b < n and 0 < c < n for b, c in counts), counts
    del graph
    fa.close()
    fb.close()
