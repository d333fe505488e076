"""A forward-and-backward pass of predicate transfer over three vector-sized tables in which every step is ONE kernel,
captured as one graph of exactly one node per step, both halves of the dynamic filter applied at every probe.

  tables    A, B, C: 2048 rows each; A joins B on b and C on c, B joins C on d
  leaf      A's kept rows (a host-known row_sel) build F_AB on A.b and F_AC on A.c         rpt_bf_insert_multi
  forward   B is probed by F_AB on B.b; its survivors build F_BC on B.d                    rpt_bf_transfer_range
            C is probed by F_AC on C.c and F_BC on C.d; its survivors build F_CB on C.d    rpt_bf_transfer_range
  backward  B's survivors (sel and count on the device) are probed by F_CB on B.d and
            what is left builds F_BA on B.b                                                rpt_bf_transfer_sel_range
            A's kept rows are probed by F_BA on A.b and what is left builds F_A on A.b     rpt_bf_transfer_sel_range

Every range is the min/max the building step folded on the device, read by the probing kernel of the same graph. The
filters are small (2^6 blocks for about 600 keys), so the Bloom test alone lets false positives through that the range
removes. The expectation is the oracle's replay of the schedule on the host; the same schedule made of the workspace
calls (rpt_bf_insert per filter, rpt_bf_transfer_range_ws, rpt_bf_transfer_sel_range_ws) must leave the same survivors
and filters."""
import ctypes

import numpy as np
import torch

import pytest
import rpt_oracle as orc
from buf_util import CAPTURE_MODE_GLOBAL, FF, GuardedBuffer, graph_destroy, graph_instantiate, graph_launch, stream_capture
from test_gpu_transfer import dev, graph_node_count, sel_of

pytestmark = pytest.mark.gpu

N = 2048
LOG = 6
FILTERS = ("AB", "AC", "BC", "CB", "BA", "A")
STEPS = 5


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


class HostFilter:
    def __init__(self):
        self.words, self.mm = orc.new_words(LOG), None

    def insert(self, keys, ids):
        ids = np.asarray(ids, dtype=np.uint32)
        orc.insert_keys(self.words, LOG, keys, key_sel=ids)
        if ids.size:
            mn, mx = orc.minmax(keys, key_sel=ids)
            self.mm = (mn, mx) if self.mm is None else (min(mn, self.mm[0]), max(mx, self.mm[1]))

    def probe(self, keys, ids):
        """(the rows of `ids` that pass the range and the Bloom test, those that pass the Bloom test), in order."""
        ids = np.asarray(ids, dtype=np.uint32)
        bloom = ids[orc.probe_keys(self.words, LOG, keys, key_sel=ids)]
        if self.mm is None:
            return bloom, bloom
        return bloom[(keys[bloom] >= self.mm[0]) & (keys[bloom] <= self.mm[1])], bloom


def host_schedule(t, a_kept):
    f = {name: HostFilter() for name in FILTERS}
    f["AB"].insert(t["A.b"], a_kept)
    f["AC"].insert(t["A.c"], a_kept)
    sel_b, bloom_b = f["AB"].probe(t["B.b"], np.arange(N))
    f["BC"].insert(t["B.d"], sel_b)
    c1, bloom_c = f["AC"].probe(t["C.c"], np.arange(N))
    sel_c, _ = f["BC"].probe(t["C.d"], c1)
    f["CB"].insert(t["C.d"], sel_c)
    sel_b2, _ = f["CB"].probe(t["B.d"], sel_b)
    f["BA"].insert(t["B.b"], sel_b2)
    sel_a, _ = f["BA"].probe(t["A.b"], a_kept)
    f["A"].insert(t["A.b"], sel_a)
    assert 0 < sel_b2.size < sel_b.size < bloom_b.size < N  # the range removes rows the Bloom test keeps
    assert 0 < sel_c.size < c1.size < bloom_c.size < N
    assert 0 < sel_a.size < a_kept.size
    return f, dict(B=sel_b, C=sel_c, B2=sel_b2, A=sel_a)


def test_three_table_pass_is_one_graph_of_one_node_per_step(rpt):
    rng = np.random.default_rng(20261)
    pool_b, pool_c, pool_d = (rng.integers(-(2**30), 2**30, 1500).astype(np.int64) for _ in range(3))

    def column(pool, frac):
        return np.where(rng.random(N) < frac, pool[rng.integers(0, pool.size, N)], rng.integers(-(2**40), 2**40, N)).astype(np.int64)

    t = {"A.b": column(pool_b, 1.0), "A.c": column(pool_c, 1.0), "B.b": column(pool_b, 0.5), "B.d": column(pool_d, 1.0),
         "C.c": column(pool_c, 0.6), "C.d": column(pool_d, 0.7)}
    a_kept = np.flatnonzero(rng.random(N) < 0.3).astype(np.uint32)  # A's local predicate
    d = {name: dev(col) for name, col in t.items()}
    d_kept = dev(a_kept)
    d_kept_count = torch.tensor([a_kept.size], dtype=torch.int64, device="cuda:0")
    i32, i64 = torch.int32, torch.int64

    def buffers():
        return {k: (GuardedBuffer(4 * N).poison(FF), GuardedBuffer(8).poison(FF)) for k in ("B", "C", "B2", "A")}

    one, ws = ({n: rpt.BloomFilter(log_num_blocks=LOG) for n in FILTERS} for _ in range(2))
    bufs, ws_bufs = buffers(), buffers()

    def out(b, k):
        return dict(out_sel=b[k][0].view(i32), out_count=b[k][1].view(i64))

    def schedule(stream):
        f, b = one, bufs
        rpt.insert_multi([f["AB"], f["AC"]], [d["A.b"], d["A.c"]], row_sel=d_kept, n=a_kept.size, stream=stream)
        rpt.transfer_range([f["AB"]], [d["B.b"]], [f["BC"]], [d["B.d"]], range_mask=1, n=N, stream=stream, **out(b, "B"))
        rpt.transfer_range([f["AC"], f["BC"]], [d["C.c"], d["C.d"]], [f["CB"]], [d["C.d"]], range_mask=0b11, n=N,
                           stream=stream, **out(b, "C"))
        rpt.transfer_sel_range([f["CB"]], [d["B.d"]], [f["BA"]], [d["B.b"]], b["B"][0].view(i32), b["B"][1].view(i64),
                               range_mask=1, stream=stream, **out(b, "B2"))
        rpt.transfer_sel_range([f["BA"]], [d["A.b"]], [f["A"]], [d["A.b"]], d_kept, d_kept_count, range_mask=1,
                               max_rows=a_kept.size, stream=stream, **out(b, "A"))

    def ws_schedule():
        f, b = ws, ws_bufs
        f["AB"].insert(d["A.b"], key_sel=d_kept, strategy=rpt.RPT_INSERT_ATOMIC)
        f["AC"].insert(d["A.c"], key_sel=d_kept, strategy=rpt.RPT_INSERT_ATOMIC)
        rpt.transfer_range_ws([f["AB"]], [d["B.b"]], [f["BC"]], [d["B.d"]], range_mask=1, n=N, **out(b, "B"))
        rpt.transfer_range_ws([f["AC"], f["BC"]], [d["C.c"], d["C.d"]], [f["CB"]], [d["C.d"]], range_mask=0b11, n=N,
                              **out(b, "C"))
        for probed, col, dst, dcol, sel, cnt, max_rows, k in (
                (f["CB"], d["B.d"], f["BA"], d["B.b"], b["B"][0].view(i32), b["B"][1].view(i64), N, "B2"),
                (f["BA"], d["A.b"], f["A"], d["A.b"], d_kept, d_kept_count, a_kept.size, "A")):
            w = torch.empty(rpt.probe_chain_sel_workspace_bytes([probed], max_rows), dtype=torch.uint8, device="cuda:0")
            rpt.transfer_sel_range_ws([probed], [col], [dst], [dcol], sel, cnt, range_mask=1, max_rows=max_rows, workspace=w,
                                      **out(b, k))

    exp_f, exp_sel = host_schedule(t, a_kept)
    print("survivors: " + ", ".join(f"{k} {v.size}" for k, v in exp_sel.items()) + f" (A kept {a_kept.size} of {N})")

    def check_against_host(what, filters, b):
        for k, e in exp_sel.items():
            got = int(b[k][1].view(i64).item())
            assert got == e.size, f"{what}: {k} count {got}, host {e.size}"
            assert np.array_equal(sel_of(b[k][0].view(i32)[:got]), e), f"{what}: {k}"
            assert bool(torch.all(b[k][0].view(i32)[got:] == -1)), f"{what}: {k} written past its count"
            b[k][0].assert_guards_intact(k)
            b[k][1].assert_guards_intact(k + " count")
        for name in FILTERS:
            assert np.array_equal(filters[name].export_words(), exp_f[name].words), f"{what}: F_{name} differs from the oracle"
            assert filters[name].minmax() == exp_f[name].mm, f"{what}: F_{name} min/max"

    def reset():
        """Outside any capture, on the current stream: the filters empty again, their deferred clears settled."""
        for bf in one.values():
            bf.clear()
            bf.settle()
        for sel, cnt in bufs.values():
            sel.poison(FF)
            cnt.poison(FF)
        torch.cuda.synchronize()

    ws_schedule()
    torch.cuda.synchronize()
    check_against_host("workspace calls", ws, ws_bufs)
    schedule(torch.cuda.current_stream())
    torch.cuda.synchronize()
    check_against_host("eager", one, bufs)

    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    reset()
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _none = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: schedule(s))
    assert end == 0, "the capture was invalidated: something in the schedule synchronized, allocated or copied back"
    assert graph_node_count(graph) == STEPS
    assert graph_instantiate(graph, exe) == 0
    for name, bf in one.items():  # capturing ran nothing
        assert not bf.export_words().any(), name
    assert graph_launch(exe, sh) == 0
    s.synchronize()
    check_against_host("replay", one, bufs)
    # ... and the workspace calls left the same survivors and filters
    for name in FILTERS:
        assert np.array_equal(one[name].export_words(), ws[name].export_words()), name
        assert one[name].minmax() == ws[name].minmax(), name
    assert graph_destroy(exe, graph)
    for bf in [*one.values(), *ws.values()]:
        bf.close()
