"""One forward step of predicate transfer over one DuckDB-sized vector (scan -> USE_BF chain -> CREATE_BF sink), three
ways, in one process, alternating; and the sink of one vector into several filters, two ways. The protocol is that of
tools/bench_probe_sel.py --small.

A full vector of n rows (2048, 8192 or 16384; row_sel null: rows 0 .. n of the columns) goes through 1, 3 or 8 filters
(all 128 KiB or all 16 MiB) and its survivors into 1 or 2 outgoing filters of the same size, about 0.1, 0.5 or 0.9 of the
rows surviving the chain:
  (a) small  rpt_bf_transfer: one launch;
  (b) ws     rpt_bf_transfer_ws with the same arguments: today's hand-over, probe_chain_small_kernel and one
             insert_sel_kernel per destination;
  (c) loop   the host loop: rpt_bf_probe_chain, synchronize, read the count, one rpt_bf_insert_sel per destination.
The sink: rpt_bf_insert_multi into 1, 2 or 4 filters against one rpt_bf_insert per filter.
Per-step time is device-event time around `--steps` steps enqueued back to back on a warmed device, over the steps
((c) synchronizes once per step, as it must); the median, minimum and maximum over `--reps` rounds are reported, after a
round that is not counted. (a), (b) and both sinks are also captured into a graph of one step each and replayed
`--steps` times. All sides produce the same selection and the same filter words, compared after the rounds. Synthetic
keys only; nothing outside the repository is read. Run on a GPU box:
    python tools/bench_transfer_small.py --out profiles/transfer_small/transfer_small.jsonl
    python tools/bench_transfer_small.py --sink --out profiles/transfer_small/insert_multi.jsonl
--rows / --fraction / --only keep a part of the configurations."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "duckdb-robust-predicate-transfer_amd"))
import rpt_amd  # noqa: E402
from rpt_amd._lib import KeyColumn, check  # noqa: E402

ROWS = (2048, 8192, 16384)
CHAINS = (1, 3, 8)
KIB_LOG = {128: 14, 16384: 21}
DSTS = (1, 2)
SINK_DSTS = (1, 2, 4)
FRACTIONS = (0.1, 0.5, 0.9)
CONFIGS = [(kib, k, n, n_dst, frac) for kib in KIB_LOG for k in CHAINS for n in ROWS for n_dst in DSTS for frac in FRACTIONS]
SINK_CONFIGS = [(kib, n, m) for kib in KIB_LOG for n in ROWS for m in SINK_DSTS]


def spread(name, values, row):
    row[name + "_median"] = round(statistics.median(values), 5)
    row[name + "_min"] = round(min(values), 5)
    row[name + "_max"] = round(max(values), 5)


class Pool:
    """The filters of one size, made once: 8 probed filters over the synthetic build keys and, per side, 4 outgoing
    filters (each side writes filters of its own, so their words can be compared)."""

    def __init__(self, kib, sides):
        self.log = KIB_LOG[kib]
        self.n_build = 1 << (self.log + 2)
        self.probed = []
        for _ in range(max(CHAINS)):
            bf = rpt_amd.BloomFilter(log_num_blocks=self.log)
            bf.insert(rpt_amd.synth_build_keys(self.n_build))
            self.probed.append(bf)
        self.dst = {s: [rpt_amd.BloomFilter(log_num_blocks=self.log) for _ in range(max(SINK_DSTS))] for s in sides}
        for side in self.dst.values():
            for bf in side:  # their first write is not the timed one
                bf.insert(rpt_amd.synth_build_keys(1024, start=1 << 40))
        torch.cuda.synchronize()

    def reset(self):
        """Every outgoing filter empty again, its deferred clear settled outside any capture."""
        for side in self.dst.values():
            for bf in side:
                bf.clear()
                bf.settle()
        torch.cuda.synchronize()

    def close(self):
        for bf in self.probed + [bf for side in self.dst.values() for bf in side]:
            bf.close()


class Timer:
    def __init__(self, steps):
        self.steps = steps

    def eager(self, step):
        stream = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(self.steps):
            step(stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / self.steps  # us per step

    def captured(self, step):
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step(torch.cuda.current_stream().cuda_stream)
        return graph

    def replayed(self, graph):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(self.steps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / self.steps

    def rounds(self, reps, eager, graphs):
        """{name: [us per step of every counted round]}; the sides alternate within a round."""
        times = {name: [] for name in list(eager) + list(graphs)}
        for rep in range(reps + 1):  # the first round warms up and is not counted
            got = {name: self.eager(step) for name, step in eager.items()}
            for name, graph in graphs.items():
                got[name] = self.replayed(graph)
            if rep:
                for name, v in got.items():
                    times[name].append(v)
        return times


def same_filters(pool, sides, n_dst, row):
    ref = [bf.export_words() for bf in pool.dst[sides[0]][:n_dst]]
    for s in sides[1:]:
        for j, bf in enumerate(pool.dst[s][:n_dst]):
            assert np.array_equal(bf.export_words(), ref[j]) and bf.minmax() == pool.dst[sides[0]][j].minmax(), \
                f"destination {j} of side {s} differs: {row}"


def measure(pool, kib, k, n, n_dst, frac, reps, steps):
    lib = rpt_amd.load()
    filters = pool.probed[:k]
    permille = int(round(frac ** (1.0 / k) * 1000))  # per filter, so that about `frac` survive the chain
    cols = [rpt_amd.synth_probe_keys(n, pool.n_build, permille, start=(j + 1) << 33) for j in range(k)]
    dcols = [rpt_amd.synth_probe_keys(n, pool.n_build, 0, start=(j + 101) << 33) for j in range(n_dst)]
    out = {m: (torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
           for m in "abc"}
    ws = torch.empty(max(rpt_amd.probe_chain_workspace_bytes(filters, n), 256), dtype=torch.uint8, device="cuda")
    handles = (ctypes.c_void_p * k)(*[f.handle for f in filters])
    arr = (KeyColumn * k)(*[rpt_amd.make_column(c) for c in cols])
    dh = {m: (ctypes.c_void_p * n_dst)(*[f.handle for f in pool.dst[m][:n_dst]]) for m in "abc"}
    darr = (KeyColumn * n_dst)(*[rpt_amd.make_column(c) for c in dcols])

    def step_a(stream):
        check(lib.rpt_bf_transfer(handles, arr, k, dh["a"], darr, n_dst, None, n, out["a"][0].data_ptr(),
                                  out["a"][1].data_ptr(), stream))

    def step_b(stream):
        check(lib.rpt_bf_transfer_ws(handles, arr, k, dh["b"], darr, n_dst, None, n, out["b"][0].data_ptr(),
                                     out["b"][1].data_ptr(), ws.data_ptr(), ws.numel(), stream))

    def step_c(stream):
        o, c = out["c"][0].data_ptr(), out["c"][1].data_ptr()
        check(lib.rpt_bf_probe_chain(handles, arr, k, None, n, o, c, stream))
        torch.cuda.current_stream().synchronize()
        int(out["c"][1].item())  # the count reaches the host, as a caller without the transfer needs it
        for j in range(n_dst):
            check(lib.rpt_bf_insert_sel(pool.dst["c"][j].handle, ctypes.byref(darr[j]), o, c, n, stream))

    row = {"op": "transfer_small", "rows": n, "filters": k, "filter_kib": kib, "destinations": n_dst,
           "survivor_fraction": frac, "row_sel": None, "steps": steps, "reps": reps}
    timer = Timer(steps)
    pool.reset()
    for step in (step_a, step_b, step_c):  # every kernel once outside any capture
        step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    graphs = {"small_graph_us": timer.captured(step_a), "ws_graph_us": timer.captured(step_b)}
    times = timer.rounds(reps, {"small_us": step_a, "ws_us": step_b, "loop_us": step_c}, graphs)
    counts = {m: int(out[m][1].item()) for m in "abc"}
    assert counts["a"] == counts["b"] == counts["c"], f"counts differ: {counts} {row}"
    for m in "bc":
        assert torch.equal(out["a"][0][: counts["a"]], out[m][0][: counts[m]]), f"selections differ: {row}"
    same_filters(pool, "abc", n_dst, row)
    row["survivors"] = counts["a"]
    for name, v in times.items():
        spread(name, v, row)
    row["ws_over_small"] = round(row["ws_us_median"] / row["small_us_median"], 3)
    row["loop_over_small"] = round(row["loop_us_median"] / row["small_us_median"], 3)
    row["ws_graph_over_small_graph"] = round(row["ws_graph_us_median"] / row["small_graph_us_median"], 3)
    return row


def measure_sink(pool, kib, n, m, reps, steps):
    lib = rpt_amd.load()
    dcols = [rpt_amd.synth_probe_keys(n, pool.n_build, 0, start=(j + 101) << 33) for j in range(m)]
    darr = (KeyColumn * m)(*[rpt_amd.make_column(c) for c in dcols])
    dh = (ctypes.c_void_p * m)(*[f.handle for f in pool.dst["a"][:m]])

    def step_multi(stream):
        check(lib.rpt_bf_insert_multi(dh, darr, m, None, n, stream))

    def step_each(stream):
        for j in range(m):
            check(lib.rpt_bf_insert(pool.dst["b"][j].handle, ctypes.byref(darr[j]), n, stream))

    row = {"op": "insert_multi", "rows": n, "filter_kib": kib, "destinations": m, "row_sel": None, "steps": steps,
           "reps": reps}
    timer = Timer(steps)
    pool.reset()
    for step in (step_multi, step_each):
        step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    graphs = {"multi_graph_us": timer.captured(step_multi), "each_graph_us": timer.captured(step_each)}
    times = timer.rounds(reps, {"multi_us": step_multi, "each_us": step_each}, graphs)
    same_filters(pool, "ab", m, row)
    for name, v in times.items():
        spread(name, v, row)
    row["each_over_multi"] = round(row["each_us_median"] / row["multi_us_median"], 3)
    row["each_graph_over_multi_graph"] = round(row["each_graph_us_median"] / row["multi_graph_us_median"], 3)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="steps per round")
    ap.add_argument("--sink", action="store_true", help="rpt_bf_insert_multi against one rpt_bf_insert per filter")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--rows", type=int, default=None, help="only the configurations of this many rows")
    ap.add_argument("--fraction", type=float, default=None, help="only this survivor fraction")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_transfer_small needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    reps, steps = max(1, args.reps), max(1, args.steps)
    if args.sink:
        configs = SINK_CONFIGS if args.only is None else [SINK_CONFIGS[args.only]]
        configs = [c for c in configs if args.rows in (None, c[1])]
    else:
        configs = CONFIGS if args.only is None else [CONFIGS[args.only]]
        configs = [c for c in configs if args.rows in (None, c[2]) and args.fraction in (None, c[4])]
    pool, pool_kib = None, None
    for c in configs:
        if c[0] != pool_kib:
            if pool is not None:
                pool.close()
            pool, pool_kib = Pool(c[0], "ab" if args.sink else "abc"), c[0]
        row = measure_sink(pool, *c, reps, steps) if args.sink else measure(pool, *c, reps, steps)
        print(json.dumps(row), file=out, flush=True)
    if pool is not None:
        pool.close()


if __name__ == "__main__":
    main()
