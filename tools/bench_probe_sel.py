"""The second probe of a table (predicate transfer's backward pass) on an HBM-resident batch, two ways, in one process,
alternating:

  (a) sel   the device-counted call: rpt_bf_probe_chain_ws over the first-pass filter, then rpt_bf_probe_chain_sel_ws
            over the second-pass filter with sel = the first probe's out_sel and count_dev = its count; nothing is read
            back in between (the second-pass filter runs rpt_bf_probe_sel_strategy_for: routed strategies demoted to the
            masked gather);
  (b) loop  what a caller had before: the same first probe, a stream synchronize, the count copied to the host, then
            rpt_bf_probe_chain_ws(row_sel = out_sel, n = count) with the second-pass filter on AUTO (free to take the
            partitioned probe over the survivors only).

The first-pass filter holds 2^19 synthetic build keys (512 KiB) and passes about `survivor fraction` of the rows; the
second-pass filter (128 KiB, 16 MiB or 128 MiB) is probed on a second key column of the same rows, of which about half
pass. Both sides produce the same selection, compared after every round. Times are host wall clock from the first
enqueue to a final synchronize, per step (batches of up to 2^20 rows run `--small-iters` steps back to back per round:
there the round trip is the whole point; (a) then synchronizes once at the end, (b) once per step, as it must), and
device-event time around the second call alone. The first round warms every kernel and is not counted; the median, the
minimum and the maximum of the counted rounds are reported. Synthetic keys only; nothing outside the repository is read.
Run on a GPU box:
    python tools/bench_probe_sel.py --out profiles/probe_sel/probe_sel.jsonl

--small: the one-launch calls for DuckDB-sized vectors instead (rpt_bf_probe_chain_sel / rpt_bf_transfer_sel), one
backward step of predicate transfer per vector: a full vector of max_rows positions (2048, 8192 or 16384; sel and the
count already on the device; sel holds max_rows of the table's 2 max_rows row ids, ascending as an earlier probe leaves
them, or in any order with --sel-order random) goes through 1, 3 or 8 filters (all 128 KiB or all 16 MiB) and its
survivors into 0, 1 or 2 outgoing filters of the same size, about 0.1, 0.5 or 0.9 of the rows surviving the chain. Three
ways, in one process, alternating:
  (a) small  the one-launch call;
  (b) ws     the workspace call it twins (rpt_bf_probe_chain_sel_ws / rpt_bf_transfer_sel_ws): 4 to 19 launches;
  (c) loop   the host loop: synchronize, read the count, rpt_bf_probe_chain(row_sel = sel, n = count), then one
             rpt_bf_insert_sel per outgoing filter.
Per-step time is device-event time around `--steps` steps enqueued back to back on a warmed device, over the steps
((c) synchronizes once per step, as it must); the median, minimum and maximum over `--reps` rounds are reported, after a
round that is not counted. (a) and (b) are also captured into a graph of one step each and replayed `--steps` times.
All three produce the same selection, compared after the rounds.
    python tools/bench_probe_sel.py --small --out profiles/probe_sel_small/probe_sel_small.jsonl
--rows / --fraction keep a part of them; RPT_GPU_LIB names another build of the library to measure (profiles/chain_call/).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "duckdb-robust-predicate-transfer_amd"))
import rpt_amd  # noqa: E402
from rpt_amd._lib import KeyColumn, check  # noqa: E402

FIRST_LOG = 16  # the first-pass filter: 512 KiB
SECOND_KIB_LOG = {128: 14, 16384: 21, 131072: 24}  # second-pass filter KiB -> log2 blocks
ROW_LOGS = (14, 20, 24, 27)
FRACTIONS = (0.05, 0.5, 0.9)
CONFIGS = [(n_log, kib, frac) for n_log in ROW_LOGS for kib in SECOND_KIB_LOG for frac in FRACTIONS]


def chain_ws(bf, col, row_sel, n, out_sel, out_count, ws):
    handles = (ctypes.c_void_p * 1)(bf.handle)
    cols = (KeyColumn * 1)(rpt_amd.make_column(col))
    check(rpt_amd.load().rpt_bf_probe_chain_ws(handles, cols, 1, None if row_sel is None else row_sel.data_ptr(), n,
                                               out_sel.data_ptr(), out_count.data_ptr(), ws.data_ptr(), ws.numel(),
                                               torch.cuda.current_stream().cuda_stream))


def chain_sel_ws(bf, col, sel, count, max_rows, out_sel, out_count, ws):
    handles = (ctypes.c_void_p * 1)(bf.handle)
    cols = (KeyColumn * 1)(rpt_amd.make_column(col))
    check(rpt_amd.load().rpt_bf_probe_chain_sel_ws(handles, cols, 1, sel.data_ptr(), count.data_ptr(), max_rows,
                                                   out_sel.data_ptr(), out_count.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))


def spread(name, values, row):
    row[name + "_median"] = round(statistics.median(values), 5)
    row[name + "_min"] = round(min(values), 5)
    row[name + "_max"] = round(max(values), 5)


def measure(n_log, kib, frac, reps, small_iters):
    n = 1 << n_log
    iters = small_iters if n_log <= 20 else 1
    n_build1 = 1 << (FIRST_LOG + 3)
    first = rpt_amd.BloomFilter(log_num_blocks=FIRST_LOG)
    first.insert(rpt_amd.synth_build_keys(n_build1))
    log2nd = SECOND_KIB_LOG[kib]
    n_build2 = 1 << (log2nd + 2)
    second = rpt_amd.BloomFilter(log_num_blocks=log2nd)
    second.insert(rpt_amd.synth_build_keys(n_build2))
    torch.cuda.synchronize()
    col1 = rpt_amd.synth_probe_keys(n, n_build1, int(round(frac * 1000)))
    col2 = rpt_amd.synth_probe_keys(n, n_build2, 500, start=1 << 33)
    sel1, sel_a, sel_b = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    cnt1, cnt_a, cnt_b = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3))
    ws1 = torch.empty(max(rpt_amd.probe_chain_workspace_bytes([first], n), 256), dtype=torch.uint8, device="cuda")
    ws_a = torch.empty(max(rpt_amd.probe_chain_sel_workspace_bytes([second], n), 256), dtype=torch.uint8, device="cuda")
    # the host loop's second call is sized for the largest count it can see
    ws_b = torch.empty(max(int(rpt_amd.load().rpt_probe_workspace_bytes(n, log2nd)) + (n // 8 + n // 512 * 8 + 4096) * 2,
                           rpt_amd.probe_chain_workspace_bytes([second], n), 256), dtype=torch.uint8, device="cuda")
    row = {"op": "probe_sel", "max_rows": n, "survivor_fraction": frac, "first_filter_kib": 8 << (FIRST_LOG - 10),
           "second_filter_kib": kib, "steps_per_round": iters, "reps": reps,
           "first_strategy": first.probe_strategy_for(n), "sel_strategy": second.probe_sel_strategy_for(n)}
    t_a, t_a_dev, t_b, t_b_dev = [], [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for rep in range(reps + 1):  # the first round warms every kernel and is not counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            chain_ws(first, col1, None, n, sel1, cnt1, ws1)
            ev[0].record()
            chain_sel_ws(second, col2, sel1, cnt1, n, sel_a, cnt_a, ws_a)
            ev[1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        a_dev = ev[0].elapsed_time(ev[1])  # the last step's second call
        count_a = int(cnt_a.item())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for _ in range(iters):
            chain_ws(first, col1, None, n, sel1, cnt1, ws1)
            torch.cuda.current_stream().synchronize()
            m = int(cnt1.item())  # the second probe takes its row count as a host argument
            need = rpt_amd.probe_chain_workspace_bytes([second], m)
            assert need <= ws_b.numel(), (need, ws_b.numel())
            ev[2].record()
            chain_ws(second, col2, sel1, m, sel_b, cnt_b, ws_b)
            ev[3].record()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        b_dev = ev[2].elapsed_time(ev[3])
        count_b = int(cnt_b.item())
        if rep:
            t_a.append((t1 - t0) * 1e3 / iters)
            t_b.append((t3 - t2) * 1e3 / iters)
            t_a_dev.append(a_dev)
            t_b_dev.append(b_dev)
        assert count_a == count_b and torch.equal(sel_a[:count_a], sel_b[:count_b]), f"selections differ: {row}"
        row["first_pass_survivors"] = m
        row["survivors"] = count_a
        row["loop_strategy"] = second.probe_strategy_for(m) if m else 0
    spread("sel_ms", t_a, row)
    spread("loop_ms", t_b, row)
    spread("sel_second_call_device_ms", t_a_dev, row)
    spread("loop_second_call_device_ms", t_b_dev, row)
    row["loop_over_sel"] = round(row["loop_ms_median"] / row["sel_ms_median"], 3)
    for bf in (first, second):
        bf.close()
    return row


# ---- --small: the one-launch calls against the workspace calls and the host loop --------------------------------------
SMALL_ROWS = (2048, 8192, 16384)
SMALL_CHAINS = (1, 3, 8)
SMALL_KIB_LOG = {128: 14, 16384: 21}
SMALL_DSTS = (0, 1, 2)
SMALL_FRACTIONS = (0.1, 0.5, 0.9)
SMALL_CONFIGS = [(kib, k, n, n_dst, frac) for kib in SMALL_KIB_LOG for k in SMALL_CHAINS for n in SMALL_ROWS
                 for n_dst in SMALL_DSTS for frac in SMALL_FRACTIONS]


class SmallPool:
    """The filters of one size, made once: 8 probed filters over the synthetic build keys and 2 outgoing filters."""

    def __init__(self, kib):
        self.log = SMALL_KIB_LOG[kib]
        self.n_build = 1 << (self.log + 2)
        self.probed = []
        for _ in range(max(SMALL_CHAINS)):
            bf = rpt_amd.BloomFilter(log_num_blocks=self.log)
            bf.insert(rpt_amd.synth_build_keys(self.n_build))
            self.probed.append(bf)
        self.dst = [rpt_amd.BloomFilter(log_num_blocks=self.log) for _ in range(max(SMALL_DSTS))]
        for bf in self.dst:  # their first write is not the timed one
            bf.insert(rpt_amd.synth_build_keys(1024, start=1 << 40))
        torch.cuda.synchronize()

    def close(self):
        for bf in self.probed + self.dst:
            bf.close()


def measure_small(pool, kib, k, n, n_dst, frac, reps, steps, sel_order):
    lib = rpt_amd.load()
    filters, dsts = pool.probed[:k], pool.dst[:n_dst]
    permille = int(round(frac ** (1.0 / k) * 1000))  # per filter, so that about `frac` survive the chain
    # the vector's positions select n of the 2 n rows of the table's columns: in ascending order, as an earlier probe
    # leaves its survivors, or in any order (every key load then its own cache line)
    rows = 2 * n
    cols = [rpt_amd.synth_probe_keys(rows, pool.n_build, permille, start=(j + 1) << 33) for j in range(k)]
    dcols = [rpt_amd.synth_probe_keys(rows, pool.n_build, 0, start=(j + 101) << 33) for j in range(n_dst)]
    sel = torch.randperm(rows, device="cuda")[:n]
    if sel_order == "ascending":
        sel = torch.sort(sel).values
    sel = sel.to(torch.int32).contiguous()
    count = torch.full((1,), n, dtype=torch.int64, device="cuda")
    out = {m: (torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
           for m in "abc"}
    ws = torch.empty(max(rpt_amd.probe_chain_sel_workspace_bytes(filters, n), 256), dtype=torch.uint8, device="cuda")
    handles = (ctypes.c_void_p * k)(*[f.handle for f in filters])
    arr = (KeyColumn * k)(*[rpt_amd.make_column(c) for c in cols])
    dhandles = (ctypes.c_void_p * max(n_dst, 1))(*[f.handle for f in dsts])
    darr = (KeyColumn * max(n_dst, 1))(*[rpt_amd.make_column(c) for c in dcols])
    p_sel, p_count = sel.data_ptr(), count.data_ptr()

    def step_a(stream):
        o, c = out["a"][0].data_ptr(), out["a"][1].data_ptr()
        if n_dst:
            check(lib.rpt_bf_transfer_sel(handles, arr, k, dhandles, darr, n_dst, p_sel, p_count, n, o, c, stream))
        else:
            check(lib.rpt_bf_probe_chain_sel(handles, arr, k, p_sel, p_count, n, o, c, stream))

    def step_b(stream):
        o, c = out["b"][0].data_ptr(), out["b"][1].data_ptr()
        if n_dst:
            check(lib.rpt_bf_transfer_sel_ws(handles, arr, k, dhandles, darr, n_dst, p_sel, p_count, n, o, c,
                                             ws.data_ptr(), ws.numel(), stream))
        else:
            check(lib.rpt_bf_probe_chain_sel_ws(handles, arr, k, p_sel, p_count, n, o, c, ws.data_ptr(), ws.numel(),
                                                stream))

    def step_c(stream):
        o, c = out["c"][0].data_ptr(), out["c"][1].data_ptr()
        torch.cuda.current_stream().synchronize()
        m = int(count.item())  # the chain takes its row count as a host argument
        check(lib.rpt_bf_probe_chain(handles, arr, k, p_sel, m, o, c, stream))
        for j in range(n_dst):
            check(lib.rpt_bf_insert_sel(dsts[j].handle, ctypes.byref(darr[j]), o, c, n, stream))

    def eager(step):
        stream = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps  # us per step

    def captured(step):
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step(torch.cuda.current_stream().cuda_stream)
        return graph

    def replayed(graph):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    row = {"op": "probe_sel_small", "max_rows": n, "filters": k, "filter_kib": kib, "destinations": n_dst,
           "survivor_fraction": frac, "sel_order": sel_order, "steps": steps, "reps": reps}
    times = {name: [] for name in ("small_us", "ws_us", "loop_us", "small_graph_us", "ws_graph_us")}
    for step in (step_a, step_b, step_c):  # every kernel once outside any capture
        step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    graphs = {"small_graph_us": captured(step_a), "ws_graph_us": captured(step_b)}
    for rep in range(reps + 1):  # the first round warms up and is not counted
        got = {"small_us": eager(step_a), "ws_us": eager(step_b), "loop_us": eager(step_c)}
        for name, graph in graphs.items():
            got[name] = replayed(graph)
        if rep:
            for name, v in got.items():
                times[name].append(v)
    counts = {m: int(out[m][1].item()) for m in "abc"}
    assert counts["a"] == counts["b"] == counts["c"], f"counts differ: {counts} {row}"
    for m in "bc":
        assert torch.equal(out["a"][0][: counts["a"]], out[m][0][: counts[m]]), f"selections differ: {row}"
    row["survivors"] = counts["a"]
    for name, v in times.items():
        spread(name, v, row)
    row["ws_over_small"] = round(row["ws_us_median"] / row["small_us_median"], 3)
    row["loop_over_small"] = round(row["loop_us_median"] / row["small_us_median"], 3)
    row["ws_graph_over_small_graph"] = round(row["ws_graph_us_median"] / row["small_graph_us_median"], 3)
    return row


def main_small(args, out):
    configs = SMALL_CONFIGS if args.only is None else [SMALL_CONFIGS[args.only]]
    configs = [c for c in configs if args.rows in (None, c[2]) and args.fraction in (None, c[4])]
    pool, pool_kib = None, None
    for kib, k, n, n_dst, frac in configs:
        if kib != pool_kib:
            if pool is not None:
                pool.close()
            pool, pool_kib = SmallPool(kib), kib
        row = measure_small(pool, kib, k, n, n_dst, frac, max(1, args.reps), max(1, args.steps), args.sel_order)
        print(json.dumps(row), file=out, flush=True)
    if pool is not None:
        pool.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-iters", type=int, default=20, help="steps per round at up to 2^20 rows")
    ap.add_argument("--max-row-log", type=int, default=max(ROW_LOGS), help="skip batches above 2^this rows")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    ap.add_argument("--small", action="store_true", help="the one-launch calls for DuckDB-sized vectors (see above)")
    ap.add_argument("--steps", type=int, default=200, help="--small: steps per round")
    ap.add_argument("--rows", type=int, default=None, help="--small: only the configurations of this many positions")
    ap.add_argument("--fraction", type=float, default=None, help="--small: only this survivor fraction")
    ap.add_argument("--sel-order", choices=("ascending", "random"), default="ascending",
                    help="--small: the order of the row ids in sel (an earlier probe leaves them ascending)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_probe_sel needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    if args.small:
        main_small(args, out)
        return
    configs = [c for c in CONFIGS if c[0] <= args.max_row_log]
    configs = configs if args.only is None else [configs[args.only]]
    for n_log, kib, frac in configs:
        row = measure(n_log, kib, frac, max(1, args.reps), max(1, args.small_iters))
        print(json.dumps(row), file=out, flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
