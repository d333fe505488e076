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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-iters", type=int, default=20, help="steps per round at up to 2^20 rows")
    ap.add_argument("--max-row-log", type=int, default=max(ROW_LOGS), help="skip batches above 2^this rows")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_probe_sel needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    configs = [c for c in CONFIGS if c[0] <= args.max_row_log]
    configs = configs if args.only is None else [configs[args.only]]
    for n_log, kib, frac in configs:
        row = measure(n_log, kib, frac, max(1, args.reps), max(1, args.small_iters))
        print(json.dumps(row), file=out, flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
