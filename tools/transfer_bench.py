"""One predicate-transfer step (USE_BF, then CREATE_BF's Sink over the survivors) on an HBM-resident batch, three
ways, in one process, alternating:

  (a) transfer  one rpt_bf_transfer_ws call: the chain's survivors go into the outgoing filter on the device (atomic
                ORs fed from the accumulated result bits, or from out_sel after the small-batch hand-over); nothing
                is read back;
  (b) loop      what a caller had before: rpt_bf_probe_chain_ws, the count copied back to the host, then
                rpt_bf_insert_ws with key_sel = out_sel and that count (free to take the PARTITIONED insert);
  (c) routed    one rpt_bf_transfer_insert_ws call: as (a), but an outgoing filter whose insert strategy resolves to
                PARTITIONED for the batch takes the routed insert (a partition pass over all rows in which a row that
                did not survive emits no record, then the LDS slice merge); nothing is read back.

The probed filter holds 2^19 synthetic build keys (512 KiB); the probe column passes about `pass fraction` of its
rows; the outgoing filter (128 KiB, 16 MiB or 128 MiB) is built on a second key column of the same rows. Both
methods start every round from a cleared, settled outgoing filter, and the filters are compared with
rpt_bf_is_same_as after every round. Large batches (2^27 rows) run one step per round; the DuckDB-sized batches
(2048 and 16384 rows) run `--small-iters` steps back to back per round, because there the saved round trip is the
whole point. Times are host wall clock around work that ends in a synchronise (per step); (a) and (c) are also timed with
device events. The tool does not load the oracle (test infrastructure): tests/test_gpu_transfer.py checks the entry
points.
Run on a GPU box:
    python tools/transfer_bench.py --out profiles/transfer/transfer.jsonl
    python tools/transfer_bench.py --set routed --out profiles/transfer/transfer_routed.jsonl
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "duckdb-robust-predicate-transfer_amd"))
import rpt_amd  # noqa: E402
from rpt_amd._lib import KeyColumn, check  # noqa: E402

SRC_LOG = 16  # the probed filter: 512 KiB
DST_KIB_LOG = {128: 14, 16384: 21, 131072: 24}  # outgoing filter KiB -> log2 blocks
FRACTIONS = [0.01, 0.1, 0.5, 0.9]
CONFIGS = [(n_log, kt, frac, kib) for n_log in (27, 11, 14) for kt in ("int64", "int32") for frac in FRACTIONS
           for kib in DST_KIB_LOG]
# --set routed: the 2^27-row lines, where (a) loses to (b), and one DuckDB-sized line (the hand-over is unchanged)
ROUTED_CONFIGS = [c for c in CONFIGS if c[0] == 27] + [(11, "int64", 0.5, 16384)]


def as_key_type(t: torch.Tensor, key_type: str) -> torch.Tensor:
    """int32 columns: the low 31 bits of the synthetic int64 keys."""
    return t if key_type == "int64" else (t & 0x7FFFFFFF).to(torch.int32)


def run_transfer(src, probe_col, dst, dst_col, n, sel, cnt, ws):
    lib = rpt_amd.load()
    handles = (ctypes.c_void_p * 1)(src.handle)
    dst_handles = (ctypes.c_void_p * 1)(dst.handle)
    cols = (KeyColumn * 1)(rpt_amd.make_column(probe_col))
    dcols = (KeyColumn * 1)(rpt_amd.make_column(dst_col))
    check(lib.rpt_bf_transfer_ws(handles, cols, 1, dst_handles, dcols, 1, None, n, sel.data_ptr(), cnt.data_ptr(),
                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))


def run_transfer_insert(src, probe_col, dst, dst_col, n, sel, cnt, ws, ins_ws):
    lib = rpt_amd.load()
    handles = (ctypes.c_void_p * 1)(src.handle)
    dst_handles = (ctypes.c_void_p * 1)(dst.handle)
    cols = (KeyColumn * 1)(rpt_amd.make_column(probe_col))
    dcols = (KeyColumn * 1)(rpt_amd.make_column(dst_col))
    check(lib.rpt_bf_transfer_insert_ws(handles, cols, 1, dst_handles, dcols, 1, None, n, sel.data_ptr(), cnt.data_ptr(),
                                        ws.data_ptr(), ws.numel(), ins_ws.data_ptr(), ins_ws.numel(),
                                        torch.cuda.current_stream().cuda_stream))


def run_loop(src, probe_col, dst, dst_col, n, sel, cnt, ws, ins_ws):
    lib = rpt_amd.load()
    stream = torch.cuda.current_stream().cuda_stream
    handles = (ctypes.c_void_p * 1)(src.handle)
    cols = (KeyColumn * 1)(rpt_amd.make_column(probe_col))
    check(lib.rpt_bf_probe_chain_ws(handles, cols, 1, None, n, sel.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream))
    m = int(cnt.item())  # the insert takes its row count as a host argument
    if m:
        col = rpt_amd.make_column(dst_col, key_sel=sel)
        check(lib.rpt_bf_insert_ws(dst.handle, ctypes.byref(col), m, ins_ws.data_ptr(), ins_ws.numel(), stream))
    return m


def measure(n_log, key_type, frac, kib, reps, small_iters):
    n = 1 << n_log
    iters = 1 if n > 16384 else small_iters
    n_build = 1 << (SRC_LOG + 3)
    src = rpt_amd.BloomFilter(log_num_blocks=SRC_LOG)
    src.insert(as_key_type(rpt_amd.synth_build_keys(n_build), key_type))
    probe_col = as_key_type(rpt_amd.synth_probe_keys(n, n_build, int(round(frac * 1000))), key_type)
    dst_col = as_key_type(rpt_amd.synth_build_keys(n, start=1 << 40), key_type)
    log_dst = DST_KIB_LOG[kib]
    dst_a, dst_b, dst_c = (rpt_amd.BloomFilter(log_num_blocks=log_dst) for _ in range(3))
    sel_a, sel_b, sel_c = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(rpt_amd.probe_chain_workspace_bytes([src], n), 256), dtype=torch.uint8, device="cuda")
    ins_ws = torch.empty(max(int(rpt_amd.load().rpt_insert_workspace_bytes(n, log_dst)), 256), dtype=torch.uint8,
                         device="cuda")
    row = {"op": "transfer", "n": n, "key_type": key_type, "pass_fraction": frac, "src_filter_kib": 8 << (SRC_LOG - 10),
           "dst_filter_kib": kib, "steps_per_round": iters, "reps": reps,
           "probe_strategy": src.probe_strategy_for(n), "routed_insert_strategy": dst_c.insert_strategy_for(n)}
    t_a, t_a_dev, t_b, t_c, t_c_dev = [], [], [], [], []
    for rep in range(reps + 1):  # the first round warms every kernel and is not counted
        for bf in (dst_a, dst_b, dst_c):
            bf.clear()
            bf.settle()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            run_transfer(src, probe_col, dst_a, dst_col, n, sel_a, cnt, ws)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        count_a = int(cnt.item())
        t2 = time.perf_counter()
        for _ in range(iters):
            count_b = run_loop(src, probe_col, dst_b, dst_col, n, sel_b, cnt, ws, ins_ws)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        e2, e3 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t4 = time.perf_counter()
        e2.record()
        for _ in range(iters):
            run_transfer_insert(src, probe_col, dst_c, dst_col, n, sel_c, cnt, ws, ins_ws)
        e3.record()
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        count_c = int(cnt.item())
        if rep:
            t_c.append((t5 - t4) * 1e3 / iters)
            t_c_dev.append(e2.elapsed_time(e3) / iters)
            t_a.append((t1 - t0) * 1e3 / iters)
            t_a_dev.append(e0.elapsed_time(e1) / iters)
            t_b.append((t3 - t2) * 1e3 / iters)
        assert count_a == count_b and torch.equal(sel_a[:count_a], sel_b[:count_b]), f"survivors differ: {row}"
        assert dst_a.is_same_as(dst_b), f"the two outgoing filters differ: {row}"
        assert count_c == count_a and torch.equal(sel_c[:count_c], sel_a[:count_a]), f"survivors differ (routed): {row}"
        assert dst_c.is_same_as(dst_a), f"the routed transfer's outgoing filter differs: {row}"
        row["survivors"] = count_a
        row["loop_insert_strategy"] = dst_b.insert_strategy_for(count_b) if count_b else 0
    for name, t in (("transfer_ms", t_a), ("transfer_device_ms", t_a_dev), ("loop_ms", t_b), ("routed_ms", t_c),
                    ("routed_device_ms", t_c_dev)):
        row[name + "_mean"] = round(sum(t) / len(t), 5)
        row[name + "_min"] = round(min(t), 5)
    for bf in (src, dst_a, dst_b, dst_c):
        bf.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small-iters", type=int, default=50, help="steps per round at 2048 / 16384 rows")
    ap.add_argument("--set", choices=["all", "routed"], default="all",
                    help="routed: the 2^27-row lines and one DuckDB-sized line")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("transfer_bench needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    configs = CONFIGS if args.set == "all" else ROUTED_CONFIGS
    configs = configs if args.only is None else [configs[args.only]]
    for n_log, key_type, frac, kib in configs:
        row = measure(n_log, key_type, frac, kib, max(1, args.reps), max(1, args.small_iters))
        print(json.dumps(row), file=out, flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
