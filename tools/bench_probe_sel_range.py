"""What a filter's min/max range costs, and saves, in the device-counted probes and in the one-launch chain: the ranged
calls against their plain twins and against the host loop, in one process, alternating. sel holds max_rows of the
table's 2 max_rows row ids, ascending as an earlier probe leaves them, and the count (= max_rows) is on the device.
Filter 0 is the flagged one; its range is pinned with set_minmax so that it covers 5, 50 or 100 % of the probed keys of
its column; about 0.9 of the rows pass every Bloom test.

default: the one-launch calls at 2048 / 8192 / 16384 positions, 1 / 3 filters of 128 KiB or 16 MiB, 0 / 1 destinations
  (a) one    rpt_bf_probe_chain_sel_range / rpt_bf_transfer_sel_range;
  (b) plain  the plain one-launch call (rpt_bf_probe_chain_sel / rpt_bf_transfer_sel): no range, more survivors;
  (c) ws     the ranged workspace call with the same arguments (rpt_bf_probe_chain_sel_range_ws / _transfer_);
  (d) loop   the host loop: synchronize, read the count, rpt_bf_probe_chain_range_ws(row_sel = sel, n = count), one
             rpt_bf_insert_sel per destination.
--ws: the workspace call at 2^20 and 2^24 rows, one filter of 128 KiB or 16 MiB
  (a) ws     rpt_bf_probe_chain_sel_range_ws;
  (b) plain  rpt_bf_probe_chain_sel_ws on the same inputs;
  (d) loop   the host loop with rpt_bf_probe_chain_range_ws over the survivors.

Per-step time is device-event time around `--steps` steps enqueued back to back ((d) synchronizes once per step, as it
must), over the steps. Every shape is warmed up first (one round that is not counted); the median, minimum and maximum
over `--reps` rounds are reported. The ranged selections are compared with each other every round, and the plain call's
must hold at least as many rows. Synthetic keys only; nothing outside the repository is read. Run on a GPU box:
    python tools/bench_probe_sel_range.py --out profiles/sel_range/one_launch.jsonl
    python tools/bench_probe_sel_range.py --ws --out profiles/sel_range/workspace.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "duckdb-robust-predicate-transfer_amd"))
import rpt_amd  # noqa: E402
from rpt_amd._lib import KeyColumn, check  # noqa: E402

KIB_LOG = {128: 14, 16384: 21}
COVERS = (0.05, 0.5, 1.0)
ONE_CONFIGS = [(kib, k, n, n_dst, cover) for kib in KIB_LOG for k in (1, 3) for n in (2048, 8192, 16384)
               for n_dst in (0, 1) for cover in COVERS]
WS_CONFIGS = [(kib, 1, 1 << n_log, 0, cover) for kib in KIB_LOG for n_log in (20, 24) for cover in COVERS]
MASK = 1  # filter 0


class Pool:
    """The filters of one size, made once: 3 probed filters over the synthetic build keys and 1 outgoing filter."""

    def __init__(self, kib):
        self.log = KIB_LOG[kib]
        self.n_build = 1 << (self.log + 2)
        self.probed = []
        for _ in range(3):
            bf = rpt_amd.BloomFilter(log_num_blocks=self.log)
            bf.insert(rpt_amd.synth_build_keys(self.n_build))
            self.probed.append(bf)
        self.dst = [rpt_amd.BloomFilter(log_num_blocks=self.log)]
        for bf in self.dst:  # their first write is not the timed one
            bf.insert(rpt_amd.synth_build_keys(1024, start=1 << 40))
        torch.cuda.synchronize()

    def close(self):
        for bf in self.probed + self.dst:
            bf.close()


def spread(name, values, row):
    row[name + "_median"] = round(statistics.median(values), 3)
    row[name + "_min"] = round(min(values), 3)
    row[name + "_max"] = round(max(values), 3)


def covering_range(keys, cover):
    """(min, max) holding the middle `cover` of the given keys; everything at 1.0."""
    s = torch.sort(keys).values
    n = s.numel()
    lo = min(n - 1, int(n * (0.5 - cover / 2)))
    hi = max(lo, min(n - 1, int(n * (0.5 + cover / 2)) - 1))
    return int(s[lo].item()), int(s[hi].item())


def measure(pool, kib, k, n, n_dst, cover, reps, steps, ws_mode):
    lib = rpt_amd.load()
    filters, dsts = pool.probed[:k], pool.dst[:n_dst]
    rows = 2 * n
    cols = [rpt_amd.synth_probe_keys(rows, pool.n_build, 900, start=(j + 1) << 33) for j in range(k)]
    dcols = [rpt_amd.synth_probe_keys(rows, pool.n_build, 0, start=(j + 101) << 33) for j in range(n_dst)]
    sel = torch.sort(torch.randperm(rows, device="cuda")[:n]).values
    mm = covering_range(cols[0][sel], cover)
    filters[0].set_minmax(mm)
    sel = sel.to(torch.int32).contiguous()
    count = torch.full((1,), n, dtype=torch.int64, device="cuda")
    names = ("ws", "plain", "loop") if ws_mode else ("one", "plain", "ws", "loop")
    out = {m: (torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
           for m in names}
    ws = torch.empty(max(rpt_amd.probe_chain_sel_workspace_bytes(filters, n), 256), dtype=torch.uint8, device="cuda")
    ws_loop = torch.empty(max(rpt_amd.probe_chain_range_workspace_bytes(filters, MASK, n), 256), dtype=torch.uint8,
                          device="cuda")
    handles = (ctypes.c_void_p * k)(*[f.handle for f in filters])
    arr = (KeyColumn * k)(*[rpt_amd.make_column(c) for c in cols])
    dhandles = (ctypes.c_void_p * max(n_dst, 1))(*[f.handle for f in dsts])
    darr = (KeyColumn * max(n_dst, 1))(*[rpt_amd.make_column(c) for c in dcols])
    p_sel, p_count = sel.data_ptr(), count.data_ptr()

    def ptrs(m):
        return out[m][0].data_ptr(), out[m][1].data_ptr()

    def step_one(stream):
        o, c = ptrs("one")
        if n_dst:
            check(lib.rpt_bf_transfer_sel_range(handles, arr, k, MASK, dhandles, darr, n_dst, p_sel, p_count, n, o, c, stream))
        else:
            check(lib.rpt_bf_probe_chain_sel_range(handles, arr, k, MASK, p_sel, p_count, n, o, c, stream))

    def step_plain(stream):
        o, c = ptrs("plain")
        if ws_mode:
            check(lib.rpt_bf_probe_chain_sel_ws(handles, arr, k, p_sel, p_count, n, o, c, ws.data_ptr(), ws.numel(), stream))
        elif n_dst:
            check(lib.rpt_bf_transfer_sel(handles, arr, k, dhandles, darr, n_dst, p_sel, p_count, n, o, c, stream))
        else:
            check(lib.rpt_bf_probe_chain_sel(handles, arr, k, p_sel, p_count, n, o, c, stream))

    def step_ws(stream):
        o, c = ptrs("ws")
        if n_dst:
            check(lib.rpt_bf_transfer_sel_range_ws(handles, arr, k, MASK, dhandles, darr, n_dst, p_sel, p_count, n, o, c,
                                                   ws.data_ptr(), ws.numel(), stream))
        else:
            check(lib.rpt_bf_probe_chain_sel_range_ws(handles, arr, k, MASK, p_sel, p_count, n, o, c, ws.data_ptr(),
                                                      ws.numel(), stream))

    def step_loop(stream):
        o, c = ptrs("loop")
        torch.cuda.current_stream().synchronize()
        m = int(count.item())  # the chain takes its row count as a host argument
        check(lib.rpt_bf_probe_chain_range_ws(handles, arr, k, MASK, p_sel, m, o, c, ws_loop.data_ptr(), ws_loop.numel(),
                                              stream))
        for j in range(n_dst):
            check(lib.rpt_bf_insert_sel(dsts[j].handle, ctypes.byref(darr[j]), o, c, n, stream))

    step_of = {"one": step_one, "plain": step_plain, "ws": step_ws, "loop": step_loop}

    def timed(step):
        stream = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps  # us per step

    row = {"op": "probe_sel_range_ws" if ws_mode else "probe_sel_range_one", "max_rows": n, "filters": k,
           "filter_kib": kib, "destinations": n_dst, "range_cover": cover, "steps": steps, "reps": reps,
           "sel_strategy": filters[0].probe_sel_strategy_for(n)}
    times = {m: [] for m in names}
    for rep in range(reps + 1):  # the first round warms every kernel of the shape and is not counted
        got = {m: timed(step_of[m]) for m in names}
        if rep:
            for m, v in got.items():
                times[m].append(v)
        counts = {m: int(out[m][1].item()) for m in names}
        ranged = [m for m in names if m != "plain"]
        for m in ranged[1:]:
            assert counts[m] == counts[ranged[0]], f"counts differ: {counts} {row}"
            assert torch.equal(out[m][0][: counts[m]], out[ranged[0]][0][: counts[m]]), f"selections differ: {row}"
        assert counts["plain"] >= counts[ranged[0]], f"the plain call kept fewer rows: {counts} {row}"
    row["survivors"], row["plain_survivors"] = counts[ranged[0]], counts["plain"]
    for m, v in times.items():
        spread(m + "_us", v, row)
    first = names[0]
    for m in names[1:]:
        row["%s_over_%s" % (first, m)] = round(row[first + "_us_median"] / row[m + "_us_median"], 3)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ws", action="store_true", help="the workspace call at 2^20 and 2^24 rows (see above)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=None, help="steps per round (default: 1000; --ws: 200, 20 at 2^24 rows)")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--rows", type=int, default=None, help="only the configurations of this many positions")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_probe_sel_range needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    configs = WS_CONFIGS if args.ws else ONE_CONFIGS
    configs = configs if args.only is None else [configs[args.only]]
    configs = [c for c in configs if args.rows in (None, c[2])]
    pool, pool_kib = None, None
    for kib, k, n, n_dst, cover in configs:
        if kib != pool_kib:
            if pool is not None:
                pool.close()
            pool, pool_kib = Pool(kib), kib
        steps = args.steps or ((20 if n > 1 << 20 else 200) if args.ws else 1000)
        row = measure(pool, kib, k, n, n_dst, cover, max(1, args.reps), max(1, steps), args.ws)
        print(json.dumps(row), file=out, flush=True)
        torch.cuda.empty_cache()
    if pool is not None:
        pool.close()


if __name__ == "__main__":
    main()
