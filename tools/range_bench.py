"""The min/max range stage on an HBM-resident column, measured in one process (device events around steady-state
steps, one warm-up round; the calls of a comparison alternate round by round):

  (a) --set bits   rpt_bf_range_bits alone on FLAT int64 and int32 columns of 2^27 rows: the read rate over the
                   algorithmic bytes (the keys read once, the bitmap written once) as a fraction of what this box
                   streams (rpt_stream_read over the same column, same process). Beside it the yardstick, measured
                   the same way: rpt_bf_probe_bits on a 128 KiB filter (the whole-filter LDS probe), which streams the
                   same keys and writes the same bitmap with more work per key.
  (b) --set chain  rpt_bf_probe_chain_range_ws (the filter flagged) against rpt_bf_probe_chain_ws: the same filter, the
                   same rows. The column holds the ids 0 .. n-1, sorted (a table clustered on its key) or shuffled;
                   the filter (128 KiB or 16 MiB) is built from ids spread evenly over a contiguous interval that
                   covers 5 %, 50 % or 100 % of the column, so its min/max, folded by the insert itself, covers that
                   share. Reported: both times and their ratio (range / plain; above 1 the extra key pass costs more
                   than the dead segments save). The two selections are compared every round: the range call may only
                   drop rows of the plain result (false positives outside the interval).

Nothing is dispatched on these numbers: the caller chooses by setting the mask. The tool does not load the oracle (test
infrastructure): tests/test_gpu_range.py checks the entry points.
Run on a GPU box:
    python tools/range_bench.py --out profiles/range/range_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "duckdb-robust-predicate-transfer_amd"))
import rpt_amd  # noqa: E402
from rpt_amd._lib import KeyColumn, check  # noqa: E402

FILTER_KIB_LOG = {128: 14, 16384: 21}  # filter KiB -> log2 blocks
BITS_CONFIGS = [("bits", 27, kt) for kt in ("int64", "int32")]
CHAIN_CONFIGS = [("chain", n_log, kib, layout, cover) for n_log in (20, 24, 27) for kib in FILTER_KIB_LOG
                 for layout, cover in (("sorted", 0.05), ("sorted", 0.5), ("sorted", 1.0), ("shuffled", 0.05),
                                       ("shuffled", 0.5), ("shuffled", 1.0))]


def timed(fn, reps):
    """Device time of fn() per call: (mean, min) ms over `reps` calls, each between its own pair of events."""
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sum(ms) / len(ms), min(ms)


def measure_bits(n_log, key_type, reps):
    lib = rpt_amd.load()
    n = 1 << n_log
    dtype = torch.int64 if key_type == "int64" else torch.int32
    keys = torch.randint(-(2**30), 2**30, (n,), dtype=dtype, device="cuda")
    nbytes = n * keys.element_size()
    bits = torch.empty(n // 512 * 8, dtype=torch.int64, device="cuda")
    sh = torch.cuda.current_stream().cuda_stream
    sink = torch.empty(int(lib.rpt_stream_sink_words(0)), dtype=torch.int64, device="cuda")
    bf = rpt_amd.BloomFilter(log_num_blocks=14)  # 128 KiB: the whole-filter LDS probe
    bf.insert(torch.randint(-(2**30), 2**30, (1 << 16,), dtype=dtype, device="cuda"))
    bf.set_minmax((-(2**29), 2**29))  # half the rows pass
    ws = torch.empty(max(bf.workspace_bytes(n), 256), dtype=torch.uint8, device="cuda")
    col = rpt_amd.make_column(keys)

    def stream_read():
        check(lib.rpt_stream_read(keys.data_ptr(), nbytes, sink.data_ptr(), sh))

    def range_bits():
        check(lib.rpt_bf_range_bits(bf.handle, ctypes.byref(col), None, n, bits.data_ptr(), sh))

    def probe_bits():
        check(lib.rpt_bf_probe_bits(bf.handle, ctypes.byref(col), None, n, bits.data_ptr(), ws.data_ptr(), ws.numel(), sh))

    t = {"stream_read": [], "range_bits": [], "lds_probe_bits": []}
    for rnd in range(3):  # the first round warms every kernel and is not counted; the calls alternate
        for name, fn in (("stream_read", stream_read), ("range_bits", range_bits), ("lds_probe_bits", probe_bits)):
            r = timed(fn, reps)
            if rnd:
                t[name].append(r)
    passed = int(torch.count_nonzero(((keys >= -(2**29)) & (keys <= 2**29))).item())
    range_bits()
    torch.cuda.synchronize()
    popc = sum(bin(w & (2**64 - 1)).count("1") for w in bits[:4096].tolist())
    assert popc == int(torch.count_nonzero((keys[: 4096 * 64] >= -(2**29)) & (keys[: 4096 * 64] <= 2**29)).item())
    algo = nbytes + n // 8
    row = {"op": "range_bits", "n": n, "key_type": key_type, "reps": reps, "pass_fraction": round(passed / n, 4),
           "algorithmic_bytes": algo, "probe_strategy": bf.probe_strategy_for(n)}
    best = {name: min(m for _mean, m in rs) for name, rs in t.items()}
    mean = {name: sum(mean for mean, _m in rs) / len(rs) for name, rs in t.items()}
    read_rate = nbytes / best["stream_read"] / 1e6  # GB/s
    row["stream_read_GBps"] = round(read_rate, 1)
    for name in ("range_bits", "lds_probe_bits"):
        row[name + "_ms_min"] = round(best[name], 4)
        row[name + "_ms_mean"] = round(mean[name], 4)
        row[name + "_GBps"] = round(algo / best[name] / 1e6, 1)
        row[name + "_fraction_of_read_stream"] = round(algo / best[name] / 1e6 / read_rate, 3)
    bf.close()
    return row


def measure_chain(n_log, kib, layout, cover, reps):
    lib = rpt_amd.load()
    n = 1 << n_log
    log_nb = FILTER_KIB_LOG[kib]
    keys = torch.arange(n, dtype=torch.int64, device="cuda")
    if layout == "shuffled":
        keys = keys[torch.randperm(n, device="cuda")].contiguous()
    # the build ids: spread evenly over [lo, lo + cover * n), at most 4 per filter block
    span = max(1, int(cover * n))
    lo = (n - span) // 2
    n_build = min(span, 4 << log_nb)
    build = lo + (torch.arange(n_build, dtype=torch.float64, device="cuda") * ((span - 1) / max(1, n_build - 1))).round().to(torch.int64)
    bf = rpt_amd.BloomFilter(log_num_blocks=log_nb)
    bf.insert(build)
    mm = bf.minmax()
    assert mm == (lo, lo + span - 1), (mm, lo, span)
    sel_p, sel_r = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    cnt_p, cnt_r = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    need = max(rpt_amd.probe_chain_workspace_bytes([bf], n), rpt_amd.probe_chain_range_workspace_bytes([bf], 1, n), 256)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    handles = (ctypes.c_void_p * 1)(bf.handle)
    cols = (KeyColumn * 1)(rpt_amd.make_column(keys))
    sh = torch.cuda.current_stream().cuda_stream

    def plain():
        check(lib.rpt_bf_probe_chain_ws(handles, cols, 1, None, n, sel_p.data_ptr(), cnt_p.data_ptr(), ws.data_ptr(),
                                        ws.numel(), sh))

    def ranged():
        check(lib.rpt_bf_probe_chain_range_ws(handles, cols, 1, 1, None, n, sel_r.data_ptr(), cnt_r.data_ptr(),
                                              ws.data_ptr(), ws.numel(), sh))

    t = {"plain": [], "range": []}
    for rnd in range(3):  # the first round warms every kernel and is not counted; the two calls alternate
        for name, fn in (("plain", plain), ("range", ranged)):
            r = timed(fn, reps)
            if rnd:
                t[name].append(r)
        c_p, c_r = int(cnt_p.item()), int(cnt_r.item())
        kept = keys[sel_p[:c_p].long()]
        inside = (kept >= mm[0]) & (kept <= mm[1])
        assert c_r == int(inside.sum().item()) and torch.equal(sel_r[:c_r], sel_p[:c_p][inside]), "range result differs"
    row = {"op": "chain", "n": n, "key_type": "int64", "filter_kib": kib, "layout": layout, "range_cover": cover,
           "reps": reps, "probe_strategy": bf.probe_strategy_for(n), "survivors_plain": c_p, "survivors_range": c_r}
    for name, rs in t.items():
        row[name + "_ms_min"] = round(min(m for _mean, m in rs), 4)
        row[name + "_ms_mean"] = round(sum(mean for mean, _m in rs) / len(rs), 4)
    row["ratio_min"] = round(row["range_ms_min"] / row["plain_ms_min"], 3)
    row["ratio_mean"] = round(row["range_ms_mean"] / row["plain_ms_mean"], 3)
    bf.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="steps per round (two counted rounds after one warm-up round)")
    ap.add_argument("--set", choices=["all", "bits", "chain"], default="all")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("range_bench needs a GPU: nothing is measured without one")
    rpt_amd.load()
    torch.manual_seed(0)
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    configs = {"all": BITS_CONFIGS + CHAIN_CONFIGS, "bits": BITS_CONFIGS, "chain": CHAIN_CONFIGS}[args.set]
    configs = configs if args.only is None else [configs[args.only]]
    for cfg in configs:
        row = measure_bits(*cfg[1:], max(1, args.reps)) if cfg[0] == "bits" else measure_chain(*cfg[1:], max(1, args.reps))
        print(json.dumps(row), file=out, flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
