"""Composite join keys hashed inside the kernels against the two-pass route, in one process, alternating. The protocol
is that of tools/bench_transfer_small.py. The baseline is always the hash passes of the same library: rpt_hash_keys on
column 0 and one rpt_hash_combine per further column, which leave an 8-byte hash column in device memory, then the
existing single-column call on that column as RPT_KEY_HASH.

Per vector (default): n rows (2048, 8192 or 16384; row_sel null) through 1 or 3 filters (all 128 KiB or all 16 MiB) with
keys of 2 or 3 int64 columns each, about 0.1, 0.5 or 0.9 of the rows surviving the chain:
  chain     rpt_bf_probe_chain_composite (one launch) against the passes + rpt_bf_probe_chain;
  transfer  rpt_bf_transfer_composite into one destination with a two-column key (one launch) against the passes (the
            destination key's too) + rpt_bf_transfer.
Every side is timed enqueued eagerly and replayed from a graph of one step.
Large (--large): 2^20, 2^24 or 2^27 rows, keys of 2 or 3 BIGINT or INTEGER columns:
  hash      rpt_hash_keys_composite against the passes; the bytes each side moves per second are reported (fused: every
            column once and the hash once; passes: pass 1 reads the column and writes the hash, every later pass reads
            the column and the hash and writes the hash) beside this box's stream rates, measured here as bench.py
            measures them (rpt_stream_read / rpt_stream_copy);
  insert    rpt_bf_insert_composite against the passes + rpt_bf_insert of the HASH column, into a 128 KiB and a 16 MiB
            filter.
Per-step time is device-event time around `--steps` steps enqueued back to back on a warmed device (fewer for the
large shapes: at least 2); the median, minimum and maximum over `--reps` rounds are reported after a round that is not
counted. Both sides' outputs are compared after the rounds. Synthetic keys only; nothing outside the repository is
read. Run on a GPU box:
    python tools/bench_composite.py --out profiles/composite/per_vector.jsonl
    python tools/bench_composite.py --large --out profiles/composite/large.jsonl
--rows / --only keep a part of the configurations."""
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
from rpt_amd._lib import CompositeKey, KeyColumn, check  # noqa: E402

ROWS = (2048, 8192, 16384)
CHAINS = (1, 3)
COLUMNS = (2, 3)
KIB_LOG = {128: 14, 16384: 21}
FRACTIONS = (0.1, 0.5, 0.9)
CONFIGS = [(kib, k, c, n, frac) for kib in KIB_LOG for k in CHAINS for c in COLUMNS for n in ROWS for frac in FRACTIONS]
LARGE_ROWS = (1 << 20, 1 << 24, 1 << 27)
DTYPES = {"i64": torch.int64, "i32": torch.int32}
LARGE_CONFIGS = [(n, c, kt) for n in LARGE_ROWS for c in COLUMNS for kt in DTYPES]
STREAM_BYTES = 2 << 30


def spread(name, values, row):
    row[name + "_median"] = round(statistics.median(values), 5)
    row[name + "_min"] = round(min(values), 5)
    row[name + "_max"] = round(max(values), 5)


def verdict(row, a, b):
    """Which side is ahead: only where its median lies outside the other side's min-max spread of the same run."""
    if row[a + "_median"] < row[b + "_min"] and row[b + "_median"] > row[a + "_max"]:
        return a
    if row[b + "_median"] < row[a + "_min"] and row[a + "_median"] > row[b + "_max"]:
        return b
    return "level"


def timed(steps, step, stream):
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


def rounds(reps, steps, eager, graphs=None):
    """{name: [us per step of every counted round]}; the sides alternate within a round."""
    graphs = graphs or {}
    times = {name: [] for name in list(eager) + list(graphs)}
    stream = torch.cuda.current_stream().cuda_stream
    for rep in range(reps + 1):  # the first round warms up and is not counted
        got = {name: timed(steps, step, stream) for name, step in eager.items()}
        for name, graph in graphs.items():
            got[name] = timed(steps, lambda _s, g=graph: g.replay(), stream)
        if rep:
            for name, v in got.items():
                times[name].append(v)
    return times


def rand_cols(n, c, dtype, gen):
    info = torch.iinfo(dtype)
    return [torch.randint(info.min, info.max, (n,), dtype=dtype, device="cuda", generator=gen) for _ in range(c)]


def key_of(cols):
    arr = (KeyColumn * len(cols))(*[rpt_amd.make_column(t) for t in cols])
    return CompositeKey(arr, len(cols)), arr


def hash_passes(lib, cols, colarr, n, out, stream):
    check(lib.rpt_hash_keys(ctypes.byref(colarr[0]), n, out.data_ptr(), stream))
    for j in range(1, len(cols)):
        check(lib.rpt_hash_combine(ctypes.byref(colarr[j]), n, out.data_ptr(), stream))


def reset(filters):
    for bf in filters:
        bf.clear()
        bf.settle()
    torch.cuda.synchronize()


# ---- per vector -----------------------------------------------------------------------------------------------------
def measure(kib, k, c, n, frac, reps, steps, gen):
    lib = rpt_amd.load()
    log = KIB_LOG[kib]
    share = frac ** (1.0 / k)  # per filter, so that about `frac` survive the chain
    cols = [rand_cols(n, c, torch.int64, gen) for _ in range(k)]
    dcols = rand_cols(n, 2, torch.int64, gen)
    filters = []
    for j in range(k):  # each filter holds about `share` of the vector's keys among 4 random hashes per block
        bf = rpt_amd.BloomFilter(log_num_blocks=log)
        h = rpt_amd.hash_columns(cols[j])
        member = torch.rand(n, device="cuda", generator=gen) < share
        bf.insert(h[member].contiguous(), key_type=rpt_amd.RPT_KEY_HASH, strategy=rpt_amd.RPT_INSERT_ATOMIC)
        bf.insert(rand_cols(4 << log, 1, torch.int64, gen)[0], key_type=rpt_amd.RPT_KEY_HASH)
        filters.append(bf)
    dst = {m: rpt_amd.BloomFilter(log_num_blocks=log) for m in ("fused", "passes")}
    for bf in dst.values():  # their first write is not the timed one
        bf.insert(rpt_amd.synth_build_keys(1024, start=1 << 40))
    handles = (ctypes.c_void_p * k)(*[f.handle for f in filters])
    keys = [key_of(cs) for cs in cols]
    karr = (CompositeKey * k)(*[kk for kk, _a in keys])
    dkey, dcolarr = key_of(dcols)
    dkarr = (CompositeKey * 1)(dkey)
    dh = {m: (ctypes.c_void_p * 1)(bf.handle) for m, bf in dst.items()}
    hashes = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(k + 1)]
    harr = (KeyColumn * (k + 1))(*[rpt_amd.make_column(h, key_type=rpt_amd.RPT_KEY_HASH) for h in hashes])
    out = {m: (torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
           for m in ("fused", "passes")}

    def passes(stream, with_dst):
        for j in range(k):
            hash_passes(lib, cols[j], keys[j][1], n, hashes[j], stream)
        if with_dst:
            hash_passes(lib, dcols, dcolarr, n, hashes[k], stream)

    def chain_fused(stream):
        check(lib.rpt_bf_probe_chain_composite(handles, karr, k, None, n, out["fused"][0].data_ptr(),
                                               out["fused"][1].data_ptr(), stream))

    def chain_passes(stream):
        passes(stream, False)
        check(lib.rpt_bf_probe_chain(handles, harr, k, None, n, out["passes"][0].data_ptr(), out["passes"][1].data_ptr(), stream))

    def transfer_fused(stream):
        check(lib.rpt_bf_transfer_composite(handles, karr, k, dh["fused"], dkarr, 1, None, n, out["fused"][0].data_ptr(),
                                            out["fused"][1].data_ptr(), stream))

    def transfer_passes(stream):
        passes(stream, True)
        check(lib.rpt_bf_transfer(handles, harr, k, dh["passes"], ctypes.byref(harr[k]), 1, None, n,
                                  out["passes"][0].data_ptr(), out["passes"][1].data_ptr(), stream))

    rows = []
    for op, fused, two_pass, launches in (("chain", chain_fused, chain_passes, k * c + 1),
                                          ("transfer", transfer_fused, transfer_passes, k * c + 2 + 1)):
        row = {"op": op + "_composite", "rows": n, "filters": k, "columns": c, "filter_kib": kib, "survivor_fraction": frac,
               "passes_launches": launches, "steps": steps, "reps": reps}
        reset(dst.values())
        for step in (fused, two_pass):  # every kernel once outside any capture
            step(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        graphs = {"fused_graph_us": captured(fused), "passes_graph_us": captured(two_pass)}
        times = rounds(reps, steps, {"fused_us": fused, "passes_us": two_pass}, graphs)
        counts = {m: int(out[m][1].item()) for m in out}
        assert counts["fused"] == counts["passes"], f"counts differ: {counts} {row}"
        assert torch.equal(out["fused"][0][: counts["fused"]], out["passes"][0][: counts["passes"]]), f"selections differ: {row}"
        if op == "transfer":
            assert np.array_equal(dst["fused"].export_words(), dst["passes"].export_words()), f"destinations differ: {row}"
        row["survivors"] = counts["fused"]
        for name, v in times.items():
            spread(name, v, row)
        row["passes_over_fused"] = round(row["passes_us_median"] / row["fused_us_median"], 3)
        row["passes_graph_over_fused_graph"] = round(row["passes_graph_us_median"] / row["fused_graph_us_median"], 3)
        row["ahead"] = verdict(row, "fused_us", "passes_us")
        row["ahead_graph"] = verdict(row, "fused_graph_us", "passes_graph_us")
        rows.append(row)
        del graphs
    for bf in filters + list(dst.values()):
        bf.close()
    return rows


# ---- large ----------------------------------------------------------------------------------------------------------
def stream_rates():
    """This box's read and copy stream rates, as bench.py's stream_calibration measures them (over 2 GiB here)."""
    lib = rpt_amd.load()
    buf = torch.empty(STREAM_BYTES, dtype=torch.uint8, device="cuda")
    buf.fill_(0x5A)
    sink = torch.empty(int(lib.rpt_stream_sink_words(0)), dtype=torch.int64, device="cuda")
    half = STREAM_BYTES // 2
    read = lambda s: check(lib.rpt_stream_read(buf.data_ptr(), STREAM_BYTES, sink.data_ptr(), s))  # noqa: E731
    copy = lambda s: check(lib.rpt_stream_copy(buf.data_ptr() + half, buf.data_ptr(), half, s))  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    best = {}
    for name, fn in (("read", read), ("copy", copy)):
        fn(stream)
        best[name] = min(timed(1, fn, stream) for _ in range(5))
    return {"op": "stream", "bytes": STREAM_BYTES, "read_GBps": round(STREAM_BYTES / best["read"] / 1e3, 1),
            "copy_GBps": round(2 * half / best["copy"] / 1e3, 1)}


def measure_large(n, c, kt, reps, steps, gen):
    lib = rpt_amd.load()
    steps = max(2, steps * (1 << 20) // n)
    cols = rand_cols(n, c, DTYPES[kt], gen)
    key, colarr = key_of(cols)
    width = cols[0].element_size()
    out = {m: torch.empty(n, dtype=torch.int64, device="cuda") for m in ("fused", "passes")}

    def hash_fused(stream):
        check(lib.rpt_hash_keys_composite(ctypes.byref(key), n, out["fused"].data_ptr(), stream))

    def hash_two_pass(stream):
        hash_passes(lib, cols, colarr, n, out["passes"], stream)

    row = {"op": "hash_composite", "rows": n, "columns": c, "key_type": kt, "steps": steps, "reps": reps}
    for step in (hash_fused, hash_two_pass):
        step(torch.cuda.current_stream().cuda_stream)
    times = rounds(reps, steps, {"fused_us": hash_fused, "passes_us": hash_two_pass})
    assert torch.equal(out["fused"], out["passes"]), f"hashes differ: {row}"
    for name, v in times.items():
        spread(name, v, row)
    moved = {"fused": n * (c * width + 8), "passes": n * (width + 8 + (c - 1) * (width + 16))}
    row["fused_bytes_per_row"], row["passes_bytes_per_row"] = moved["fused"] // n, moved["passes"] // n
    row["fused_GBps"] = round(moved["fused"] / row["fused_us_median"] / 1e3, 1)
    row["passes_GBps"] = round(moved["passes"] / row["passes_us_median"] / 1e3, 1)
    row["passes_over_fused"] = round(row["passes_us_median"] / row["fused_us_median"], 3)
    row["ahead"] = verdict(row, "fused_us", "passes_us")
    rows = [row]
    harr = rpt_amd.make_column(out["passes"], key_type=rpt_amd.RPT_KEY_HASH)
    for kib, log in KIB_LOG.items():
        dst = {m: rpt_amd.BloomFilter(log_num_blocks=log) for m in ("fused", "passes")}
        for bf in dst.values():  # the atomic insert on both sides, whatever n
            check(lib.rpt_bf_set_insert_strategy(bf.handle, rpt_amd.RPT_INSERT_ATOMIC))
            bf.insert(rpt_amd.synth_build_keys(1024, start=1 << 40))

        def insert_fused(stream):
            check(lib.rpt_bf_insert_composite(dst["fused"].handle, ctypes.byref(key), n, stream))

        def insert_two_pass(stream):
            hash_passes(lib, cols, colarr, n, out["passes"], stream)
            check(lib.rpt_bf_insert(dst["passes"].handle, ctypes.byref(harr), n, stream))

        row = {"op": "insert_composite", "rows": n, "columns": c, "key_type": kt, "filter_kib": kib, "steps": steps, "reps": reps}
        reset(dst.values())
        for step in (insert_fused, insert_two_pass):
            step(torch.cuda.current_stream().cuda_stream)
        times = rounds(reps, steps, {"fused_us": insert_fused, "passes_us": insert_two_pass})
        assert np.array_equal(dst["fused"].export_words(), dst["passes"].export_words()), f"filters differ: {row}"
        for name, v in times.items():
            spread(name, v, row)
        row["passes_over_fused"] = round(row["passes_us_median"] / row["fused_us_median"], 3)
        row["ahead"] = verdict(row, "fused_us", "passes_us")
        rows.append(row)
        for bf in dst.values():
            bf.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="steps per round (--large: per round at 2^20 rows)")
    ap.add_argument("--large", action="store_true", help="rpt_hash_keys_composite and rpt_bf_insert_composite")
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--rows", type=int, default=None, help="only the configurations of this many rows")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_composite needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    reps, steps = max(1, args.reps), max(1, args.steps)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    all_configs = LARGE_CONFIGS if args.large else CONFIGS
    configs = all_configs if args.only is None else [all_configs[args.only]]
    configs = [c for c in configs if args.rows in (None, c[0] if args.large else c[3])]
    if args.large:
        print(json.dumps(stream_rates()), file=out, flush=True)
    for c in configs:
        for row in (measure_large(*c, reps, steps, gen) if args.large else measure(*c, reps, steps, gen)):
            print(json.dumps(row), file=out, flush=True)


if __name__ == "__main__":
    main()
