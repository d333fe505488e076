"""USE_BF's filter chain over one large HBM-resident batch, two ways, in one process, alternating:

  (a) chain_ws  one rpt_bf_probe_chain_ws call: the survivors stay on the device as result bits between the
                filters, one compaction at the end, no host round trip (timed with device events);
  (b) loop      what a caller had before: one rpt_bf_probe per filter with the previous filter's selection
                vector as row_sel, the count read back to the host in between (timed with a host clock around
                work that ends in a synchronise).

Chains of 2 and 3 filters of 128 KiB, 512 KiB and 16 MiB (the supplementary JOB sizes and C2) over int64 or int32
key columns of 2^27 rows, per-filter pass fractions 0.1 / 0.5 / 0.9 (synth_probe_keys' p_permille), the filter
order both ways round. `masked_large` repeats (a) with the 16 MiB filter forced to GATHER, so that it runs as a
masked stage instead of partitioning every row. The two methods' selection vectors are compared at the size timed.
The tool does not load the oracle (test infrastructure): tests/test_gpu_chain_ws.py checks the entry point.
Run on a GPU box:
    python tools/chain_probe_bench.py --out profiles/chain_ws/chain_probe.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/chain_probe_bench.py --only 10 --reps 1
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

KIB_LOG = {128: 14, 512: 16, 16384: 21}  # filter KiB -> log2 blocks
# (filter KiB, pass fraction) per stage, in chain order
CHAINS = [
    [(128, 0.1), (16384, 0.9)],
    [(16384, 0.9), (128, 0.1)],
    [(16384, 0.1), (128, 0.9)],
    [(128, 0.9), (16384, 0.1)],
    [(128, 0.5), (16384, 0.5)],
    [(16384, 0.5), (128, 0.5)],
    [(512, 0.1), (16384, 0.5)],
    [(16384, 0.5), (512, 0.1)],
    [(128, 0.1), (512, 0.5), (16384, 0.9)],
    [(16384, 0.9), (512, 0.5), (128, 0.1)],
    [(16384, 0.1), (512, 0.5), (128, 0.9)],
    [(128, 0.9), (512, 0.5), (16384, 0.1)],
]
CONFIGS = [(kt, chain) for kt in ("int64", "int32") for chain in CHAINS]


def as_key_type(t: torch.Tensor, key_type: str) -> torch.Tensor:
    """int32 columns: the low 31 bits of the synthetic int64 keys (a member's truncation is a member of the
    filter built from the truncated build keys)."""
    return t if key_type == "int64" else (t & 0x7FFFFFFF).to(torch.int32)


class Stage:
    """A filter of `kib` KiB holding 2^(log blocks + 3) synthetic build keys (8 bits per key, the sizing rule) and a
    probe column of n rows of which about `frac` are build keys."""

    def __init__(self, kib, frac, n, key_type, index):
        log_nb = KIB_LOG[kib]
        n_build = 1 << (log_nb + 3)
        self.kib, self.frac = kib, frac
        self.bf = rpt_amd.BloomFilter(log_num_blocks=log_nb)
        self.bf.insert(as_key_type(rpt_amd.synth_build_keys(n_build), key_type))
        self.keys = as_key_type(rpt_amd.synth_probe_keys(n, n_build, int(round(frac * 1000)), start=index * n), key_type)


def run_chain_ws(stages, n, sel, cnt, ws):
    """The call alone (rpt_amd.probe_chain_ws would read the count back inside the timed window)."""
    lib = rpt_amd.load()
    handles = (ctypes.c_void_p * len(stages))(*[s.bf.handle for s in stages])
    cols = (KeyColumn * len(stages))(*[rpt_amd.make_column(s.keys) for s in stages])
    check(lib.rpt_bf_probe_chain_ws(handles, cols, len(stages), None, n, sel.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream().cuda_stream))


def run_loop(stages, n, sels, cnt, ws):
    """rpt_bf_probe per filter over the previous survivors; returns (the buffer holding the result, its count)."""
    row_sel, m = None, n
    for i, s in enumerate(stages):
        out = sels[i & 1]
        s.bf.probe_async(s.keys, row_sel=row_sel, n=m, out_sel=out, out_count=cnt, workspace=ws)
        m = int(cnt.item())  # the next call takes n as a host argument
        row_sel = out
        if m == 0:
            break
    return row_sel, m


def measure(key_type, chain, n, reps, masked_large):
    stages = [Stage(kib, frac, n, key_type, i) for i, (kib, frac) in enumerate(chain)]
    filters = [s.bf for s in stages]
    row = {"op": "chain_probe", "n": n, "key_type": key_type, "filters_kib": [s.kib for s in stages],
           "pass_fractions": [s.frac for s in stages], "reps": reps}
    sel_a = torch.empty(n, dtype=torch.int32, device="cuda")
    sels_b = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws_b = torch.empty(max(s.bf.workspace_bytes(n) for s in stages), dtype=torch.uint8, device="cuda")
    variants = {"chain_ws": []}
    if masked_large:
        variants["chain_ws_masked_large"] = [s.bf for s in stages if s.kib >= 1024]
    ws_a = {}
    for name, forced in variants.items():
        for bf in forced:
            bf.probe_strategy = rpt_amd.RPT_PROBE_GATHER
        ws_a[name] = torch.empty(rpt_amd.probe_chain_workspace_bytes(filters, n), dtype=torch.uint8, device="cuda")
        row[name + "_strategies"] = [s.bf.probe_strategy_for(n) for s in stages]
        for bf in forced:
            bf.probe_strategy = rpt_amd.RPT_PROBE_AUTO
    times = {name: [] for name in variants}
    times["loop"] = []
    for rep in range(reps + 1):  # the first round warms every kernel and is not counted
        for name, forced in variants.items():
            for bf in forced:
                bf.probe_strategy = rpt_amd.RPT_PROBE_GATHER
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run_chain_ws(stages, n, sel_a, cnt, ws_a[name])
            e1.record()
            torch.cuda.synchronize()
            for bf in forced:
                bf.probe_strategy = rpt_amd.RPT_PROBE_AUTO
            count_a = int(cnt.item())
            if rep:
                times[name].append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            sel_b, count_b = run_loop(stages, n, sels_b, cnt, ws_b)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep:
                times["loop"].append((t1 - t0) * 1e3)
            assert count_a == count_b and torch.equal(sel_a[:count_a], sel_b[:count_b]), \
                f"{name} and the rpt_bf_probe loop disagree: {row}"
            row["survivors"] = count_a
    for name, t in times.items():
        row[name + "_ms_mean"] = round(sum(t) / len(t), 4)
        row[name + "_ms_min"] = round(min(t), 4)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-rows", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, help="index into the configurations (default: all)")
    ap.add_argument("--no-masked-large", action="store_true")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chain_probe_bench needs a GPU: nothing is measured without one")
    rpt_amd.load()
    out = sys.stdout
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")
    configs = CONFIGS if args.only is None else [CONFIGS[args.only]]
    for key_type, chain in configs:
        row = measure(key_type, chain, 1 << args.log_rows, max(1, args.reps), not args.no_masked_large)
        print(json.dumps(row), file=out, flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
