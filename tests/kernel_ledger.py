"""The kernel ledger: which kernel instantiation each small call through the C-ABI must launch (imported as a plain
module, like buf_util; not a conftest, and it needs neither torch nor a GPU).

librpt_gpu.so picks one of about 110 kernel instantiations at run time (dispatch_kd, launch_partition_tm,
launch_probe_bits_lds_t, launch_bucket_scatter_t and the strategy resolvers in csrc/rpt_gpu.hip) and records every
launch under its instantiation name (rpt_profiling_*: "partition_kernel<0,true,false,1,0>"). ROWS lists one small
call per instantiation the product build can reach, with the exact set of names, and launches of each, the call must
leave in that record. tests/test_gpu_kernel_ledger.py runs every row on the GPU (result bit-exact against the oracle,
kernels exactly the expected set); tests/test_kernel_ledger_names.py checks without a GPU that no kernel of
csrc/rpt_gpu.hip is missing from the table.

A pull request that adds a kernel, or reroutes a shape to another one, adds or moves a row here (or adds an EXEMPT
line with its reason)."""
from __future__ import annotations

import collections
import itertools
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "duckdb-robust-predicate-transfer_amd", "csrc")
HOST_SOURCE = os.path.join(CSRC, "rpt_gpu.hip")

NAME_BYTES = 48  # rpt_kernel_stat::name; a longer name is cut silently


def header_constant(name: str) -> int:
    """The value of `constexpr <type> name = <integer>;` (or an enumerator `name = <integer>`) in the kernel headers."""
    for path in (os.path.join(CSRC, "kernels", "common.hpp"), os.path.join(CSRC, "rpt_bloom_device.hpp")):
        with open(path) as f:
            m = re.search(r"\b%s\s*=\s*(\d+)\s*[;,}]" % re.escape(name), f.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


# ---- template arguments ------------------------------------------------------------------------------------------
KEYS = {kt: header_constant(c) for kt, c in (("i64", "kKeyI64"), ("i32", "kKeyI32"), ("hash", "kKeyHash"))}
KEY_SPLIT = header_constant("kKeySplit")  # the bucketed strategies' level-2 hash array (internal)
BLOCK_THREADS = header_constant("kBlockThreads")  # the direct (gather) probes' workgroup
LDS_THREADS = header_constant("kLdsProbeThreads")  # the whole-filter LDS probes' workgroup

# Row mappings. "dense": no row_sel, no key_sel, keys 16-byte aligned (dense_ok); the other three are the ways a call
# reaches the general mapping.
DENSE, DICT, ROW_SEL, MISALIGNED = "dense", "dict", "row_sel", "misaligned"
GENERAL = (DICT, ROW_SEL, MISALIGNED)

# Shapes (the smallest that still reach the variants)
N_TILES = 3 * 16384 + 5  # three full 16 Ki-row tiles and a 5-row tail; a full and a partial tile at tile multiple 2
N_SMALL = 513            # the fused small-batch kernels: one full 512-row segment and a one-row tail
# partition_kernel's (tile multiple, <= 4-slice variant) by filter size (log2 blocks): <= 4 slices, 16 slices, 256
PARTITION_SHAPES = {16: (1, 4), 18: (1, 0), 22: (2, 0)}
LOG_BUCKETED = 22  # the smallest filter the bucketed strategies route (and the largest the ledger uses: 32 MiB)
LOG_LDS, LOG_HYBRID, LOG_GATHER = 13, 16, 16

AUTO, GATHER, LDS, PARTITIONED, BUCKETED = 0, 1, 2, 3, 4  # rpt_probe_strategy
INS_ATOMIC, INS_PARTITIONED, INS_BUCKETED = 1, 2, 3  # rpt_insert_strategy


def targ(v) -> str:
    """A template argument as recorded_name<> (csrc/rpt_launch.hpp) spells it."""
    return ("true" if v else "false") if isinstance(v, bool) else str(int(v))


def inst(base: str, *args) -> str:
    return base + "<" + ",".join(targ(a) for a in args) + ">" if args else base


def kd_product(base: str, *extra):
    """Every name of a K x D dispatch (dispatch_kd): base<K,D,extra...>."""
    return [inst(base, k, d, *extra) for k in KEYS.values() for d in (True, False)]


# ---- kernel sets of the pipelines ----------------------------------------------------------------------------------
SEL_TAIL = ("group_sum_kernel", "group_scan_kernel", "compact_kernel")  # result bits -> selection vector
FUSED_SEL_TAIL = ("tile_count_kernel", "tile_block_scan_kernel", "group_scan_kernel")  # + unpermute_sel_kernel<TM>


def once(*names) -> dict:
    out = collections.Counter(names)
    return dict(out)


def partition_name(k: int, dense: bool, minmax: bool, log_nb: int) -> str:
    tm, sp = PARTITION_SHAPES[log_nb]
    return inst("partition_kernel", k, dense, minmax, tm, sp)


LEVEL2_PARTITION = inst("partition_kernel", KEY_SPLIT, True, False, 1, 0)


def carries_minmax(kt: str) -> bool:
    return kt != "hash"  # KeyTraits<K>::kValues: HASH columns carry no key values


Row = collections.namedtuple("Row", "id op args kernels")
# id       the pytest id
# op       the call, a function of tests/test_gpu_kernel_ledger.py (OPS)
# args     its arguments: kt (key type), dkind (row mapping), log_nb, strategy, n, ...
# kernels  {profiling name: launches} the call must leave in the record, nothing else


def _general_kinds(allowed):
    """An endless rotation over the general mappings a call supports, so each is used about equally often."""
    return itertools.cycle([g for g in GENERAL if g in allowed])


def build_rows():
    rows = []
    with_row_sel = _general_kinds(GENERAL)
    without_row_sel = _general_kinds((DICT, MISALIGNED))

    def add(op, kernels, **args):
        tag = "-".join(str(args[k]) for k in ("what", "kt", "dkind", "log_nb") if k in args)
        rows.append(Row("%s-%s" % (op, tag) if tag else op, op, args, kernels))

    def kd(rotation):
        for kt in KEYS:
            for dense in (True, False):
                yield kt, KEYS[kt], dense, (DENSE if dense else next(rotation))

    # rpt_bf_find_bits: the gather probe alone
    for kt, k, dense, dkind in kd(without_row_sel):
        add("find_bits", once(inst("probe_bits_kernel", k, dense, False, BLOCK_THREADS)), kt=kt, dkind=dkind,
            log_nb=LOG_GATHER, n=N_TILES)
    # rpt_bf_probe, direct strategies: the probe and the selection-vector tail
    for what, strategy, log_nb in (("gather", GATHER, LOG_GATHER), ("lds", LDS, LOG_LDS), ("hybrid", LDS, LOG_HYBRID)):
        for kt, k, dense, dkind in kd(with_row_sel):
            probe = {"gather": inst("probe_bits_kernel", k, dense, False, BLOCK_THREADS),
                     "lds": inst("probe_bits_kernel", k, dense, True, LDS_THREADS),
                     "hybrid": inst("probe_bits_hybrid_kernel", k, dense)}[what]
            add("probe", once(probe, *SEL_TAIL), what=what, kt=kt, dkind=dkind, log_nb=log_nb, strategy=strategy,
                n=N_TILES)
    # rpt_bf_probe, AUTO at a small batch: one fused kernel
    for kt, k, dense, dkind in kd(with_row_sel):
        add("probe", once(inst("probe_small_kernel", k, dense)), what="small", kt=kt, dkind=dkind, log_nb=LOG_GATHER,
            strategy=AUTO, n=N_SMALL)
    # rpt_bf_probe, PARTITIONED: partition (no min/max) -> run table -> slice probe -> fused selection-vector tail
    for log_nb, (tm, _sp) in PARTITION_SHAPES.items():
        for kt, k, dense, dkind in kd(with_row_sel):
            add("probe", once(partition_name(k, dense, False, log_nb), "runs_transpose_kernel", "slice_probe_kernel",
                              *FUSED_SEL_TAIL, inst("unpermute_sel_kernel", tm)),
                what="partitioned", kt=kt, dkind=dkind, log_nb=log_nb, strategy=PARTITIONED, n=N_TILES)
    # rpt_bf_probe_bits, PARTITIONED: the pipeline ends in the result bits (unpermute_kernel<TM>)
    for log_nb in (18, 22):
        tm = PARTITION_SHAPES[log_nb][0]
        add("probe_bits", once(partition_name(KEYS["i64"], True, False, log_nb), "runs_transpose_kernel",
                               "slice_probe_kernel", inst("unpermute_kernel", tm)),
            what="partitioned", kt="i64", dkind=DENSE, log_nb=log_nb, strategy=PARTITIONED, n=N_TILES)
    # rpt_bf_probe, BUCKETED: level 1 (scatter, lists), level 2 over the hash array, both unpermutes, the tail
    for kt, k, dense, dkind in kd(with_row_sel):
        add("probe", once(inst("bucket_scatter_kernel", k, dense, False), "bucket_lists_kernel", LEVEL2_PARTITION,
                          "runs_transpose_kernel", "slice_probe_kernel", inst("unpermute_kernel", 1),
                          "bucket_unpermute_kernel", *SEL_TAIL),
            what="bucketed", kt=kt, dkind=dkind, log_nb=LOG_BUCKETED, strategy=BUCKETED, n=N_TILES)
    # rpt_bf_probe_chain: the one-launch chain
    add("chain_small", once("probe_chain_small_kernel"), n=N_SMALL)
    # rpt_bf_probe_chain_ws: stage 0 a forced gather over a dense int64 column (general once the call has a row_sel),
    # stage 1 the masked twin of each direct probe, then the tail once
    for what, strategy, log_nb in (("gather", GATHER, LOG_GATHER), ("lds", LDS, LOG_LDS), ("hybrid", LDS, LOG_HYBRID)):
        for kt, k, dense, dkind in kd(with_row_sel):
            masked = {"gather": inst("probe_bits_masked_kernel", k, dense, False, BLOCK_THREADS),
                      "lds": inst("probe_bits_masked_kernel", k, dense, True, LDS_THREADS),
                      "hybrid": inst("probe_bits_masked_hybrid_kernel", k, dense)}[what]
            stage0 = inst("probe_bits_kernel", KEYS["i64"], dkind != ROW_SEL, False, BLOCK_THREADS)
            add("chain_ws", once(stage0, masked, *SEL_TAIL), what=what, kt=kt, dkind=dkind, log_nb=log_nb,
                strategy=strategy, n=N_TILES)
    # ... and a PARTITIONED later stage: its whole phase 1 into temporary bits, then the AND + recount
    add("chain_ws", once(inst("probe_bits_kernel", KEYS["i64"], True, False, BLOCK_THREADS),
                         partition_name(KEYS["i64"], True, False, 18), "runs_transpose_kernel", "slice_probe_kernel",
                         inst("unpermute_kernel", 1), "bits_and_count_kernel", *SEL_TAIL),
        what="partitioned", kt="i64", dkind=DENSE, log_nb=18, strategy=PARTITIONED, n=N_TILES)
    # rpt_bf_insert: one atomic OR per key
    for kt, k, dense, dkind in kd(without_row_sel):
        add("insert", once(inst("insert_kernel", k, dense)), what="atomic", kt=kt, dkind=dkind, log_nb=LOG_GATHER,
            strategy=INS_ATOMIC, n=N_TILES)
    # rpt_bf_insert_ws, PARTITIONED: the partition folds the min/max of I64 / I32 keys (HASH columns carry none)
    for log_nb in PARTITION_SHAPES:
        for kt, k, dense, dkind in kd(without_row_sel):
            add("insert", once(partition_name(k, dense, carries_minmax(kt), log_nb), "runs_transpose_kernel",
                               "slice_insert_kernel"),
                what="partitioned", kt=kt, dkind=dkind, log_nb=log_nb, strategy=INS_PARTITIONED, n=N_TILES)
    # rpt_bf_insert_ws, BUCKETED: the scatter folds the min/max; level 2 partitions the hash array
    for kt, k, dense, dkind in kd(without_row_sel):
        add("insert", once(inst("bucket_scatter_kernel", k, dense, carries_minmax(kt)), "bucket_lists_kernel",
                           LEVEL2_PARTITION, "runs_transpose_kernel", "slice_insert_kernel"),
            what="bucketed", kt=kt, dkind=dkind, log_nb=LOG_BUCKETED, strategy=INS_BUCKETED, n=N_TILES)
    # the inserts whose rows are chosen on the device
    for kt, k, dense, dkind in kd(with_row_sel):
        add("insert_bits", once(inst("insert_bits_kernel", k, dense)), kt=kt, dkind=dkind, log_nb=LOG_GATHER, n=N_TILES)
    for kt, k in KEYS.items():
        add("insert_sel", once(inst("insert_sel_kernel", k)), kt=kt, dkind=DENSE, log_nb=LOG_GATHER, n=N_TILES)
    # hashing
    for kt, k in KEYS.items():
        for combine in (False, True):
            add("hash", once(inst("hash_kernel", k, combine)), what="combine" if combine else "keys", kt=kt,
                dkind=DENSE, combine=combine, n=N_TILES)
    add("widen", once("widen_keys_kernel"))
    # OR merges
    add("merge_or", once("or_slices_kernel"), log_nb=LOG_GATHER)
    add("words_or", once("or_slices_kernel"), n_words=4097)
    add("words_or_slices", once("or_slices_kernel"), n_words=4098, k=3)
    # rpt_bf_fold launches once per round of folds; the GPU test counts the rounds on the oracle's words
    add("fold", {"or_slices_kernel(fold)": None}, log_nb=LOG_LDS)
    # workload generators
    add("synth_build", once("synth_build_kernel"), n=N_TILES)
    add("synth_probe", once("synth_probe_kernel"), n=N_TILES)
    return rows


ROWS = build_rows()

# Kernels no ledger row launches, one reason per line.
EXEMPT = {
    "or_slices_kernel(allreduce)": "the multi-GPU merge's OR: needs a communicator (tests/loopback runs it in the test-hook build)",
    "stream_read_kernel": "calibration only (bench.py's stream rates); computes nothing the oracle restates",
    "stream_copy_kernel": "calibration only (bench.py's stream rates); computes nothing the oracle restates",
}
# Kernels the host can record but a product build must never launch: none (every recorded kernel has a row above
# or an exemption)
NEVER_LAUNCHED = ()


def base_name(name: str) -> str:
    """'partition_kernel<0,true,false,1,0>' -> 'partition_kernel'; names without arguments are their own base."""
    return name.split("<", 1)[0]


def expected_names(rows=None) -> set:
    return {name for r in (ROWS if rows is None else rows) for name in r.kernels}


def source_base_names(path: str = HOST_SOURCE) -> set:
    """The base name of every kernel the host runtime can record: the name literal of every launch_kernel<...>() call
    in csrc/rpt_gpu.hip (csrc/rpt_launch.hpp) that is kRecorded; a kUnrecorded call contributes no name."""
    with open(path) as f:
        src = f.read()
    calls = re.findall(r"\blaunch_kernel\s*<[^;\"]*?>\s*\(\s*\"([^\"]+)\"\s*,\s*(kRecorded|kUnrecorded)\b", src, re.S)
    # every launch_kernel call of the source was understood (a new spelling must not slip through unseen)
    if len(calls) != len(re.findall(r"\blaunch_kernel\s*<", src)):
        raise AssertionError("a launch_kernel call in %s is spelled in a way source_base_names() does not parse" % path)
    return {base_name(name) for name, flag in calls if flag == "kRecorded"}


def kernel_set_problems(expected: dict, observed: dict) -> list:
    """Compare what a call should have launched, {name: launches or None (any count >= 1)}, with what
    rpt_profiling_read returned, {name: (launches, total_ms)}: a list of findings, empty when they agree."""
    problems = []
    for name in sorted(set(expected) - set(observed)):
        problems.append("missing: %s did not run" % name)
    for name in sorted(set(observed) - set(expected)):
        problems.append("extra: %s ran (%d launches)" % (name, observed[name][0]))
    for name in sorted(set(expected) & set(observed)):
        want, got = expected[name], observed[name][0]
        if got < 1 or (want is not None and got != want):
            problems.append("count: %s launched %d times, expected %s" % (name, got, want if want is not None else ">= 1"))
    return problems
