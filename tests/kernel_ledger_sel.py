"""The kernel ledger of csrc/rpt_probe_sel.hpp: which instantiation of probe_bits_sel_kernel each device-counted chain
must launch as its first stage (a plain module, like kernel_ledger, whose helpers and shapes it reuses; it needs
neither torch nor a GPU).

probe_bits_sel_kernel<K, MODE>: K the key type; MODE 0 the gather, 1 the whole filter in LDS (<= 2^14 blocks), 2 the
hybrid (the first 128 KiB in LDS, the rest from L2). The row mapping is always the general one (a selection vector), so
there is no DENSE argument. Every row's call is rpt_bf_probe_chain_sel_ws over two filters with max_rows = N_SMALL:
its instantiation once, then the shared tail: one masked later stage (the int64 whole-filter LDS twin, over a
dictionary column) and the selection-vector tail, all recorded by csrc/rpt_gpu.hip, where they have rows of their own.
The demotion rows force a routed strategy on the first or on the later stage: the gather runs in its place, and no
partition or bucket kernel.

tests/test_gpu_kernel_ledger_sel.py runs every row on the GPU; tests/test_kernel_ledger_sel_names.py checks without one
that the header records no kernel this table lacks."""
from __future__ import annotations

import itertools
import os

import kernel_ledger as kl

SEL_SOURCE = os.path.join(kl.CSRC, "rpt_probe_sel.hpp")
BASE = "probe_bits_sel_kernel"
MODE_GATHER, MODE_LDS, MODE_HYBRID = 0, 1, 2
# what -> (MODE, log2 blocks of the first filter, its forced strategy)
MODES = {"gather": (MODE_GATHER, kl.LOG_GATHER, kl.GATHER), "lds": (MODE_LDS, kl.LOG_LDS, kl.LDS),
         "hybrid": (MODE_HYBRID, kl.LOG_HYBRID, kl.LDS)}
LOG_LATER = 11  # the later stage's filter: whole-filter LDS under AUTO
LATER_STAGE = kl.inst("probe_bits_masked_kernel", kl.KEYS["i64"], False, True, kl.LDS_THREADS)
TAIL = (LATER_STAGE,) + kl.SEL_TAIL  # recorded by csrc/rpt_gpu.hip; rows of their own there
N = kl.N_SMALL


def sel_name(k: int, mode: int) -> str:
    return kl.inst(BASE, k, mode)


def masked_gather_name(k: int) -> str:
    return kl.inst("probe_bits_masked_kernel", k, False, False, kl.BLOCK_THREADS)


def build_rows():
    rows = []
    kinds = itertools.cycle((kl.DENSE, kl.DICT, kl.MISALIGNED))  # the column under the selection vector

    def add(what, kernels, **args):
        rows.append(kl.Row("chain_sel-%s-%s-%s" % (what, args["kt"], args["dkind"]), "chain_sel", dict(args, what=what),
                           kernels))

    for what, (mode, log_nb, strategy) in MODES.items():
        for kt, k in kl.KEYS.items():
            add(what, kl.once(sel_name(k, mode), *TAIL), kt=kt, dkind=next(kinds), log_nb=log_nb, strategy=strategy,
                later_strategy=kl.AUTO, later_log_nb=LOG_LATER, n=N)
    # demotions: a first stage forced to PARTITIONED runs the gather instantiation ...
    add("demoted_first", kl.once(sel_name(kl.KEYS["i64"], MODE_GATHER), *TAIL), kt="i64", dkind=next(kinds),
        log_nb=kl.LOG_GATHER, strategy=kl.PARTITIONED, later_strategy=kl.AUTO, later_log_nb=LOG_LATER, n=N)
    # ... and a later stage forced to PARTITIONED the masked gather (over the later stage's int64 dictionary column)
    add("demoted_later", kl.once(sel_name(kl.KEYS["i32"], MODE_LDS), masked_gather_name(kl.KEYS["i64"]), *kl.SEL_TAIL),
        kt="i32", dkind=next(kinds), log_nb=kl.LOG_LDS, strategy=kl.LDS, later_strategy=kl.PARTITIONED,
        later_log_nb=kl.LOG_GATHER, n=N)
    return rows


ROWS = build_rows()
DEMOTION_ROWS = [r for r in ROWS if r.args["what"].startswith("demoted")]


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launchers of rpt_probe_sel.hpp can produce in the product build."""
    return [sel_name(k, mode) for k in kl.KEYS.values() for mode in (MODE_GATHER, MODE_LDS, MODE_HYBRID)]
