"""The kernel ledger of csrc/rpt_transfer_small.hpp: the one-launch row-list transfer and the multi-filter sink of one
vector (a plain module, like kernel_ledger, whose helpers and shapes it reuses; it needs neither torch nor a GPU).

transfer_small_kernel<RANGED, PROBED>: <false,true> for rpt_bf_transfer (and rpt_bf_transfer_range with a zero mask),
<true,true> for rpt_bf_transfer_range, <false,false> for rpt_bf_insert_multi. The key type and the column kind are
run-time branches of the one kernel, so there is one row per column kind and per row mapping (row_sel null or given) for
each instantiation, the key types rotating over them. Every row's call runs n = N_SMALL rows: the transfers over two
probed filters into one destination, the sink into two destinations. Each must leave exactly one launch of its one name
in the record: no probe_chain_small_kernel, no insert_sel_kernel or insert_kernel, no selection-vector tail.

tests/test_gpu_kernel_ledger_transfer_small.py runs every row on the GPU;
tests/test_kernel_ledger_transfer_small_names.py checks without one that the header records no kernel this table
lacks."""
from __future__ import annotations

import itertools
import os

import kernel_ledger as kl

TRANSFER_SMALL_SOURCE = os.path.join(kl.CSRC, "rpt_transfer_small.hpp")
BASE = "transfer_small_kernel"
KINDS = (kl.DENSE, kl.DICT, kl.MISALIGNED)  # the column (under the row list, where one is given)
LOG_LATER = 11  # the second probed filter of every transfer row
N = kl.N_SMALL
# (RANGED, PROBED) -> the call
OPS = {(False, True): "transfer_small", (True, True): "transfer_range_small", (False, False): "insert_multi_small"}
N_DST = {True: 1, False: 2}  # by PROBED


def small_name(ranged: bool, probed: bool) -> str:
    return kl.inst(BASE, bool(ranged), bool(probed))


def build_rows():
    rows = []
    kts = itertools.cycle(kl.KEYS)
    ranged_kts = itertools.cycle(k for k in kl.KEYS if kl.carries_minmax(k))  # a flagged column holds key values
    logs = itertools.cycle((kl.LOG_LDS, kl.LOG_GATHER))  # 2^13 and 2^16 blocks: both at most 2^16
    for (ranged, probed), op in OPS.items():
        for dkind in KINDS:
            for row_sel in (False, True):
                kt = next(ranged_kts) if ranged else next(kts)
                args = dict(kt=kt, dkind=dkind, row_sel=row_sel, log_nb=next(logs), later_log_nb=LOG_LATER, n=N,
                            ranged=ranged, probed=probed, n_dst=N_DST[probed])
                rows.append(kl.Row("%s-%s-%s-%s" % (op, kt, dkind, "rowsel" if row_sel else "rows"), op, args,
                                   kl.once(small_name(ranged, probed))))
    return rows


ROWS = build_rows()


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launcher of rpt_transfer_small.hpp can produce."""
    return [small_name(*tp) for tp in OPS]
