"""The kernel ledger of csrc/rpt_probe_sel_small.hpp: the one-launch device-counted chain and transfer (a plain module,
like kernel_ledger, whose helpers and shapes it reuses; it needs neither torch nor a GPU).

probe_chain_sel_small_kernel<TRANSFER>: false for rpt_bf_probe_chain_sel, true for rpt_bf_transfer_sel. The key type
and the column kind are run-time branches of the one kernel, so there is one row per column kind for each
instantiation, the key types rotating over them. Every row's call runs over two filters with max_rows = N_SMALL (the
transfer rows with one destination) and must leave exactly one launch of its one name in the record: no masked stage,
no selection-vector tail (group_sum, group_scan, compact) and no insert_sel_kernel.

tests/test_gpu_kernel_ledger_sel_small.py runs every row on the GPU; tests/test_kernel_ledger_sel_small_names.py checks
without one that the header records no kernel this table lacks."""
from __future__ import annotations

import itertools
import os

import kernel_ledger as kl

SMALL_SOURCE = os.path.join(kl.CSRC, "rpt_probe_sel_small.hpp")
BASE = "probe_chain_sel_small_kernel"
KINDS = (kl.DENSE, kl.DICT, kl.MISALIGNED)  # the column under the selection vector
LOG_LATER = 11  # the second filter of every row
N = kl.N_SMALL
OPS = {False: "chain_sel_small", True: "transfer_sel_small"}


def small_name(transfer: bool) -> str:
    return kl.inst(BASE, bool(transfer))


def build_rows():
    rows = []
    kts = itertools.cycle(kl.KEYS)
    logs = itertools.cycle((kl.LOG_LDS, kl.LOG_GATHER))  # 2^13 and 2^16 blocks: both at most 2^16
    for transfer in (False, True):
        for dkind in KINDS:
            kt = next(kts)
            args = dict(kt=kt, dkind=dkind, log_nb=next(logs), later_log_nb=LOG_LATER, n=N, transfer=transfer)
            rows.append(kl.Row("%s-%s-%s" % (OPS[transfer], kt, dkind), OPS[transfer], args,
                               kl.once(small_name(transfer))))
    return rows


ROWS = build_rows()


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launcher of rpt_probe_sel_small.hpp can produce."""
    return [small_name(False), small_name(True)]
