"""The kernel ledger of csrc/rpt_routed_insert.hpp: which instantiation of partition_masked_kernel each routed
device-side insert must launch (a plain module, like kernel_ledger, whose helpers and shapes it reuses; it needs
neither torch nor a GPU).

partition_masked_kernel<K, DENSE, SEL, TM, SP>: K the key type; SEL false: the rows are chosen by result bits, over
the dense or the general row mapping; SEL true: by a selection vector with a device-side count (always the general
mapping); (TM, SP) the tile shape the filter size asks for (kernel_ledger.PARTITION_SHAPES). The key min/max is not a
template argument: the kernel folds it for every key type that carries values. Every row's call launches its
instantiation once, then the run-table transpose and the slice merge of rpt_bf_insert_ws.

tests/test_gpu_kernel_ledger_routed.py runs every row on the GPU; tests/test_kernel_ledger_routed_names.py checks
without one that the header records no kernel this table lacks."""
from __future__ import annotations

import os

import kernel_ledger as kl

ROUTED_SOURCE = os.path.join(kl.CSRC, "rpt_routed_insert.hpp")
BASE = "partition_masked_kernel"
TAIL = ("runs_transpose_kernel", "slice_insert_kernel")  # recorded by csrc/rpt_gpu.hip; rows of their own there


def masked_name(k: int, dense: bool, sel: bool, log_nb: int) -> str:
    tm, sp = kl.PARTITION_SHAPES[log_nb]
    return kl.inst(BASE, k, dense, sel, tm, sp)


def build_rows():
    rows = []
    general = kl._general_kinds(kl.GENERAL)
    sel_kinds = kl._general_kinds((kl.DENSE, kl.DICT, kl.MISALIGNED))  # the column under the selection vector

    def add(op, kernels, **args):
        tag = "-".join(str(args[k]) for k in ("kt", "dkind", "log_nb"))
        rows.append(kl.Row("%s-%s" % (op, tag), op, args, kernels))

    for log_nb in kl.PARTITION_SHAPES:
        for kt, k in kl.KEYS.items():
            for dense in (True, False):
                add("insert_bits_ws", kl.once(masked_name(k, dense, False, log_nb), *TAIL), kt=kt,
                    dkind=kl.DENSE if dense else next(general), log_nb=log_nb, n=kl.N_TILES)
            add("insert_sel_ws", kl.once(masked_name(k, False, True, log_nb), *TAIL), kt=kt, dkind=next(sel_kinds),
                log_nb=log_nb, n=kl.N_TILES)
    return rows


ROWS = build_rows()


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launchers of rpt_routed_insert.hpp can produce in the product build."""
    want = []
    for tm, sp in kl.PARTITION_SHAPES.values():
        want += [kl.inst(BASE, k, d, False, tm, sp) for k in kl.KEYS.values() for d in (True, False)]  # result bits
        want += [kl.inst(BASE, k, False, True, tm, sp) for k in kl.KEYS.values()]  # selection vector
    return want
