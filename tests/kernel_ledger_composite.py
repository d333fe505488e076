"""The kernel ledger of csrc/rpt_composite.hpp: composite join keys hashed inside the kernels (a plain module, like
kernel_ledger, whose helpers and shapes it reuses; it needs neither torch nor a GPU).

hash_composite_kernel<DENSE> (rpt_hash_keys_composite) and insert_composite_kernel<DENSE> (rpt_bf_insert_composite):
one row per instantiation and column-kind mix. All columns flat and aligned is <true>; one column a dictionary, or one
column misaligned by an element, is <false>. Each exactly one launch, over n = N_TILES rows.

chain_composite_small_kernel<PROBED, TRANSFER>: <true,false> for rpt_bf_probe_chain_composite, <true,true> for
rpt_bf_transfer_composite, <false,true> for rpt_bf_insert_multi_composite; one row per instantiation and per row mapping
(row_sel null or given), n = N_SMALL rows. Each must leave exactly one launch of its one name in the record: no
hash_kernel, insert_kernel, insert_sel_kernel, probe_chain_small_kernel and no selection-vector tail.

A column's key type is a run-time branch of every kernel here, so the key types rotate over the rows.

tests/test_gpu_kernel_ledger_composite.py runs every row on the GPU; tests/test_kernel_ledger_composite_names.py checks
without one that the header records no kernel this table lacks."""
from __future__ import annotations

import itertools
import os

import kernel_ledger as kl

COMPOSITE_SOURCE = os.path.join(kl.CSRC, "rpt_composite.hpp")
HASH_BASE, INSERT_BASE, SMALL_BASE = "hash_composite_kernel", "insert_composite_kernel", "chain_composite_small_kernel"
BASES = (HASH_BASE, INSERT_BASE, SMALL_BASE)
MIXES = (kl.DENSE, kl.DICT, kl.MISALIGNED)  # all dense; one column a dictionary; one column off by an element
# the key types of a key's columns ("hash": a prefix already hashed, column 0 only)
KEY_TYPES = (("i64", "i32"), ("i32", "i64", "i32"), ("hash", "i64", "i32", "i64"), ("i32", "i32"), ("i64", "i64", "i32"))
# (PROBED, TRANSFER) -> the call
SMALL_OPS = {(True, False): "chain_composite", (True, True): "transfer_composite", (False, True): "insert_multi_composite"}
ABSENT = ("hash_kernel", "insert_kernel", "insert_sel_kernel", "probe_chain_small_kernel") + kl.SEL_TAIL


def small_name(probed: bool, transfer: bool) -> str:
    return kl.inst(SMALL_BASE, bool(probed), bool(transfer))


def build_rows():
    rows = []
    kts = itertools.cycle(KEY_TYPES)
    logs = itertools.cycle((10, kl.LOG_GATHER))  # 2^10 and 2^16 blocks: both at most 2^16
    for op, base in (("hash_composite", HASH_BASE), ("insert_composite", INSERT_BASE)):
        for mix in MIXES:
            kt = next(kts)
            args = dict(kts=kt, mix=mix, n=kl.N_TILES, log_nb=next(logs))
            rows.append(kl.Row("%s-%s-%s" % (op, "+".join(kt), mix), op, args, kl.once(kl.inst(base, mix == kl.DENSE))))
    for (probed, transfer), op in SMALL_OPS.items():
        for row_sel in (False, True):
            # two keys a side where the side exists: the rotation's next key, and a key of one column beside it
            kt = next(kts)
            args = dict(kts=kt, row_sel=row_sel, n=kl.N_SMALL, log_nb=next(logs), later_log_nb=11, probed=probed,
                        transfer=transfer)
            rows.append(kl.Row("%s-%s-%s" % (op, "+".join(kt), "rowsel" if row_sel else "rows"), op, args,
                               kl.once(small_name(probed, transfer))))
    return rows


ROWS = build_rows()


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launchers of rpt_composite.hpp can produce."""
    return ([kl.inst(HASH_BASE, d) for d in (True, False)] + [kl.inst(INSERT_BASE, d) for d in (True, False)] +
            [small_name(*tp) for tp in SMALL_OPS])
