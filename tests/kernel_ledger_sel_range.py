"""The kernel ledger of csrc/rpt_probe_sel_range.hpp: the min/max range in the device-counted probes and in the
one-launch chains (a plain module, like kernel_ledger, whose helpers and shapes it reuses; it needs neither torch nor a
GPU).

range_bits_sel_kernel<K>: K int64 / int32 (a flagged HASH column is refused); the row mapping is always the general one
(a selection vector). probe_chain_range_small_kernel<COUNTED, TRANSFER>: <false,false> rpt_bf_probe_chain_range,
<true,false> rpt_bf_probe_chain_sel_range, <true,true> rpt_bf_transfer_sel_range; key types and column kinds are
run-time branches. Five instantiations, one row each, all at n = max_rows = N over two flagged filters.

  chain_sel_range_ws  rpt_bf_probe_chain_sel_range_ws, both filters forced to GATHER: filter 0 probes the row's column
                      and takes range_bits_sel_kernel<K>; filter 1 (an int64 dictionary column) takes the masked
                      range_bits_kernel; then both filters run as masked gather stages, then the selection-vector tail
                      once. Every kernel of the call is listed.
  *_range_small       the one-launch calls: exactly one launch of the row's instantiation; no range stage, no masked
                      stage, no selection-vector tail and no insert kernel.

tests/test_gpu_kernel_ledger_sel_range.py runs every row on the GPU; tests/test_kernel_ledger_sel_range_names.py checks
without one that the header records no kernel this table lacks."""
from __future__ import annotations

import collections
import os

import kernel_ledger as kl
import kernel_ledger_range as klg

SEL_RANGE_SOURCE = os.path.join(kl.CSRC, "rpt_probe_sel_range.hpp")
BASE_STAGE = "range_bits_sel_kernel"
BASE_SMALL = "probe_chain_range_small_kernel"
BASES = (BASE_STAGE, BASE_SMALL)
RANGE_KEYS = klg.RANGE_KEYS
N = klg.N  # four full segments and a five-row tail
LOG_NB = kl.LOG_GATHER  # the first filter of every row: 2^16 blocks
LOG_LATER = kl.LOG_LDS  # the second: 2^13 blocks
# (COUNTED, TRANSFER) -> the call
SMALL_OPS = {(False, False): "chain_range_small", (True, False): "chain_sel_range_small",
             (True, True): "transfer_sel_range_small"}
WS_OP = "chain_sel_range_ws"


def stage_name(kt: str) -> str:
    return kl.inst(BASE_STAGE, kl.KEYS[kt])


def small_name(counted: bool, transfer: bool) -> str:
    return kl.inst(BASE_SMALL, bool(counted), bool(transfer))


def build_rows():
    rows = []
    # the column under the selection vector (the row-list chain: under no row_sel) and its key type, rotating
    kinds = {"i64": kl.DICT, "i32": kl.MISALIGNED}
    for kt in RANGE_KEYS:
        kernels = dict(collections.Counter([
            stage_name(kt), klg.range_name("i64", False, True), klg.masked_probe_name(kt, False),
            klg.masked_probe_name("i64", False), *kl.SEL_TAIL]))
        args = dict(kt=kt, dkind=kinds[kt], log_nb=LOG_NB, later_log_nb=LOG_LATER, n=N)
        rows.append(kl.Row("%s-%s-%s" % (WS_OP, kt, kinds[kt]), WS_OP, args, kernels))
    small_kts = ("i64", "i32", "i64")
    small_kinds = (kl.DENSE, kl.DICT, kl.MISALIGNED)
    for (counted, transfer), kt, dkind in zip(SMALL_OPS, small_kts, small_kinds):
        op = SMALL_OPS[(counted, transfer)]
        args = dict(kt=kt, dkind=dkind, log_nb=LOG_NB, later_log_nb=LOG_LATER, n=N, counted=counted, transfer=transfer)
        rows.append(kl.Row("%s-%s-%s" % (op, kt, dkind), op, args, kl.once(small_name(counted, transfer))))
    return rows


ROWS = build_rows()


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launchers of rpt_probe_sel_range.hpp can produce."""
    return [stage_name(kt) for kt in RANGE_KEYS] + [small_name(*ct) for ct in SMALL_OPS]
