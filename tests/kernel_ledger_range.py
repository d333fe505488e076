"""The kernel ledger of csrc/rpt_probe_range.hpp: the min/max range stage (a plain module, like kernel_ledger, whose
helpers and shapes it reuses; it needs neither torch nor a GPU).

range_bits_kernel<K, DENSE, MASKED>: K int64 / int32 (a HASH column carries no key values and is refused), DENSE as
everywhere else, MASKED false for the first range stage of a call and true for the later ones: eight instantiations,
and one row per (key type, row mapping, masked), the general mapping reached in each of its three ways.

  range_bits   rpt_bf_range_bits over the row's column: exactly one launch of the unmasked instantiation.
  chain_range  rpt_bf_probe_chain_range_ws over two filters, both flagged and both forced to GATHER: filter 0 probes a
               dense int64 column (general once the call has a row_sel) and takes the unmasked range stage, filter 1
               probes the row's column and takes the masked one; then both filters run as masked gather stages, then
               the selection-vector tail once. Every kernel of the call is listed.

tests/test_gpu_kernel_ledger_range.py runs every row on the GPU; tests/test_kernel_ledger_range_names.py checks
without one that the header records no kernel this table lacks."""
from __future__ import annotations

import collections
import os

import kernel_ledger as kl

RANGE_SOURCE = os.path.join(kl.CSRC, "rpt_probe_range.hpp")
BASE = "range_bits_kernel"
RANGE_KEYS = ("i64", "i32")
KINDS = (kl.DENSE,) + kl.GENERAL
N = 4 * 512 + 5  # four full segments and a five-row tail: two workgroups of the persistent grid
LOG_NB = kl.LOG_GATHER  # both filters of every row: 2^16 blocks
OPS = {False: "range_bits", True: "chain_range"}


def range_name(kt: str, dense: bool, masked: bool) -> str:
    return kl.inst(BASE, kl.KEYS[kt], bool(dense), bool(masked))


def masked_probe_name(kt: str, dense: bool) -> str:
    return kl.inst("probe_bits_masked_kernel", kl.KEYS[kt], bool(dense), False, kl.BLOCK_THREADS)


def build_rows():
    rows = []
    for masked in (False, True):
        for kt in RANGE_KEYS:
            for dkind in KINDS:
                dense = dkind == kl.DENSE
                if masked:
                    dense0 = dkind != kl.ROW_SEL  # filter 0's dense int64 column under the call's row_sel
                    kernels = dict(collections.Counter([
                        range_name("i64", dense0, False), range_name(kt, dense, True),
                        masked_probe_name("i64", dense0), masked_probe_name(kt, dense), *kl.SEL_TAIL]))
                else:
                    kernels = kl.once(range_name(kt, dense, False))
                args = dict(kt=kt, dkind=dkind, log_nb=LOG_NB, n=N, masked=masked)
                rows.append(kl.Row("%s-%s-%s" % (OPS[masked], kt, dkind), OPS[masked], args, kernels))
    return rows


ROWS = build_rows()


def expected_names() -> set:
    return kl.expected_names(ROWS)


def reachable_names() -> list:
    """Every instantiation the launchers of rpt_probe_range.hpp can produce."""
    return [range_name(kt, d, m) for kt in RANGE_KEYS for d in (True, False) for m in (False, True)]
