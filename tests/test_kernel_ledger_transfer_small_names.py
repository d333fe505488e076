"""The ledger of csrc/rpt_transfer_small.hpp (tests/kernel_ledger_transfer_small.py) is complete, without a GPU: the
header records exactly one kernel, all three of its instantiations have rows, csrc/rpt_gpu.hip and the other six host
headers do not record it, and no name is cut in rpt_kernel_stat::name or collides with a name or a row id of the other
six ledgers."""
import collections
import os

import kernel_ledger as kl
import kernel_ledger_range as klg
import kernel_ledger_routed as klr
import kernel_ledger_sel as kls
import kernel_ledger_sel_range as klsr
import kernel_ledger_sel_small as klss
import kernel_ledger_transfer_small as klts

OTHER_LEDGERS = (kl, klr, kls, klss, klg, klsr)
OTHER_SOURCES = (kl.HOST_SOURCE, klr.ROUTED_SOURCE, kls.SEL_SOURCE, klss.SMALL_SOURCE, klg.RANGE_SOURCE,
                 klsr.SEL_RANGE_SOURCE, os.path.join(kl.CSRC, "rpt_chain_call.hpp"))


def test_the_header_records_exactly_the_new_kernel():
    assert kl.source_base_names(klts.TRANSFER_SMALL_SOURCE) == {klts.BASE}
    assert {kl.base_name(n) for n in klts.expected_names()} == {klts.BASE}
    assert len(OTHER_SOURCES) == 7 and all(os.path.isfile(p) for p in OTHER_SOURCES)
    for path in OTHER_SOURCES:
        # no other host file records a launcher of the new kernel
        assert klts.BASE not in kl.source_base_names(path), path
        assert '"%s"' % klts.BASE not in open(path).read(), path
    assert '"%s"' % klts.BASE in open(klts.TRANSFER_SMALL_SOURCE).read()
    # rpt_chain_call.hpp launches nothing
    assert kl.source_base_names(OTHER_SOURCES[-1]) == set()


def test_all_three_instantiations_have_rows_and_no_strays():
    want = klts.reachable_names()
    assert want == ["transfer_small_kernel<false,true>", "transfer_small_kernel<true,true>",
                    "transfer_small_kernel<false,false>"]
    assert klts.expected_names() == set(want)
    for (ranged, probed), op in klts.OPS.items():
        rows = [r for r in klts.ROWS if (r.args["ranged"], r.args["probed"]) == (ranged, probed)]
        # one row per column kind and per row mapping for each instantiation
        assert sorted((r.args["dkind"], r.args["row_sel"]) for r in rows) == sorted(
            (k, s) for k in klts.KINDS for s in (False, True)), op
        assert {r.op for r in rows} == {op}
        assert {r.args["n_dst"] for r in rows} == {1 if probed else 2}
        if ranged:
            assert "hash" not in {r.args["kt"] for r in rows}  # refused: a HASH column carries no key values
    assert {r.args["kt"] for r in klts.ROWS} == set(kl.KEYS)
    assert len(klts.ROWS) == 18


def test_every_row_is_exactly_one_launch_of_its_one_name():
    for r in klts.ROWS:
        assert r.kernels == {klts.small_name(r.args["ranged"], r.args["probed"]): 1}, r.id
        for absent in ("insert_sel_kernel", "insert_kernel", "probe_chain_small_kernel") + kl.SEL_TAIL:
            assert absent not in {kl.base_name(n) for n in r.kernels}, (r.id, absent)


def test_names_are_short_unique_and_new():
    names = klts.expected_names()
    for n in names:
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    others = set().union(*(m.expected_names() for m in OTHER_LEDGERS))
    assert not names & others
    everything = names | others
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert klts.BASE not in {kl.base_name(n) for n in others}
    # row ids are unique across all seven ledgers
    ids = [r.id for m in OTHER_LEDGERS + (klts,) for r in m.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]


def test_rows_stay_small():
    for r in klts.ROWS:
        assert r.args["n"] == kl.N_SMALL and max(r.args["log_nb"], r.args["later_log_nb"]) <= 16, r.id
