"""The ledger of csrc/rpt_composite.hpp (tests/kernel_ledger_composite.py) is complete, without a GPU: the header
records exactly the three composite kernels, all seven of their instantiations have rows, csrc/rpt_gpu.hip and the other
host headers do not record them, and no name is cut in rpt_kernel_stat::name or collides with a name or a row id of the
other seven ledgers."""
import collections
import os

import kernel_ledger as kl
import kernel_ledger_composite as klc
import kernel_ledger_range as klg
import kernel_ledger_routed as klr
import kernel_ledger_sel as kls
import kernel_ledger_sel_range as klsr
import kernel_ledger_sel_small as klss
import kernel_ledger_transfer_small as klts

OTHER_LEDGERS = (kl, klr, kls, klss, klg, klsr, klts)
OTHER_SOURCES = (kl.HOST_SOURCE, klr.ROUTED_SOURCE, kls.SEL_SOURCE, klss.SMALL_SOURCE, klg.RANGE_SOURCE,
                 klsr.SEL_RANGE_SOURCE, klts.TRANSFER_SMALL_SOURCE, os.path.join(kl.CSRC, "rpt_chain_call.hpp"))


def test_the_header_records_exactly_the_three_new_kernels():
    assert kl.source_base_names(klc.COMPOSITE_SOURCE) == set(klc.BASES)
    assert {kl.base_name(n) for n in klc.expected_names()} == set(klc.BASES)
    assert len(OTHER_SOURCES) == 8 and all(os.path.isfile(p) for p in OTHER_SOURCES)
    own = open(klc.COMPOSITE_SOURCE).read()
    for base in klc.BASES:
        assert '"%s"' % base in own, base
        for path in OTHER_SOURCES:
            # no other host file records a launcher of the new kernels
            assert base not in kl.source_base_names(path), (path, base)
            assert '"%s"' % base not in open(path).read(), (path, base)
    # rpt_gpu.hip gains the include lines and nothing else names the header's entry points
    host = open(kl.HOST_SOURCE).read()
    assert host.count('#include "rpt_composite.hpp"') == 1 and host.count('#include "kernels/composite.hpp"') == 1
    assert host.index('#include "rpt_transfer_small.hpp"') < host.index('#include "rpt_composite.hpp"')
    assert host.index('#include "kernels/transfer_small.hpp"') < host.index('#include "kernels/composite.hpp"')
    assert "_composite(" not in host


def test_all_seven_instantiations_have_rows_and_no_strays():
    want = klc.reachable_names()
    assert want == ["hash_composite_kernel<true>", "hash_composite_kernel<false>", "insert_composite_kernel<true>",
                    "insert_composite_kernel<false>", "chain_composite_small_kernel<true,false>",
                    "chain_composite_small_kernel<true,true>", "chain_composite_small_kernel<false,true>"]
    assert klc.expected_names() == set(want)
    for op, base in (("hash_composite", klc.HASH_BASE), ("insert_composite", klc.INSERT_BASE)):
        rows = [r for r in klc.ROWS if r.op == op]
        # one row per column-kind mix; only the all-dense mix is the dense instantiation
        assert [r.args["mix"] for r in rows] == list(klc.MIXES), op
        for r in rows:
            assert r.kernels == {kl.inst(base, r.args["mix"] == kl.DENSE): 1}, r.id
    for (probed, transfer), op in klc.SMALL_OPS.items():
        rows = [r for r in klc.ROWS if r.op == op]
        assert [(r.args["probed"], r.args["transfer"], r.args["row_sel"]) for r in rows] == [
            (probed, transfer, False), (probed, transfer, True)], op
    assert len(klc.ROWS) == 12
    # the key types rotate: every key type, a HASH prefix and every key width is used
    used = [r.args["kts"] for r in klc.ROWS]
    assert {kt for kts in used for kt in kts} == set(kl.KEYS)
    assert {len(kts) for kts in used} == {2, 3, 4}
    assert all(2 <= len(kts) <= 4 and "hash" not in kts[1:] for kts in used)


def test_every_row_is_exactly_one_launch_of_its_one_name():
    for r in klc.ROWS:
        assert len(r.kernels) == 1 and list(r.kernels.values()) == [1], r.id
        assert kl.base_name(next(iter(r.kernels))) in klc.BASES, r.id
        for absent in klc.ABSENT:
            assert absent not in {kl.base_name(n) for n in r.kernels}, (r.id, absent)


def test_names_are_short_unique_and_new():
    names = klc.expected_names()
    for n in names:
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    others = set().union(*(m.expected_names() for m in OTHER_LEDGERS))
    assert not names & others
    everything = names | others
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert not set(klc.BASES) & {kl.base_name(n) for n in others}
    # row ids are unique across all eight ledgers
    ids = [r.id for m in OTHER_LEDGERS + (klc,) for r in m.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]


def test_rows_stay_small():
    for r in klc.ROWS:
        small = kl.base_name(next(iter(r.kernels))) == klc.SMALL_BASE
        assert r.args["n"] == (kl.N_SMALL if small else kl.N_TILES), r.id
        assert max(r.args["log_nb"], r.args.get("later_log_nb", 0)) <= 16, r.id
