"""The ledger of csrc/rpt_probe_range.hpp (tests/kernel_ledger_range.py) is complete, without a GPU: the header records
exactly one kernel, all eight of its instantiations have rows, csrc/rpt_gpu.hip and the other host headers do not record
it, and no name is cut in rpt_kernel_stat::name or collides with a name or a row id of the other four ledgers."""
import collections

import kernel_ledger as kl
import kernel_ledger_range as klg
import kernel_ledger_routed as klr
import kernel_ledger_sel as kls
import kernel_ledger_sel_small as klss

OTHER_LEDGERS = (kl, klr, kls, klss)


def own_names():
    return {n for n in klg.expected_names() if kl.base_name(n) == klg.BASE}


def test_the_header_records_exactly_the_one_new_kernel():
    assert kl.source_base_names(klg.RANGE_SOURCE) == {klg.BASE}
    # the host source and the other headers record no launcher of the new kernel
    assert klg.BASE not in kl.source_base_names()
    assert klg.BASE not in kl.source_base_names(kls.SEL_SOURCE)
    assert klg.BASE not in kl.source_base_names(klss.SMALL_SOURCE)
    assert klg.BASE not in kl.source_base_names(klr.ROUTED_SOURCE)
    # ... and the launch-error literal is the header's too
    assert '"%s"' % klg.BASE in open(klg.RANGE_SOURCE).read()
    assert '"%s"' % klg.BASE not in open(kl.HOST_SOURCE).read()


def test_all_eight_instantiations_have_rows_and_no_strays():
    want = klg.reachable_names()
    assert len(want) == len(set(want)) == 8
    assert kl.inst(klg.BASE, 0, True, False) == "range_bits_kernel<0,true,false>" in want
    assert own_names() == set(want)
    # one row per (key type, row mapping, masked); the general mapping reached in all three ways
    cells = collections.Counter((r.args["kt"], r.args["dkind"], r.args["masked"]) for r in klg.ROWS)
    assert set(cells) == {(kt, d, m) for kt in klg.RANGE_KEYS for d in klg.KINDS for m in (False, True)}
    assert set(cells.values()) == {1}
    assert set(klg.KINDS) == {kl.DENSE, *kl.GENERAL}
    assert "hash" not in klg.RANGE_KEYS  # refused: a HASH column carries no key values


def test_every_row_lists_every_kernel_of_its_call():
    for r in klg.ROWS:
        a = r.args
        dense = a["dkind"] == kl.DENSE
        assert r.op == klg.OPS[a["masked"]], r.id
        if not a["masked"]:
            assert r.kernels == {klg.range_name(a["kt"], dense, False): 1}, r.id
            continue
        # two range stages (the first unmasked, the row's own masked), two masked gather stages, the tail once
        assert sum(r.kernels.values()) == 2 + 2 + len(kl.SEL_TAIL), r.id
        assert r.kernels[klg.range_name(a["kt"], dense, True)] == 1, r.id
        assert sum(c for n, c in r.kernels.items() if kl.base_name(n) == klg.BASE) == 2, r.id
        assert sum(c for n, c in r.kernels.items() if kl.base_name(n) == "probe_bits_masked_kernel") == 2, r.id
        for t in kl.SEL_TAIL:
            assert r.kernels[t] == 1, r.id
        assert "probe_bits_kernel" not in {kl.base_name(n) for n in r.kernels}, r.id  # filter 0 is a masked stage


def test_names_are_short_unique_and_new():
    names = own_names()
    for n in klg.expected_names():
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    others = set().union(*(m.expected_names() for m in OTHER_LEDGERS))
    assert not names & others
    everything = names | others
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert klg.BASE not in {kl.base_name(n) for n in others}
    # the kernels a chain row shares with the first ledger are spelled as that ledger spells them
    assert klg.expected_names() - names <= kl.expected_names()
    # row ids are unique across all five ledgers
    ids = [r.id for m in OTHER_LEDGERS + (klg,) for r in m.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]


def test_rows_stay_small():
    for r in klg.ROWS:
        assert r.args["n"] <= 50_000 and r.args["log_nb"] <= 16, r.id
    assert klg.N % 512 == 5 and klg.N > 512 * 4
