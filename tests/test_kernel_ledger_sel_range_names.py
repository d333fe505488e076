"""The ledger of csrc/rpt_probe_sel_range.hpp (tests/kernel_ledger_sel_range.py) is complete, without a GPU: the header
records exactly its two kernels, all five instantiations have one row each, csrc/rpt_gpu.hip and the other five host
headers do not record them, and no name is cut in rpt_kernel_stat::name or collides with a name or a row id of the
other five ledgers."""
import collections
import os

import kernel_ledger as kl
import kernel_ledger_range as klg
import kernel_ledger_routed as klr
import kernel_ledger_sel as kls
import kernel_ledger_sel_range as klsr
import kernel_ledger_sel_small as klss

OTHER_LEDGERS = (kl, klr, kls, klss, klg)
OTHER_SOURCES = (kl.HOST_SOURCE, klr.ROUTED_SOURCE, kls.SEL_SOURCE, klss.SMALL_SOURCE, klg.RANGE_SOURCE,
                 os.path.join(kl.CSRC, "rpt_chain_call.hpp"))


def own_names():
    return {n for n in klsr.expected_names() if kl.base_name(n) in klsr.BASES}


def test_the_header_records_exactly_the_two_new_kernels():
    assert kl.source_base_names(klsr.SEL_RANGE_SOURCE) == set(klsr.BASES)
    text = open(klsr.SEL_RANGE_SOURCE).read()
    assert len(OTHER_SOURCES) == 6 and all(os.path.isfile(p) for p in OTHER_SOURCES)
    for base in klsr.BASES:
        # the host source and the other headers record no launcher of the new kernels
        for path in OTHER_SOURCES:
            assert base not in kl.source_base_names(path), path
            assert '"%s"' % base not in open(path).read(), path
        # ... and the launch-error literals are the header's too
        assert '"%s"' % base in text


def test_all_five_instantiations_have_one_row_each_and_no_strays():
    want = klsr.reachable_names()
    assert len(want) == len(set(want)) == 5
    assert kl.inst(klsr.BASE_STAGE, 0) == "range_bits_sel_kernel<0>" in want
    assert kl.inst(klsr.BASE_SMALL, True, False) == "probe_chain_range_small_kernel<true,false>" in want
    assert own_names() == set(want)
    per_name = collections.Counter(n for r in klsr.ROWS for n in r.kernels if kl.base_name(n) in klsr.BASES)
    assert per_name == {n: 1 for n in want}
    assert len(klsr.ROWS) == 5
    assert "hash" not in klsr.RANGE_KEYS  # refused: a HASH column carries no key values
    assert "probe_chain_range_small_kernel<false,true>" not in want  # no one-launch row-list transfer


def test_every_row_lists_every_kernel_of_its_call():
    for r in klsr.ROWS:
        a = r.args
        if r.op != klsr.WS_OP:
            # one launch, nothing else
            assert r.op == klsr.SMALL_OPS[(a["counted"], a["transfer"])], r.id
            assert r.kernels == {klsr.small_name(a["counted"], a["transfer"]): 1}, r.id
            continue
        # the device-counted range stage, the masked range stage, two masked gather stages, the tail once
        assert sum(r.kernels.values()) == 1 + 1 + 2 + len(kl.SEL_TAIL), r.id
        assert r.kernels[klsr.stage_name(a["kt"])] == 1, r.id
        assert r.kernels[klg.range_name("i64", False, True)] == 1, r.id
        assert sum(c for n, c in r.kernels.items() if kl.base_name(n) == klg.BASE) == 1, r.id
        assert sum(c for n, c in r.kernels.items() if kl.base_name(n) == "probe_bits_masked_kernel") == 2, r.id
        for t in kl.SEL_TAIL:
            assert r.kernels[t] == 1, r.id
        bases = {kl.base_name(n) for n in r.kernels}
        assert "probe_bits_sel_kernel" not in bases and "probe_bits_kernel" not in bases, r.id  # filter 0 is a masked stage


def test_names_are_short_unique_and_new():
    names = own_names()
    for n in klsr.expected_names():
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    others = set().union(*(m.expected_names() for m in OTHER_LEDGERS))
    assert not names & others
    everything = names | others
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert not set(klsr.BASES) & {kl.base_name(n) for n in others}
    # the kernels a workspace row shares with the first and the range ledgers are spelled as those ledgers spell them
    assert klsr.expected_names() - names <= kl.expected_names() | klg.expected_names()
    # row ids are unique across all six ledgers
    ids = [r.id for m in OTHER_LEDGERS + (klsr,) for r in m.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]


def test_rows_stay_small():
    for r in klsr.ROWS:
        assert r.args["n"] == klsr.N and max(r.args["log_nb"], r.args["later_log_nb"]) <= 16, r.id
    assert klsr.N == 4 * 512 + 5
