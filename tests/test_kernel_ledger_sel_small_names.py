"""The ledger of csrc/rpt_probe_sel_small.hpp (tests/kernel_ledger_sel_small.py) is complete, without a GPU: the header
records exactly one kernel, both of its instantiations have rows, neither csrc/rpt_gpu.hip nor csrc/rpt_probe_sel.hpp
records it, and no name is cut in rpt_kernel_stat::name or collides with a name of the other three ledgers."""
import collections

import kernel_ledger as kl
import kernel_ledger_routed as klr
import kernel_ledger_sel as kls
import kernel_ledger_sel_small as klss

OTHER_LEDGERS = (kl, klr, kls)


def test_every_kernel_of_the_header_has_a_row():
    source = kl.source_base_names(klss.SMALL_SOURCE)
    assert source == {klss.BASE}
    assert {kl.base_name(n) for n in klss.expected_names()} == source
    # neither the host source nor the header of the workspace calls records a launcher of the new kernel
    assert klss.BASE not in kl.source_base_names()
    assert klss.BASE not in kl.source_base_names(kls.SEL_SOURCE)
    assert kl.source_base_names(kls.SEL_SOURCE) == {kls.BASE}


def test_both_instantiations_have_rows_and_no_strays():
    want = klss.reachable_names()
    assert want == ["probe_chain_sel_small_kernel<false>", "probe_chain_sel_small_kernel<true>"]
    assert klss.expected_names() == set(want)
    for transfer in (False, True):
        rows = [r for r in klss.ROWS if r.args["transfer"] == transfer]
        # one row per column kind for each instantiation
        assert sorted(r.args["dkind"] for r in rows) == sorted(klss.KINDS), transfer
        assert {r.op for r in rows} == {klss.OPS[transfer]}
    assert {r.args["kt"] for r in klss.ROWS} == set(kl.KEYS)


def test_every_row_is_exactly_one_launch_of_its_one_name():
    for r in klss.ROWS:
        assert r.kernels == {klss.small_name(r.args["transfer"]): 1}, r.id
        for absent in ("insert_sel_kernel", "probe_bits_sel_kernel") + kl.SEL_TAIL:
            assert absent not in {kl.base_name(n) for n in r.kernels}, (r.id, absent)


def test_names_are_short_unique_and_new():
    names = klss.expected_names()
    for n in names:
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    others = set().union(*(m.expected_names() for m in OTHER_LEDGERS))
    assert not names & others
    everything = names | others
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert klss.BASE not in {kl.base_name(n) for n in others}
    # row ids are unique across all four ledgers
    ids = [r.id for m in OTHER_LEDGERS + (klss,) for r in m.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]


def test_rows_stay_small():
    for r in klss.ROWS:
        assert r.args["n"] == kl.N_SMALL and max(r.args["log_nb"], r.args["later_log_nb"]) <= 16, r.id
