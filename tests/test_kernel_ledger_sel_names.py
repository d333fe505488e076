"""The ledger of csrc/rpt_probe_sel.hpp (tests/kernel_ledger_sel.py) is complete, without a GPU: every kernel the header
can record has a row, probe_bits_sel_kernel's reachable instantiations are covered as the full product with no strays,
and no name is cut in rpt_kernel_stat::name or collides with a name of csrc/rpt_gpu.hip."""
import collections
import os
import re

import kernel_ledger as kl
import kernel_ledger_sel as kls


def test_every_kernel_of_the_header_has_a_row():
    source = kl.source_base_names(kls.SEL_SOURCE)
    assert source == {kls.BASE}
    shared = set(kls.TAIL) | {n for r in kls.DEMOTION_ROWS for n in r.kernels if kl.base_name(n) != kls.BASE}
    covered = {kl.base_name(n) for n in kls.expected_names() - shared}
    assert covered == source
    # the shared tail and the later stages are recorded by the host source, where they have rows of their own
    assert {kl.base_name(n) for n in shared} <= kl.source_base_names() and shared <= kl.expected_names()
    # the host source itself records no launcher of the new kernel (its ledger may not change)
    assert kls.BASE not in kl.source_base_names()
    assert kls.BASE not in {kl.base_name(n) for n in kl.expected_names()}


def test_mode_numbers_are_the_kernel_header_s():
    with open(os.path.join(kl.CSRC, "kernels", "probe_sel.hpp")) as f:
        src = f.read()
    for name, value in (("kSelGather", kls.MODE_GATHER), ("kSelLds", kls.MODE_LDS), ("kSelHybrid", kls.MODE_HYBRID)):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[;,]" % name, src)
        assert m and int(m.group(1)) == value, name


def test_reachable_instantiations_are_the_full_product_with_no_strays():
    want = kls.reachable_names()
    assert len(want) == len(set(want)) == 3 * 3
    have = {n for n in kls.expected_names() if kl.base_name(n) == kls.BASE}
    assert not (set(want) - have), "instantiations without a ledger row: %s" % sorted(set(want) - have)
    assert not (have - set(want)), sorted(have - set(want))
    assert kl.inst(kls.BASE, 1, 2) == "probe_bits_sel_kernel<1,2>"
    # one row per instantiation, apart from the demotion rows
    plain = [r for r in kls.ROWS if r not in kls.DEMOTION_ROWS]
    firsts = [n for r in plain for n in r.kernels if kl.base_name(n) == kls.BASE]
    assert sorted(firsts) == sorted(want)


def test_every_row_launches_its_instantiation_once_then_the_shared_tail():
    for r in kls.ROWS:
        assert set(r.kernels.values()) == {1} and len(r.kernels) == 5, r.id
        assert set(kl.SEL_TAIL) < set(r.kernels), r.id
        (name,) = [n for n in r.kernels if kl.base_name(n) == kls.BASE]
        k, mode = name[len(kls.BASE) + 1:-1].split(",")
        assert k == str(kl.KEYS[r.args["kt"]]), r.id
        log_nb, strategy = r.args["log_nb"], r.args["strategy"]
        if strategy in (kl.GATHER, kl.PARTITIONED):
            assert int(mode) == kls.MODE_GATHER, r.id
        else:
            assert strategy == kl.LDS and int(mode) == (kls.MODE_LDS if log_nb <= 14 else kls.MODE_HYBRID), r.id
        if r not in kls.DEMOTION_ROWS:
            assert kls.LATER_STAGE in r.kernels, r.id
    assert {r.args["what"] for r in kls.DEMOTION_ROWS} == {"demoted_first", "demoted_later"}
    by_kind = collections.Counter(r.args["dkind"] for r in kls.ROWS)
    for kind in (kl.DENSE, kl.DICT, kl.MISALIGNED):
        assert by_kind[kind] >= 3, (kind, by_kind)


def test_names_are_short_unique_and_new():
    names = kls.expected_names()
    for n in names:
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    everything = names | kl.expected_names()
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert not ({n for n in names if kl.base_name(n) == kls.BASE} & kl.expected_names())
    ids = [r.id for r in kls.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]
    assert not set(ids) & {r.id for r in kl.ROWS}


def test_rows_stay_small():
    for r in kls.ROWS:
        assert r.args["n"] == kl.N_SMALL and max(r.args["log_nb"], r.args["later_log_nb"]) <= 16, r.id
