"""The ledger of csrc/rpt_routed_insert.hpp (tests/kernel_ledger_routed.py) is complete, without a GPU: every kernel
the header can record has a row, partition_masked_kernel's reachable instantiations are covered as the full product
with no strays, and no name is cut in rpt_kernel_stat::name or collides with a name of csrc/rpt_gpu.hip."""
import collections

import kernel_ledger as kl
import kernel_ledger_routed as klr


def test_every_kernel_of_the_routed_header_has_a_row():
    source = kl.source_base_names(klr.ROUTED_SOURCE)
    assert source == {klr.BASE}
    covered = {kl.base_name(n) for n in klr.expected_names()} - set(klr.TAIL)
    assert covered == source
    # the shared tail is recorded by the host source, where it has rows of its own
    assert set(klr.TAIL) <= kl.source_base_names() and set(klr.TAIL) <= kl.expected_names()
    # the host source itself records no launcher of the new kernel (its ledger may not change)
    assert klr.BASE not in kl.source_base_names()


def test_reachable_instantiations_are_the_full_product_with_no_strays():
    want = klr.reachable_names()
    assert len(want) == len(set(want)) == 3 * (3 * 2 + 3)
    assert sorted(kl.PARTITION_SHAPES.values()) == [(1, 0), (1, 4), (2, 0)]
    have = {n for n in klr.expected_names() if kl.base_name(n) == klr.BASE}
    assert not (set(want) - have), "instantiations without a ledger row: %s" % sorted(set(want) - have)
    assert not (have - set(want)), sorted(have - set(want))
    assert kl.inst(klr.BASE, 1, True, False, 2, 0) == "partition_masked_kernel<1,true,false,2,0>"
    # a selection vector is never the dense mapping
    assert not [n for n in have if n.split(",")[1:3] == ["true", "true"]]


def test_every_row_launches_its_instantiation_once_then_the_shared_tail():
    for r in klr.ROWS:
        assert set(r.kernels.values()) == {1} and len(r.kernels) == 3, r.id
        assert set(klr.TAIL) < set(r.kernels), r.id
        (name,) = set(r.kernels) - set(klr.TAIL)
        args = name[len(klr.BASE) + 1:-1].split(",")
        assert args[0] == str(kl.KEYS[r.args["kt"]]), r.id
        assert args[2] == kl.targ(r.op == "insert_sel_ws"), r.id
        if r.op == "insert_bits_ws":
            assert args[1] == kl.targ(r.args["dkind"] == kl.DENSE), r.id
        assert (int(args[3]), int(args[4])) == kl.PARTITION_SHAPES[r.args["log_nb"]], r.id
    by_kind = collections.Counter(r.args["dkind"] for r in klr.ROWS if r.op == "insert_bits_ws")
    for kind in kl.GENERAL:
        assert by_kind[kind] >= 3, (kind, by_kind)


def test_names_are_short_unique_and_new():
    names = klr.expected_names()
    for n in names:
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    everything = names | kl.expected_names()
    assert len({n[: kl.NAME_BYTES - 1] for n in everything}) == len(everything)
    assert not ({n for n in names if kl.base_name(n) == klr.BASE} & kl.expected_names())
    ids = [r.id for r in klr.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]
    assert not set(ids) & {r.id for r in kl.ROWS}


def test_rows_stay_small():
    for r in klr.ROWS:
        assert r.args["n"] == kl.N_TILES and r.args["log_nb"] <= 22, r.id
