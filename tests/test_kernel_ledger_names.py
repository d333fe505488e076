"""The kernel ledger (tests/kernel_ledger.py) is complete, without a GPU: every kernel csrc/rpt_gpu.hip can record
has a row or a written exemption, every K x D dispatch is covered as the full product, no expected name is cut or
collides in rpt_kernel_stat::name, and the comparison the GPU test relies on rejects what it should."""
import collections
import glob
import os
import re

import kernel_ledger as kl


def test_every_kernel_of_the_host_runtime_has_a_row_or_an_exemption():
    source = kl.source_base_names()
    # the scan itself works: a few names of each spelling (plain literal, with name arguments, behind dispatch_tm)
    for name in ("slice_probe_kernel", "partition_kernel", "unpermute_sel_kernel", "hash_kernel", "or_slices_kernel(fold)",
                 "probe_bits_masked_hybrid_kernel", "stream_copy_kernel"):
        assert name in source, name
    assert len(source) >= 33  # every kernel the host records today
    covered = {kl.base_name(n) for n in kl.expected_names()}
    exempt = set(kl.EXEMPT)
    missing = source - covered - exempt
    assert not missing, "kernels with neither a ledger row nor an exemption: %s" % sorted(missing)
    # nothing stale either: a row or an exemption names a kernel the source still has
    assert not (covered - source), sorted(covered - source)
    assert not (exempt - source), sorted(exempt - source)
    assert not (covered & exempt), sorted(covered & exempt)


def test_exemptions_are_the_agreed_ones_each_with_a_reason():
    assert set(kl.EXEMPT) == {"or_slices_kernel(allreduce)", "stream_read_kernel", "stream_copy_kernel"}
    assert all(isinstance(r, str) and len(r) > 20 for r in kl.EXEMPT.values())
    assert kl.NEVER_LAUNCHED == ()  # no kernel is compiled in but switched off: what the host can record, it launches


def test_dispatch_products_are_complete():
    """Every name dispatch_kd and the launchers behind it can produce in the product build."""
    want = []
    want += kl.kd_product("probe_bits_kernel", False, kl.BLOCK_THREADS)  # GATHER; rpt_bf_find_bits
    want += kl.kd_product("probe_bits_kernel", True, kl.LDS_THREADS)  # LDS, whole filter
    want += kl.kd_product("probe_bits_hybrid_kernel")
    want += kl.kd_product("probe_small_kernel")
    want += kl.kd_product("probe_bits_masked_kernel", False, kl.BLOCK_THREADS)
    want += kl.kd_product("probe_bits_masked_kernel", True, kl.LDS_THREADS)
    want += kl.kd_product("probe_bits_masked_hybrid_kernel")
    want += kl.kd_product("insert_kernel")
    want += kl.kd_product("insert_bits_kernel")
    for tm, sp in kl.PARTITION_SHAPES.values():
        want += kl.kd_product("partition_kernel", False, tm, sp)  # probes; HASH inserts
        want += [n for n in kl.kd_product("partition_kernel", True, tm, sp)  # inserts that fold the min/max
                 if not n.startswith("partition_kernel<%d," % kl.KEYS["hash"])]
    want.append(kl.inst("partition_kernel", kl.KEY_SPLIT, True, False, 1, 0))  # level 2 of the bucketed strategies
    want += kl.kd_product("bucket_scatter_kernel", False)
    want += [n for n in kl.kd_product("bucket_scatter_kernel", True)
             if not n.startswith("bucket_scatter_kernel<%d," % kl.KEYS["hash"])]
    want += [kl.inst("insert_sel_kernel", k) for k in kl.KEYS.values()]
    want += [kl.inst("hash_kernel", k, c) for k in kl.KEYS.values() for c in (False, True)]
    want += [kl.inst(base, tm) for base in ("unpermute_kernel", "unpermute_sel_kernel") for tm in (1, 2)]
    assert len(want) == len(set(want)) == 6 * 9 + 3 * (6 + 4) + 1 + 6 + 4 + 3 + 6 + 4
    assert sorted(kl.PARTITION_SHAPES.values()) == [(1, 0), (1, 4), (2, 0)]
    have = kl.expected_names()
    assert not (set(want) - have), "instantiations without a ledger row: %s" % sorted(set(want) - have)
    # and the table expects no instantiation of these kernels beyond the reachable ones
    templated = {kl.base_name(n) for n in want}
    stray = {n for n in have if kl.base_name(n) in templated} - set(want)
    assert not stray, sorted(stray)
    # spelled as the library spells them
    assert kl.inst("partition_kernel", 0, True, False, 1, 0) == "partition_kernel<0,true,false,1,0>"
    assert kl.inst("probe_bits_kernel", 2, False, True, 1024) == "probe_bits_kernel<2,false,true,1024>"
    assert (kl.KEYS, kl.KEY_SPLIT) == ({"i64": 0, "i32": 1, "hash": 2}, 3)


def test_the_general_mapping_is_reached_in_all_three_ways():
    by_kind = collections.Counter(r.args.get("dkind") for r in kl.ROWS)
    for kind in kl.GENERAL:
        assert by_kind[kind] >= 6, (kind, by_kind)
    # a general row expects a general instantiation and a dense row a dense one, wherever the kernel has the argument
    for r in kl.ROWS:
        if r.op in ("find_bits", "insert_bits") or (r.op == "insert" and r.args["what"] == "atomic"):
            (name,) = r.kernels
            assert name.split(",")[1].rstrip(">") == kl.targ(r.args["dkind"] == kl.DENSE), r.id


def test_names_are_short_and_unique():
    names = kl.expected_names()
    assert len(names) >= 100
    for n in names:
        assert len(n) <= kl.NAME_BYTES - 1, "%s would be cut in rpt_kernel_stat::name" % n
    assert len({n[: kl.NAME_BYTES - 1] for n in names}) == len(names)
    ids = [r.id for r in kl.ROWS]
    assert len(ids) == len(set(ids)), [i for i, c in collections.Counter(ids).items() if c > 1]


def test_rows_stay_small():
    for r in kl.ROWS:
        assert r.args.get("n", 0) <= 50_000 and r.args.get("log_nb", 0) <= 22, r.id
    assert kl.N_TILES == 3 * 16384 + 5 and kl.N_SMALL == 513


def test_set_comparison_rejects_missing_extra_and_wrong_count():
    expected = {"a_kernel<0,true>": 1, "b_kernel": 2, "c_kernel(fold)": None}
    ok = {"a_kernel<0,true>": (1, 0.01), "b_kernel": (2, 0.5), "c_kernel(fold)": (3, 0.1)}
    assert kl.kernel_set_problems(expected, ok) == []
    missing = {k: v for k, v in ok.items() if k != "b_kernel"}
    assert kl.kernel_set_problems(expected, missing) == ["missing: b_kernel did not run"]
    extra = dict(ok, **{"a_kernel<0,false>": (1, 0.01)})
    assert kl.kernel_set_problems(expected, extra) == ["extra: a_kernel<0,false> ran (1 launches)"]
    wrong = dict(ok, b_kernel=(3, 0.5))
    assert kl.kernel_set_problems(expected, wrong) == ["count: b_kernel launched 3 times, expected 2"]
    zero = dict(ok, **{"c_kernel(fold)": (0, 0.0)})
    assert kl.kernel_set_problems(expected, zero) == ["count: c_kernel(fold) launched 0 times, expected >= 1"]
    assert len(kl.kernel_set_problems(expected, {})) == 3
    assert kl.kernel_set_problems({}, {}) == []
    # a wrong template argument is both a missing and an extra name
    swapped = {"a_kernel<0,false>": (1, 0.01), "b_kernel": (2, 0.5), "c_kernel(fold)": (1, 0.1)}
    assert [p.split(":")[0] for p in kl.kernel_set_problems(expected, swapped)] == ["missing", "extra"]


def test_every_launch_goes_through_the_helper():
    """csrc/rpt_launch.hpp holds the one hipLaunchKernelGGL of the host runtime; rpt_gpu.hip and the other host headers
    launch through it and keep no once-flag of their own around the dynamic-LDS opt-in."""
    helper = os.path.join(kl.CSRC, "rpt_launch.hpp")
    others = [kl.HOST_SOURCE] + sorted(p for p in glob.glob(os.path.join(kl.CSRC, "rpt_*.hpp")) if p != helper)
    assert len(others) >= 8 and os.path.isfile(helper), others
    for path in others:
        text = open(path).read()
        assert "hipLaunchKernelGGL" not in text, path
        assert not re.search(r"std::once_flag.{0,400}?allow_dynamic_lds", text, re.S), path
    assert open(helper).read().count("hipLaunchKernelGGL") == 1
