"""A forward and a backward step of predicate transfer that apply both halves of the dynamic filter, captured as ONE
graph: the ranges are read from device memory at every replay.

  tables    B: 40 000 rows with key columns x, y and z; V: one vector of 2048 rows with the same columns
  forward   B and V are probed by F on x, range and Bloom test; the survivors' z go into D_B / D_V
                                                                             rpt_bf_transfer_range_ws (twice)
  backward  B's survivors (sel and count on the device) are probed by G on y, range and Bloom test, and what is left
            goes into E_B on z                                               rpt_bf_transfer_insert_sel_range_ws
            V's survivors likewise into E_V, in one launch                   rpt_bf_transfer_sel_range

The expectation is computed on the host: a numpy range test written here, the oracle's probe, the oracle's insert of
exactly the survivors. Between two replays F's and G's ranges are changed with set_minmax and more build keys are
inserted into G, all outside the capture: the second replay's results follow the new ranges and the new words."""
import ctypes

import numpy as np
import pytest
import torch

import rpt_oracle as orc
from buf_util import (CAPTURE_MODE_GLOBAL, FF, GuardedBuffer, graph_destroy, graph_instantiate, graph_launch, hip_graph_api,
                      stream_capture)
from test_gpu_transfer import dev, graph_node_count, sel_of

pytestmark = pytest.mark.gpu

N_B, N_V = 40000, 2048
LOG_F, LOG_G, LOG_D = 13, 12, 14
POOL = 4000  # build keys per probed filter, drawn from +-2^40


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


def in_range(keys, mm):
    """The range test of a flat int64 column without NULLs: min <= key <= max."""
    return (keys >= mm[0]) & (keys <= mm[1])


def host_step(words, log_nb, mm, keys, ids):
    """The rows `ids` whose key passes the filter's range and Bloom tests, in order."""
    ids = np.asarray(ids, dtype=np.uint32)
    kept = ids[orc.probe_keys(words, log_nb, keys, key_sel=ids)]
    return kept[in_range(keys[kept], mm)], kept


def host_schedule(f_words, g_words, mm_f, mm_g, tables):
    out = {}
    for name, (x, y, z) in tables.items():
        fwd, f_bloom = host_step(f_words, LOG_F, mm_f, x, np.arange(x.size))
        bwd, g_bloom = host_step(g_words, LOG_G, mm_g, y, fwd)
        assert 0 < bwd.size < fwd.size < f_bloom.size < x.size, name  # every test of the schedule removes rows
        assert bwd.size < g_bloom.size, name
        d, e = orc.new_words(LOG_D), orc.new_words(LOG_D)
        orc.insert_keys(d, LOG_D, z, key_sel=fwd)
        orc.insert_keys(e, LOG_D, z, key_sel=bwd)
        out[name] = dict(fwd=fwd, bwd=bwd, d=d, e=e, d_mm=orc.minmax(z, key_sel=fwd), e_mm=orc.minmax(z, key_sel=bwd))
    return out


def test_forward_and_backward_steps_with_ranges_are_one_graph(rpt):
    rng = np.random.default_rng(4242)
    kf = rng.integers(-(2**40), 2**40, POOL).astype(np.int64)
    kg = rng.integers(-(2**40), 2**40, POOL).astype(np.int64)
    kg_more = rng.integers(-(2**40), 2**40, POOL).astype(np.int64)

    def table(n):
        x = np.where(rng.random(n) < 0.8, kf[rng.integers(0, POOL, n)], rng.integers(-(2**41), 2**41, n)).astype(np.int64)
        both = np.concatenate([kg, kg_more])
        y = np.where(rng.random(n) < 0.8, both[rng.integers(0, both.size, n)], rng.integers(-(2**41), 2**41, n))
        return x, y.astype(np.int64), rng.integers(-(2**50), 2**50, n).astype(np.int64)

    tables = {"B": table(N_B), "V": table(N_V)}
    f_words, g_words = orc.new_words(LOG_F), orc.new_words(LOG_G)
    orc.insert_keys(f_words, LOG_F, kf)
    orc.insert_keys(g_words, LOG_G, kg)
    f, g = rpt.BloomFilter(log_num_blocks=LOG_F), rpt.BloomFilter(log_num_blocks=LOG_G)
    f.insert(dev(kf))
    g.insert(dev(kg))
    assert f.minmax() == (int(kf.min()), int(kf.max())) and g.minmax() == (int(kg.min()), int(kg.max()))
    built = {(t, w): rpt.BloomFilter(log_num_blocks=LOG_D) for t in tables for w in "de"}
    cols = {t: tuple(dev(c) for c in tables[t]) for t in tables}
    i32, i64 = torch.int32, torch.int64
    n_of = {"B": N_B, "V": N_V}
    bufs = {}
    for t, n in n_of.items():
        bufs[t] = dict(fwd=GuardedBuffer(4 * n).poison(FF), fwd_cnt=GuardedBuffer(8).poison(FF),
                       bwd=GuardedBuffer(4 * n).poison(FF), bwd_cnt=GuardedBuffer(8).poison(FF),
                       ws_fwd=GuardedBuffer(rpt.probe_chain_range_workspace_bytes([f], 1, n)).poison(FF))
    bufs["B"]["ws_bwd"] = GuardedBuffer(rpt.probe_chain_sel_workspace_bytes([g], N_B)).poison(FF)
    need = rpt.transfer_insert_workspace_bytes([built[("B", "e")]], N_B)
    iws = GuardedBuffer(need).poison(FF) if need else None

    def schedule(stream):
        for t, n in n_of.items():  # forward
            x, _y, z = cols[t]
            b = bufs[t]
            rpt.transfer_range_ws([f], [x], [built[(t, "d")]], [z], range_mask=1, n=n, out_sel=b["fwd"].view(i32),
                                  out_count=b["fwd_cnt"].view(i64), workspace=b["ws_fwd"].bytes(), stream=stream)
        b, (_x, y, z) = bufs["B"], cols["B"]  # backward
        rpt.transfer_insert_sel_range_ws([g], [y], [built[("B", "e")]], [z], b["fwd"].view(i32), b["fwd_cnt"].view(i64),
                                         range_mask=[True], out_sel=b["bwd"].view(i32), out_count=b["bwd_cnt"].view(i64),
                                         workspace=b["ws_bwd"].bytes(), insert_workspace=iws.bytes() if iws else None,
                                         stream=stream)
        b, (_x, y, z) = bufs["V"], cols["V"]
        rpt.transfer_sel_range([g], [y], [built[("V", "e")]], [z], b["fwd"].view(i32), b["fwd_cnt"].view(i64),
                               range_mask=1, out_sel=b["bwd"].view(i32), out_count=b["bwd_cnt"].view(i64), stream=stream)

    def check_against_host(what, g_words, mm_f, mm_g):
        exp = host_schedule(f_words, g_words, mm_f, mm_g, tables)
        for t in tables:
            for name in ("fwd", "bwd"):
                got = int(bufs[t][name + "_cnt"].view(i64).item())
                assert got == exp[t][name].size, f"{what}: {t} {name} count {got}, host {exp[t][name].size}"
                assert np.array_equal(sel_of(bufs[t][name].view(i32)[:got]), exp[t][name]), f"{what}: {t} {name}"
                assert bool(torch.all(bufs[t][name].view(i32)[got:] == -1)), f"{what}: {t} {name} written past the count"
            for w in "de":
                assert np.array_equal(built[(t, w)].export_words(), exp[t][w]), f"{what}: {t} {w} differs from the oracle"
                assert built[(t, w)].minmax() == exp[t][w + "_mm"], f"{what}: {t} {w} min/max"
            for name, gb in bufs[t].items():
                gb.assert_guards_intact(f"{t} {name}")
        if iws is not None:
            iws.assert_guards_intact("insert workspace")
        return {t: (exp[t]["fwd"].size, exp[t]["bwd"].size) for t in tables}

    def reset_built():
        """Outside any capture, on the current stream: the built filters empty again, their deferred clears settled."""
        for bf in built.values():
            bf.clear()
            bf.settle()
        for t in tables:
            for name in ("fwd", "fwd_cnt", "bwd", "bwd_cnt"):
                bufs[t][name].poison(FF)
        torch.cuda.synchronize()

    mm_f, mm_g = (-(2**39), 2**39), (-(2**39), 2**38)
    f.set_minmax(mm_f)
    g.set_minmax(mm_g)
    # eagerly, on the current stream (a kernel's first launch may set its LDS allowance outside any capture)
    schedule(torch.cuda.current_stream())
    torch.cuda.synchronize()
    counts = [check_against_host("eager", g_words, mm_f, mm_g)]

    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    reset_built()
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _none = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: schedule(s))
    assert end == 0, "the capture was invalidated: something in the schedule synchronized, allocated or copied back"
    assert graph_instantiate(graph, exe) == 0
    for key, bf in built.items():  # capturing ran nothing
        assert not bf.export_words().any(), key
    assert graph_launch(exe, sh) == 0
    s.synchronize()
    counts.append(check_against_host("replay 0", g_words, mm_f, mm_g))
    # outside the capture: more build keys into G (its words and its folded min/max change), then other ranges
    g.insert(dev(kg_more))
    g_words2 = g_words.copy()
    orc.insert_keys(g_words2, LOG_G, kg_more)
    assert np.array_equal(g.export_words(), g_words2)
    mm_f2, mm_g2 = (-(2**38), 2**40), (-(2**40), 2**37)
    f.set_minmax(mm_f2)
    g.set_minmax(mm_g2)
    reset_built()
    assert graph_launch(exe, sh) == 0
    s.synchronize()
    counts.append(check_against_host("replay 1", g_words2, mm_f2, mm_g2))
    assert counts[0] == counts[1] != counts[2]  # the same ranges eagerly and replayed; other ranges, other counts
    assert graph_destroy(exe, graph)
    for bf in [f, g, *built.values()]:
        bf.close()


@pytest.mark.parametrize("call", ["transfer_sel_range", "transfer_insert_sel_range_ws"])
@pytest.mark.parametrize("cleared", ["probed", "destination"])
def test_pending_clear_is_refused_inside_the_capture(rpt, cleared, call):
    """A deferred clear cannot be settled inside a capture: a cleared probed filter and a cleared destination refuse the
    ranged transfers before anything is enqueued (the captured graph has no node, the destination is not marked);
    outside a capture the same call settles it."""
    rng = np.random.default_rng(77)
    max_rows, used = (N_V, 1500) if call == "transfer_sel_range" else (N_B, 30000)
    keys = rng.integers(-(2**40), 2**40, 1000).astype(np.int64)
    probed, dst = rpt.BloomFilter(log_num_blocks=12), rpt.BloomFilter(log_num_blocks=12)
    probed.insert(dev(keys))
    stale = dst if cleared == "destination" else probed
    if cleared == "destination":
        stale.insert(dev(keys))
    stale.clear()
    torch.cuda.synchronize()
    col = dev(np.where(rng.random(max_rows) < 0.5, keys[rng.integers(0, 1000, max_rows)],
                       rng.integers(-(2**41), 2**41, max_rows)).astype(np.int64))
    d_sel = dev(rng.integers(0, max_rows, max_rows).astype(np.uint32))
    d_count = torch.tensor([used], dtype=torch.int64, device="cuda:0")
    out, cnt = GuardedBuffer(4 * max_rows).poison(FF), GuardedBuffer(8).poison(FF)
    kw = dict(range_mask=1, max_rows=max_rows, out_sel=out.view(torch.int32), out_count=cnt.view(torch.int64))
    if call == "transfer_insert_sel_range_ws":
        kw["workspace"] = torch.empty(rpt.probe_chain_sel_workspace_bytes([probed], max_rows), dtype=torch.uint8,
                                      device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)

    def caught():
        try:
            getattr(rpt, call)([probed], [col], [dst], [col], d_sel, d_count, stream=s, **kw)
        except rpt.RptError as e:
            return e
        return None

    graph = ctypes.c_void_p()
    end, err = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, caught)
    assert end == 0
    assert err is not None and err.status == 1 and "rpt_bf_settle" in str(err)
    assert graph_node_count(graph) == 0
    assert hip_graph_api().hipGraphDestroy(graph) == 0
    assert dst.is_empty()  # a refused call has not marked the destination either
    s.synchronize()
    assert int(cnt.view(torch.int64).item()) == -1 and bool(torch.all(out.view(torch.int32) == -1))
    assert caught() is None  # outside a capture the clear is settled
    s.synchronize()
    got = int(cnt.view(torch.int64).item())
    assert (got == 0) == (cleared == "probed")  # nothing passes the cleared (now settled, empty) probed filter
    assert not dst.is_empty()
    for name, gb in (("out_sel", out), ("out_count", cnt)):
        gb.assert_guards_intact(name)
    probed.close()
    dst.close()
