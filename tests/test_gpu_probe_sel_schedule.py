"""A whole forward-and-backward predicate-transfer schedule over three tables as ONE captured graph, which is what the
device-counted probes exist for: the second probe of a table takes its rows from the first probe's out_sel and count,
still on the device.

  tables    A: a dimension of 3001 rows (key), of which a local predicate keeps some (they build F_A, outside the graph)
            B: a fact table of 40003 rows with key columns a_id and c_id
            C: a dimension of 20011 rows (key), of which a local predicate keeps half (a host-known row_sel)
  forward   B is probed by F_A and its survivors go into F_BC on c_id        rpt_bf_transfer_ws
            C's kept rows are probed by F_BC                                 rpt_bf_probe_chain_ws
  backward  C's survivors go into G_C                                        rpt_bf_insert_sel
            B's survivors (sel and count on the device) are probed by G_C
            and what is left goes into G_BA on a_id                          rpt_bf_transfer_sel_ws
            A is probed by G_BA                                              rpt_bf_probe_chain_ws

All on one stream, captured under hipStreamCaptureModeGlobal: a synchronize, an allocation or a copy to the host inside
the capture would invalidate it. Every filter's words and every table's final selection equal the oracle's replay of
the same schedule, eagerly and after each of two graph replays between which B's keys are rewritten on the device."""
import ctypes

import numpy as np
import pytest
import torch

import rpt_oracle as orc
from buf_util import CAPTURE_MODE_GLOBAL, FF, GuardedBuffer, graph_destroy, graph_instantiate, graph_launch, stream_capture
from test_gpu_transfer import dev, sel_of

pytestmark = pytest.mark.gpu

N_A, N_B, N_C = 3001, 40003, 20011
LOG_FA, LOG_FBC, LOG_GC, LOG_GBA = 11, 15, 14, 12


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


def oracle_schedule(fa_words, a_key, b_a_id, b_c_id, c_key, c_kept):
    """The schedule on the host: every built filter's words and every table's final selection."""
    sel_b = orc.probe_keys(fa_words, LOG_FA, b_a_id).astype(np.uint32)
    f_bc = orc.new_words(LOG_FBC)
    orc.insert_keys(f_bc, LOG_FBC, b_c_id, key_sel=sel_b)
    sel_c = c_kept[orc.probe_keys(f_bc, LOG_FBC, c_key, key_sel=c_kept)]
    g_c = orc.new_words(LOG_GC)
    orc.insert_keys(g_c, LOG_GC, c_key, key_sel=sel_c)
    sel_b2 = sel_b[orc.probe_keys(g_c, LOG_GC, b_c_id, key_sel=sel_b)]
    g_ba = orc.new_words(LOG_GBA)
    orc.insert_keys(g_ba, LOG_GBA, b_a_id, key_sel=sel_b2)
    sel_a = orc.probe_keys(g_ba, LOG_GBA, a_key).astype(np.uint32)
    return dict(f_bc=f_bc, g_c=g_c, g_ba=g_ba, sel_b=sel_b, sel_c=sel_c, sel_b2=sel_b2, sel_a=sel_a)


def raw_chain_ws(rpt, bf, keys, row_sel, n, out_sel, out_count, ws, stream_handle):
    """rpt_bf_probe_chain_ws through ctypes: nothing but the call (the Python wrapper reads the count back)."""
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * 1)(bf.handle)
    arr = (KeyColumn * 1)(rpt.make_column(keys))
    st = rpt.load().rpt_bf_probe_chain_ws(handles, arr, 1, None if row_sel is None else row_sel.data_ptr(), n,
                                          out_sel.data_ptr(), out_count.data_ptr(), ws.data_ptr(), ws.numel(),
                                          stream_handle)
    assert st == 0, rpt.load().rpt_last_error()


def test_forward_and_backward_schedule_is_one_graph(rpt):
    rng = np.random.default_rng(2024)
    a_key = rng.permutation(np.arange(10**6, 10**6 + N_A, dtype=np.int64))
    c_key = rng.permutation(np.arange(5 * 10**6, 5 * 10**6 + N_C, dtype=np.int64))
    a_kept = np.flatnonzero(rng.random(N_A) < 0.3).astype(np.uint32)  # A's local predicate: builds F_A
    c_kept = np.flatnonzero(rng.random(N_C) < 0.5).astype(np.uint32)  # C's local predicate: a host-known row_sel

    def fact_keys(hit):
        """B's key columns: a_id mostly in A (a fraction `hit`), c_id in C."""
        a_id = np.where(rng.random(N_B) < hit, a_key[rng.integers(0, N_A, N_B)], rng.integers(0, 10**5, N_B))
        return a_id.astype(np.int64), c_key[rng.integers(0, N_C, N_B)]

    fa_words = orc.new_words(LOG_FA)
    orc.insert_keys(fa_words, LOG_FA, a_key, key_sel=a_kept)
    f_a = rpt.BloomFilter(log_num_blocks=LOG_FA)
    f_a.insert(dev(a_key[a_kept]))
    assert np.array_equal(f_a.export_words(), fa_words)
    f_bc, g_c, g_ba = (rpt.BloomFilter(log_num_blocks=L) for L in (LOG_FBC, LOG_GC, LOG_GBA))
    built = {"f_bc": f_bc, "g_c": g_c, "g_ba": g_ba}

    b_a_id, b_c_id = (dev(k) for k in fact_keys(0.9))
    d_a_key, d_c_key, d_c_kept = dev(a_key), dev(c_key), dev(c_kept)
    # every buffer of the schedule, allocated before the capture
    sel_b, cnt_b = GuardedBuffer(4 * N_B).poison(FF), GuardedBuffer(8).poison(FF)
    sel_b2, cnt_b2 = GuardedBuffer(4 * N_B).poison(FF), GuardedBuffer(8).poison(FF)
    sel_c, cnt_c = GuardedBuffer(4 * c_kept.size).poison(FF), GuardedBuffer(8).poison(FF)
    sel_a, cnt_a = GuardedBuffer(4 * N_A).poison(FF), GuardedBuffer(8).poison(FF)
    ws_b = GuardedBuffer(rpt.probe_chain_workspace_bytes([f_a], N_B)).poison(FF)
    ws_c = GuardedBuffer(rpt.probe_chain_workspace_bytes([f_bc], c_kept.size)).poison(FF)
    ws_b2 = GuardedBuffer(rpt.probe_chain_sel_workspace_bytes([g_c], N_B)).poison(FF)
    ws_a = GuardedBuffer(rpt.probe_chain_workspace_bytes([g_ba], N_A)).poison(FF)
    guarded = dict(sel_b=sel_b, cnt_b=cnt_b, sel_b2=sel_b2, cnt_b2=cnt_b2, sel_c=sel_c, cnt_c=cnt_c, sel_a=sel_a,
                   cnt_a=cnt_a, ws_b=ws_b, ws_c=ws_c, ws_b2=ws_b2, ws_a=ws_a)
    i32, i64 = torch.int32, torch.int64

    def schedule(stream):
        sh = ctypes.c_void_p(stream.cuda_stream)
        # forward
        rpt.transfer_ws([f_a], [b_a_id], [f_bc], [b_c_id], n=N_B, out_sel=sel_b.view(i32), out_count=cnt_b.view(i64),
                        workspace=ws_b.bytes(), stream=stream)
        raw_chain_ws(rpt, f_bc, d_c_key, d_c_kept, c_kept.size, sel_c.view(i32), cnt_c.view(i64), ws_c.bytes(), sh)
        # backward
        g_c.insert_sel(d_c_key, sel_c.view(i32), cnt_c.view(i64), stream=stream)
        rpt.transfer_sel_ws([g_c], [b_c_id], [g_ba], [b_a_id], sel_b.view(i32), cnt_b.view(i64), out_sel=sel_b2.view(i32),
                            out_count=cnt_b2.view(i64), workspace=ws_b2.bytes(), stream=stream)
        raw_chain_ws(rpt, g_ba, d_a_key, None, N_A, sel_a.view(i32), cnt_a.view(i64), ws_a.bytes(), sh)

    def check_against_oracle(what):
        exp = oracle_schedule(fa_words, a_key, b_a_id.cpu().numpy(), b_c_id.cpu().numpy(), c_key, c_kept)
        for name, bf in built.items():
            assert np.array_equal(bf.export_words(), exp[name]), f"{what}: {name} differs from the oracle"
        for name, sel, cnt in (("sel_b", sel_b, cnt_b), ("sel_c", sel_c, cnt_c), ("sel_b2", sel_b2, cnt_b2),
                               ("sel_a", sel_a, cnt_a)):
            got = int(cnt.view(i64).item())
            assert got == exp[name].size, f"{what}: {name} count {got}, oracle {exp[name].size}"
            assert np.array_equal(sel_of(sel.view(i32)[:got]), exp[name]), f"{what}: {name}"
        for name, g in guarded.items():
            g.assert_guards_intact(name)
        # the schedule reduces every table, and the backward pass reduces B further
        assert 0 < exp["sel_a"].size < N_A and 0 < exp["sel_c"].size < c_kept.size
        assert 0 < exp["sel_b2"].size < exp["sel_b"].size < N_B
        return {k: v.size for k, v in exp.items() if k.startswith("sel")}

    def reset_built():
        """Outside any capture: the built filters empty again, their deferred clears settled. On the current stream, not
        the one captured below (as tests/test_gpu_transfer.py's captured transfer does): the capture asks whether a
        filter's previous write has completed by querying the event recorded on that write's stream."""
        for bf in built.values():
            bf.clear()
            bf.settle()
        for g in (sel_b, cnt_b, sel_b2, cnt_b2, sel_c, cnt_c, sel_a, cnt_a):
            g.poison(FF)
        torch.cuda.synchronize()

    # eagerly, on the current stream (a kernel's first launch may set its LDS allowance outside any capture)
    schedule(torch.cuda.current_stream())
    torch.cuda.synchronize()
    counts = [check_against_oracle("eager")]

    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    reset_built()
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, _none = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, lambda: schedule(s))
    assert end == 0, "the capture was invalidated: something in the schedule synchronized, allocated or copied back"
    assert graph_instantiate(graph, exe) == 0
    for name, bf in built.items():  # capturing ran nothing
        assert not bf.export_words().any(), name
    for replay, hit in enumerate((0.9, 0.5)):
        if replay:
            new_a_id, new_c_id = fact_keys(hit)
            b_a_id.copy_(dev(new_a_id))
            b_c_id.copy_(dev(new_c_id))
            reset_built()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        counts.append(check_against_oracle(f"replay {replay}"))
    assert counts[0] == counts[1] != counts[2]  # the same keys eagerly and replayed; other keys, other counts
    assert graph_destroy(exe, graph)
    for bf in (f_a, f_bc, g_c, g_ba):
        bf.close()
