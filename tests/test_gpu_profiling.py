"""The kernel timing API (rpt_profiling_enable / reset / read) itself: what is recorded and when, the capacity
contract of rpt_profiling_read, calls from two streams and two host threads, and stream capture (a captured launch and
its replays stay out of the record, and the record stays readable). bench.py matches its PMC records by these names
and tests/test_gpu_kernel_ledger.py reads which kernel ran through this API.

No time is asserted beyond finite and > 0."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import kernel_ledger as kl
import rpt_oracle as orc
from buf_util import (CAPTURE_MODE_GLOBAL, FilterCache, graph_destroy, graph_instantiate, graph_launch,
                      stream_capture)

pytestmark = pytest.mark.gpu

N = 40003
GATHER_PROBE = {kl.inst("probe_bits_kernel", kl.KEYS["i64"], True, False, kl.BLOCK_THREADS): 1, "group_sum_kernel": 1,
                "group_scan_kernel": 1, "compact_kernel": 1}


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def plib(rpt):
    from rpt_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def caches(rpt):
    a, b = FilterCache(), FilterCache()
    yield a, b
    a.close()
    b.close()


@pytest.fixture(autouse=True)
def profiling_clean(plib):
    """Profiling is process-wide: every test starts from, and leaves, a disabled and empty record (failure included)."""
    torch.cuda.synchronize()
    plib.profiling(False)
    plib.profiling_reset()
    yield
    torch.cuda.synchronize()
    plib.profiling(False)
    plib.profiling_reset()


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def probe_keys_for(build, n, seed):
    rng = np.random.default_rng(seed)
    miss = rng.integers(-(2**62), 2**62, size=n, dtype=np.int64)
    return np.where(rng.random(n) < 0.5, build[rng.integers(0, build.size, n)], miss)


class Probe:
    """One rpt_bf_probe of N dense int64 keys against the shared 2^16-block filter with GATHER forced, through ctypes
    with buffers of its own (so several can be in flight), and the oracle's answer."""

    def __init__(self, rpt, caches, seed, stream=None):
        self.rpt, self.lib = rpt, rpt.load()
        self.bf, words, build = caches[0].get(16)
        self.bf.probe_strategy = kl.GATHER
        keys = probe_keys_for(build, N, seed)
        self.ref = orc.probe_keys(words, 16, keys)
        self.d_keys = dev(keys)
        self.col = rpt.make_column(self.d_keys)
        self.out_sel = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
        self.out_count = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
        self.ws = torch.empty(self.bf.workspace_bytes(N), dtype=torch.uint8, device="cuda:0")
        self.stream = stream
        self.handle = ctypes.c_void_p(stream.cuda_stream if stream is not None else 0)
        torch.cuda.synchronize()

    def __call__(self):
        st = self.lib.rpt_bf_probe(self.bf.handle, ctypes.byref(self.col), None, N, self.out_sel.data_ptr(),
                                   self.out_count.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.handle)
        assert st == 0, self.lib.rpt_last_error()

    def check(self):
        torch.cuda.synchronize()
        assert int(self.out_count.item()) == self.ref.size
        assert np.array_equal(self.out_sel[: self.ref.size].cpu().numpy().view(np.uint32), self.ref)


def launches(plib):
    return {name: n for name, (n, _ms) in plib.kernel_times().items()}


def times(k, expected):
    return {name: k * n for name, n in expected.items()}


def test_nothing_is_recorded_while_disabled(rpt, plib, caches):
    probe = Probe(rpt, caches, 1)
    probe()
    bf = rpt.BloomFilter(log_num_blocks=10)
    bf.insert(probe.d_keys, strategy=kl.INS_ATOMIC)
    probe.check()
    assert plib.load().rpt_profiling_read(None, 0) == 0
    assert plib.kernel_times() == {}
    bf.close()


def test_one_probe_records_its_four_kernels_once(rpt, plib, caches):
    probe = Probe(rpt, caches, 2)
    plib.profiling(True)
    probe()
    probe.check()
    got = plib.kernel_times()
    assert kl.kernel_set_problems(GATHER_PROBE, got) == []
    for name, (_n, ms) in got.items():
        assert np.isfinite(ms) and ms > 0, name


def test_accumulation_reset_and_disable(rpt, plib, caches):
    probe = Probe(rpt, caches, 3)
    plib.profiling(True)
    k = 3
    for _ in range(k):
        probe()
    probe.check()
    assert launches(plib) == times(k, GATHER_PROBE)
    assert launches(plib) == times(k, GATHER_PROBE)  # reading consumes nothing
    probe()
    torch.cuda.synchronize()
    assert launches(plib) == times(k + 1, GATHER_PROBE)
    # disabling stops the recording and keeps what was recorded
    plib.profiling(False)
    probe()
    probe.check()
    assert launches(plib) == times(k + 1, GATHER_PROBE)
    # a reset empties the record, pending launches included
    plib.profiling(True)
    probe()
    plib.profiling_reset()
    assert plib.load().rpt_profiling_read(None, 0) == 0
    probe()
    torch.cuda.synchronize()
    assert launches(plib) == GATHER_PROBE
    plib.profiling(False)
    plib.profiling_reset()
    assert plib.kernel_times() == {}


def test_read_capacity(rpt, plib, caches):
    lib = plib.load()
    probe = Probe(rpt, caches, 4)
    plib.profiling(True)
    probe()
    probe()
    torch.cuda.synchronize()
    plib.profiling(False)
    total = len(GATHER_PROBE)
    assert lib.rpt_profiling_read(None, 0) == total
    assert lib.rpt_profiling_read(None, 100) == total  # no buffer: only the count
    full = (plib.KernelStat * total)()
    assert lib.rpt_profiling_read(full, total) == total
    assert {s.name.decode(): s.launches for s in full} == times(2, GATHER_PROBE)
    # a smaller capacity fills only that many entries, in the same order, and still returns the full count
    for capacity in (0, 1, total - 1):
        arr = (plib.KernelStat * (total + 2))()
        ctypes.memset(arr, 0xAB, ctypes.sizeof(arr))
        sentinel = bytes(arr)[: ctypes.sizeof(plib.KernelStat)]
        assert lib.rpt_profiling_read(arr, capacity) == total
        raw = bytes(arr)
        size = ctypes.sizeof(plib.KernelStat)
        for i in range(total + 2):
            entry = raw[i * size: (i + 1) * size]
            if i < capacity:
                assert arr[i].name == full[i].name and arr[i].launches == full[i].launches == 2
                assert arr[i].total_ms == full[i].total_ms
            else:
                assert entry == sentinel, "entry %d behind capacity %d was written" % (i, capacity)
    # names are NUL-terminated inside their 48 bytes
    assert all(len(s.name) < kl.NAME_BYTES for s in full)


def test_two_streams_are_both_counted(rpt, plib, caches):
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    a, b = Probe(rpt, caches, 5, s1), Probe(rpt, caches, 6, s2)
    plib.profiling(True)
    for _ in range(2):
        a()
        b()
    a.check()
    b.check()
    assert launches(plib) == times(4, GATHER_PROBE)


def test_two_host_threads_give_exact_counts(rpt, plib, caches):
    per_thread = 25
    probes = [Probe(rpt, caches, 7 + i, torch.cuda.Stream(device="cuda:0")) for i in range(2)]
    errors = []
    start = threading.Barrier(2)

    def work(p):
        try:
            start.wait()
            for _ in range(per_thread):
                p()
            p.stream.synchronize()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    plib.profiling(True)
    threads = [threading.Thread(target=work, args=(p,)) for p in probes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for p in probes:
        p.check()
    assert launches(plib) == times(2 * per_thread, GATHER_PROBE)


def chain_call(rpt, filters, cols, n, out_sel, out_count, ws, stream_handle):
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * len(filters))(*[f.handle for f in filters])
    arr = (KeyColumn * len(cols))(*cols)
    return rpt.load().rpt_bf_probe_chain_ws(handles, arr, len(filters), None, n, out_sel.data_ptr(),
                                            out_count.data_ptr(), ws.data_ptr(), ws.numel(), stream_handle)


def test_captured_launches_stay_out_of_the_record(rpt, plib, caches):
    """rpt_bf_probe_chain_ws (an LDS stage, then a masked gather stage) with profiling enabled: eagerly once, then
    captured on a side stream under hipStreamCaptureModeGlobal and replayed twice with other keys in place, then
    eagerly again. The capture succeeds, the replays match the oracle, and the record holds the two eager calls only."""
    n = N
    f0, w0, b0 = caches[0].get(13)
    f1, w1, b1 = caches[1].get(16)
    f0.probe_strategy = kl.LDS
    f1.probe_strategy = kl.GATHER
    eager = {kl.inst("probe_bits_kernel", kl.KEYS["i64"], True, True, kl.LDS_THREADS): 1,
             kl.inst("probe_bits_masked_kernel", kl.KEYS["i64"], True, False, kl.BLOCK_THREADS): 1,
             "group_sum_kernel": 1, "group_scan_kernel": 1, "compact_kernel": 1}
    k0, k1 = dev(probe_keys_for(b0, n, 20)), dev(probe_keys_for(b1, n, 21))
    cols = [rpt.make_column(k0), rpt.make_column(k1)]
    out_sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(rpt.probe_chain_workspace_bytes([f0, f1], n), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)

    def check_result(what):
        s.synchronize()
        exp = np.intersect1d(orc.probe_keys(w0, 13, k0.cpu().numpy()),
                             orc.probe_keys(w1, 16, k1.cpu().numpy())).astype(np.uint32)
        assert 0 < exp.size < n
        assert int(out_count.item()) == exp.size, what
        assert np.array_equal(out_sel[: exp.size].cpu().numpy().view(np.uint32), exp), what

    torch.cuda.synchronize()
    plib.profiling(True)
    assert chain_call(rpt, [f0, f1], cols, n, out_sel, out_count, ws, sh) == 0, rpt.load().rpt_last_error()
    check_result("eager")
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph,
                             lambda: chain_call(rpt, [f0, f1], cols, n, out_sel, out_count, ws, sh))
    assert end == 0 and st == 0, rpt.load().rpt_last_error()
    assert graph_instantiate(graph, exe) == 0
    for replay in range(2):
        k0.copy_(dev(probe_keys_for(b0, n, 30 + replay)))
        k1.copy_(dev(probe_keys_for(b1, n, 40 + replay)))
        out_sel.fill_(-1)
        out_count.fill_(-1)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        check_result("replay %d" % replay)
    assert plib.load().rpt_profiling_read(None, 0) >= 0
    assert launches(plib) == eager
    assert chain_call(rpt, [f0, f1], cols, n, out_sel, out_count, ws, sh) == 0, rpt.load().rpt_last_error()
    check_result("eager again")
    got = plib.kernel_times()
    assert {name: c for name, (c, _ms) in got.items()} == times(2, eager)
    assert all(np.isfinite(ms) and ms > 0 for _c, ms in got.values())
    assert graph_destroy(exe, graph)
    f0.probe_strategy = kl.AUTO
    f1.probe_strategy = kl.AUTO
