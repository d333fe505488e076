"""The eleven chain and transfer entry points as one family, on the GPU: the refusals that need a look into a real
filter, one table over every call that takes them (tests/test_chain_family_abi.py has the ones that need none):
    a workspace one byte short            RPT_ERR_WORKSPACE           the nine calls with a chain workspace
    a workspace at base + 8               RPT_ERR_INVALID_ARGUMENT    the same nine
    a forced strategy the filter size     RPT_ERR_INVALID_ARGUMENT    the row-list calls, plain and range (a device-counted
      does not support                                                chain runs a forced PARTITIONED as GATHER)
    a bad key type on a destination       RPT_ERR_INVALID_ARGUMENT    the eight transfers
    a routed destination whose insert     RPT_ERR_WORKSPACE           the three transfer_insert calls
      workspace is one byte short
After every refused call no kernel was recorded, the sentinels in out_count and out_sel[0] are untouched, and every
destination's words and has_data are what they were. A refusal returns on the host before anything is enqueued.

Shapes: 513 rows (two 512-row segments, the second holding one row), int64 keys, filters of 2^10 blocks; the routed
destination is the smallest filter the PARTITIONED strategy accepts, forced to RPT_INSERT_PARTITIONED."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 513
LOG_NB = 10
RPT_ERR_INVALID_ARGUMENT, RPT_ERR_WORKSPACE = 1, 4
SENTINEL32, SENTINEL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

# name -> (has destinations, has an insert workspace, device-counted, has a range mask, has a chain workspace)
CALLS = {
    "probe_chain_ws": (False, False, False, False, True),
    "transfer_ws": (True, False, False, False, True),
    "transfer_insert_ws": (True, True, False, False, True),
    "probe_chain_sel_ws": (False, False, True, False, True),
    "transfer_sel_ws": (True, False, True, False, True),
    "transfer_insert_sel_ws": (True, True, True, False, True),
    "probe_chain_sel": (False, False, True, False, False),
    "transfer_sel": (True, False, True, False, False),
    "probe_chain_range_ws": (False, False, False, True, True),
    "transfer_range_ws": (True, False, False, True, True),
    "transfer_insert_range_ws": (True, True, False, True, True),
}
WITH_WORKSPACE = [c for c, s in CALLS.items() if s[4]]
WITH_STRATEGIES = [c for c, s in CALLS.items() if s[4] and not s[2]]
TRANSFERS = [c for c, s in CALLS.items() if s[0]]
ROUTED = [c for c, s in CALLS.items() if s[1]]


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd
    from rpt_amd import _lib

    rpt_amd.load()
    torch.cuda.set_device(0)
    _lib.profiling(True)
    yield rpt_amd
    _lib.profiling(False)


class Env:
    """Two probed filters, two destinations (one holding keys, one fresh), a routed destination, and bitwise copies of
    the three destinations, all made once: no refused call may change any of them."""

    def __init__(self, rpt):
        dev = "cuda:0"
        g = torch.Generator().manual_seed(7)
        self.keys = torch.randint(-2**40, 2**40, (N,), dtype=torch.int64, generator=g).to(dev)
        self.dst_keys = torch.randint(-2**40, 2**40, (N,), dtype=torch.int64, generator=g).to(dev)
        self.filters = [rpt.BloomFilter(log_num_blocks=LOG_NB, device=dev) for _ in range(2)]
        for bf in self.filters:
            bf.insert(self.keys[::2].contiguous())
        self.dsts = [rpt.BloomFilter(log_num_blocks=LOG_NB, device=dev) for _ in range(2)]
        self.dsts[0].insert(self.dst_keys[:100].contiguous())
        lib = rpt.load()
        self.routed_log = next(L for L in range(41) if lib.rpt_probe_strategy_supported(rpt.RPT_PROBE_PARTITIONED, L))
        self.routed = rpt.BloomFilter(log_num_blocks=self.routed_log, device=dev)
        self.routed.insert(self.dst_keys[:100].contiguous())
        assert lib.rpt_bf_set_insert_strategy(self.routed.handle, rpt.RPT_INSERT_PARTITIONED) == 0
        assert self.routed.insert_strategy_for(N) == rpt.RPT_INSERT_PARTITIONED
        self.watched = self.dsts + [self.routed]
        self.copies = []
        for bf in self.watched:
            copy = rpt.BloomFilter(log_num_blocks=bf.log_num_blocks, device=dev)
            copy.import_words(bf.export_words())
            self.copies.append(copy)
        self.has_data = [not bf.is_empty() for bf in self.watched]
        assert self.has_data == [True, False, True]
        self.sel = torch.arange(N, dtype=torch.int32, device=dev)
        self.count = torch.tensor([N], dtype=torch.int64, device=dev)
        self.out_sel = torch.empty(N, dtype=torch.int32, device=dev)
        self.out_count = torch.empty(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def close(self):
        for bf in self.filters + self.watched + self.copies:
            bf.close()


@pytest.fixture(scope="module")
def env(rpt):
    e = Env(rpt)
    yield e
    e.close()


def chain_workspace_bytes(rpt, env, name):
    counted, mask = CALLS[name][2], CALLS[name][3]
    if counted:
        return rpt.probe_chain_sel_workspace_bytes(env.filters, N)
    if mask:
        return rpt.probe_chain_range_workspace_bytes(env.filters, 1, N)
    return rpt.probe_chain_workspace_bytes(env.filters, N)


def refused(rpt, env, name, status, text, *, workspace=None, insert_workspace=None, dsts=None, dst_columns=None):
    """Make the call with one thing wrong and assert the refusal and everything it must leave alone."""
    from rpt_amd import _lib

    has_dst, has_iws, counted, mask, has_ws = CALLS[name]
    dsts = env.dsts if dsts is None else dsts
    args = [env.filters, [env.keys, env.keys]]
    if has_dst:
        args += [dsts, [env.dst_keys] * len(dsts) if dst_columns is None else dst_columns]
    if counted:
        args += [env.sel, env.count]
    kw = dict(out_sel=env.out_sel, out_count=env.out_count)
    if not counted:
        kw["n"] = N
    if mask:
        kw["range_mask"] = 1
    if has_ws:
        kw["workspace"] = (torch.empty(chain_workspace_bytes(rpt, env, name), dtype=torch.uint8, device="cuda:0")
                           if workspace is None else workspace)
    if has_iws and insert_workspace is not None:
        kw["insert_workspace"] = insert_workspace
    env.out_sel.fill_(SENTINEL32)
    env.out_count.fill_(SENTINEL64)
    torch.cuda.synchronize()
    _lib.profiling_reset()
    with pytest.raises(rpt.RptError) as e:
        getattr(rpt, name)(*args, **kw)
    assert e.value.status == status, e.value
    assert text in str(e.value), e.value
    torch.cuda.synchronize()
    assert _lib.kernel_times() == {}
    assert int(env.out_count.item()) == SENTINEL64
    assert int(env.out_sel[0].item()) == SENTINEL32
    for bf, copy, had in zip(env.watched, env.copies, env.has_data):
        assert bf.is_same_as(copy)
        assert (not bf.is_empty()) == had


@pytest.mark.parametrize("name", WITH_WORKSPACE)
def test_a_workspace_one_byte_short_is_refused(rpt, env, name):
    need = chain_workspace_bytes(rpt, env, name)
    assert need > 1
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda:0")
    refused(rpt, env, name, RPT_ERR_WORKSPACE, "workspace %d bytes < required %d" % (need - 1, need), workspace=short)


@pytest.mark.parametrize("name", WITH_WORKSPACE)
def test_a_workspace_at_base_plus_8_is_refused(rpt, env, name):
    need = chain_workspace_bytes(rpt, env, name)
    base = torch.empty(need + 16, dtype=torch.uint8, device="cuda:0")
    assert base.data_ptr() % 16 == 0
    refused(rpt, env, name, RPT_ERR_INVALID_ARGUMENT, "is not 16-byte aligned", workspace=base[8:])


@pytest.mark.parametrize("name", WITH_STRATEGIES)
def test_a_forced_strategy_the_filter_size_does_not_support_is_refused(rpt, env, name):
    assert not rpt.load().rpt_probe_strategy_supported(rpt.RPT_PROBE_PARTITIONED, LOG_NB)
    big = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")  # the size cannot be asked for: it is the refusal
    env.filters[1].probe_strategy = rpt.RPT_PROBE_PARTITIONED
    try:
        refused(rpt, env, name, RPT_ERR_INVALID_ARGUMENT,
                "probe strategy %d unsupported for a 2^%d-block filter (filter 1)" % (rpt.RPT_PROBE_PARTITIONED, LOG_NB),
                workspace=big)
    finally:
        env.filters[1].probe_strategy = rpt.RPT_PROBE_AUTO


@pytest.mark.parametrize("name", TRANSFERS)
def test_a_bad_key_type_on_a_destination_column_is_refused(rpt, env, name):
    refused(rpt, env, name, RPT_ERR_INVALID_ARGUMENT, "bad key_type 7",
            dst_columns=[env.dst_keys, {"keys": env.dst_keys, "key_type": 7}])


@pytest.mark.parametrize("name", ROUTED)
def test_a_routed_destination_with_a_short_insert_workspace_is_refused(rpt, env, name):
    need = rpt.transfer_insert_workspace_bytes([env.dsts[0], env.routed], N)
    assert need > 1
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda:0")
    refused(rpt, env, name, RPT_ERR_WORKSPACE, "workspace %d bytes < required %d" % (need - 1, need),
            dsts=[env.dsts[0], env.routed], insert_workspace=short)
