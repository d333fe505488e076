"""The eleven chain and transfer entry points as one family, without a GPU: one table of the argument faults that need
no look into a handle, run against every call that can have them. Each fault alone gives its status and message, and of
two faults in one call the earlier check wins; which one is earlier was recorded from the library before the calls were
given one shared body, so the table is the specification of every family's check order. The per-family files
(test_chain_ws_abi.py, test_transfer_abi.py, test_probe_sel_abi.py, test_probe_sel_small_abi.py,
test_probe_range_abi.py) keep their own cases. The handles and device pointers here are made-up values: no case may
reach a check that looks into one."""
import ctypes

import pytest

from rpt_amd import _lib

BF, BF2, BF3, DST = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000, 0x7F0000040000  # "filters"
KEYS, SEL, COUNT = 0x7F0000100000, 0x7F0000300000, 0x7F0000400000  # "device memory", 16-byte aligned
OUT_SEL, OUT_COUNT, WS, IWS = 0x7F0000500000, 0x7F0000600000, 0x7F0000700000, 0x7F0000800000
INVALID = _lib.RPT_ERR_INVALID_ARGUMENT
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS


class Call:
    """One entry point: which argument groups its signature has."""

    def __init__(self, name, dst=False, insert_ws=False, counted=False, mask=False, ws=True):
        self.name, self.dst, self.insert_ws, self.counted, self.mask, self.ws = name, dst, insert_ws, counted, mask, ws
        # the row bound that is checked before a handle is looked into (the row-list calls check n after the handles)
        self.row_bound = None if not counted else (2**32 if ws else SMALL_ROWS + 1)
        self.bound_text = b"exceeds uint32 sel_t" if ws else b"exceeds RPT_SMALL_PROBE_ROWS"

    def __repr__(self):
        return self.name

    def __call__(self, lib, **over):
        a = dict(filters=handles(BF), cols=columns(1), k=1, mask=1, dst=handles(DST), dst_cols=columns(1), n_dst=1,
                 sel=SEL if self.counted else None, count=COUNT, n=1000, out_sel=OUT_SEL, out_count=OUT_COUNT)
        assert set(over) <= set(a), over
        a.update(over)
        args = [a["filters"], a["cols"], a["k"]]
        if self.mask:
            args.append(a["mask"])
        if self.dst:
            args += [a["dst"], a["dst_cols"], a["n_dst"]]
        args += [a["sel"], a["count"], a["n"]] if self.counted else [a["sel"], a["n"]]
        args += [a["out_sel"], a["out_count"]]
        if self.ws:
            args += [WS, 1 << 20]
        if self.insert_ws:
            args += [IWS, 1 << 20]
        return getattr(lib, self.name)(*args, None)


CALLS = (
    Call("rpt_bf_probe_chain_ws"),
    Call("rpt_bf_transfer_ws", dst=True),
    Call("rpt_bf_transfer_insert_ws", dst=True, insert_ws=True),
    Call("rpt_bf_probe_chain_sel_ws", counted=True),
    Call("rpt_bf_transfer_sel_ws", dst=True, counted=True),
    Call("rpt_bf_transfer_insert_sel_ws", dst=True, insert_ws=True, counted=True),
    Call("rpt_bf_probe_chain_sel", counted=True, ws=False),
    Call("rpt_bf_transfer_sel", dst=True, counted=True, ws=False),
    Call("rpt_bf_probe_chain_range_ws", mask=True),
    Call("rpt_bf_transfer_range_ws", dst=True, mask=True),
    Call("rpt_bf_transfer_insert_range_ws", dst=True, insert_ws=True, mask=True),
)


def handles(*values):
    return (ctypes.c_void_p * len(values))(*values)


def columns(k, hash_at=None, bad_at=None):
    def key_type(f):
        return 7 if f == bad_at else _lib.RPT_KEY_HASH if f == hash_at else _lib.RPT_KEY_I64

    return (_lib.KeyColumn * k)(*[_lib.KeyColumn(key_type(f), KEYS, None, None) for f in range(k)])


def three():
    return dict(filters=handles(BF, BF2, BF3), cols=columns(3), k=3)


def always(c):
    return True


def lists_first(c):
    """Does the call compare every handle before it looks into one? All but the plain chain (and the range chain with an
    empty mask, which is the plain chain): their first look at the handles is the device comparison, filter by filter."""
    return c.dst or c.counted or c.mask


# name -> (which calls can have the fault, the arguments that make it, the message it gives)
FAULTS = {
    "null filters": (always, lambda c: dict(filters=None), lambda c: b"null argument"),
    "null cols": (always, lambda c: dict(cols=None), lambda c: b"null argument"),
    "null out_count": (always, lambda c: dict(out_count=None), lambda c: b"null argument"),
    "null dst list": (lambda c: c.dst, lambda c: dict(dst=None), lambda c: b"null argument"),
    "null dst cols": (lambda c: c.dst, lambda c: dict(dst_cols=None), lambda c: b"null argument"),
    "no filter": (always, lambda c: dict(k=0), lambda c: b"n_filters=0 outside 1..8"),
    "nine filters": (always, lambda c: dict(filters=handles(*[BF] * 9), cols=columns(9), k=9),
                     lambda c: b"n_filters=9 outside 1..8"),
    "no dst": (lambda c: c.dst, lambda c: dict(n_dst=0), lambda c: b"n_dst=0 outside 1..8"),
    "nine dst": (lambda c: c.dst, lambda c: dict(dst=handles(*[DST + 4096 * j for j in range(9)]), dst_cols=columns(9),
                                                  n_dst=9), lambda c: b"n_dst=9 outside 1..8"),
    "null filter 0": (always, lambda c: dict(filters=handles(None)), lambda c: b"null filter 0"),
    "null filter 2": (lists_first, lambda c: dict(three(), filters=handles(BF, BF2, None)), lambda c: b"null filter 2"),
    "null dst 1": (lambda c: c.dst, lambda c: dict(dst=handles(DST, None), dst_cols=columns(2), n_dst=2),
                   lambda c: b"null destination filter 1"),
    "dst is probed": (lambda c: c.dst, lambda c: dict(three(), dst=handles(DST, BF3), dst_cols=columns(2), n_dst=2),
                      lambda c: b"destination filter 1 is probed filter 2 of the same call"),
    "null count_dev": (lambda c: c.counted, lambda c: dict(count=None), lambda c: b"null count_dev"),
    "rows past the bound": (lambda c: c.counted, lambda c: dict(n=c.row_bound), lambda c: c.bound_text),
    "rows far past the bound": (lambda c: c.counted, lambda c: dict(n=2**63), lambda c: c.bound_text),
    "null sel": (lambda c: c.counted, lambda c: dict(sel=None), lambda c: b"null sel"),
    "null out_sel": (lambda c: c.counted, lambda c: dict(out_sel=None), lambda c: b"null out_sel"),
    "out_sel overlaps sel": (lambda c: c.counted, lambda c: dict(out_sel=SEL + 4 * 999), lambda c: b"out_sel overlaps sel"),
    "mask bit above": (lambda c: c.mask, lambda c: dict(mask=0b10), lambda c: b"at or above n_filters=1"),
    "mask bit 31": (lambda c: c.mask, lambda c: dict(three(), mask=1 << 31), lambda c: b"at or above n_filters=3"),
    "bad key type": (lambda c: c.mask, lambda c: dict(three(), cols=columns(3, bad_at=2), mask=1), lambda c: b"bad key_type 7"),
    "flagged hash column": (lambda c: c.mask, lambda c: dict(three(), cols=columns(3, hash_at=1), mask=0b10),
                            lambda c: b"range_mask flags filter 1"),
}

# Two faults in one call: (which calls, the arguments, the fault that is reported). The arguments are written out where
# the two faults set the same argument; otherwise they are the two faults' own, merged.
PAIRS = (
    ("no filter", "no dst", "no filter"),
    ("null dst list", "no filter", "null dst list"),
    ("null out_count", "nine filters", "null out_count"),
    ("nine dst", "null filter 0", "nine dst"),
    ("no filter", "null count_dev", "no filter"),
    ("null filter 0", "null count_dev", "null filter 0"),
    ("null filter 2", "null count_dev", "null filter 2"),
    ("null dst 1", "null count_dev", "null dst 1"),
    ("dst is probed", "null count_dev", "dst is probed"),
    ("dst is probed", "rows past the bound", "dst is probed"),
    ("null count_dev", "rows past the bound", "null count_dev"),
    ("rows past the bound", "null sel", "rows past the bound"),
    ("rows past the bound", "null out_sel", "rows past the bound"),
    ("null sel", "null out_sel", "null sel"),
    ("null count_dev", "null sel", "null count_dev"),
    ("mask bit above", "no dst", "no dst"),
    ("mask bit above", "null dst 1", "null dst 1"),
    ("mask bit above", "null filter 0", "null filter 0"),
    ("mask bit above", "null cols", "null cols"),
    ("no filter", "mask bit above", "no filter"),
)
# ... and the pairs whose two faults share an argument
WRITTEN_OUT = (
    ("a null filter after a probed destination", lambda c: c.dst,
     lambda c: dict(filters=handles(BF, BF2, None), cols=columns(3), k=3, dst=handles(BF2), dst_cols=columns(1), n_dst=1),
     b"null filter 2"),
    ("a null destination after a probed one", lambda c: c.dst,
     lambda c: dict(dst=handles(BF, None), dst_cols=columns(2), n_dst=2), b"destination filter 0 is probed filter 0"),
    ("a null destination before a probed one", lambda c: c.dst,
     lambda c: dict(dst=handles(None, BF), dst_cols=columns(2), n_dst=2), b"null destination filter 0"),
    ("a mask bit above and a probed destination", lambda c: c.mask and c.dst,
     lambda c: dict(three(), mask=1 << 31, dst=handles(BF3)), b"destination filter 0 is probed filter 2"),
    ("a mask bit above and a flagged hash column", lambda c: c.mask,
     lambda c: dict(three(), cols=columns(3, hash_at=0), mask=0b1001), b"at or above n_filters=3"),
    ("a bad key type before a flagged hash column", lambda c: c.mask,
     lambda c: dict(three(), cols=columns(3, hash_at=1, bad_at=0), mask=0b10), b"bad key_type 7"),
    ("a flagged hash column before a bad key type", lambda c: c.mask,
     lambda c: dict(three(), cols=columns(3, hash_at=1, bad_at=2), mask=0b10), b"range_mask flags filter 1"),
    ("a bad key type on an unflagged column of a range call", lambda c: c.mask,
     lambda c: dict(three(), cols=columns(3, bad_at=0), mask=0b100), b"bad key_type 7"),
    ("a probed destination at zero rows", lambda c: c.dst,
     lambda c: dict(three(), dst=handles(BF3), n=0), b"destination filter 0 is probed filter 2"),
    ("a null count_dev at zero rows", lambda c: c.counted, lambda c: dict(count=None, n=0), b"null count_dev"),
    ("a mask bit above at zero rows", lambda c: c.mask, lambda c: dict(mask=0b10, n=0), b"at or above n_filters=1"),
)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, status, message, what):
    assert status == INVALID, (what, status, lib.rpt_last_error())
    assert message in lib.rpt_last_error(), (what, lib.rpt_last_error())


def test_the_table_covers_the_eleven_entry_points(lib):
    assert len(CALLS) == len({c.name for c in CALLS}) == 11
    for c in CALLS:
        assert hasattr(lib, c.name) and c.name in _lib.SIGNATURES, c.name
    assert lib.rpt_abi_version() == 1


@pytest.mark.parametrize("call", CALLS, ids=repr)
def test_each_fault_alone_is_refused_with_its_message(lib, call):
    seen = 0
    for name, (applies, make, message) in FAULTS.items():
        if applies(call):
            refused(lib, call(lib, **make(call)), message(call), name)
            seen += 1
    assert seen >= 6  # every call has the faults of its probed list at least


@pytest.mark.parametrize("call", CALLS, ids=repr)
def test_of_two_faults_the_earlier_check_wins(lib, call):
    for first, second, winner in PAIRS:
        if not (FAULTS[first][0](call) and FAULTS[second][0](call)):
            continue
        a, b = FAULTS[first][1](call), FAULTS[second][1](call)
        assert not set(a) & set(b), (first, second)  # such a pair belongs in WRITTEN_OUT
        refused(lib, call(lib, **a, **b), FAULTS[winner][2](call), (first, second))
    for what, applies, make, message in WRITTEN_OUT:
        if applies(call):
            refused(lib, call(lib, **make(call)), message, what)


def test_an_empty_mask_is_the_plain_twin(lib):
    """range_mask == 0: no mask fault can be reported, and the lists are checked as the plain call checks them."""
    for call in CALLS:
        if not call.mask:
            continue
        refused(lib, call(lib, mask=0, filters=None), b"null argument", call)
        refused(lib, call(lib, mask=0, k=9), b"n_filters=9 outside 1..8", call)
        refused(lib, call(lib, mask=0, filters=handles(None)), b"null filter 0", call)
        if call.dst:
            refused(lib, call(lib, mask=0, **FAULTS["dst is probed"][1](call)),
                    b"destination filter 1 is probed filter 2 of the same call", call)
