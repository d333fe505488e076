"""Device-side transfer (rpt_bf_insert_bits, rpt_bf_insert_sel, rpt_bf_transfer_ws) vs the oracle, bit-exact: after
a call the filter's words are a copy of its words before the call plus orc.insert_keys of exactly the selected rows,
and its min/max is orc.minmax over the selected valid rows.

Destination filters are made once per (size, empty / pre-filled) and put back to their known words before every
use; the probed filters of the transfer tests come from buf_util.FilterCache and are never inserted into."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import golden_util as gu
import rpt_oracle as orc
from buf_util import (A5, CAPTURE_MODE_GLOBAL, FF, FilterCache, GuardedBuffer, graph_destroy, graph_instantiate,
                      graph_launch, hip_graph_api, int32_build_keys, stream_capture)

pytestmark = pytest.mark.gpu

AUTO, GATHER, LDS, PARTITIONED = 0, 1, 2, 3
SIZES = [1, 63, 64, 65, 511, 512, 513, 1025, 16384, 16385, 40003]
LOGS = [3, 10, 14, 17]
DTYPES = {"i64": np.int64, "i32": np.int32, "hash": np.uint64}
KINDS = ["flat", "valid", "dict", "row_sel"]
SMALL_ROWS = 16384  # RPT_SMALL_PROBE_ROWS


@pytest.fixture(scope="module")
def rpt():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run without a visible GPU")
    import rpt_amd

    rpt_amd.load()
    torch.cuda.set_device(0)
    return rpt_amd


@pytest.fixture(scope="module")
def caches(rpt):
    a = FilterCache()
    yield a
    a.close()


def dev(a):
    if a is None:
        return None
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def sel_of(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def rand_keys(dtype, n, rng):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)


class Col:
    """A key column of `rows` rows on the host and on the device: flat, flat with 15 % NULLs ("valid"), or a
    dictionary ("dict": rows // 2 + 1 physical entries with NULLs, or the key_sel given). kt "hash": precomputed
    hashes, to which validity does not apply (it is passed all the same and must be ignored)."""

    def __init__(self, rng, kt, kind, rows, keys=None, key_sel=None):
        self.kt, self.rows = kt, rows
        if kind == "dict" and key_sel is None:
            key_sel = rng.integers(0, rows // 2 + 1, rows).astype(np.uint32)
        self.key_sel = key_sel
        m = keys.size if keys is not None else (rows if key_sel is None else int(key_sel.max()) + 1)
        self.keys = rand_keys(DTYPES[kt], m, rng) if keys is None else keys
        assert m >= (rows if key_sel is None else int(key_sel.max()) + 1)
        self.validity = gu.validity_words(rng.random(m) < 0.85) if kind in ("valid", "dict") else None
        self.d_keys, self.d_key_sel, self.d_validity = dev(self.keys), dev(self.key_sel), dev(self.validity)

    def kwargs(self, rpt):
        kw = {"key_sel": self.d_key_sel, "validity": self.d_validity}
        if self.kt == "hash":
            kw["key_type"] = rpt.RPT_KEY_HASH
        return kw

    def as_dict(self, rpt):
        return dict(keys=self.d_keys, **self.kwargs(rpt))

    def phys(self, row_ids):
        """Physical key indices of the given row ids (in the given order)."""
        r = np.asarray(row_ids, dtype=np.int64)
        return (self.key_sel[r] if self.key_sel is not None else r).astype(np.uint32)

    def expect(self, base_words, log_nb, row_ids):
        """(words, minmax) of a filter holding base_words after the insert of exactly these rows."""
        p = self.phys(row_ids)
        w = base_words.copy()
        if self.kt == "hash":
            orc.insert_hashes(w, log_nb, self.keys[p])
            return w, None
        orc.insert_keys(w, log_nb, self.keys, key_sel=p, validity=self.validity)
        return w, (orc.minmax(self.keys, key_sel=p, validity=self.validity) if p.size else None)


class Targets:
    """One destination filter per (log_num_blocks, pre-filled), put back to its known words, no min/max and
    has_data = 0 by reset(): the words a call starts from are `base` exactly."""

    def __init__(self, rpt):
        self.rpt, self._made = rpt, {}

    def reset(self, log_nb, prefilled, tag=0):
        key = (log_nb, prefilled, tag)
        if key not in self._made:
            base = orc.new_words(log_nb)
            if prefilled:
                rng = np.random.default_rng(900 + log_nb)
                orc.insert_keys(base, log_nb, rand_keys(np.int64, min(1 << (log_nb + 1), 60000), rng))
            base.setflags(write=False)
            self._made[key] = (self.rpt.BloomFilter(log_num_blocks=log_nb), base)
        bf, base = self._made[key]
        bf.import_words(base)
        bf.set_minmax(None)
        bf.set_has_data(False)
        return bf, base

    def close(self):
        for bf, _b in self._made.values():
            bf.close()
        self._made.clear()


@pytest.fixture(scope="module")
def targets(rpt):
    t = Targets(rpt)
    yield t
    t.close()


def check(bf, exp, what=""):
    words, mm = exp
    got = bf.export_words()
    assert np.array_equal(got, words), f"{what}: {int((got != words).sum())} filter words differ from the oracle"
    assert bf.minmax() == mm, what
    assert not bf.is_empty(), what


# ---- result bits -------------------------------------------------------------------------------------------
PATTERNS = ["none", "all", "first", "last", "alternating", "dead_segments", "random0.1", "random0.5", "random0.9"]


def pattern_mask(name, n, rng):
    m = np.zeros(n, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[n - 1] = True
    elif name == "alternating":
        m[1::2] = True  # ...0,1
    elif name == "dead_segments":  # whole 512-row segments dead between live ones
        m[:] = True
        for s in range(1, (n + 511) // 512, 2):
            m[s * 512: (s + 1) * 512] = False
    elif name.startswith("random"):
        m = rng.random(n) < float(name[6:])
    return m


def bits_words(mask, ones_past_n=False):
    """The mask in the layout of rpt_bf_probe_bits: ceil(n / 512) * 8 words, LSB first."""
    n = mask.size
    b = np.zeros((n + 511) // 512 * 512, dtype=bool)
    b[:n] = mask
    b[n:] = ones_past_n
    return np.packbits(b, bitorder="little").view(np.uint64)


def guarded_bits(words):
    """The bits in an exactly sized buffer (guard bytes behind the last word read as set bits)."""
    g = GuardedBuffer(words.size * 8)
    g.view(torch.int64).copy_(dev(words))
    return g


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kt", list(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_insert_bits_patterns(rpt, targets, n, kt, kind):
    """Every pattern, with the bits past n clear and set, on one column per (key type, column kind); the filter size
    (2^3, 2^10, 2^14, 2^17 blocks) and empty / pre-filled rotate over the calls, so each pairing occurs."""
    rng = np.random.default_rng(n * 100 + KINDS.index(kind) * 10 + list(DTYPES).index(kt))
    rows = n + n // 2 + 3 if kind == "row_sel" else n
    col = Col(rng, kt, "valid" if kind == "row_sel" else kind, rows)
    row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if kind == "row_sel" else None
    d_row_sel = dev(row_sel)
    for idx, (pattern, ones_past_n) in enumerate(itertools.product(PATTERNS, [False, True])):
        log_nb, prefilled = LOGS[(idx + n) % 4], bool((idx // 4 + n) % 2)
        bf, base = targets.reset(log_nb, prefilled)
        mask = pattern_mask(pattern, n, rng)
        pos = np.flatnonzero(mask)
        bits = guarded_bits(bits_words(mask, ones_past_n))
        bf.insert_bits(col.d_keys, bits.view(torch.int64), n=n, row_sel=d_row_sel, **col.kwargs(rpt))
        check(bf, col.expect(base, log_nb, row_sel[pos] if row_sel is not None else pos),
              f"{pattern}, ones past n {ones_past_n}, 2^{log_nb} blocks, prefilled {prefilled}")


def test_insert_bits_more_than_one_segment_per_wave(rpt, targets):
    """The persistent grid holds 8 workgroups of 4 waves per CU and a wave owns whole 512-row segments: with
    2 * waves + 1 segments and one row more (about 2^23 rows on 256 CUs) every wave strides to a second segment, one
    to a third, and the last segment holds a single row. int32, flat with NULLs, half the rows selected."""
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4
    n = (2 * waves + 1) * 512 + 1
    rng = np.random.default_rng(23)
    col = Col(rng, "i32", "valid", n)
    mask = rng.random(n) < 0.5
    mask[n - 1] = True
    bf, base = targets.reset(17, True)
    bf.insert_bits(col.d_keys, dev(bits_words(mask)), n=n, **col.kwargs(rpt))
    check(bf, col.expect(base, 17, np.flatnonzero(mask)))


@pytest.mark.parametrize("kind", ["flat", "dict"])
@pytest.mark.parametrize("kt", list(DTYPES))
def test_insert_bits_alive_row_after_a_dead_row_with_the_same_hash(rpt, targets, kt, kind):
    """A column of equal keys with a single alive row, or bits ...0,1 only: the row before an alive row has the same
    hash but inserts nothing, so the alive row's atomic must not be dropped as a duplicate. Positions next to
    every boundary of the two row mappings (lane, 16-byte load, 64-row word, segment)."""
    rng = np.random.default_rng(31)
    n = 1025
    key = rand_keys(DTYPES[kt], 1, rng)
    if kind == "flat":
        col = Col(rng, kt, "flat", n, keys=np.repeat(key, n))
    else:
        col = Col(rng, kt, "flat", n, keys=np.repeat(key, 7), key_sel=rng.integers(0, 7, n).astype(np.uint32))
    masks = []
    for p in (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 511, 512, 513, 1023, 1024):
        m = np.zeros(n, dtype=bool)
        m[p] = True
        masks.append(m)
    masks.append(pattern_mask("alternating", n, rng))
    exp = col.expect(orc.new_words(14), 14, [0])
    assert orc.count_bits(exp[0]) >= 4
    for m in masks:
        bf, base = targets.reset(14, False)
        bf.insert_bits(col.d_keys, dev(bits_words(m)), n=n, **col.kwargs(rpt))
        check(bf, exp, f"alive rows {np.flatnonzero(m)[:4]}")


@pytest.mark.parametrize("kind", ["valid", "dict", "row_sel"])
@pytest.mark.parametrize("kt", ["i64", "i32"])
def test_insert_bits_dead_and_null_rows_do_not_move_minmax(rpt, targets, kt, kind):
    """Keys of the selected valid rows lie in [-1000, 1000]; the dead rows and the NULL rows hold the type's
    minimum and maximum."""
    rng = np.random.default_rng(37)
    n = 40003
    dtype = DTYPES[kt]
    rows = n + 1000 if kind == "row_sel" else n
    col = Col(rng, kt, "valid" if kind == "row_sel" else kind, rows)
    m = col.keys.size
    valid = ((col.validity[np.arange(m) >> 6] >> (np.arange(m) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if kind == "row_sel" else None
    mask = rng.random(n) < 0.5
    pos = np.flatnonzero(mask)
    sel_rows = row_sel[pos] if row_sel is not None else pos
    keep = np.zeros(m, dtype=bool)
    keep[col.phys(sel_rows)] = True
    keep &= valid
    extremes = np.where(rng.random(m) < 0.5, np.iinfo(dtype).min, np.iinfo(dtype).max).astype(dtype)
    col.keys = np.where(keep, rng.integers(-1000, 1001, m).astype(dtype), extremes)
    col.d_keys = dev(col.keys)
    bf, base = targets.reset(14, False)
    bf.insert_bits(col.d_keys, dev(bits_words(mask)), n=n, row_sel=dev(row_sel), **col.kwargs(rpt))
    exp = col.expect(base, 14, sel_rows)
    assert exp[1] is not None and -1000 <= exp[1][0] <= exp[1][1] <= 1000
    check(bf, exp)


# ---- selection vector with a device-side count ---------------------------------------------------------------
def sel_column(rng, kt, kind, rows):
    """A column whose rows >= rows // 2 hold keys that no row below holds (a dictionary keeps the halves apart
    too): a selection's tail points there, so an entry read past the count shows as wrong words, not as a fault."""
    key_sel = None
    if kind == "dict":
        m = rows // 2 + 2
        key_sel = np.concatenate([rng.integers(0, m // 2, rows // 2), rng.integers(m // 2, m, rows - rows // 2)])
        key_sel[-1] = m - 1
        key_sel = key_sel.astype(np.uint32)
    return Col(rng, kt, kind, rows, key_sel=key_sel)


@pytest.mark.parametrize("count_kind", ["zero", "one", "max_rows", "past_max_rows"])
@pytest.mark.parametrize("n", SIZES)
def test_insert_sel_counts(rpt, targets, n, count_kind):
    """max_rows = n; the device count is 0, 1, max_rows or max_rows + 100 (clamped; the buffer holds that many valid
    ids). Key type, column kind, filter size and empty / pre-filled rotate with n and the count."""
    ci = ["zero", "one", "max_rows", "past_max_rows"].index(count_kind)
    si = SIZES.index(n)
    rng = np.random.default_rng(n * 10 + ci)
    kt, kind = list(DTYPES)[(si + ci) % 3], ["flat", "valid", "dict"][(si // 3 + ci) % 3]
    log_nb, prefilled = LOGS[(si + 2 * ci) % 4], bool((si + ci // 2) % 2)
    count = {"zero": 0, "one": 1, "max_rows": n, "past_max_rows": n + 100}[count_kind]
    used = min(count, n)
    rows = 2 * (n + 100)
    col = sel_column(rng, kt, kind, rows)
    sel = np.empty(n + 100, dtype=np.uint32)
    sel[:used] = rng.integers(0, rows // 2, used)  # any order, repeats allowed
    sel[used:] = rng.integers(rows // 2, rows, n + 100 - used)
    bf, base = targets.reset(log_nb, prefilled)
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda:0")
    bf.insert_sel(col.d_keys, dev(sel), d_count, max_rows=n, **col.kwargs(rpt))
    check(bf, col.expect(base, log_nb, sel[:used]), f"{kt} {kind} 2^{log_nb} blocks, prefilled {prefilled}")
    assert int(d_count.item()) == count


def raw_chain_ws(rpt, filters, cols, n, out_sel, out_count, ws, row_sel=None):
    """rpt_bf_probe_chain_ws through ctypes: nothing but the call (the Python wrapper reads the count back)."""
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * len(filters))(*[f.handle for f in filters])
    arr = (KeyColumn * len(cols))(*cols)
    return rpt.load().rpt_bf_probe_chain_ws(handles, arr, len(filters), row_sel, n, out_sel.data_ptr(),
                                            out_count.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream)


def hits(rng, build, n, dtype, frac):
    """n keys of `dtype`: a fraction `frac` drawn from the filter's build keys, the rest random."""
    pool = build if dtype == np.int64 else int32_build_keys(build)
    return np.where(rng.random(n) < frac, pool[rng.integers(0, pool.size, n)], rand_keys(dtype, n, rng)).astype(dtype)


@pytest.mark.parametrize("source", ["probe", "chain_ws"])
@pytest.mark.parametrize("n", [2048, 16385, 40003])
def test_insert_sel_straight_from_a_probe(rpt, caches, targets, source, n):
    """out_sel and *out_count_dev of rpt_bf_probe (2048 rows: its fused kernel) and of rpt_bf_probe_chain_ws go into
    rpt_bf_insert_sel on another column of the same rows with no host read in between."""
    rng = np.random.default_rng(n + (source == "probe"))
    f, w, b = caches.get(16)
    f.probe_strategy = AUTO
    pk = hits(rng, b, n, np.int64, 0.4)
    exp_sel = orc.probe_keys(w, 16, pk)
    assert 0 < exp_sel.size < n
    col = Col(rng, "i32", "dict", n)
    bf, base = targets.reset(14, True)
    out_sel = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out_count = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    d_pk = dev(pk)
    if source == "probe":
        f.probe_async(d_pk, out_sel=out_sel, out_count=out_count)
    else:
        ws = torch.empty(rpt.probe_chain_workspace_bytes([f], n), dtype=torch.uint8, device="cuda:0")
        assert raw_chain_ws(rpt, [f], [rpt.make_column(d_pk)], n, out_sel, out_count, ws) == 0
    bf.insert_sel(col.d_keys, out_sel, out_count, **col.kwargs(rpt))
    check(bf, col.expect(base, 14, exp_sel))
    assert np.array_equal(sel_of(out_sel[: int(out_count.item())]), exp_sel)


# ---- the fused call ----------------------------------------------------------------------------------------------
PROBED = {13: ("i64", "flat"), 16: ("i32", "valid"), 18: ("i64", "dict")}  # filter size -> its probed column


def probed_column(rng, caches, log_nb, rows):
    """A column of which about 80 % of the rows pass the shared 2^log_nb-block filter, and the rows that do."""
    _f, w, b = caches.get(log_nb)
    kt, kind = PROBED[log_nb]
    m = rows // 2 + 1 if kind == "dict" else rows
    col = Col(rng, kt, kind, rows, keys=hits(rng, b, m, DTYPES[kt], 0.8),
              key_sel=rng.integers(0, m, rows).astype(np.uint32) if kind == "dict" else None)
    return col, orc.probe_keys(w, log_nb, col.keys, key_sel=col.key_sel, validity=col.validity)


def chain_for(caches, path, k, n):
    """k of the shared filters (2^13, 2^16, 2^18 blocks), the forced one second (first when k = 1)."""
    forced = {"auto": None, "gather": 16, "partitioned": 18}[path]
    order = [13, 16, 18] if forced is None else [L for L in (13, 16, 18) if L != forced]
    if forced is not None:
        order.insert(min(1, k - 1), forced)
    order = order[:k]
    for L in (13, 16, 18):
        caches.get(L)[0].probe_strategy = AUTO
    if forced is not None:
        f = caches.get(forced)[0]
        f.probe_strategy = GATHER if path == "gather" else PARTITIONED
        assert f.probe_strategy_for(n) == f.probe_strategy
    return order


@pytest.mark.parametrize("use_row_sel", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 1)])
@pytest.mark.parametrize("path", ["auto", "gather", "partitioned"])
@pytest.mark.parametrize("n", [1, 513, 16384, 16385, 40003])
def test_transfer_ws_vs_oracle(rpt, caches, targets, n, path, shape, use_row_sel):
    """1-3 probed filters and 1-2 destinations on columns of their own. "auto": every probed filter on AUTO, so
    n <= 16384 hands over to the one-launch chain and feeds the destinations from out_sel; "gather" / "partitioned":
    one filter forced, so every size takes the workspace path and feeds them from the accumulated bits. out_sel and
    the count equal rpt_bf_probe_chain_ws's and the oracle's; every destination equals the oracle's filter over the
    oracle's survivors. Outputs and workspace are exactly sized between guard bands."""
    k, n_dst = shape
    rng = np.random.default_rng(n * 7 + k + 10 * use_row_sel + 100 * ["auto", "gather", "partitioned"].index(path))
    order = chain_for(caches, path, k, n)
    filters = [caches.get(L)[0] for L in order]
    rows = n + n // 2 + 1 if use_row_sel else n
    cols, refs = zip(*[probed_column(rng, caches, L, rows) for L in order])
    exp = functools.reduce(np.intersect1d, refs)
    row_sel = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32) if use_row_sel else None
    if row_sel is not None:
        exp = np.intersect1d(exp, row_sel)
    exp = exp.astype(np.uint32)
    dst_specs = [("i64", "flat", 17, False), ("i32", "dict", 10, True)][:n_dst]
    if n % 2 == 0:
        dst_specs = [("i32", "valid", 14, True), ("hash", "flat", 3, False)][:n_dst]
    dst_cols = [Col(rng, kt, kind, rows) for kt, kind, _L, _p in dst_specs]
    dst = [targets.reset(L, p, tag=j) for j, (_kt, _kind, L, p) in enumerate(dst_specs)]
    need = rpt.probe_chain_workspace_bytes(filters, n)
    ws, sel, cnt = GuardedBuffer(need).poison(A5), GuardedBuffer(4 * n).poison(FF), GuardedBuffer(8).poison(FF)
    col_args = [c.as_dict(rpt) for c in cols]
    out_sel, out_count = rpt.transfer_ws(filters, col_args, [bf for bf, _b in dst], [c.as_dict(rpt) for c in dst_cols],
                                         row_sel=dev(row_sel), n=n, out_sel=sel.view(torch.int32),
                                         out_count=cnt.view(torch.int64), workspace=ws.bytes())
    for (bf, base), c, spec in zip(dst, dst_cols, dst_specs):
        check(bf, c.expect(base, spec[2], exp), f"destination {spec}")
    assert int(out_count.item()) == exp.size
    assert np.array_equal(sel_of(out_sel[: exp.size]), exp)
    handed_over = path == "auto" and n <= SMALL_ROWS
    assert bool(torch.all(ws.bytes() == 0xA5)) == handed_over, "the other path was taken"
    for name, g in (("workspace", ws), ("out_sel", sel), ("out_count", cnt)):
        g.assert_guards_intact(name)
    got = rpt.probe_chain_ws(filters, col_args, row_sel=dev(row_sel), n=n)
    assert np.array_equal(sel_of(got), exp)
    if n >= 16384:
        assert 0 < exp.size < n


@pytest.mark.parametrize("n", [1000, 20000])
def test_transfer_ws_without_survivors(rpt, caches, targets, n):
    """An empty probed filter passes nothing: the destinations keep their words and get no min/max, the count is 0;
    has_data is 1 all the same (the host cannot know) until the caller, having read the count, takes it back."""
    rng = np.random.default_rng(n)
    order = chain_for(caches, "auto", 1, n)
    empty = rpt.BloomFilter(log_num_blocks=12)
    col0, _ref = probed_column(rng, caches, order[0], n)
    col1 = Col(rng, "i64", "flat", n)
    dcol = Col(rng, "i64", "valid", n)
    bf, base = targets.reset(14, True)
    assert bf.is_empty()
    _sel, count = rpt.transfer_ws([caches.get(order[0])[0], empty], [col0.as_dict(rpt), col1.as_dict(rpt)], [bf],
                                  [dcol.as_dict(rpt)])
    assert int(count.item()) == 0
    check(bf, (base, None))
    bf.set_has_data(False)
    assert bf.is_empty()
    # n == 0 touches no destination at all
    count.fill_(7)
    rpt.transfer_ws([empty], [col1.as_dict(rpt)], [bf], [dcol.as_dict(rpt)], n=0, out_count=count)
    assert int(count.item()) == 0 and bf.is_empty()
    assert np.array_equal(bf.export_words(), base)
    empty.close()


def test_has_data_after_an_empty_selection(rpt, targets):
    rng = np.random.default_rng(5)
    col = Col(rng, "i64", "flat", 1000)
    bf, base = targets.reset(10, False)
    bf.insert_bits(col.d_keys, dev(bits_words(np.zeros(1000, dtype=bool))))
    check(bf, (base, None))
    bf, base = targets.reset(10, False)
    bf.insert_sel(col.d_keys, dev(np.arange(1000, dtype=np.uint32)), torch.zeros(1, dtype=torch.int64, device="cuda:0"))
    check(bf, (base, None))
    bf, base = targets.reset(10, False)
    bf.insert_bits(col.d_keys, dev(bits_words(np.zeros(0, dtype=bool))), n=0)  # n == 0: a no-op
    assert bf.is_empty()


# ---- ordering and capture -----------------------------------------------------------------------------------------
def test_insert_right_after_clear(rpt):
    """rpt_bf_clear defers its zeroing to the next operation: each insert settles it first, so the filter holds the
    selected rows only."""
    rng = np.random.default_rng(41)
    n = 5000
    col = Col(rng, "i64", "valid", n)
    mask = rng.random(n) < 0.3
    pos = np.flatnonzero(mask)
    exp = col.expect(orc.new_words(12), 12, pos)
    bf = rpt.BloomFilter(log_num_blocks=12)
    for how in ("bits", "sel", "transfer"):
        bf.insert(dev(rand_keys(np.int64, 3000, rng)))
        bf.clear()
        if how == "bits":
            bf.insert_bits(col.d_keys, dev(bits_words(mask)), **col.kwargs(rpt))
        elif how == "sel":
            bf.insert_sel(col.d_keys, dev(pos.astype(np.uint32)),
                          torch.tensor([pos.size], dtype=torch.int64, device="cuda:0"), **col.kwargs(rpt))
        else:  # the probed filter holds every key of its column: every selected row survives
            src = rpt.BloomFilter(log_num_blocks=12)
            src.insert(col.d_keys)
            rpt.transfer_ws([src], [col.d_keys], [bf], [col.as_dict(rpt)], row_sel=dev(pos.astype(np.uint32)))
            torch.cuda.synchronize()
            src.close()
        check(bf, exp, how)
    bf.close()


def graph_node_count(graph) -> int:
    hip = hip_graph_api()
    hip.hipGraphGetNodes.restype = ctypes.c_int
    count = ctypes.c_size_t(12345)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(count)) == 0
    return count.value


def raw_transfer(rpt, filters, cols, dst, dst_cols, n, out_sel, out_count, ws, stream_handle):
    from rpt_amd._lib import KeyColumn

    handles = (ctypes.c_void_p * len(filters))(*[f.handle for f in filters])
    dst_handles = (ctypes.c_void_p * len(dst))(*[f.handle for f in dst])
    return rpt.load().rpt_bf_transfer_ws(handles, (KeyColumn * len(cols))(*cols), len(filters), dst_handles,
                                         (KeyColumn * len(dst_cols))(*dst_cols), len(dst), None, n,
                                         out_sel.data_ptr(), out_count.data_ptr(), ws.data_ptr(), ws.numel(),
                                         stream_handle)


def test_cleared_destination_is_refused_inside_a_capture(rpt, caches):
    """A deferred clear cannot be settled inside a capture: the three calls are refused there and have enqueued
    nothing (the captured graph has no node); outside a capture the same calls settle it."""
    lib = rpt.load()
    hip = hip_graph_api()
    rng = np.random.default_rng(43)
    n = 20000
    f, _w, b = caches.get(16)
    f.probe_strategy = GATHER
    pk = dev(hits(rng, b, n, np.int64, 0.5))
    col = Col(rng, "i64", "flat", n)
    kc = rpt.make_column(col.d_keys)
    bits = dev(bits_words(rng.random(n) < 0.5))
    sel = dev(np.arange(n, dtype=np.uint32))
    out_sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    count = torch.full((1,), n, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(rpt.probe_chain_workspace_bytes([f], n), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    bf = rpt.BloomFilter(log_num_blocks=12)
    bf.insert(dev(rand_keys(np.int64, 1000, rng)))
    bf.clear()
    torch.cuda.synchronize()
    calls = {
        "bits": lambda: lib.rpt_bf_insert_bits(bf.handle, ctypes.byref(kc), None, n, bits.data_ptr(), sh),
        "sel": lambda: lib.rpt_bf_insert_sel(bf.handle, ctypes.byref(kc), sel.data_ptr(), count.data_ptr(), n, sh),
        "transfer": lambda: raw_transfer(rpt, [f], [rpt.make_column(pk)], [bf], [kc], n, out_sel, count, ws, sh),
    }
    for name, call in calls.items():
        graph = ctypes.c_void_p()
        end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph, call)
        assert end == 0, name
        assert st == 1 and b"rpt_bf_settle" in lib.rpt_last_error(), name
        assert graph_node_count(graph) == 0, name
        assert hip.hipGraphDestroy(graph) == 0
    assert bf.is_empty()  # a refused call has not marked the filter either
    assert calls["bits"]() == 0
    s.synchronize()
    assert not bf.is_empty()
    bf.close()


@pytest.mark.parametrize("n", [2048, 20000])
def test_transfer_ws_graph_capture(rpt, caches, n):
    """One rpt_bf_transfer_ws captured on a side stream (2048 rows: the hand-over, fed from out_sel; 20000 rows: the
    workspace path, fed from the bits) and replayed over three key contents written into the same tensors: the
    destination ORs each replay's survivors and folds their min/max."""
    rng = np.random.default_rng(47 + n)
    f0, w0, b0 = caches.get(13)
    f1, w1, b1 = caches.get(16)
    f0.probe_strategy = AUTO
    f1.probe_strategy = AUTO
    k0, k1 = dev(hits(rng, b0, n, np.int64, 0.6)), dev(hits(rng, b1, n, np.int64, 0.6))
    dk = dev(rand_keys(np.int64, n, rng))
    cols = [rpt.make_column(k0), rpt.make_column(k1)]
    dcols = [rpt.make_column(dk)]
    out_sel = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(rpt.probe_chain_workspace_bytes([f0, f1], n), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    sh = ctypes.c_void_p(s.cuda_stream)
    bf = rpt.BloomFilter(log_num_blocks=14)
    words, lo, hi = orc.new_words(14), None, None

    def expect_one_more():
        nonlocal lo, hi
        surv = np.intersect1d(orc.probe_keys(w0, 13, k0.cpu().numpy()), orc.probe_keys(w1, 16, k1.cpu().numpy()))
        assert 0 < surv.size < n
        keys = dk.cpu().numpy()
        orc.insert_keys(words, 14, keys, key_sel=surv.astype(np.uint32))
        mn, mx = orc.minmax(keys, key_sel=surv.astype(np.uint32))
        lo, hi = (mn if lo is None else min(lo, mn)), (mx if hi is None else max(hi, mx))
        return surv

    # once outside any capture (a kernel's first launch may set its LDS allowance), on another stream than the one
    # captured below, as tests/test_gpu_deferred_clear.py's captured inserts do: the capture asks whether the
    # destination's previous write has completed by querying the event recorded on that write's stream
    assert raw_transfer(rpt, [f0, f1], cols, [bf], dcols, n, out_sel, out_count, ws,
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    expect_one_more()
    check(bf, (words, (lo, hi)), "before the capture")
    graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
    end, st = stream_capture(sh, CAPTURE_MODE_GLOBAL, graph,
                             lambda: raw_transfer(rpt, [f0, f1], cols, [bf], dcols, n, out_sel, out_count, ws, sh))
    assert end == 0 and st == 0, rpt.load().rpt_last_error()
    assert graph_instantiate(graph, exe) == 0
    for replay in range(3):
        k0.copy_(dev(hits(rng, b0, n, np.int64, 0.3 + 0.2 * replay)))
        k1.copy_(dev(hits(rng, b1, n, np.int64, 0.9 - 0.2 * replay)))
        dk.copy_(dev(rand_keys(np.int64, n, rng)))
        out_count.fill_(-1)
        torch.cuda.synchronize()
        assert graph_launch(exe, sh) == 0
        s.synchronize()
        surv = expect_one_more()
        assert int(out_count.item()) == surv.size
        assert np.array_equal(sel_of(out_sel[: surv.size]), surv.astype(np.uint32))
        check(bf, (words, (lo, hi)), f"replay {replay}")
    assert graph_destroy(exe, graph)
    bf.close()
