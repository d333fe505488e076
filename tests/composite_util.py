"""Helpers of the composite-key GPU tests (tests/test_gpu_composite.py, tests/test_gpu_kernel_ledger_composite.py;
imported as a plain module, not a conftest): composite keys over test_gpu_transfer's columns with the oracle's
HashColumns beside them, and probed filters whose members are chosen rows of such a key."""
import numpy as np
import torch

import rpt_oracle as orc
from test_gpu_transfer import Col, dev

DENSE, DICT, MISALIGNED = "dense", "dict", "misaligned"  # kernel_ledger's row mappings
LAYOUTS = (DENSE, DICT, MISALIGNED)


def misalign(col):
    """Move a flat column's device keys one element past a 16-byte boundary."""
    raw = torch.empty(col.d_keys.numel() + 5, dtype=col.d_keys.dtype, device="cuda:0")
    at = 1 if raw.data_ptr() % 16 == 0 else 1 + (16 - raw.data_ptr() % 16) // raw.element_size()
    view = raw[at: at + col.d_keys.numel()]
    view.copy_(col.d_keys)
    col.d_keys, col._raw = view, raw
    assert col.d_keys.data_ptr() % 16 == col.d_keys.element_size()
    return col


class Key:
    """A composite key of `rows` rows: one column per entry of kts ("i64" / "i32", "hash" only first). nulls: the
    column indices that carry 15 % NULLs. layout: all flat and aligned (DENSE), or column `special` a dictionary (DICT)
    or misaligned by an element (MISALIGNED)."""

    def __init__(self, rng, kts, rows, layout=DENSE, nulls=(), special=None, prefix=None):
        self.rows, self.kts = rows, tuple(kts)
        special = len(kts) - 1 if special is None else special
        self.cols = []
        for j, kt in enumerate(kts):
            assert kt != "hash" or j == 0
            keys = prefix if kt == "hash" and prefix is not None else None
            if layout == DICT and j == special:
                col = Col(rng, kt, "dict", rows)
            else:
                col = Col(rng, kt, "valid" if j in nulls else "flat", rows, keys=keys)
            if layout == MISALIGNED and j == special:
                misalign(col)
            self.cols.append(col)
        self.dense = all(c.d_key_sel is None and c.d_keys.data_ptr() % 16 == 0 for c in self.cols)
        assert self.dense == (layout == DENSE)

    def columns(self, rpt):
        """The key as the Python wrappers take it: a list of make_column dicts."""
        return [c.as_dict(rpt) for c in self.cols]

    def oracle_columns(self, row_ids):
        out = []
        for c in self.cols:
            out.append(dict(keys=c.keys, key_sel=c.phys(row_ids), validity=None if c.kt == "hash" else c.validity))
        return out

    def hashes(self, row_ids=None):
        """The oracle's HashColumns of the given rows (all rows by default); a HASH column 0 is the hashed prefix."""
        row_ids = np.arange(self.rows, dtype=np.uint32) if row_ids is None else np.asarray(row_ids, dtype=np.uint32)
        cols = self.oracle_columns(row_ids)
        if self.kts[0] != "hash":
            return orc.hash_columns(cols)
        h = np.ascontiguousarray(self.cols[0].keys[cols[0]["key_sel"]], dtype=np.uint64)
        for c in cols[1:]:
            h = orc.hash_combine(h, c["keys"], c["key_sel"], c["validity"])
        return h

    def expect(self, base_words, log_nb, row_ids):
        """(words, minmax) of a filter holding base_words after the insert of exactly these rows: a key of two or more
        columns folds no min/max, a key of one column is the column's."""
        if len(self.cols) == 1:
            return self.cols[0].expect(base_words, log_nb, row_ids)
        w = base_words.copy()
        orc.insert_hashes(w, log_nb, self.hashes(row_ids))
        return w, None


def member_filter(rpt, rng, key, log_nb, share=0.5):
    """(BloomFilter, oracle words, per-row pass mask): a filter of 2^log_nb blocks holding about `share` of the key's
    rows, made in the oracle and imported."""
    h = key.hashes()
    words = orc.new_words(log_nb)
    orc.insert_hashes(words, log_nb, h[rng.random(key.rows) < share])
    bf = rpt.BloomFilter(log_num_blocks=log_nb)
    bf.import_words(words)
    bf.set_has_data(True)
    passes = np.zeros(key.rows, dtype=bool)
    passes[orc.lookup_sel_hashes(words, log_nb, h)] = True
    return bf, words, passes


def row_list(rng, kind, n, rows):
    """(the listed row ids, the device row_sel or None) for n positions over a table of `rows` rows: None (rows 0..n-1),
    "ascending" (a sorted subset) or "shuffled" (any order, with repeats)."""
    if kind is None:
        return np.arange(n, dtype=np.uint32), None
    if kind == "ascending":
        ids = np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint32)
    else:
        ids = rng.integers(0, rows, n).astype(np.uint32)
    return ids, dev(ids)
