"""The data and index lists of the dense list tests (test infrastructure, numpy only): tests/test_dense_list_abi.py shows
on the CPU that they make the bit equalities of tests/test_gpu_dense_lists.py sensitive, with tests/dense_bound.py's
`emulate` as the candidate.

Every shard has a HOT row, its last: under the shard's start weights its label speaks against its logit (|r| >= 1/2),
and row 0 carries the opposite label.  Every list starts with the hot row, so position 0 and the row it names disagree
in their labels: a kernel that took labels by position would move the weights by a whole x_hot / n.
"""

from __future__ import annotations

import numpy as np

import dense_bound as db

LENGTHS = (1, 7, 8, 9, 15, 16, 17)
KINDS = ("perm", "reverse", "repeat", "longer")
WIDTHS = (512, 1024, 4096, 8192)
WIDE_N = 37          # 5 blocks of 8 / 3 of 16, ragged
SMALL_ROWS = 48      # the shard of the lists longer than n_rows, and of the width cases
LIST_FAULTS = ("label_by_position", "first_of_block", "last_dropped", "reads_position_n")


def big_len(D, n_cu):
    """case_a's row counts: 3 or 4 blocks per workgroup with a ragged tail (D = 512); 16 n_cu + 24 rows (D = 4096)."""
    return 3 * 16 * n_cu + 8 * n_cu + 5 if D == 512 else 16 * n_cu + 24


_shards = {}


def shard(D, n_rows, seed=0):
    """(X, y, w0) with logits of sigma ~ 1; hot row n_rows - 1.  Built once per shape: callers leave it unchanged."""
    key = (D, n_rows, seed)
    if key not in _shards:
        X, y, w = db._make(n_rows, D, 4000 + 7 * D + seed, 1.0)
        hot = n_rows - 1
        db._misclassify(X, y, w, [hot])
        y[0] = 1.0 - y[hot]
        for a in (X, y, w):
            a.setflags(write=False)
        _shards[key] = (X, y, w)
    return _shards[key]


def make_list(kind, n, n_rows, seed=0):
    """A list of n positions over a shard of n_rows rows ("longer": n_rows + n positions), starting with the hot row."""
    rng = np.random.default_rng(100 * n + seed)
    hot = n_rows - 1
    if kind == "reverse":
        assert n <= n_rows
        return np.arange(n_rows - 1, n_rows - 1 - n, -1, dtype=np.int32)
    if kind == "longer":
        idx = rng.integers(0, n_rows, size=n_rows + n).astype(np.int32)
        idx[0] = hot
        return idx
    assert n <= n_rows
    idx = rng.permutation(n_rows)[:n].astype(np.int32)
    at = np.flatnonzero(idx == hot)
    if len(at):
        idx[at[0]] = idx[0]
    idx[0] = hot
    if kind == "repeat" and n > 1:   # one row five times (a list of fewer than 6: as often as it has room), spread over the blocks
        idx[np.unique(np.linspace(1, n - 1, 5).astype(int))] = idx[1]
    return idx


def is_sensitive(X, y, w, idx):
    """Not the identity, and some position k has another label than the row it names while that row's |r| >= 1/4."""
    n = min(len(idx), len(y))
    k = np.arange(n)
    rows = idx[:n]
    r = db.sigmoid(X[rows].astype(np.float64) @ w.astype(np.float64)) - y[rows]
    return bool((rows != k).any() and ((y[k] != y[rows]) & (np.abs(r) >= 0.25)).any())


def emulate_list(X, y, w, lr, idx, variant, grid, fault=None):
    """dense_bound.emulate over the rows a list names: the honest candidate (fault None) is the range step over
    (X[idx], y[idx]); the faults are what an indexing mistake of the list kernel would compute instead."""
    assert fault is None or fault in LIST_FAULTS
    n = len(idx)
    rows = np.asarray(idx, dtype=np.int64)
    Xg, yg = X[rows], y[rows]
    inner = None
    if fault == "label_by_position":
        yg = y[np.arange(n) % len(y)]
    elif fault == "first_of_block":
        rpb = db.rows_per_block(variant)
        first = rows[np.arange(n) // rpb * rpb]
        Xg, yg = X[first], y[first]
    elif fault == "last_dropped":
        inner = "last_row_dropped"
    elif fault == "reads_position_n":      # what lies behind the list: here the hot row
        Xg = np.concatenate([Xg, X[-1:]])
        yg = np.concatenate([yg, y[-1:]])
        inner = "row_end_included"
    return db.emulate(Xg, yg, w, lr, 0, n, variant, grid, fault=inner)[0]


def step2_list(n_rows, seed=0):
    """The list of the second step (from the weights the first step left): 23 positions, another draw."""
    return make_list("perm", min(23, n_rows), n_rows, seed=seed + 991)


def cases(n_cu):
    """(D, n_rows, kind, n) of every first-step list of `test_any_list_is_the_range_step_on_permuted_data`."""
    out = []
    big512, big4096 = big_len(512, n_cu), big_len(4096, n_cu)
    for kind in KINDS:
        if kind == "longer":
            out += [(512, SMALL_ROWS, kind, n) for n in LENGTHS]
        else:
            out += [(512, big512 + 8, kind, n) for n in LENGTHS + (big512,)]
            out += [(4096, big4096 + 8, kind, big4096)]
        out += [(D, SMALL_ROWS, kind, WIDE_N) for D in WIDTHS]
    return out
