"""Matrices for the reload tests (a plain helper module: tests/test_reload_data.py pins the traits on the CPU,
tests/test_gpu_reload.py loads one after the other into ONE context and compares with a fresh context).

A context caches a great deal that depends on the loaded matrix; a second load of the SAME matrix reproduces the right
answer from every stale cache.  The pairs here differ in everything a cache is keyed by or sized from:

  A       synth.generate(12000, seed=3): RCV1-like, ~75 non-zeros per row, values <= 1.
  B       synth.generate(9000, seed=8, nnz_mean=150) with the columns MIRRORED in rank order (its column of rank r goes to
          the key that A ranks D - 1 - r, rows re-sorted: A's hottest columns are B's coldest -- another ranking, another
          hot / cold split; synth's rank -> key map is a seeded permutation, so the plain key mirror D + 1 - col would leave
          40 % of the hot columns shared), every value times 8 (exact; vexp
          moves by 3), every 50th row emptied and two rows of 3,000 entries (the long-row list).  Fewer rows than A, a mean
          row length above 96 against below (another lane group of the evaluation kernels).
  A_long  A with the 100 rows of LONG_LIST replaced by rows of 3,000 entries: the same row count, so a plan's "fits the
          staged sub-batch" keyed by the row count alone would survive the load.  The replaced rows carry positive values and
          ONE label: 300,000 contributions over 47,236 columns, six to eight per column, and with mixed signs one or two columns'
          exact sums fall below the grid of a 21-bit launch (measured: key 13,145, eight entries summing to less than a
          unit; the column leaves the engine's support and loses the regulariser, lr * s = 3.8e-6).  That is the
          vanishing-column term of oracle/bounds.py, which tests/test_gpu_hard_values.py prices and plan_step's bound does
          not; with one sign no sum can cancel.
  N       a narrow pair at D = 3,000 (every rank hot: no cold stream), 6,000 and 4,000 rows.

Everything is deterministic from the seeds."""

from __future__ import annotations

import os
import re

import numpy as np

from dsgd_amd import synth
from hard_data import _replace_rows

DIM = synth.RCV1_DIM
HOT = 18396            # the library's default hot / cold split of the ranks (dsgd_tuning_info "hsplit" at D = 47,236)
LANE_GROUP_MEAN = 96   # load_csr_impl: mean row length > 96 -> 32 lanes per row, > 12 -> 16
ROWS_A, ROWS_B = 12000, 9000
N_TRAIN_A, N_TRAIN_B = 9600, 7200
LONG_LEN = 3000
B_LONG_ROWS = (1234, 7777)
_CACHE = {}


def _long_row(rng, dim, n, scale=1.0):
    c = np.sort(rng.choice(np.arange(1, dim + 1), size=n, replace=False)).astype(np.int32)
    v = (rng.random(n) + 0.1).astype(np.float32)
    v = (v / np.float32(np.sqrt(np.sum(v.astype(np.float64) ** 2)))).astype(np.float32)   # L2-normalised, as synth's rows
    return c, (v * np.float32(scale)).astype(np.float32)


def matrix_a():
    if "A" not in _CACHE:
        _CACHE["A"] = synth.generate(ROWS_A, seed=3)
    return _CACHE["A"]


def _keys_by_rank(data):
    """the keys 1..D by descending count over the rows, ties by ascending key (the library's ranking without key 0)"""
    cnt = np.bincount(data.col, minlength=data.dim + 1)[1:]
    return np.argsort(-cnt, kind="stable") + 1


def matrix_b():
    if "B" not in _CACHE:
        base = synth.generate(ROWS_B, seed=8, nnz_mean=150)
        # mirrored IN RANK ORDER: the column of rank r in the base goes to the key A ranks D - 1 - r (synth maps ranks to
        # keys by a seeded random permutation, so the plain key mirror D + 1 - col leaves the two hot sets as independent
        # as they were: 40 % shared)
        keys_a = _keys_by_rank(matrix_a())
        rank_b = np.empty(base.dim + 1, np.int64)
        rank_b[_keys_by_rank(base)] = np.arange(base.dim)
        rng = np.random.default_rng(88)
        row_ptr, col, val = [0], [], []
        for i in range(base.n_rows):
            b, e = int(base.row_ptr[i]), int(base.row_ptr[i + 1])
            if i in B_LONG_ROWS:
                c, v = _long_row(rng, base.dim, LONG_LEN, 8.0)
            elif i % 50 == 0:
                c, v = np.zeros(0, np.int32), np.zeros(0, np.float32)   # Sparse.zeros
            else:
                c = keys_a[base.dim - 1 - rank_b[base.col[b:e]]]
                at = np.argsort(c, kind="stable")                       # each row ascending again
                c, v = c[at].astype(np.int32), (base.val[b:e][at] * np.float32(8.0)).astype(np.float32)
            col.append(c); val.append(v)
            row_ptr.append(row_ptr[-1] + len(c))
        _CACHE["B"] = synth.Csr(base.dim, np.asarray(row_ptr, np.int64), np.concatenate(col).astype(np.int32),
                                np.concatenate(val).astype(np.float32), base.label.copy())
    return _CACHE["B"]


def mirror_of_b(col):
    """where matrix_b sends the base's columns (tests/test_reload_data.py pins the construction with it)"""
    base = synth.generate(ROWS_B, seed=8, nnz_mean=150)
    rank_b = np.empty(base.dim + 1, np.int64)
    rank_b[_keys_by_rank(base)] = np.arange(base.dim)
    return _keys_by_rank(matrix_a())[base.dim - 1 - rank_b[np.asarray(col)]]


# the 100 rows of the one-workgroup plan (inside B's rows too) -- and of A_long's replaced rows
LONG_LIST = (np.arange(100, dtype=np.int32) * 71 + 13)


def matrix_a_long():
    if "A_long" not in _CACHE:
        rng = np.random.default_rng(33)
        _CACHE["A_long"] = _replace_rows(matrix_a(), {int(r): _long_row(rng, DIM, LONG_LEN) for r in LONG_LIST},
                                         labels={int(r): 1 for r in LONG_LIST})
    return _CACHE["A_long"]


def narrow_pair():
    if "N" not in _CACHE:
        _CACHE["N"] = (synth.generate(6000, seed=5, dim=3000), synth.generate(4000, seed=6, dim=3000, nnz_mean=40))
    return _CACHE["N"]


def perturbed_doubles(data, seed=4):
    """the values as doubles that are NOT floats: each times (1 + k 2^-40), k in 1..1023 (zero stays zero)"""
    rng = np.random.default_rng(seed)
    v = data.val.astype(np.float64) * (1.0 + rng.integers(1, 1024, size=len(data.val)) * 2.0 ** -40)
    return synth.Csr(data.dim, data.row_ptr, data.col, v.astype(np.float32), data.label, v)


# ---- index lists --------------------------------------------------------------------------------------------------------------
def lists_inside(k, b, seed, n_rows=N_TRAIN_B):
    """k lists of b distinct rows of [0, n_rows): inside BOTH matrices' train rows at the default (B's are the fewer)"""
    rng = np.random.default_rng([seed, k, b])
    bounds = np.linspace(0, n_rows, k + 1).astype(np.int64)
    return [rng.permutation(np.arange(bounds[i], bounds[i + 1]))[:b].astype(np.int32) for i in range(k)]


def lists_beyond_b(k, b, seed):
    """k lists of b rows of A of which the LAST list reaches beyond B's rows (the others lie inside them)"""
    out = lists_inside(k, b, seed)
    rng = np.random.default_rng([seed, 99])
    out[-1] = np.sort(rng.choice(np.arange(ROWS_B - b // 2, ROWS_A), size=b, replace=False)).astype(np.int32)
    return out


def nonzero_weights(seed, dim=DIM, n=6000):
    rng = np.random.default_rng(seed)
    w0 = np.zeros(dim + 1, dtype=np.float32)
    w0[rng.choice(np.arange(1, dim + 1), size=n, replace=False)] = rng.normal(scale=0.05, size=n).astype(np.float32)
    return w0


# ---- the host rules restated --------------------------------------------------------------------------------------------------
def stage_constants():
    """PLAN_STAGE_CAP, PLAN_STAGE_CH as csrc/dsgd_plan_check.hpp states them"""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "distributed-sgd_amd", "csrc", "dsgd_plan_check.hpp")) as f:
        text = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("PLAN_STAGE_CAP", "PLAN_STAGE_CH"))


def internal_row_len(data):
    """row lengths as the library holds them: an empty row owns one explicit zero (load_csr_impl)"""
    return np.maximum(np.diff(data.row_ptr), 1)


def list_fits_staged(data, idx):
    """plan_list_fits_staged: at most CAP rows and CAP work items of CH non-zeros"""
    cap, ch = stage_constants()
    idx = np.asarray(idx, dtype=np.int64)
    if len(idx) > cap or idx.min() < 0 or idx.max() >= data.n_rows:
        return False
    return int(((internal_row_len(data)[idx] + ch - 1) // ch).sum()) <= cap


def lane_group(data):
    """lanes per row of the evaluation kernels, from the mean row length (load_csr_impl)"""
    mean = float(internal_row_len(data).sum()) / data.n_rows
    return 64 if mean > 192 else 32 if mean > LANE_GROUP_MEAN else 16 if mean > 12 else 8


def hottest(data, n=HOT):
    """the n keys the library ranks first: count over all rows descending, ties by ascending key (hard_data.column_ranks)"""
    cnt = np.bincount(data.col, minlength=data.dim + 1)
    return np.argsort(-cnt, kind="stable")[:n]
