"""Hostile feature VALUES for the parity tests (a plain helper module: tests/test_hard_data.py pins the traits on the CPU,
tests/test_gpu_hard_values.py feeds them to every gradient kernel family).

synth.generate draws |N(0,1)| + 0.1 and L2-normalises every row: positive values, at most 1, within about ten binades of
the row's largest, no empty row.  Every function here takes such a base and a seed and returns a `Hard`: the transformed
CSR, a weight vector built for it (float64, every entry a float32 value, so both precisions can load it unchanged) and
what the trait planted.  Everything is deterministic from the seed.

  scaled(k)     every value times 2^k (exact in fp32): vexp = vexp(base) + k in every ldexp of every family.
  signed        a seeded half of the entries negated; m PAIRS of rows with one label, the same private columns (columns no
                other row has, weight 0) and opposite values: both rows sit on the gate (d = 0: active) and their private
                columns sum to the integer 0 exactly -- they leave the support and get no regulariser.
  wide          each entry times 2^-u, u uniform in 0..45; a few private columns that occur ONLY with u >= 42: entries below
                the fp32 grid and outside the fp64 exact range, columns whose whole sum vanishes on a grid.
  zero_margin   rows ON the gate at non-zero weights: (a) {c1: a, c2: a} with w[c1] = -w[c2], both labels; (b) rows whose
                every product is <= 1e-20 in magnitude (x = 2^-34, w = +-2^-34: 3.4e-21) with the sign that would gate the
                row OFF if the product survived the filter of math/Sparse.scala:46; (c) rows supported only where w == 0.
  ragged64      the ragged recipe of the parity tests (ragged_data below: empty rows, one-element rows, a 1e-25 entry) plus rows of
                3,000 and 8,000 entries.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from dsgd_amd import synth

SPARSE_EPS = 1e-20   # math/Sparse.scala:108-118


@dataclass
class Hard:
    data: synth.Csr
    w: np.ndarray                      # float64 [dim + 1], float32 values
    planted: dict = field(default_factory=dict)


# ---- the grid's anchor and the fp64 mode's exact range ---------------------------------------------------------------
def vexp_of(val):
    """The engine's vexp (dsgd_load_csr): the smallest e with max |x| <= 2^e, by frexp."""
    vmax = float(np.abs(np.asarray(val, dtype=np.float32)).max()) if len(val) else 0.0
    if not vmax > 0.0:
        return 1   # (the engine takes vmax = 1.0f there: frexp(1) = 0.5 * 2^1, and no power-of-two correction at vmax = 0)
    m, e = math.frexp(vmax)
    return e - 1 if m == 0.5 else e


def _entries(data, rows):
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    parts = [data.val[data.row_ptr[r]:data.row_ptr[r + 1]] for r in rows]
    v = np.concatenate(parts).astype(np.float64) if parts else np.zeros(0)
    return v[np.abs(v) > SPARSE_EPS]


def exact_range_floor(data, n):
    """the lowest float exponent that is exact on the grid of a list of n rows: vexp - (39 - ceil(log2 n)) (include/dsgd.h)"""
    return vexp_of(data.val) - (39 - math.ceil(math.log2(n)) if n > 1 else 39)


def check_exact_range(data, rows, n):
    """every entry of the rows lies inside the exact range of a list of n rows: e >= vexp - (39 - ceil(log2 n))"""
    v = _entries(data, rows)
    _, e = np.frexp(np.abs(v))   # |v| = f * 2^e, f in [0.5, 1): the float's exponent is e - 1
    lo = exact_range_floor(data, n)
    assert (e - 1).min() >= lo, ((e - 1).min(), lo)


def outside_exact_range(data, rows, n):
    """how many entries of the rows lie OUTSIDE the exact range of a list of n rows (the complement of check_exact_range)"""
    v = _entries(data, rows)
    if not len(v):
        return 0
    _, e = np.frexp(np.abs(v))
    return int(((e - 1) < exact_range_floor(data, n)).sum())


# ---- helpers ---------------------------------------------------------------------------------------------------------
def base_weights(dim, seed, n=3000, scale=0.1):
    """n non-zero weights N(0, scale) as float32 values (the w of the issue's CPU checks)"""
    rng = np.random.default_rng(seed)
    w = np.zeros(dim + 1, dtype=np.float32)
    w[rng.choice(np.arange(1, dim + 1), n, replace=False)] = rng.normal(scale=scale, size=n).astype(np.float32)
    return w.astype(np.float64)


def unused_columns(data, n, rng):
    """n columns no row of the data has (RCV1's width leaves thousands with a few thousand Zipf rows)"""
    free = np.setdiff1d(np.arange(1, data.dim + 1), np.unique(data.col))
    assert len(free) >= n, (len(free), n)
    return np.sort(rng.choice(free, n, replace=False)).astype(np.int32)


def _replace_rows(base, new_rows, labels=None):
    """base with the rows of the dict {row: (cols, vals)} replaced (cols ascending)"""
    row_ptr, col, val = [0], [], []
    for i in range(base.n_rows):
        if i in new_rows:
            c, v = new_rows[i]
        else:
            b, e = int(base.row_ptr[i]), int(base.row_ptr[i + 1])
            c, v = base.col[b:e], base.val[b:e]
        col.append(np.asarray(c, np.int32)); val.append(np.asarray(v, np.float32))
        row_ptr.append(row_ptr[-1] + len(c))
    label = base.label.copy()
    for r, y in (labels or {}).items():
        label[r] = y
    return synth.Csr(base.dim, np.asarray(row_ptr, np.int64), np.concatenate(col).astype(np.int32),
                     np.concatenate(val).astype(np.float32), label)


# ---- the traits ------------------------------------------------------------------------------------------------------
def scaled(base, seed, k):
    """X' = 2^k X and w' = 2^-k w: every product x'w' is bit-equal to x w"""
    data = synth.Csr(base.dim, base.row_ptr.copy(), base.col.copy(), np.ldexp(base.val, k).astype(np.float32), base.label.copy())
    assert np.array_equal(np.ldexp(data.val.astype(np.float64), -k), base.val.astype(np.float64))   # exact: no under/overflow
    w = base_weights(base.dim, seed)
    return Hard(data, np.ldexp(w, -k), {"k": k, "w_unscaled": w, "vexp": vexp_of(base.val) + k})


def signed(base, seed, m=8, n_train=None):
    """planted pair p = rows (2p, 2p + 1) * stride: one worker's contiguous split holds both (they are < n_train / 8 apart)"""
    rng = np.random.default_rng(seed)
    n_train = base.n_rows if n_train is None else n_train
    val = base.val.copy()
    flip = rng.random(len(val)) < 0.5
    val[flip] = -val[flip]
    neg = synth.Csr(base.dim, base.row_ptr, base.col, val, base.label)
    priv = unused_columns(base, 3 * m, rng)
    stride = max(1, n_train // (4 * m))
    new_rows, labels, pairs = {}, {}, []
    for p in range(m):
        ra, rb = p * stride, p * stride + 1
        cols = priv[3 * p:3 * p + 3]
        v = (np.abs(rng.normal(size=3)) + 0.1).astype(np.float32)
        v /= np.float32(np.sqrt((v * v).sum()))
        y = 1 if p % 2 == 0 else -1
        new_rows[ra], new_rows[rb] = (cols, v), (cols, -v)
        labels[ra] = labels[rb] = y
        pairs.append((ra, rb))
    data = _replace_rows(neg, new_rows, labels)
    w = base_weights(base.dim, seed)
    w[priv] = 0.0
    return Hard(data, w, {"pairs": pairs, "private_columns": priv, "negated": int(flip.sum())})


def wide(base, seed, n_vanishing=6, per_column=5, n_train=None):
    """every entry times 2^-u, u uniform in 0..45; n_vanishing private columns appended to `per_column` rows each with
    u in 42..45 only"""
    rng = np.random.default_rng(seed)
    n_train = base.n_rows if n_train is None else n_train
    u = rng.integers(0, 46, size=len(base.val))
    val = np.ldexp(base.val, -u).astype(np.float32)
    spread = synth.Csr(base.dim, base.row_ptr, base.col, val, base.label)
    priv = unused_columns(base, n_vanishing, rng)
    hosts = rng.choice(n_train, size=n_vanishing * per_column, replace=False)
    new_rows = {}
    for t, r in enumerate(hosts.tolist()):
        b, e = int(spread.row_ptr[r]), int(spread.row_ptr[r + 1])
        c = np.append(spread.col[b:e], priv[t // per_column])
        v = np.append(spread.val[b:e], np.float32(math.ldexp(0.5 + 0.4 * rng.random(), -int(rng.integers(42, 46)))))
        order = np.argsort(c, kind="stable")
        new_rows[r] = (c[order], v[order])
    data = _replace_rows(spread, new_rows)
    w = base_weights(base.dim, seed)
    w[priv] = 0.0
    return Hard(data, w, {"vanishing_columns": priv, "host_rows": np.sort(hosts)})


def zero_margin(base, seed, m=12, n_train=None):
    """3 * m planted rows (kinds a, b, c in turn), spread over the first n_train rows; rows of kind (a) and (b) alternate
    labels.  planted: rows_a / rows_b / rows_c, and the columns they own."""
    rng = np.random.default_rng(seed)
    n_train = base.n_rows if n_train is None else n_train
    w = base_weights(base.dim, seed)
    priv = unused_columns(base, 5 * m, rng)
    ca, cb, cc = priv[:2 * m].reshape(m, 2), priv[2 * m:3 * m], priv[3 * m:].reshape(m, 2)
    rows = np.sort(rng.choice(n_train, size=3 * m, replace=False))
    tiny = np.float32(2.0 ** -34)   # above the constructor's filter as a value, below it as a product with itself
    new_rows, labels, out = {}, {}, {"rows_a": [], "rows_b": [], "rows_c": []}
    for t in range(m):
        ra, rb, rc = (int(r) for r in rows[3 * t:3 * t + 3])
        y = 1 if t % 2 == 0 else -1
        a = np.float32(0.25 + 0.5 * rng.random())
        wa = np.float32(rng.normal(scale=0.1) or 0.1)
        w[ca[t, 0]], w[ca[t, 1]] = float(wa), -float(wa)          # (a) a * wa + a * (-wa): +0.0 or -0.0, whatever the order
        new_rows[ra], labels[ra] = (ca[t], np.asarray([a, a], np.float32)), y
        w[cb[t]] = -y * 2.0 ** -34                                # (b) y * (x * w) = -2^-68 < 0 if the product survived
        new_rows[rb], labels[rb] = (cb[t:t + 1], np.asarray([tiny], np.float32)), y
        w[cc[t]] = 0.0                                            # (c) only columns of weight 0
        new_rows[rc], labels[rc] = (cc[t], np.asarray([0.6, -0.8], np.float32)), -y
        out["rows_a"].append(ra); out["rows_b"].append(rb); out["rows_c"].append(rc)
    data = _replace_rows(base, new_rows, labels)
    out.update(columns_a=ca, columns_b=cb, columns_c=cc)
    return Hard(data, w, out)


def ragged_data(seed, n_rows=6000):
    base = synth.generate(n_rows, seed=seed)
    rng = np.random.default_rng(seed)
    row_ptr, col, val = [0], [], []
    for i in range(n_rows):
        b, e = int(base.row_ptr[i]), int(base.row_ptr[i + 1])
        kind = rng.integers(0, 10)
        if kind == 0:
            pass  # empty row: Sparse.zeros
        elif kind == 1:
            col.append(base.col[b]); val.append(np.float32(1.0))  # single-element row
        else:
            c, v = base.col[b:e], base.val[b:e].copy()
            if kind == 2:
                v[0] = np.float32(1e-25)  # dropped by the Sparse constructor (math/Sparse.scala:112-114)
            col.extend(c.tolist()); val.extend(v.tolist())
        row_ptr.append(len(col))
    return synth.Csr(base.dim, np.asarray(row_ptr, np.int64), np.asarray(col, np.int32),
                              np.asarray(val, np.float32), base.label.copy())


def ragged64(seed, n_rows=6000, long_rows=((3000, 4), (8000, 2))):
    """ragged_data with `count` rows of `n` entries each for every (n, count) of long_rows"""
    base = ragged_data(seed, n_rows=n_rows)
    rng = np.random.default_rng(seed + 1)
    total = sum(c for _, c in long_rows)
    at = np.sort(rng.choice(n_rows * 3 // 4, size=total, replace=False)).tolist()
    new_rows, longs = {}, []
    for n, count in long_rows:
        for _ in range(count):
            r = at.pop(0)
            keys = np.sort(rng.choice(np.arange(1, base.dim + 1), size=n, replace=False))
            v = (np.abs(rng.normal(size=n)) + 0.1).astype(np.float32)
            v /= np.float32(np.sqrt((v * v).sum()))
            new_rows[r] = (keys, v)
            longs.append((r, n))
    return Hard(_replace_rows(base, new_rows), base_weights(base.dim, seed), {"long_rows": longs})


def lists_with(rng, n_train, k_workers, batch, must_hold=()):
    """k_workers lists of `batch` distinct rows from SplitStrategy.vanilla's contiguous splits of [0, n_train); every row of
    must_hold is in the list of the worker whose split holds it"""
    from oracle import ref_dict as rd

    split = rd.split_vanilla(n_train, k_workers)
    out = []
    for r in split:
        r = np.asarray(r)
        forced = np.asarray([x for x in must_hold if r[0] <= x <= r[-1]], dtype=np.int64)
        assert len(forced) <= batch, (len(forced), batch)
        rest = np.setdiff1d(r, forced)
        pick = rng.permutation(rest)[:batch - len(forced)]
        out.append(rng.permutation(np.concatenate([forced, pick])).astype(np.int32))
    return out


# ---- the cases both test modules use: one base, one data set per trait, the same lists on the CPU and on the GPU -------
N_ROWS, N_TRAIN, SEED = 12000, 10000, 3
TRAITS = ("scaled_p10", "scaled_m30", "signed", "wide", "zero_margin", "ragged64")
LISTS = {"k1b100": (1, 100), "k3b100": (3, 100), "k2b700": (2, 700), "k1b4096": (1, 4096)}   # name -> (workers, rows each)
RANGES = {"whole": [(0, N_TRAIN)], "halves": [(0, N_TRAIN // 2), (N_TRAIN // 2, N_TRAIN)]}
_CACHE = {}


def base():
    if "base" not in _CACHE:
        _CACHE["base"] = synth.generate(N_ROWS, seed=SEED)
    return _CACHE["base"]


def build(trait):
    """the Hard of a trait name (cached: the modules share them)"""
    if trait not in _CACHE:
        if trait == "plain":
            h = Hard(base(), base_weights(base().dim, SEED))
        elif trait.startswith("scaled_"):
            h = scaled(base(), SEED, {"p10": 10, "m30": -30}[trait[7:]])
        elif trait == "ragged64":
            h = ragged64(SEED, n_rows=N_ROWS)
        else:
            h = {"signed": signed, "wide": wide, "zero_margin": zero_margin}[trait](base(), SEED, n_train=N_TRAIN)
        _CACHE[trait] = h
    return _CACHE[trait]


def planted_rows(trait, h, small=False):
    """the rows a list of the trait must hold (small: lists of 100 rows per worker -- the one-workgroup kernel takes 192 work
    items per step, so those hold ONE 3,000-entry row and no 8,000-entry row)"""
    p = h.planted
    if trait == "signed":
        return [r for pair in p["pairs"] for r in pair]
    if trait == "wide":
        return p["host_rows"].tolist()
    if trait == "zero_margin":
        return p["rows_a"] + p["rows_b"] + p["rows_c"]
    if trait == "ragged64":
        return [r for r, n in p["long_rows"] if not small or n <= 3000][:1 if small else None]
    return []


def lists_of(trait, name):
    """the index lists `name` of a trait: seeded by both names, the planted rows inside"""
    key = (trait, name)
    if key not in _CACHE:
        k, b = LISTS[name]
        rng = np.random.default_rng([SEED, TRAITS.index(trait) if trait in TRAITS else 99, list(LISTS).index(name)])
        _CACHE[key] = lists_with(rng, N_TRAIN, k, b, planted_rows(trait, build(trait), small=b <= 100))
    return _CACHE[key]
