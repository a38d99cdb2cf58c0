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
  concentrated  NOT the RCV1-like base: rows of 2 to 4 entries, column P in EVERY row with y * vmax and column M with
                -y * vmax (every contribution y * x is +vmax / -vmax: the largest value of the data in one column of every
                row with one sign), vmax = 1 (vexp's power-of-two branch) or the largest value below 2 (a contribution that
                rounds UP to 2^shift).  With the weights at zero every row is active and the sums are n * vmax in closed form:
                every integer accumulator of every family runs at the full scale its host rule allows (concentrated below,
                and the host rules restated in Python beside it).
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


# ---- concentrated columns: every accumulator at full scale --------------------------------------------------------------
# Host rules of csrc/dsgd_hip.hip restated (tests/test_hard_data.py pins them on the CPU, tests/test_gpu_hard_values.py
# holds the shift a launch REPORTS against them).
WS_SLOTS, WS_MAXROWS, CT_MAXROWS, FIX_SHIFT_CAP, RP64_HOT, FSTEP_ROWS = 512, 254, 128, 21, 1024, 512
HSPLIT_DEFAULT = 18000   # (any rank the concentrated data uses is far below the library's default split)
N_CU = 256               # MI355X; the GPU tests pass the device's own count


def ceil_log2(n):
    b = 0
    while (1 << b) < n:
        b += 1
    return b


def shift_of_rows(rows, cap=None):
    """the general rule: rows(b) <= 2^bits, shift = 30 - bits (capped where the launch caps it)"""
    s = 30 - ceil_log2(rows)
    return s if cap is None else max(1, min(cap, s))


def refined_shift(shift0, a_max, rows, cap=FIX_SHIFT_CAP):
    """dsgd_wseg_bound_kernel / dsgd_fstep_bound_kernel's host side: the finest s with 2^(s - s0) * A + rows <= 2^30"""
    s = shift0
    while s < cap and math.ldexp(float(a_max), s + 1 - shift0) <= float((1 << 30) - rows):
        s += 1
    return s


def column_ranks(data):
    """the library's ranking: count over ALL loaded rows descending, ties by ascending key -> rank_of_key [dim + 1]"""
    cnt = np.bincount(data.col, minlength=data.dim + 1)
    order = np.argsort(-cnt, kind="stable")
    rank = np.empty(data.dim + 1, np.int64)
    rank[order] = np.arange(data.dim + 1)
    return rank


def stream_slots(data, hsplit=HSPLIT_DEFAULT):
    """slot offsets of the hot and the cold stream (build_split: a tiled row owns at least one slot in each)"""
    hot_e = column_ranks(data)[data.col] < min(hsplit, data.dim + 1)
    row_id = np.repeat(np.arange(data.n_rows), np.diff(data.row_ptr))
    hot = np.bincount(row_id, weights=hot_e, minlength=data.n_rows).astype(np.int64)
    cold = np.diff(data.row_ptr) - hot
    assert hot.max() <= WS_SLOTS - 8 and cold.max() <= WS_SLOTS - 8   # (no long rows here)
    hrp = np.concatenate([[0], np.cumsum(np.maximum(hot, 1))])
    ctp = np.concatenate([[0], np.cumsum(np.maximum(cold, 1))])
    return hrp, ctp


def wave_tiles(slot_ptr, rb, re, max_rows=WS_MAXROWS):
    """append_wave_tiles for rows without empty or long ones: the first row of every tile of [rb, re)"""
    r0, start = [], -1
    for i in range(rb, re):
        if start >= 0 and (slot_ptr[i + 1] - (slot_ptr[start] & ~7) > WS_SLOTS - 1 or i - start >= max_rows):
            start = -1
        if start < 0:
            start = i
            r0.append(i)
    return r0


def streaming_worst_rows(data, ranges, n_cu=N_CU, hsplit=HSPLIT_DEFAULT):
    """launch_stream: workgroup b of a worker owns the 16-tile groups b, b + grid.x, ...; the rows of a group are counted
    between the first rows of tiles (the tiles cover ALL loaded rows)"""
    import bisect

    hrp, _ = stream_slots(data, hsplit)
    wr0 = wave_tiles(hrp, 0, data.n_rows) + [data.n_rows]
    spans = []
    for lo, hi in ranges:
        tb = max(0, bisect.bisect_right(wr0, lo, 0, len(wr0) - 1) - 1)
        te = max(tb, bisect.bisect_left(wr0, hi, 0, len(wr0) - 1))
        spans.append((tb, te))
    per_worker = max(1, n_cu // len(ranges))
    gx = max(1, min(per_worker, (max(max(te - tb for tb, te in spans), 1) + 15) // 16))
    worst = 1
    for tb, te in spans:
        rows_of = [0] * gx
        for g, t in enumerate(range(tb, te, 16)):
            rows_of[g % gx] += wr0[min(t + 16, te)] - wr0[t]
        worst = max(worst, max(rows_of))
    return worst


def chunk_worst_rows(data, ranges, n_cu=N_CU, hsplit=HSPLIT_DEFAULT, fstep_rows=FSTEP_ROWS):
    """fstep_grid + fstep_build before any rebalance: n_wg chunks per worker of equal WEIGHT (slots of both streams + 2 per
    row), cut at the first row whose weight prefix reaches the target; the largest chunk's rows"""
    hrp, ctp = stream_slots(data, hsplit)
    W = hrp + ctp + 2 * np.arange(data.n_rows + 1)
    per_worker = max(1, n_cu // len(ranges))
    n_wg = max(1, min(per_worker, min(hi - lo for lo, hi in ranges) // fstep_rows))
    worst = 1
    for lo, hi in ranges:
        w0, wtot, cut = int(W[lo]), int(W[hi] - W[lo]), lo
        for b in range(n_wg):
            nxt = hi
            if b + 1 < n_wg:
                target = w0 + int(float(wtot) * float(b + 1) / float(n_wg))
                nxt = cut + int(np.searchsorted(W[cut:hi + 1], target, side="left"))
            worst = max(worst, nxt - cut)
            cut = nxt
    return worst, n_wg


def cold_shift_rule(data, hsplit=HSPLIT_DEFAULT):
    """build_split's scale of the cold words (dsgd_cold_bound_kernel): A = the largest column sum of ceil(|x| 2^21 / vmax2)
    inside one cold tile; the finest s <= 21 with 2^28 + 2^s + 32 * (2^(s - 21) A + 256) < 2^30"""
    rank = column_ranks(data)
    h = min(hsplit, data.dim + 1)
    _, ctp = stream_slots(data, hsplit)
    r0 = wave_tiles(ctp, 0, data.n_rows, CT_MAXROWS) + [data.n_rows]
    _, e = math.frexp(float(np.abs(data.val).max()))
    vexp = e - 1 if float(np.abs(data.val).max()) == 2.0 ** (e - 1) else e
    a = 0
    for t in range(len(r0) - 1):
        lo = int(ctp[r0[t]]) & ~7   # (the window starts at a multiple of 8 slots: up to 7 slots of the rows before count too)
        first = int(np.searchsorted(ctp, lo, side="right")) - 1
        b, e_ = int(data.row_ptr[first]), int(data.row_ptr[r0[t + 1]])
        cold = rank[data.col[b:e_]] >= h
        if cold.any():
            q = np.ceil(np.abs(data.val[b:e_][cold].astype(np.float32)) * np.float32(2.0 ** (21 - vexp))).astype(np.int64)
            a = max(a, int(np.bincount(data.col[b:e_][cold], weights=q).max()))
    s = FIX_SHIFT_CAP
    while s > 1 and 2 ** 28 + 2 ** s + 32 * (math.ldexp(a, s - 21) + 256) >= 2 ** 30:
        s -= 1
    return s, a


VMAX = {"one": 1.0, "below2": float(np.float32(2.0) - np.float32(2.0 ** -23))}   # vexp 0 (power-of-two branch) / vexp 1
VMAX64 = {"one": 1.0, "below2": 2.0 - 2.0 ** -52}                                 # the Double twins
CONC_DIM, CONC_P, CONC_M, CONC_SEED, CONC_POOL = 47236, 7, 9, 17, 16384
CONC_ORDINARY = np.arange(20, 26, dtype=np.int32)     # the third and fourth entries
CONC_FILLER = np.arange(1000, 2200, dtype=np.int32)   # four tail rows of 300: 1,200 columns ranked before CONC_COLD
CONC_COLD = CONC_DIM                                  # the duplicate list's column: count 1, the largest key
CONC_RANGE_MIN = 8192   # tests/test_gpu_hard_values.py RANGE_FAMILIES: DSGD_STREAM_MIN (row_chunks start at 4,096)


def _conc_rows(which, double):
    """the pool of CONC_POOL candidate train rows: (row_ptr, col, val float64, label); the same shape and labels for both vmax"""
    vmax = (VMAX64 if double else VMAX)[which]
    rng = np.random.default_rng(CONC_SEED)
    extra = rng.integers(0, 3, size=CONC_POOL)                  # 0, 1 or 2 ordinary entries
    label = np.where(rng.random(CONC_POOL) < 0.5, 1, -1).astype(np.int8)
    row_ptr = np.concatenate([[0], np.cumsum(2 + extra)]).astype(np.int64)
    col = np.empty(row_ptr[-1], np.int32)
    val = np.empty(row_ptr[-1], np.float64)
    for i in range(CONC_POOL):
        b, y = int(row_ptr[i]), float(label[i])
        col[b], val[b], col[b + 1], val[b + 1] = CONC_P, y * vmax, CONC_M, -y * vmax
        c = np.sort(rng.choice(CONC_ORDINARY, size=int(extra[i]), replace=False))
        v = 0.25 * vmax * (1.0 - 0.999 * rng.random(len(c)))    # in (0, vmax / 4]
        col[b + 2:b + 2 + len(c)] = c
        val[b + 2:b + 2 + len(c)] = v if double else v.astype(np.float32)
    return row_ptr, col, val, label


def _conc_data(which, double, n_train):
    """n_train pool rows, four filler rows and the duplicate list's row (its only full-scale entry in CONC_COLD)"""
    vmax = (VMAX64 if double else VMAX)[which]
    row_ptr, col, val, label = _conc_rows(which, double)
    rng = np.random.default_rng(CONC_SEED + 1)
    e = int(row_ptr[n_train])
    cols, vals, lens, labels = [col[:e]], [val[:e]], [np.diff(row_ptr[:n_train + 1])], [label[:n_train]]
    for part in CONC_FILLER.reshape(4, -1):
        v = 0.25 * vmax * (1.0 - 0.999 * rng.random(len(part)))
        cols.append(part); vals.append(v if double else v.astype(np.float32)); lens.append([len(part)]); labels.append([1])
    cols.append(np.asarray([CONC_ORDINARY[0], CONC_COLD], np.int32)); vals.append(np.asarray([0.125 * vmax, -vmax]))
    lens.append([2]); labels.append([-1])   # y * x = +vmax on CONC_COLD
    val_all = np.concatenate(vals)
    data = synth.Csr(CONC_DIM, np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64), np.concatenate(cols).astype(np.int32),
                     val_all if double else val_all.astype(np.float32), np.concatenate(labels).astype(np.int8))
    return data


def concentrated_rows():
    """The smallest number of train rows (a multiple of 256, at least what the range families' dispatch needs) at which
    BOTH the streaming launch and the row chunks get shift0 < 21 over the whole range: the worst workgroup's rows above 512,
    by the 16-tile groups of launch_stream and the weight cut of fstep_build at 256 CUs."""
    if "conc_rows" not in _CACHE:
        n = CONC_RANGE_MIN
        while True:
            d = _conc_data("one", False, n)
            if streaming_worst_rows(d, [(0, n)]) > 512 and chunk_worst_rows(d, [(0, n)])[0] > 512:
                break
            n += 256
            assert n <= CONC_POOL
        _CACHE["conc_rows"] = n
    return _CACHE["conc_rows"]


def concentrated(which, double=False):
    """Hard: data (float32 values, or float64 for the Double twin), w = 0, planted = P, M, vmax, n_train, the row the
    duplicate list names and its cold column"""
    key = ("concentrated", which, double)
    if key not in _CACHE:
        n = concentrated_rows()
        data = _conc_data(which, double, n)
        _CACHE[key] = Hard(data, np.zeros(CONC_DIM + 1), {"P": CONC_P, "M": CONC_M, "vmax": (VMAX64 if double else VMAX)[which], "n_train": n,
                                                          "dup_row": data.n_rows - 1, "cold_column": CONC_COLD})
    return _CACHE[key]


def conc_lists(n_train, k, b, seed=0):
    """k lists of b DISTINCT train rows, one per contiguous split (k and b powers of two in the exact legs)"""
    rng = np.random.default_rng([CONC_SEED, k, b, seed])
    bounds = np.linspace(0, n_train, k + 1).astype(np.int64)
    return [np.sort(rng.choice(np.arange(bounds[i], bounds[i + 1]), size=b, replace=False)).astype(np.int32) for i in range(k)]
