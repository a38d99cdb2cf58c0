"""ORACLE side (test infrastructure): the DERIVED error bound of a whole-range synchronous step.

The engine's whole-range gradient is a sum of fixed-point contributions round(y*x * 2^shift / vmax2) accumulated
EXACTLY (integers) and rounded to fp32 once.  Against the fp64 oracle fed the same weights the update of coordinate
j can therefore differ by at most

    lr/K * ( cnt_j * 2^-(shift+1) * vmax2        every contribution is off by at most half a grid unit
           + near_j )                            rows whose margin is within 1e-5 of zero may be gated differently
    + 8 * 2^-24 * (|w_j| + |w_j - w_j_before|)   fp32 roundings of the sum, the mean, the product and the subtraction
    + 2 * 2^-24 * lr/K * sum_k |g_k,j|           (index lists) EACH worker's exact sum is rounded to fp32 once and regularised
                                                 before the workers are folded: when two workers' gradients nearly cancel
                                                 in a coordinate, those roundings are large against the NET update the
                                                 line above prices (found at 2 workers x batch 7, lr 1)
    + 1e-9                                       the regulariser scalar s = 2*lambda*(w.ds) in fp32 vs fp64

cnt_j = non-zeros of column j in the rows of the step, near_j = sum of |x_j| over the near-zero-margin rows
(oracle.c orc_range_gate_profile).  No blanket tolerance: tests and bench.py's parity gate assert this bound per
coordinate and report the worst ratio error / bound.

DATA THAT IS NOT UNIT-NORM (tests/hard_data.py).  Three things above are tuned to rows of norm 1 and become optional
arguments that default to the behaviour above:

  rel_eps   The near-gate allowance |d| < 1e-5 is absolute.  The fp32 dot of a row of n entries, every product and every
            add rounded once (u = 2^-24, the weights and values already fp32), differs from the exact one by at most
            (n + 2) u * sum_i |x_i w_i| to first order, whatever the order of the adds.  So a row can be gated differently
            from the oracle only if 0 < |d| < rel_eps * sum_i |x_i w_i| with rel_eps = (n_max + 2) * 2^-24, n_max the
            longest row of the data (rel_gate_eps: 7.2e-5 at 1,200 entries, 4.8e-4 at 8,000).  d == 0 exactly is ON the
            gate, is decided the same way by both sides, and is never near.
  s_abs     The 1e-9 is an allowance on s.  With X' = 2^k X, w' = 2^-k w and the same lambda, s' = 2 lambda (w' . ds) is
            2^-k s exactly, so the same allowance in the scaled frame is 1e-9 * 2^-k.
  vanishing The VANISHING-COLUMN term (vanishing / vanished).  The regulariser is added on the support of a worker's sum
            only (math/Vec.scala:65-75).  A column whose exact sum g0_j is not 0 but whose fixed-point sum IS 0 leaves
            the engine's support and loses s: an error of exactly lr/K * s in the weight, which is no grid unit.  Every
            contribution is off by at most half a grid unit, so the integer sum can be 0 only when 0 < |g0_j| <= cnt_j *
            quantum (cand_j workers), and it must be 0 when every entry of the column is below half a unit (must_j).
            The allowance is therefore QUANTISED: the error minus m_j * lr/K * s, m_j an integer with must_j <= m_j <=
            cand_j, has to be within the bound above.  Nothing else fits under it.

OUTSIDE THE FP64 EXACT RANGE (out_of_range_bound).  The fp64 families sum round(y x 2^(shift - vexp)) in 64-bit integers
(shift = 62 - ceil(log2 n) for a list of n rows in csrc/dsgd_rp64.hpp, the layout's shift + 32 in csrc/dsgd_cs64.hpp).  An
entry whose lowest mantissa bit is at or above the grid unit 2^(vexp - shift) is exact; any other is off by at most half
a unit.  With out_j the number of such inexact entries of column j in a worker's ACTIVE-or-not rows (an upper count) the
worker's sum is off by at most out_j * 2^(vexp - shift - 1), a column that may vanish (|g0_j| <= out_j * that) loses
s as above (the same quantised term), and what is left is the in-range statement of the fp64 tests, 1e-12 * max(1, |ref|_inf).  No gate
allowance: the dots are fp64 on both sides.
"""

from __future__ import annotations

import numpy as np

GATE_EPS = 1e-5


def vmax2_of(val):
    m = float(np.abs(val).max()) if len(val) else 1.0
    if m <= 0.0:
        return 1.0
    return float(2.0 ** np.ceil(np.log2(m)))


def column_counts(o, lo, hi):
    b, e = int(o.row_ptr[lo]), int(o.row_ptr[hi])
    keep = np.abs(o.val[b:e]) > 1e-20
    return np.bincount(o.col[b:e][keep], minlength=o.dim + 1).astype(np.float64)


def step_bound(o, w_before, w_after_ref, ranges, lr, shift, vmax2=None, parts=False):
    """Per-coordinate bound on |w_engine - w_after_ref| after ONE synchronous step over `ranges` (one range per worker,
    mean over the workers) starting from w_before on both sides.  Returns (tol vector, rows near the gate)."""
    if vmax2 is None:
        vmax2 = vmax2_of(o.val)
    k = len(ranges)
    cnt = np.zeros(o.dim + 1)
    near = np.zeros(o.dim + 1)
    n_near = 0
    for lo, hi in ranges:
        cnt += column_counts(o, lo, hi)
        n, l1 = o.gate_profile(np.ascontiguousarray(w_before, dtype=np.float64), lo, hi, GATE_EPS)
        n_near += n
        near += l1
    quantum = vmax2 * 2.0 ** (-(shift + 1))
    tol = (lr / k) * (cnt * quantum + near)
    tol += 8.0 * 2.0 ** -24 * (np.abs(w_after_ref) + np.abs(w_after_ref - w_before)) + 1e-9
    if parts:
        return tol, n_near, (lr / k) * near   # (tol - this = the bound with every near-gate row gated as the oracle does)
    return tol, n_near


def worst_ratio(w_engine, w_ref, tol):
    r = np.abs(np.asarray(w_engine, dtype=np.float64) - w_ref) / tol
    j = int(np.argmax(r))
    return float(r[j]), j


def rel_gate_eps(o):
    """(n_max + 2) * 2^-24: the fp32 dot's round-off relative to sum |x_i w_i| for the longest row of the data"""
    n_max = int(np.diff(o.row_ptr).max()) if o.n_rows else 0
    return (n_max + 2) * 2.0 ** -24


def _flat(o, rows):
    rows = np.asarray(rows, dtype=np.int64)
    starts = o.row_ptr[rows]
    lens = o.row_ptr[rows + 1] - starts
    total = int(lens.sum())
    first = np.cumsum(lens) - lens
    flat = np.arange(total, dtype=np.int64) + np.repeat(starts - first, lens)
    return flat, np.repeat(np.arange(len(rows), dtype=np.int64), lens)


def _g0(o, w, rows):
    """a worker's sum WITHOUT the regulariser (orc_gradient at lambda = 0)"""
    keep, lam = o.last_stats, o.lam
    o.lam = 0.0
    try:
        return o.gradient(np.ascontiguousarray(w, dtype=np.float64), rows)
    finally:
        o.lam, o.last_stats = lam, keep


def reg_scalar(o, w):
    """s = 2 lambda (w . ds) (core/ml/SparseSVM.scala:31)"""
    p = np.asarray(w, dtype=np.float64) * o.ds
    p[np.abs(p) <= 1e-20] = 0.0
    return 2.0 * o.lam * float(p.sum())


def support_columns(o, w, rows, cnt, quantum):
    """columns of ONE worker whose exact sum is not 0 while the fixed-point sum may be: 0 < |g0_j| <= cnt_j * quantum"""
    g0 = np.abs(_g0(o, w, rows))
    return (g0 > 0.0) & (g0 <= cnt * quantum)


def _list_profile(o, w, rows, eps, rel_eps=None):
    """(cnt_j, near_j, rows near the gate) over the rows of an index list (numpy restatement of column_counts +
    orc_range_gate_profile for rows that are not a contiguous range).  rel_eps: near means 0 < |d| < rel_eps * sum |x_i w_i|."""
    rows = np.asarray(rows, dtype=np.int64)
    starts = o.row_ptr[rows]
    lens = o.row_ptr[rows + 1] - starts
    total = int(lens.sum())
    if total == 0:
        z = np.zeros(o.dim + 1)
        return z, z.copy(), 0
    first = np.cumsum(lens) - lens
    flat = np.arange(total, dtype=np.int64) + np.repeat(starts - first, lens)
    row_id = np.repeat(np.arange(len(rows), dtype=np.int64), lens)
    cols = o.col[flat]
    vals = o.val[flat].astype(np.float64)
    keep = np.abs(vals) > 1e-20                       # math/Sparse.scala:108-118
    cnt = np.bincount(cols[keep], minlength=o.dim + 1).astype(np.float64)
    prod = vals * np.asarray(w, dtype=np.float64)[cols]
    prod[np.abs(prod) <= 1e-20] = 0.0                 # math/Sparse.scala:46 -> :112-114
    d = np.bincount(row_id, weights=prod, minlength=len(rows))
    if rel_eps is None:
        near_rows = (np.abs(d) > 0.0) & (np.abs(d) < eps)
    else:
        near_rows = (np.abs(d) > 0.0) & (np.abs(d) < rel_eps * np.bincount(row_id, weights=np.abs(prod), minlength=len(rows)))
    mask = near_rows[row_id] & keep
    near = np.bincount(cols[mask], weights=np.abs(vals[mask]), minlength=o.dim + 1)
    return cnt, near, int(near_rows.sum())


def list_bound(o, w_before, w_after_ref, lists, lr, shift, vmax2=None, parts=False, rel_eps=None, s_abs=1e-9, rounding=True):
    """step_bound for index lists (one list per worker, mean over the workers): the index-list kernels accumulate the
    same fixed-point contributions exactly, at the shift the launch reports.  rel_eps / s_abs: see the module docstring;
    rounding=False leaves the per-worker rounding line out (row ranges: step_bound's statement, which has none)."""
    if vmax2 is None:
        vmax2 = vmax2_of(o.val)
    k = len(lists)
    cnt = np.zeros(o.dim + 1)
    near = np.zeros(o.dim + 1)
    n_near = 0
    for rows in lists:
        c, nr, n = _list_profile(o, w_before, rows, GATE_EPS, rel_eps)
        cnt += c
        near += nr
        n_near += n
    quantum = vmax2 * 2.0 ** (-(shift + 1))
    tol = (lr / k) * (cnt * quantum + near)
    tol += 8.0 * 2.0 ** -24 * (np.abs(w_after_ref) + np.abs(w_after_ref - w_before)) + s_abs
    if rounding:
        # every worker's own regularised sum, rounded once before the fold over the workers (Vec.sum, math/Vec.scala:128-131)
        keep = o.last_stats
        gabs = np.zeros(o.dim + 1)
        for rows in lists:
            gabs += np.abs(o.gradient(np.ascontiguousarray(w_before, dtype=np.float64), rows))
        o.last_stats = keep
        tol += 2.0 * 2.0 ** -24 * (lr / k) * gabs
    if parts:
        return tol, n_near, (lr / k) * near
    return tol, n_near


def gradient_bound(o, w, g_ref, rows, shift, vmax2=None, rel_eps=None, s_abs=1e-9):
    """list_bound for ONE worker's gradient (dsgd_gradient) instead of a step: half a grid unit per entry, the rows near
    the gate, two fp32 roundings of g (the exact sum, then g0 + s) with as many again for s_abs's scale, and s itself.
    Returns (tol, rows near the gate)."""
    if vmax2 is None:
        vmax2 = vmax2_of(o.val)
    cnt, near, n_near = _list_profile(o, w, rows, GATE_EPS, rel_eps)
    return cnt * vmax2 * 2.0 ** (-(shift + 1)) + near + 4.0 * 2.0 ** -24 * np.abs(g_ref) + s_abs, n_near


def vanishing(o, w_before, lists, half_units, counts=None):
    """The vanishing-column term, per coordinate, over the workers of a step (half_units[k]: half a grid unit of worker k;
    counts[k]: the entries that can be off by it, default every entry).  Returns (cand, must):
      cand_j  workers whose fixed-point sum of column j MAY be 0 while the exact sum is not: 0 < |g0_j| <= cnt_j * half
      must_j  of those, workers where it MUST be: every entry of the column in the worker's rows is below half a unit,
              so every contribution rounds to 0."""
    cand = np.zeros(o.dim + 1)
    must = np.zeros(o.dim + 1)
    for i, (rows, half) in enumerate(zip(lists, half_units)):
        cnt = _list_profile(o, w_before, rows, GATE_EPS)[0] if counts is None else counts[i]
        c = support_columns(o, w_before, rows, cnt, half)
        flat, _ = _flat(o, rows)
        big = np.zeros(o.dim + 1)
        np.maximum.at(big, o.col[flat], np.abs(o.val[flat].astype(np.float64)))
        cand += c
        must += c & (big < half)
    return cand, must


def vanished(diff, base_tol, unit, cand):
    """How many workers' sums of each column vanished in the engine, read off the error: a worker whose column left the
    support misses exactly `unit` (lr/K * s in a weight, -s in a gradient).  m_j = the integer in [0, cand_j] nearest
    diff_j / unit; returns (m, residual |diff - m * unit| / base_tol): the residual must be within the bound that has NO
    support term, so the allowance is quantised -- whole regularisers of candidate workers, nothing else."""
    diff = np.asarray(diff, dtype=np.float64)
    m = np.zeros(len(diff)) if unit == 0.0 else np.clip(np.rint(diff / unit), 0, cand)
    return m, np.abs(diff - m * unit) / base_tol


def inexact_counts(o, rows, vexp, shift):
    """out_j: entries of column j in the rows (duplicates count) that are NOT a whole number of grid units 2^(vexp - shift)"""
    flat, _ = _flat(o, rows)
    vals = o.val[flat].astype(np.float64)
    q = np.ldexp(vals, shift - vexp)
    bad = (np.abs(vals) > 1e-20) & (q != np.rint(q))
    return np.bincount(o.col[flat][bad], minlength=o.dim + 1).astype(np.float64)


def out_of_range_bound(o, w_before, ref, lists, shifts, vexp, lr=None):
    """Per-coordinate bound for the fp64 families on entries outside the exact range (module docstring) WITHOUT the
    support term: on a worker's gradient (lr None, one list, ref = orc_gradient) or on the weights after a synchronous
    step (ref = orc_sync_step's).  Returns (base tol, cand, must, unit): see vanishing / vanished."""
    k = len(lists)
    scale = 1.0 if lr is None else lr / k
    halves = [2.0 ** (vexp - shift - 1) for shift in shifts]
    outs = [inexact_counts(o, rows, vexp, shift) for rows, shift in zip(lists, shifts)]
    grid = sum(out * half for out, half in zip(outs, halves))
    cand, must = vanishing(o, w_before, lists, halves, outs)
    s = reg_scalar(o, w_before)
    return scale * grid + 1e-12 * max(1.0, float(np.abs(ref).max())), cand, must, (-s if lr is None else scale * s)
