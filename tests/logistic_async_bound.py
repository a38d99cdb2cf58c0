"""Error bounds of the logistic model's ASYNCHRONOUS update (csrc/dsgd_logistic.hpp: dsgd_lg_async_finish_kernel; csrc/dsgd_lg_cs_async.hpp:
dsgd_lg_cs_async_kernel) against tests/logistic_async_ref.py, DERIVED from the operation order, and an honest emulation of that order.
tests/logistic_bound.py and tests/logistic_cs_bound.py are imported untouched.

u = 2^-24, v = 2^-53, E_j >= |w_j - w_ref,j| carried from update to update: as there.  One update over a list of n rows:

data_j   on |G_dev,j - G_ref,j|, G the sum of c_i x_ij over the list.  The sums are lg_grad_body's with K = 1 on S = lg_shift(n) and
         the finish converts them as LG_STEP does, so this is logistic_bound.dsum (row form: its dz) or logistic_cs_bound.dsum
         (slice form: the slice dz) WITHOUT the term the regulariser's E adds:   data_j = dsum_j - 2 lambda E_j
         (dsum's 4 v (|G| + |2 lambda w|) stays in: it covers the conversion's rounding and is kept as slack).
dr_j     gm = G / n (one rounding, v |gm|); 2 lambda w_j (v |reg|, and the device's w_j is within E_j); their sum (v |r|):
             base_j = data_j / n + 2 lambda E_j,      dr_j = base_j + 4 v (|gm_ref,j| + |reg_ref,j| + base_j)
ddelta_j delta = lr r, one rounding, lr the same double on both sides:   ddelta_j = lr dr_j + v lr (|r_ref,j| + dr_j)
dw_j     w - delta in fp64 (one rounding), then the ONE rounding to float:
             e_j = E_j + ddelta_j + v (|w_ref,j| + E_j + |delta_ref,j| + ddelta_j),      dw_j = e_j + u (|w'_ref,j| + e_j) + 2^-150
No measured constant.  A peer's update w_k = (float)((double)w_k - dv_k) with the SAME dv is the last line with ddelta = 0.
"""

import numpy as np

import logistic_async_ref as aref
import logistic_bound as lb
import logistic_cs_bound as cb

U, V = lb.U, lb.V


def dstep(csr, w, idx, lr, lam, E=None, slices=False):
    """(dw, ddelta, w'_ref, delta_ref): E' >= |w' - w'_ref| and the bound on |delta - delta_ref| of one update from weights
    within E of w (the reference's, float64)."""
    w64 = np.asarray(w, dtype=np.float64)
    E = np.zeros_like(w64) if E is None else np.asarray(E, dtype=np.float64)
    n = float(len(idx))
    ds, Gref, reg = (cb.dsum if slices else lb.dsum)(csr, w64, idx, lam, E)
    data = ds - 2.0 * lam * E
    base = data / n + 2.0 * lam * E
    gm = Gref / n
    dr = base + 4.0 * V * (np.abs(gm) + np.abs(reg) + base)
    lr = float(lr)
    r = gm + reg
    ddelta = lr * dr + V * lr * (np.abs(r) + dr)
    delta = lr * r
    wn = w64 - delta
    e = E + ddelta + V * (np.abs(w64) + E + np.abs(delta) + ddelta)
    return e + U * (np.abs(wn) + e) + 2.0 ** -150, ddelta, wn, delta


def dupdate(w, dv, E=None):
    """E' after a peer's update with the same dv on both sides"""
    w64 = np.asarray(w, dtype=np.float64)
    E = np.zeros_like(w64) if E is None else np.asarray(E, dtype=np.float64)
    wn = w64 - np.asarray(dv, dtype=np.float64)
    e = E + V * (np.abs(w64) + E + np.abs(dv))
    return e + U * (np.abs(wn) + e) + 2.0 ** -150


# ---- the emulation: the kernels' own order, in numpy ---------------------------------------------------------------------
# The mistakes this finish invites (tests/test_logistic_async_bound.py):
#   mean_over_K        the mean over the K = 1 workers (LG_STEP's), not over the n rows
#   reg_over_n         the regulariser divided by n too: (G + 2 lambda w) / n
#   shift_from_batch   the finish scales with the shift of the PLAN's batch, not of the list's own length (a short last list)
#   delta_float        the delta rounded to float before the subtraction
#   lr_data_only       lr applied to the data term only: w - (lr gm + 2 lambda w)
MUTATIONS = ("mean_over_K", "reg_over_n", "shift_from_batch", "delta_float", "lr_data_only")


def emu_step(csr, w32, idx, lr, lam, mut=None, plan_batch=None, d=None):
    """(w' float32, delta float64) of dsgd_lg_grad_kernel (logistic_bound.emu_acc) + dsgd_lg_async_finish_kernel"""
    _, _, val, _ = lb._csr(csr)
    w32 = np.asarray(w32, dtype=np.float32)
    wj = w32.astype(np.float64)
    acc, S = lb.emu_acc(csr, w32, idx, d=d)
    if mut == "shift_from_batch":
        S = lb.shift(plan_batch)
    n = float(len(idx))
    G = acc.astype(np.float64) * 2.0 ** (lb.vexp_of(val) - S)
    reg = (2.0 * lam) * wj
    lr = float(lr)
    if mut == "reg_over_n":
        r = (G + reg) / n
    else:
        gm = G if mut == "mean_over_K" else G / n
        r = gm + reg
    delta = lr * gm + reg if mut == "lr_data_only" else lr * r
    if mut == "delta_float":
        delta = delta.astype(np.float32).astype(np.float64)
    return (wj - delta).astype(np.float32), delta


def reference_inside(csr, w32, idx, lr, lam, slices=False):
    """the float64 reference, rounded to float, against its own bound (a bound the reference left would be no bound)"""
    dw, dd, wn, delta = dstep(csr, w32, idx, lr, lam, slices=slices)
    w2, d2 = aref.async_step(csr, np.asarray(w32, dtype=np.float64), idx, lr, lam)
    return bool(np.all(np.abs(wn.astype(np.float32).astype(np.float64) - w2) <= dw) and np.all(np.abs(delta - d2) <= dd))
