"""Error bounds of the logistic kernels against tests/logistic_ref.py, DERIVED from the kernels' operation order
(csrc/dsgd_logistic.hpp), and an honest emulation of those kernels in numpy.  The pattern of tests/dense_bound.py.

u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64).  gamma(k) = k u / (1 - k u).  E_j >= |w_j - w_ref,j| is what the weights
already differ by when the call starts (zero for set weights; carried from step to step by `step`).

dz_i   on |d_i - d_ref,i|.  A row of nnz_i entries is read by 16 lanes, lane s taking entries s, s + 16, ...: m_i =
       ceil(nnz_i / 16) products, each rounded once, added sequentially from 0 (m_i - 1 roundings), then the four steps of
       group_sum: a term passes through at most m_i + 4 roundings, so
           dz_i = gamma(m_i + 4) * sum_j |x_ij| (|w_j| + E_j)  +  sum_j |x_ij| E_j  +  nnz_i * (1e-20 + 2^-149)
       (a product of magnitude <= 1e-20 is dropped by the engine's filter; a product may round into the subnormals).
dc_i   c = -y / (1 + exp(y d)) has |dc/dd| = sigma' <= 1/4; the fp64 evaluation on either side makes at most 8 roundings of
       relative 2^-52 on a value of magnitude <= 1:   dc_i = dz_i / 4 + 2^-49.   The same bounds |p - p_ref| before p's one
       rounding to float (+ 2^-25: half an ulp of a float in [0.5, 1]).
dg_j   one worker's regularised sum.  Every added entry is c x 2^(S - vexp) rounded in fp64 (v |x|) and to the integer grid
       (half a unit, 2^(vexp - S - 1)); the finish converts the sum (v |G|), forms 2 lambda w (v) and adds (v); the
       regulariser sees E_j; g is rounded to float once:
           dsum_j = sum_i |x_ij| (dc_i + v) + cnt_j 2^(vexp - S - 1) + 2 lambda E_j + 4 v (|G_j| + |2 lambda w_j|)
           dg_j   = dsum_j + u (|r_j| + dsum_j) + 2^-150
dw_j   after a step: the mean of the workers' dsum, times lr, the fp64 update (2 v) and the ONE rounding to float:
           dw_j = E_j + lr mean_k dsum_kj + 2 v (|w_j| + lr |mean_j|) + u (|w'_j| + that) + 2^-150
dloss  every l_i has |dl/da| <= 1:  mean_i (dz_i + 8 v (1 + l_i)); the fixed-order tree adds (n + 64) v of the mean; |w|^2 is
       taken from the same float weights on both sides in fp64: (dp + 8) v |w|^2.  (E = 0: the loss is compared on equal
       weights.)
"""

import numpy as np

import logistic_ref as ref

U = 2.0 ** -24
V = 2.0 ** -53
G = 16
UNR = 4


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def vexp_of(val):
    """The library's rule: the smallest e with 2^e >= max |value| (vmax a power of two: e itself)."""
    vmax = float(np.max(np.abs(val))) if len(val) else 0.0
    if vmax <= 0.0:
        return 1   # frexp(1.0) = (0.5, 1), and 1.0 is a power of two only when vmax > 0 is
    m, e = np.frexp(np.float32(vmax))
    return int(e) - 1 if m == 0.5 else int(e)


def shift(n):
    n = int(n)
    return 62 - (n - 1).bit_length() if n > 1 else 62


def _csr(csr):
    row_ptr = np.asarray(csr[0], dtype=np.int64)
    nnz = int(row_ptr[-1])
    return row_ptr, np.asarray(csr[1][:nnz], dtype=np.int64), np.asarray(csr[2][:nnz], dtype=np.float32), np.asarray(csr[3])


def dz(csr, w, E=None):
    row_ptr, col, val, _ = _csr(csr)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    w = np.abs(np.asarray(w, dtype=np.float64))
    E = np.zeros_like(w) if E is None else np.asarray(E, dtype=np.float64)
    ax = np.abs(val.astype(np.float64))
    A = np.bincount(rows, weights=ax * (w + E)[col], minlength=n)
    P = np.bincount(rows, weights=ax * E[col], minlength=n)
    nnz = np.diff(row_ptr).astype(np.float64)
    m = np.ceil(nnz / G)
    return gamma(m + 4) * A + P + nnz * (1e-20 + 2.0 ** -149)


def dc(dz_i):
    return dz_i / 4.0 + 2.0 ** -49


def dsum(csr, w, idx, lam, E=None):
    """(dsum_j, G_ref, reg_ref) of one worker's list."""
    row_ptr, col, val, _ = _csr(csr)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    w64 = np.asarray(w, dtype=np.float64)
    E = np.zeros_like(w64) if E is None else np.asarray(E, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    mult = np.bincount(idx, minlength=n).astype(np.float64)
    dci = dc(dz(csr, w, E)) + V
    ax = np.abs(val.astype(np.float64))
    t1 = np.bincount(col, weights=ax * (dci * mult)[rows], minlength=len(w64))
    cnt = np.bincount(col, weights=mult[rows], minlength=len(w64))
    unit = 2.0 ** (vexp_of(val) - shift(len(idx)) - 1)
    Gref, _ = ref.data_sum(csr, w64, idx)
    reg = 2.0 * lam * w64
    return t1 + cnt * unit + 2.0 * lam * E + 4.0 * V * (np.abs(Gref) + np.abs(reg)), Gref, reg


def dg(csr, w, idx, lam):
    ds, Gref, reg = dsum(csr, w, idx, lam)
    return ds + U * (np.abs(Gref + reg) + ds) + 2.0 ** -150


def dw(csr, w, lists, lr, lam, E=None):
    """E' >= |w' - w'_ref| after one step from weights that differ by at most E."""
    w64 = np.asarray(w, dtype=np.float64)
    E = np.zeros_like(w64) if E is None else np.asarray(E, dtype=np.float64)
    tot = np.zeros_like(w64)
    mean = np.zeros_like(w64)
    for idx in lists:
        ds, Gref, reg = dsum(csr, w, idx, lam, E)
        tot += ds
        mean += Gref + reg
    tot /= len(lists)
    mean /= len(lists)
    lr = float(lr)
    wn = w64 - lr * mean
    e = E + lr * tot + 2.0 * V * (np.abs(w64) + lr * np.abs(mean))
    return e + U * (np.abs(wn) + e) + 2.0 ** -150


def dloss(csr, w, row_begin, row_end, lam):
    y = np.asarray(csr[3], dtype=np.float64)[row_begin:row_end]
    w64 = np.asarray(w, dtype=np.float64)
    d = ref.dots(csr, w64)[row_begin:row_end]
    li = ref.row_loss(d, y)
    n = row_end - row_begin
    per = np.mean(dz(csr, w)[row_begin:row_end] + 8.0 * V * (1.0 + li))
    return per + (n + 64) * V * float(np.mean(li)) + lam * (len(w64) + 8) * V * float(np.dot(w64, w64))


# ---- the emulation: the kernels' own order, in numpy ------------------------------------------------------------------
_PERMS = [np.arange(G) ^ 1, np.arange(G) ^ 2, (np.arange(G) & 8) | (7 - (np.arange(G) & 7)), 15 - np.arange(G)]


def emu_dot(row_ptr, col, val, w32, row):
    """row_dot<16, 4> + group_sum<16>: lane s adds its products in entry order from 0, then the four pairings."""
    st, en = int(row_ptr[row]), int(row_ptr[row + 1])
    acc = np.zeros(G, dtype=np.float32)
    for p0 in range(st, en, G):
        k = min(G, en - p0)
        prod = val[p0:p0 + k] * w32[col[p0:p0 + k]]          # float32 * float32, rounded once
        prod = np.where(np.abs(prod) > np.float32(1e-20), prod, np.float32(0.0))
        acc[:k] = acc[:k] + prod
    for pm in _PERMS:
        acc = acc + acc[pm]
    return acc[0]


def emu_dots(csr, w32, rows):
    row_ptr, col, val, _ = _csr(csr)
    w32 = np.asarray(w32, dtype=np.float32)
    return {int(r): emu_dot(row_ptr, col, val, w32, int(r)) for r in np.unique(np.asarray(rows, dtype=np.int64))}


def ranks_of(csr, dp):
    """The library's column ranking: the count over ALL loaded rows descending, ties by ascending key -> rank of every key."""
    _, col, _, _ = _csr(csr)
    order = np.argsort(-np.bincount(col, minlength=dp), kind="stable")
    rank = np.empty(dp, dtype=np.int64)
    rank[order] = np.arange(dp)
    return rank


ACC_MUTATIONS = ("drop_last", "label_by_position", "flip_sign", "vexp_qscale", "fold_2048")


def emu_acc(csr, w32, idx, mut=None, n_for_shift=None, d=None):
    """One worker's int64 column sums (python ints: exact) and its shift.  mut: a mutation's name (tests only).  d: the dots
    of emu_dots for (at least) the listed rows, where the caller has them already."""
    row_ptr, col, val, label = _csr(csr)
    idx = np.asarray(idx, dtype=np.int64)
    S = shift(len(idx) if n_for_shift is None else n_for_shift)
    if mut == "drop_last":
        idx = idx[:-1]
    # vexp_qscale: vexp one too large where the entries are scaled ONLY (the finish keeps the right one)
    qscale = 2.0 ** (S - vexp_of(val) - (1 if mut == "vexp_qscale" else 0))
    if d is None:
        d = emu_dots(csr, w32, idx)
    at = col
    if mut == "fold_2048" and len(w32) > 2048:   # the first rank beyond the LDS head lands on the head's last word
        rank = ranks_of(csr, len(w32))
        at = np.where(rank[col] == 2048, int(np.where(rank == 2047)[0][0]), col)
    acc = np.zeros(len(w32), dtype=np.int64)
    for t, r in enumerate(idx):
        y = float(label[t % len(label)] if mut == "label_by_position" else label[r])
        with np.errstate(over="ignore"):
            c = -y / (1.0 + np.exp(y * float(d[int(r)])))
        if mut == "flip_sign":
            c = -c
        st, en = int(row_ptr[r]), int(row_ptr[r + 1])
        q = np.rint(val[st:en].astype(np.float64) * (c * qscale)).astype(np.int64)
        np.add.at(acc, at[st:en], q)
    return acc, S


def _finish_vexp(val, mut):
    """vexp_finish: vexp one too large in the finish ONLY"""
    return vexp_of(val) + (1 if mut == "vexp_finish" else 0)


def emu_gradient(csr, w32, idx, lam, mut=None, d=None):
    _, _, val, _ = _csr(csr)
    w32 = np.asarray(w32, dtype=np.float32)
    acc, S = emu_acc(csr, w32, idx, mut if mut in ACC_MUTATIONS else None, d=d)
    Gk = acc.astype(np.float64) * 2.0 ** (_finish_vexp(val, mut) - S)
    g = (Gk + (2.0 * lam) * w32.astype(np.float64)).astype(np.float32)
    if mut == "skip_last_column":   # the gradient goes out in KEY order: key dp - 1 keeps the zero of the output buffer
        g[-1] = 0.0
    return g


def emu_step(csr, w32, lists, lr, lam, mut=None, d=None):
    _, _, val, _ = _csr(csr)
    w32 = np.asarray(w32, dtype=np.float32)
    wj = w32.astype(np.float64)
    reg = (2.0 * lam) * wj
    total = np.zeros_like(wj)
    for k, idx in enumerate(lists):
        wrong_n = len(lists[(k + 1) % len(lists)]) if mut == "wrong_worker_shift" else None
        acc, S = emu_acc(csr, w32, idx, mut if mut in ACC_MUTATIONS else None, d=d)
        if wrong_n is not None:
            S = shift(wrong_n)   # (the finish reads another worker's length)
        Gk = acc.astype(np.float64) * 2.0 ** (_finish_vexp(val, mut) - S)
        if mut == "support_only_reg":
            total = total + (Gk + np.where(acc != 0, reg, 0.0))
        else:
            total = total + (Gk + reg)
    mean = total if mut == "no_mean" else total / float(len(lists))
    wn = (wj - float(np.float32(lr)) * mean).astype(np.float32)
    if mut == "skip_last_column":   # a step walks the columns in RANK order: the column of rank dp - 1 keeps its weight
        last = int(np.where(ranks_of(csr, len(w32)) == len(w32) - 1)[0][0])
        wn[last] = w32[last]
    return wn
