"""The fp64 reference of softmax regression (include/dsgd.h "SOFTMAX") in numpy over CSR arrays -- z_ic = x_i . w_c, p = softmax(z_i),
l_i = logsumexp(z_i) - z_iy, G_c = sum_i (p_ic - [c == y_i]) x_i + 2 lambda w_c, w_c <- w_c - lr mean_k G_kc -- and the kernels' error
bounds against it (csrc/dsgd_lg_softmax.hpp), on tests/logistic_bound.py's dz, vexp_of, shift, U and V.

dc_i   softmax's Jacobian has rows of 1-norm 2 p_c (1 - p_c) <= 1/2, every logit is off by at most max_c dz_i(w_c), and the fp64 side
       makes at most C + 16 roundings of 2^-52 on values <= 1:  dc_i = max_c dz_i(w_c) / 2 + (C + 16) 2^-52  (p: + 2^-25, its float).
dw     logistic_bound.dw's expressions with that dc_i (E = 0: a step from set weights).
dloss  l has a gradient of 1-norm <= 2: per row 2 max_c dz_i + (C + 16) 2^-52 (1 + l_i); the tree adds (n + 64) v of the mean;
       sum_c |w_c|^2 comes from the same float weights on both sides: (dp + C + 8) v of it.

Behind the bounds: `decided` (the rows whose arg-max the reference decides), the evaluation's chains, and an honest emulation of one
softmax step and of the evaluation's rows in the kernels' own order, on logistic_bound's emulation of the dot, the shift and the
finish.  tests/test_softmax_bound.py holds the emulation inside the bounds and a set of seeded mistakes outside them.
"""

import numpy as np

import logistic_bound as lb
import logistic_ref as ref
from logistic_bound import U, V, dz, shift, vexp_of


def logits(csr, W):
    return np.stack([ref.dots(csr, w) for w in np.asarray(W, dtype=np.float64)], axis=1)   # [n, C]


def probs(Z, pad=0):
    """(p [n, C], row logsumexp).  pad: a MUTATION -- that many zero logits join S, as padding classes would."""
    m = Z.max(axis=1, keepdims=True)
    e = np.exp(Z - m)
    S = e.sum(axis=1, keepdims=True) + pad * np.exp(-m)
    return e / S, (np.log(S) + m)[:, 0]


def row_loss(Z, cls):
    return probs(Z)[1] - Z[np.arange(len(cls)), cls]


def _entries(csr):
    row_ptr, nnz = np.asarray(csr[0], dtype=np.int64), int(csr[0][-1])
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)), np.asarray(csr[1][:nnz], dtype=np.int64), np.asarray(csr[2][:nnz], dtype=np.float64)


def data_sums(csr, W, cls, idx, pad=0):
    """sum_{i in idx} (p_ic - [c == y_i]) x_i for every class, [C, dp] (duplicates count), without the regulariser."""
    rows, col, val = _entries(csr)
    W = np.asarray(W, dtype=np.float64)
    coef = probs(logits(csr, W), pad)[0]
    coef[np.arange(len(cls)), cls] -= 1.0
    coef = coef * np.bincount(np.asarray(idx, dtype=np.int64), minlength=len(cls))[:, None]
    C, dp = W.shape
    at = (np.arange(C)[:, None] * dp + col[None, :]).ravel()                       # one bincount over (class, column)
    return np.bincount(at, weights=(coef[rows].T * val[None, :]).ravel(), minlength=C * dp).reshape(C, dp)


def sync_step(csr, W, cls, lists, lr, lam, pad=0):
    W = np.asarray(W, dtype=np.float64)
    return W - lr * (sum(data_sums(csr, W, cls, idx, pad) + 2.0 * lam * W for idx in lists) / len(lists))


def loss_acc(csr, W, cls, row_begin, row_end, lam, Z=None):
    """(loss, acc, the rows' logits).  Z: logits(csr, W) of ALL rows, where the caller has them already."""
    W = np.asarray(W, dtype=np.float64)
    Z = (logits(csr, W) if Z is None else Z)[row_begin:row_end]
    y = np.asarray(cls[row_begin:row_end], dtype=np.int64)
    return lam * float(np.sum(W * W)) + float(np.mean(row_loss(Z, y))), float(np.mean(np.argmax(Z, axis=1) == y)), Z


def dz_max(csr, W):
    return np.max(np.stack([dz(csr, w) for w in W]), axis=0)


def dc(dz_i, C):
    return dz_i / 2.0 + (C + 16) * 2.0 ** -52


def dw(csr, W, cls, lists, lr, lam):
    """>= |w' - w'_ref| after one step from set weights, [C, dp].  (logistic_bound.dsum / dw at E = 0, written out for C classes at
    once because dsum takes neither dc_i nor the classes' G: a change to those two must be carried over here.)"""
    (rows, col, val), W64 = _entries(csr), np.asarray(W, dtype=np.float64)
    C, dp = W64.shape
    dci, ax, reg = dc(dz_max(csr, W), C) + V, np.abs(val), 2.0 * lam * W64
    tot, mean = np.zeros_like(W64), np.zeros_like(W64)
    for idx in lists:
        mult = np.bincount(np.asarray(idx, dtype=np.int64), minlength=len(cls)).astype(np.float64)
        t1 = np.bincount(col, weights=ax * (dci * mult)[rows], minlength=dp)
        cnt = np.bincount(col, weights=mult[rows], minlength=dp)
        unit = 2.0 ** (vexp_of(csr[2]) - shift(len(idx)) - 1)
        G = data_sums(csr, W64, cls, idx)
        tot += (t1 + cnt * unit)[None, :] + 4.0 * V * (np.abs(G) + np.abs(reg))
        mean += G + reg
    tot, mean, lr = tot / len(lists), mean / len(lists), float(lr)
    e = lr * tot + 2.0 * V * (np.abs(W64) + lr * np.abs(mean))
    return e + U * (np.abs(W64 - lr * mean) + e) + 2.0 ** -150


def dloss(csr, W, cls, row_begin, row_end, lam, Z=None, dzm=None):
    """Z, dzm: logits(csr, W) and dz_max(csr, W) of ALL rows, where the caller has them already"""
    W64 = np.asarray(W, dtype=np.float64)
    (C, dp), n = W64.shape, row_end - row_begin
    li = row_loss((logits(csr, W64) if Z is None else Z)[row_begin:row_end], np.asarray(cls[row_begin:row_end], dtype=np.int64))
    per = np.mean(2.0 * (dz_max(csr, W) if dzm is None else dzm)[row_begin:row_end] + (C + 16) * 2.0 ** -52 * (1.0 + li))
    return per + (n + 64) * V * float(np.mean(li)) + lam * (dp + C + 8) * V * float(np.sum(W64 * W64))


def decided(Z, dzm):
    """bool [n]: the reference decides the row's arg-max -- top1 - top2 > 2 dz_max_i, or dz_max_i == 0 (an empty row: every logit is
    exactly 0 on both sides and the answer is class 0).  The other rows are UNCERTAIN: their class may go either way."""
    top = np.sort(np.asarray(Z, dtype=np.float64), axis=1)
    return (np.asarray(dzm) == 0.0) | (top[:, -1] - top[:, -2] > 2.0 * np.asarray(dzm))


def chain_rows(n, n_cu):
    """(chain count, the evaluation's pass of every row of a range of n rows): lgsm_eval_blocks workgroups (one per 32 rows, at most
    one per compute unit) of 32 chains; chain g serves rows g, g + chains, g + 2 chains, ...: passes 0, 1, 2, ..."""
    chains = 32 * max(1, min(-(-n // 32), n_cu))
    return chains, np.arange(n) // chains


def loss_chain_skips(csr, W, cls, row_begin, row_end, lam, n_cu, Z=None):
    """loss_acc's loss under the MUTATION chain_skips: every chain drops its second row (the mean still divides by n)"""
    W = np.asarray(W, dtype=np.float64)
    li = row_loss((logits(csr, W) if Z is None else Z)[row_begin:row_end], np.asarray(cls[row_begin:row_end], dtype=np.int64))
    li = np.where(chain_rows(row_end - row_begin, n_cu)[1] == 1, 0.0, li)
    return lam * float(np.sum(W * W)) + float(np.sum(li)) / (row_end - row_begin)


# ---- the emulation: the kernels' own order (csrc/dsgd_lg_softmax.hpp), in numpy ---------------------------------------------------
# MUTATIONS (tests only; tests/test_softmax_bound.py says where each one applies and on which named case it must show):
#   pad_in_S              the TP - C padding classes' zero logits join S
#   drop_class_from_S     the last real class does not join S
#   label_from_neighbour  [c == y] is read from the lane's OTHER class: y0 and y1 swapped (a padding class's plane holds +1)
#   highest_argmax        a tie gives the highest class (evaluation)
#   loss_uses_pred        the loss takes z_pred where z_y belongs (evaluation)
#   vexp_qscale / vexp_finish   logistic_bound's: vexp one too large where the entries are scaled / in the finish ONLY
#   fold_head             the first rank beyond the LDS head (4096 / TP) is added to the head's last word
STEP_MUTATIONS = ("pad_in_S", "drop_class_from_S", "label_from_neighbour", "vexp_qscale", "vexp_finish", "fold_head")
EVAL_MUTATIONS = ("pad_in_S", "drop_class_from_S", "highest_argmax", "loss_uses_pred")


def tp_of(C):
    return (C + 3) & ~3


def group_width(C):
    return 16 if tp_of(C) <= 32 else (32 if tp_of(C) <= 64 else 64)


def hot_of(C):
    """the ranks of the gradient's LDS head (lgtw_hot)"""
    return 4096 // tp_of(C)


def emu_logits(csr, W32):
    """float32 [n, C]: lgtw_row_dots -- per class logistic_bound.emu_dot's order and bits (accumulator j takes the products of the
    positions = j mod 16 in order from 0, then group_sum<16>'s four pairings), all classes of a row at once."""
    row_ptr, col, val, _ = lb._csr(csr)
    W32 = np.ascontiguousarray(W32, dtype=np.float32)
    C, n = len(W32), len(row_ptr) - 1
    Z = np.zeros((n, C), dtype=np.float32)
    for r in np.nonzero(np.diff(row_ptr))[0]:
        st, en = int(row_ptr[r]), int(row_ptr[r + 1])
        k, m = en - st, -(-(en - st) // lb.G)
        prod = val[st:en][None, :] * W32[:, col[st:en]]            # float32 * float32, rounded once
        padded = np.zeros((C, m * lb.G), dtype=np.float32)
        padded[:, :k] = np.where(np.abs(prod) > np.float32(1e-20), prod, np.float32(0.0))
        padded = padded.reshape(C, m, lb.G)
        acc = np.zeros((C, lb.G), dtype=np.float32)
        for j in range(m):
            acc = acc + padded[:, j, :]
        for pm in lb._PERMS:
            acc = acc + acc[:, pm]
        Z[r] = acc[:, 0]
    return Z


def emu_rows(Z32, mut=None):
    """lgsm_row on the emulated logits: (p [n, C] float64, S [n], m [n] float32) -- the float max, fp64 exps, the lane's own two
    terms and then the xor butterfly of fp64 adds over the group's lanes"""
    Z32 = np.asarray(Z32, dtype=np.float32)
    (n, C), GW = Z32.shape, group_width(Z32.shape[1])
    m = Z32.max(axis=1)                                             # (the maximum of finite floats has no order)
    md = m.astype(np.float64)
    e = np.zeros((n, 2 * GW))                                       # exp(-inf) = 0.0 for a class the lane does not own
    e[:, :C] = np.exp(Z32.astype(np.float64) - md[:, None])
    p_top = e[:, :C].copy()
    if mut == "pad_in_S":
        with np.errstate(over="ignore"):
            e[:, C:tp_of(C)] = np.exp(0.0 - md)[:, None]
    if mut == "drop_class_from_S":
        e[:, C - 1] = 0.0
    S = e[:, 0::2] + e[:, 1::2]
    lanes, off = np.arange(GW), 1
    while off < GW:
        S = S + S[:, lanes ^ off]
        off <<= 1
    assert np.all((S == S[:, :1]) | np.isnan(S))                    # every lane ends with the same bits
    with np.errstate(divide="ignore", invalid="ignore"):            # (drop_class_from_S can leave S = 0: a mutation's own nonsense)
        return p_top / S[:, :1], S[:, 0], m


def _indicator(cls, C, mut=None):
    """[n, C]: [c == y]; label_from_neighbour: the plane byte of class c ^ 1 (+1 at the row's class AND at a padding class)"""
    n = len(cls)
    plane = np.zeros((n, tp_of(C) + 1))
    plane[np.arange(n), np.asarray(cls, dtype=np.int64)] = 1.0
    plane[:, C:] = 1.0
    return plane[:, np.arange(C) ^ 1] if mut == "label_from_neighbour" else plane[:, :C]


def emu_acc(csr, p, cls, idx, mut=None):
    """One worker's int64 sums [dp, C] and its shift: (p - [c == y]) qscale per class, __double2ll_rn per entry"""
    row_ptr, col, val, _ = lb._csr(csr)
    n, C = p.shape
    S = lb.shift(len(idx))
    coef = (p - _indicator(cls, C, mut)) * 2.0 ** (S - vexp_of(val) - (1 if mut == "vexp_qscale" else 0))
    mult = np.bincount(np.asarray(idx, dtype=np.int64), minlength=n)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    use = np.nonzero(mult[rows])[0]
    with np.errstate(invalid="ignore"):                             # (a mutation's NaN becomes some integer: far outside any bound)
        q = np.rint(val[use].astype(np.float64)[:, None] * coef[rows[use]]).astype(np.int64)
    return rows[use], col[use], q * mult[rows[use]][:, None], S


def emu_step(csr, W32, cls, lists, lr, lam, mut=None, Z32=None):
    """float32 [C, dp]: one softmax step from the float weights W32 (list form and ranges form: the same sums, the same finish)"""
    assert mut is None or mut in STEP_MUTATIONS, mut
    W32 = np.ascontiguousarray(W32, dtype=np.float32)
    C, dp = W32.shape
    p = emu_rows(emu_logits(csr, W32) if Z32 is None else Z32, mut)[0]
    fold = None
    if mut == "fold_head" and dp > hot_of(C):
        rank = lb.ranks_of(csr, dp)
        fold = (int(np.where(rank == hot_of(C))[0][0]), int(np.where(rank == hot_of(C) - 1)[0][0]))
    accs = []
    for idx in lists:
        _, at, q, S = emu_acc(csr, p, cls, idx, mut)
        if fold is not None:
            at = np.where(at == fold[0], fold[1], at)
        acc = np.zeros((dp, C), dtype=np.int64)
        if len(at):
            order = np.argsort(at, kind="stable")
            ats = at[order]
            starts = np.flatnonzero(np.concatenate([[True], ats[1:] != ats[:-1]]))
            acc[ats[starts]] = np.add.reduceat(q[order], starts, axis=0)
        accs.append((acc, S))
    return np.stack([lb.emu_finish(csr, W32[c], [(acc[:, c], S) for acc, S in accs], lr, lam, mut) for c in range(C)])


def emu_eval(Z32, cls, mut=None):
    """(per-row loss float64 [n], predicted class [n]) from the emulated logits: l = log(S) - (z_y - m), the LOWEST class of the
    largest logit"""
    assert mut is None or mut in EVAL_MUTATIONS, mut
    Z32 = np.asarray(Z32, dtype=np.float32)
    n, C = Z32.shape
    _, S, m = emu_rows(Z32, mut)
    pred = np.argmax(Z32 == m[:, None], axis=1)
    if mut == "highest_argmax":
        pred = C - 1 - np.argmax((Z32 == m[:, None])[:, ::-1], axis=1)
    zy = Z32[np.arange(n), pred if mut == "loss_uses_pred" else np.asarray(cls, dtype=np.int64)]
    return np.log(S) - (zy.astype(np.float64) - m.astype(np.float64)), pred


def emu_loss_acc(W32, cls, row_begin, row_end, lam, Z32, mut=None):
    """(loss, correct rows) over [row_begin, row_end) from the emulated logits of ALL rows"""
    W64 = np.asarray(W32, dtype=np.float32).astype(np.float64)
    li, pred = emu_eval(Z32[row_begin:row_end], cls[row_begin:row_end], mut)
    return lam * float(np.sum(W64 * W64)) + float(np.mean(li)), int(np.count_nonzero(pred == np.asarray(cls[row_begin:row_end], dtype=np.int64)))
