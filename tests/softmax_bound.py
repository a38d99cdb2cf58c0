"""The fp64 reference of softmax regression (include/dsgd.h "SOFTMAX") in numpy over CSR arrays -- z_ic = x_i . w_c, p = softmax(z_i),
l_i = logsumexp(z_i) - z_iy, G_c = sum_i (p_ic - [c == y_i]) x_i + 2 lambda w_c, w_c <- w_c - lr mean_k G_kc -- and the kernels' error
bounds against it (csrc/dsgd_lg_softmax.hpp), on tests/logistic_bound.py's dz, vexp_of, shift, U and V.

dc_i   softmax's Jacobian has rows of 1-norm 2 p_c (1 - p_c) <= 1/2, every logit is off by at most max_c dz_i(w_c), and the fp64 side
       makes at most C + 16 roundings of 2^-52 on values <= 1:  dc_i = max_c dz_i(w_c) / 2 + (C + 16) 2^-52  (p: + 2^-25, its float).
dw     logistic_bound.dw's expressions with that dc_i (E = 0: a step from set weights).
dloss  l has a gradient of 1-norm <= 2: per row 2 max_c dz_i + (C + 16) 2^-52 (1 + l_i); the tree adds (n + 64) v of the mean;
       sum_c |w_c|^2 comes from the same float weights on both sides: (dp + C + 8) v of it.
"""

import numpy as np

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


def loss_acc(csr, W, cls, row_begin, row_end, lam):
    """(loss, acc, the rows' logits)"""
    W = np.asarray(W, dtype=np.float64)
    Z = logits(csr, W)[row_begin:row_end]
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


def dloss(csr, W, cls, row_begin, row_end, lam):
    W64 = np.asarray(W, dtype=np.float64)
    (C, dp), n = W64.shape, row_end - row_begin
    li = row_loss(logits(csr, W64)[row_begin:row_end], np.asarray(cls[row_begin:row_end], dtype=np.int64))
    per = np.mean(2.0 * dz_max(csr, W)[row_begin:row_end] + (C + 16) * 2.0 ** -52 * (1.0 + li))
    return per + (n + 64) * V * float(np.mean(li)) + lam * (dp + C + 8) * V * float(np.sum(W64 * W64))
