"""The fp64 reference of the logistic model (include/dsgd.h "THE LOGISTIC MODEL"), in numpy over CSR arrays.

A literal restatement of the model, nothing of the kernels' order:

    d_i   = x_i . w                                      P(y = +1 | x) = sigma(d), class = signum(d)  (the textbook sign)
    l_i   = max(-a, 0) + log1p(exp(-|a|)),  a = y_i d_i   reported loss = lambda |w|^2 + mean_i l_i
    c_i   = -y_i / (1 + exp(y_i d_i))                     (= sigma(d_i) - (1 + y_i) / 2)
    g     = sum_{i in list} c_i x_i + 2 lambda w          one worker's regularised SUM, on every column
    step  w <- w - lr * mean_k g_k

`csr` is (row_ptr, col, val, label) with keys in [0, D]; vectors have D + 1 entries.  tests/test_logistic_ref.py pins this file
against a finite difference of its own loss and two hand-computed answers.
"""

import numpy as np


def _rows(csr):
    row_ptr = np.asarray(csr[0], dtype=np.int64)
    return row_ptr, np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def dots(csr, w):
    """x_i . w of every row, float64."""
    row_ptr, rows = _rows(csr)
    nnz = int(row_ptr[-1])
    col = np.asarray(csr[1][:nnz], dtype=np.int64)
    val = np.asarray(csr[2][:nnz], dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    return np.bincount(rows, weights=val * w[col], minlength=len(row_ptr) - 1)


def coef(d, y):
    with np.errstate(over="ignore"):
        return -y / (1.0 + np.exp(y * d))


def row_loss(d, y):
    a = y * d
    return np.maximum(-a, 0.0) + np.log1p(np.exp(-np.abs(a)))


def proba(d):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(d, dtype=np.float64)))


def classes(d):
    return np.sign(d).astype(np.int64)


def data_sum(csr, w, idx, d=None):
    """sum_{i in idx} c_i x_i (duplicates count), without the regulariser; also the c of every listed position."""
    row_ptr, rows = _rows(csr)
    nnz = int(row_ptr[-1])
    col = np.asarray(csr[1][:nnz], dtype=np.int64)
    val = np.asarray(csr[2][:nnz], dtype=np.float64)
    y = np.asarray(csr[3], dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    if d is None:
        d = dots(csr, w)
    c_row = coef(d, y)
    mult = np.bincount(idx, minlength=len(y)).astype(np.float64)   # how often a row is listed
    g = np.bincount(col, weights=(c_row * mult)[rows] * val, minlength=len(w))
    return g, c_row[idx]


def gradient(csr, w, idx, lam):
    """One worker's regularised sum, float64 [D + 1]."""
    g, _ = data_sum(csr, w, idx)
    return g + 2.0 * lam * np.asarray(w, dtype=np.float64)


def sync_step(csr, w, lists, lr, lam):
    """The weights after one step over the workers' lists, float64."""
    w = np.asarray(w, dtype=np.float64)
    d = dots(csr, w)
    total = np.zeros_like(w)
    for idx in lists:
        g, _ = data_sum(csr, w, idx, d)
        total = total + (g + 2.0 * lam * w)
    return w - lr * (total / len(lists))


def loss_acc(csr, w, row_begin, row_end, lam):
    """(loss, acc, tallies [signum(d) == y, == 0, == -y], d of the rows)."""
    w = np.asarray(w, dtype=np.float64)
    d = dots(csr, w)[row_begin:row_end]
    y = np.asarray(csr[3], dtype=np.float64)[row_begin:row_end]
    s = np.sign(d)
    t = [int(np.sum(s == y)), int(np.sum(s == 0)), int(np.sum(s == -y))]
    loss = lam * float(np.dot(w, w)) + float(np.mean(row_loss(d, y)))
    return loss, t[0] / float(row_end - row_begin), t, d
