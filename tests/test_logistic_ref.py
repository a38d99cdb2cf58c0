"""tests/logistic_ref.py pinned (CPU): against a central finite difference of its own loss, and two hand-computed answers."""

import math

import numpy as np

import logistic_ref as ref


def _tiny(seed=0, n=12, dp=7):
    rng = np.random.default_rng(seed)
    row_ptr, col, val = [0], [], []
    for _ in range(n):
        k = int(rng.integers(1, 5))
        col += list(rng.choice(dp, size=k, replace=False))
        val += list(rng.uniform(-1, 1, size=k))
        row_ptr.append(len(col))
    label = rng.choice([-1, 1], size=n).astype(np.int8)
    return (np.array(row_ptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64), label), dp


def test_gradient_is_the_derivative_of_the_reported_loss():
    """One worker over ALL rows: gradient / n, the regulariser included once, is dL/dw of loss_acc's loss -- so the data part
    is divided by n and 2 lambda w is not."""
    csr, dp = _tiny()
    n = len(csr[3])
    lam = 0.05
    w = np.random.default_rng(1).normal(size=dp)
    data, _ = ref.data_sum(csr, w, np.arange(n))
    g = data / n + 2.0 * lam * w
    assert np.allclose(ref.gradient(csr, w, np.arange(n), lam), data + 2.0 * lam * w, rtol=0, atol=1e-15)
    h = 1e-6
    for j in range(dp):
        e = np.zeros(dp)
        e[j] = h
        fd = (ref.loss_acc(csr, w + e, 0, n, lam)[0] - ref.loss_acc(csr, w - e, 0, n, lam)[0]) / (2 * h)
        assert abs(fd - g[j]) < 1e-8, (j, fd, g[j])


def test_zero_weights():
    """w = 0: loss = ln 2, every c_i = -y_i / 2, every probability 0.5, class 0."""
    csr, dp = _tiny(2)
    n = len(csr[3])
    w = np.zeros(dp)
    loss, acc, tallies, d = ref.loss_acc(csr, w, 0, n, 0.3)
    assert abs(loss - math.log(2.0)) < 1e-15 and acc == 0.0 and tallies == [0, n, 0]
    _, c = ref.data_sum(csr, w, np.arange(n))
    assert np.array_equal(c, -csr[3].astype(np.float64) / 2.0)
    assert np.array_equal(ref.proba(d), np.full(n, 0.5)) and np.array_equal(ref.classes(d), np.zeros(n, dtype=np.int64))
    # a step from zero: w' = -lr * mean_k sum_i c_i x_i
    w1 = ref.sync_step(csr, w, [np.arange(n)], 0.5, 0.3)
    g, _ = ref.data_sum(csr, w, np.arange(n))
    assert np.array_equal(w1, -0.5 * g)


def test_two_rows_three_columns_by_hand():
    """x_0 = (1, 2, 0), y_0 = +1;  x_1 = (0, -1, 3), y_1 = -1;  w = (0.5, -0.25, 1);  lambda = 0.1.

        d_0 = 0.5 - 0.5 = 0         c_0 = -1 / (1 + e^0) = -1/2          l_0 = ln 2            p_0 = 1/2, class 0
        d_1 = 0.25 + 3 = 3.25       c_1 = +1 / (1 + e^-3.25) = s         l_1 = 3.25 + ln(1 + e^-3.25)   p_1 = s, class +1 (wrong)
        s = 0.962673112652...
        sum c x = (-1/2, -1 - s, 3 s)          g = sum + 2 lambda w = (-0.5 + 0.1, -1 - s - 0.05, 3 s + 0.2)
        loss = 0.1 * (0.25 + 0.0625 + 1) + (l_0 + l_1) / 2
        two workers, one row each, lr = 0.5:   w' = w - 0.5 * ((c_0 x_0 + c_1 x_1) / 2 + 2 lambda w)
    """
    csr = (np.array([0, 2, 4], dtype=np.int64), np.array([0, 1, 1, 2], dtype=np.int32), np.array([1.0, 2.0, -1.0, 3.0]),
           np.array([1, -1], dtype=np.int8))
    w = np.array([0.5, -0.25, 1.0])
    s = 1.0 / (1.0 + math.exp(-3.25))
    assert abs(s - 0.962673112652) < 1e-11
    assert np.array_equal(ref.dots(csr, w), [0.0, 3.25])
    g = ref.gradient(csr, w, [0, 1], 0.1)
    assert np.allclose(g, [-0.4, -1.05 - s, 3 * s + 0.2], rtol=0, atol=1e-15)
    loss, acc, tallies, d = ref.loss_acc(csr, w, 0, 2, 0.1)
    want = 0.1 * 1.3125 + (math.log(2.0) + 3.25 + math.log1p(math.exp(-3.25))) / 2
    assert abs(loss - want) < 1e-15 and acc == 0.0 and tallies == [0, 1, 1]
    assert np.allclose(ref.proba(d), [0.5, s], rtol=0, atol=1e-16) and list(ref.classes(d)) == [0, 1]
    w1 = ref.sync_step(csr, w, [[0], [1]], 0.5, 0.1)
    assert np.allclose(w1, w - 0.5 * (np.array([-0.5, -1 - s, 3 * s]) / 2 + 0.2 * w), rtol=0, atol=1e-15)
