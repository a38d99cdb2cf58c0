"""Round-off bounds for K8, the dense logistic step (csrc/dsgd_dense.hpp), derived from the kernels' own operation
order -- test infrastructure, fp64 numpy, no GPU.  tests/test_dense_bound.py shows the bounds hold for an honest fp32
candidate and catch seeded faults; tests/test_gpu_dense_edges.py asserts them of the kernels.

u = 2^-24 (half an ulp of fp32, the relative error of one rounding).  All bounds are first order in u.

Logit, dz[i] = n_z * u * sum_j |x_ij w_j|, n_z = roundings on the longest path to z_i:
  VALU (dsgd_dense_step_kernel): a lane's 8 columns are one multiply and 7 fmaf (8 roundings); group_sum<64> is 6
    pairing levels (4 DPP adds, 2 __shfl_xor adds: 6); thread i then adds the D/512 wave partials one after the other,
    starting from 0.0f (D/512 - 1 roundings, counted as D/512 <= 16).   n_z = 8 + 6 + D/512.
  MFMA (dsgd_dense_step_mfma_kernel): a wave owns 256 columns and issues 16 macro-steps x 4 components = 64
    v_mfma_f32_16x16x4_f32 that accumulate into one register; each adds 4 products, and how the matrix core rounds
    inside one instruction is not documented, so each counts as 4 roundings: 256.  Thread i then adds the D/256 wave
    partials sequentially.   n_z = 256 + D/256.
Residual r = p - y, dr[i] = p(1-p) * (dz[i] + (|z|+2) u) + 4u:  p(1-p) is d sigmoid / dz.  __expf(-z) is
  v_exp_f32(z * log2e): the rounded product and the rounded constant move the argument by <= 1.5 |z| u in units of
  the exponent, which the p(1-p) in front turns into <= 0.34 u of p (max p(1-p)|z| = 0.224): it is carried as |z| u
  inside the bracket; the 1-ulp exponential (2u relative in e, the +2, again times p(1-p)); then three operations of
  <= 1 ulp each on values <= 1, where an ulp is <= u: the sum 1 + e seen from p, the reciprocal and the subtraction
  p - y: 3u, stated as the flat 4u.
Weight, dw[j] = (lr/B) * (sum_i dr[i] |x_ij| + n_g u sum_i |r_i x_ij|) + 2u |w_j'|:
  n_g = (blocks per workgroup) * (rows per block) + ceil(grid/16) + 16.  A lane's g accumulates one fmaf per row of
  every block of its workgroup (VALU: 8 per block; MFMA: one product, 4 levels of group_sum<16> and one add per
  16-row block, 6 <= 16); dsgd_dense_reduce_kernel adds ceil(grid/16) partials per phase sequentially and then the
  16 phases.  Both sequential sums start from 0.0f, which leaves two roundings spare: they pay for the rounding of
  scale = lr / (B * world) and of scale * t.  The subtraction w - scale * t is one rounding of w' (2u |w'| has one
  spare).
Loss of a range under given weights: |d softplus(z) - y z / dz| = |p - y| <= 1, and evaluating
  fmaxf(z, 0) + log1pf(__expf(-|z|)) - y z costs <= 4u max(1, |z|) (three roundings of values <= max(1, |z|) and a
  1-ulp log1pf of a value <= ln 2); the sums are in double.   dloss = mean_i (dz[i] + 4u max(1, |z_i|)).

The reference is oracle.dense_ref in fp64 fed the same fp32 data; its own error (~1e-16 relative) is ignored.

`emulate` is an HONEST fp32 candidate with the kernels' block / partial structure (not their bits), with optional
seeded faults.  `case_*` build the data of the GPU tests; the CPU test calls them with a small `n_cu` where the GPU
test's row count follows the device.
"""

from __future__ import annotations

import numpy as np

from oracle import dense_ref

U = 2.0 ** -24
FAULTS = ("last_row_dropped", "row_end_included", "second_block_skipped", "halves_swapped", "world_forgotten")
N_SENT = 64   # sentinel columns: the last 64


def rows_per_block(variant):
    return 16 if variant else 8


def launch_grid(variant, n_cu, n):
    """dn_launch: at most 2 n_cu workgroups of 8 rows (VALU) or n_cu of 16 rows (MFMA)."""
    rpb = rows_per_block(variant)
    return max(1, min(n_cu if variant else 2 * n_cu, -(-n // rpb)))


def n_z(variant, D):
    return 256 + D // 256 if variant else 8 + 6 + D // 512


def n_g(variant, n, grid):
    rpb = rows_per_block(variant)
    n_blocks = -(-n // rpb)
    return -(-n_blocks // grid) * rpb + -(-grid // 16) + 16


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


class Bound:
    """Everything the tests compare against, for one step over rows [rb, re) from weights w."""

    def __init__(self, X, y, w, lr, rb, re, variant, grid):
        D = X.shape[1]
        Xb = np.asarray(X[rb:re], dtype=np.float64)
        yb = np.asarray(y[rb:re], dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        B = re - rb
        aX = np.abs(Xb)
        self.z = Xb @ w
        self.dz = n_z(variant, D) * U * (aX @ np.abs(w))
        p = sigmoid(self.z)
        self.r = p - yb
        self.dr = p * (1.0 - p) * (self.dz + (np.abs(self.z) + 2.0) * U) + 4.0 * U
        self.w_ref, self.loss_ref, self.acc_ref = dense_ref.step(Xb, yb, w, lr)
        self.dw = lr / B * (aX.T @ self.dr + n_g(variant, B, grid) * U * (aX.T @ np.abs(self.r))) + 2.0 * U * np.abs(self.w_ref)
        self.dloss = float(np.mean(self.dz + 4.0 * U * np.maximum(1.0, np.abs(self.z))))
        self.certain = np.abs(self.z) > self.dz          # rows whose predicted class round-off cannot change
        self.correct = (self.z > 0) == (yb > 0.5)


# ---- an honest fp32 candidate, with seeded faults -------------------------------------------------------------------
def _tree(v):
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _forward32(Xb, w, variant):
    n, D = Xb.shape
    P = Xb * w
    if variant:   # per wave of 256 columns: 64 accumulating steps (macro-step m, component c) of 4 products (q)
        T = P.reshape(n, D // 256, 16, 4, 4)
        acc = np.zeros((n, D // 256), dtype=np.float32)
        for m in range(16):
            for c in range(4):
                acc = acc + ((T[:, :, m, 0, c] + T[:, :, m, 1, c]) + (T[:, :, m, 2, c] + T[:, :, m, 3, c]))
        parts = acc
    else:         # lane t: columns 4t .. 4t+3 and D/2 + 4t .. +3 in turn, 64 lanes pair up, waves in turn
        L = P.reshape(n, 2, D // 8, 4).transpose(0, 2, 1, 3).reshape(n, D // 8, 8)
        lane = L[:, :, 0]
        for k in range(1, 8):
            lane = lane + L[:, :, k]
        parts = _tree(lane.reshape(n, D // 512, 64))
    z = np.zeros(n, dtype=np.float32)
    for v in range(parts.shape[1]):
        z = z + parts[:, v]
    return z


def emulate(X, y, w, lr, rb, re, variant, grid, world=1, fault=None):
    """One step in fp32 numpy: blocks of 8 / 16 rows dealt round-robin to `grid` workgroups, per-workgroup partials,
    the 16-phase reduce, the update.  world = 2 models two ranks holding the same batch (the all-reduce doubles t).
    Returns (w', z of the rows the candidate used)."""
    assert fault is None or fault in FAULTS
    X = np.asarray(X, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    D = w.size
    rpb = rows_per_block(variant)
    B = re - rb
    end = re - 1 if fault == "last_row_dropped" else re + 1 if fault == "row_end_included" else re
    n_blocks = -(-(end - rb) // rpb)
    gpart = np.zeros((grid, D), dtype=np.float32)
    zs = np.zeros(end - rb, dtype=np.float32)
    one = np.float32(1.0)
    for wg in range(grid):
        g = np.zeros(D, dtype=np.float32)
        for k, blk in enumerate(range(wg, n_blocks, grid)):
            if fault == "second_block_skipped" and wg == 0 and k == 1:
                continue
            r0 = rb + blk * rpb
            r1 = min(end, r0 + rpb)
            Xb = X[r0:r1]
            z = _forward32(Xb, w, variant)
            zs[r0 - rb:r1 - rb] = z
            with np.errstate(over="ignore"):
                r = one / (one + np.exp(-z)) - y[r0:r1]
            if variant:
                pr = np.zeros((16, D), dtype=np.float32)
                pr[:r1 - r0] = r[:, None] * Xb
                g = g + _tree(pr.T)
            else:
                for i in range(r1 - r0):
                    g = g + r[i] * Xb[i]
        gpart[wg] = g
    if fault == "halves_swapped":
        gpart = np.concatenate([gpart[:, D // 2:], gpart[:, :D // 2]], axis=1)
    t = np.zeros(D, dtype=np.float32)
    for ph in range(16):
        s = np.zeros(D, dtype=np.float32)
        for b in range(ph, grid, 16):
            s = s + gpart[b]
        t = t + s
    if world == 2:
        t = t + t
    scale = np.float32(lr) / (np.float32(B) * np.float32(1 if fault == "world_forgotten" else world))
    return w - scale * t, zs


# ---- the data of the GPU tests --------------------------------------------------------------------------------------
def _make(n, D, seed, w_sigma, live=None):
    """x ~ N(0,1)/sqrt(live) in the first `live` columns, w ~ N(0, w_sigma^2) there; labels from a planted separator."""
    live = D if live is None else live
    rng = np.random.default_rng(seed)
    X = np.zeros((n, D), dtype=np.float32)
    X[:, :live] = rng.normal(size=(n, live)) / np.sqrt(live)
    w = np.zeros(D, dtype=np.float32)
    w[:live] = w_sigma * rng.normal(size=live)
    sep = rng.normal(size=live)
    y = (X[:, :live].astype(np.float64) @ sep + 0.1 * rng.normal(size=n) > 0).astype(np.float32)
    return X, y, w


def _misclassify(X, y, w, rows):
    """Edge rows get the label their logit speaks against: |r| >= 1/2, so a leaked or dropped edge row is visible."""
    for i in rows:
        if 0 <= i < len(y):
            y[i] = 1.0 if float(X[i].astype(np.float64) @ w.astype(np.float64)) < 0 else 0.0


def case_a(D, n_cu, seed=0):
    """Several blocks per workgroup with unequal counts: (X, y, w0, lr, the ranges of successive steps)."""
    if D == 512:
        n = 3 * 16 * n_cu + 8 * n_cu + 5     # 3 or 4 blocks per workgroup in either variant, ragged tail
        ranges = [(3, 3 + n), (0, n - 11), (7, min(107, n))]   # the last: fewer workgroups than gpart holds rows of
    else:
        n = 16 * n_cu + 24
        ranges = [(3, 3 + n), (1, n), (7, min(107, n))]
    X, y, w = _make(n + 8, D, seed + D, 1.0)
    _misclassify(X, y, w, [ranges[0][0] - 1, ranges[0][0], ranges[0][1] - 1, ranges[0][1]])
    return X, y, w, 4.0, ranges


B_D = 512
B_ROWS = 4160
B_RANGES = [(rb, rb + n) for rb in (0, 5) for n in (1, 7, 8, 9, 15, 16, 17, 4099)] + [(B_ROWS - 23, B_ROWS), (B_ROWS - 1, B_ROWS)]
_b_base = {}


def case_b(rb, re, variant, n_cu):
    """Sentinel columns.  Returns (X, y, w0, lr, inside, outside): inside / outside map a sentinel ROW to its COLUMN."""
    if "base" not in _b_base:
        _b_base["base"] = _make(B_ROWS, B_D, 77, 2.0, live=B_D - N_SENT)
    X, y, w = (a.copy() for a in _b_base["base"])
    n = re - rb
    rpb = rows_per_block(variant)
    grid = launch_grid(variant, n_cu, n)
    tail0 = rb + (n - 1) // rpb * rpb             # first row of the last (ragged or full) block
    want = [rb, re - 1, rb + 7, rb + 8, rb + 15, rb + 16, rb + grid * rpb - 1, rb + grid * rpb, tail0 - 1, tail0, tail0 + 1, re - 2]
    rows_in = sorted({i for i in want if rb <= i < re})
    rows_out = [i for i in [rb - 1] + list(range(re, re + 16)) if 0 <= i < B_ROWS]
    assert len(rows_in) + len(rows_out) <= N_SENT
    X[rows_out] *= 8.0                            # large features (the sentinel columns are still zero here)
    _misclassify(X, y, w, rows_out + [rb, re - 1])
    col = B_D - N_SENT
    inside, outside = {}, {}
    for i in rows_in:
        X[i, col] = 1.0
        inside[i] = col
        col += 1
    for i in rows_out:
        X[i, col] = 1.0
        outside[i] = col
        col += 1
    return X, y, w, float(n), inside, outside


D_WIDTHS = {0: list(range(512, 8192 + 1, 512)), 1: list(range(512, 4096 + 1, 512))}
D_RANGES = [(3, 40), (8, 45)]
D_LOSS = (5, 38)


def case_d(D):
    """37 rows at every width, logits of sigma ~ 10; rows with |z| < 1 are pushed away from 0 along w, so no
    predicted class hangs on round-off under the given weights or after two small steps."""
    X, y, w = _make(45, D, 1000 + D, 10.0)
    w64 = w.astype(np.float64)
    z = X.astype(np.float64) @ w64
    near = np.abs(z) < 1.0
    X[near] = (X[near] + np.where(z[near] < 0, -2.0, 2.0)[:, None] * w64 / (w64 @ w64)).astype(np.float32)
    _misclassify(X, y, w, [2, 3, 39, 40, 7, 8, 44])
    return X, y, w, 2.0
