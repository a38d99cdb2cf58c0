"""Error bounds of the logistic COLUMN-SLICE kernel (csrc/dsgd_lg_cs.hpp) against tests/logistic_ref.py, DERIVED from the
kernel's operation order, and an honest emulation of that order in numpy.  tests/logistic_bound.py and tests/logistic_ref.py
are imported untouched; only dz is replaced, and dc, dsum and dw follow from it by logistic_bound.py's own expressions.

u = 2^-24, v = 2^-53, gamma(k) = k u / (1 - k u), E_j >= |w_j - w_ref,j| carried from step to step: as there.

dz_i   on |d_i - d_ref,i|.  The G = 16 slices hold the columns of rank r = g (mod G).  Inside slice g, the n_ig entries of row i
       (in the row's order) are cut into slots of at most 16.  A lane owns a slot: its products, each rounded once, are added in
       sequence from 0 -- a term passes through at most 16 roundings (its product, at most 15 additions; the padding of a slot
       adds exact zeros).  One lane adds the row's m_ig = ceil(n_ig / 16) slots of the slice in order from 0: at most m_ig more.
       The G partials are added in slice order from 0: at most G more.  With m_i = max_g m_ig,
           dz_i = gamma(16 + m_i + G) * sum_j |x_ij| (|w_j| + E_j)  +  sum_j |x_ij| E_j  +  nnz_i * (1e-20 + 2^-149)
       (the engine's 1e-20 product filter and the subnormal products, as in logistic_bound.dz).
       No REORDERING of these additions can leave this bound -- it holds for any order of at most that depth -- which is why
       the order itself is pinned by bit equalities (the determinism tests), not by the bound.
dc, dsum, dw   logistic_bound.dc unchanged; dsum and dw are logistic_bound's expressions over this dz: the scatter is lg_add's
       expression (one fp64 product, one rounding to the 2^(vexp - S_k) grid), the finish is dsgd_lg_finish_kernel<LG_STEP>'s
       arithmetic column for column.
"""

import functools

import numpy as np

import logistic_bound as lb
import logistic_ref as ref

G = 16      # LG_CS_G
L = 16      # CS_L: entries per slot


def slice_of(csr, dp, g=G):
    """(rank of every key, slice of every entry)"""
    rank = lb.ranks_of(csr, dp)
    _, col, _, _ = lb._csr(csr)
    return rank, rank[col] % g


def dz(csr, w, E=None, g=G):
    row_ptr, col, val, _ = lb._csr(csr)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    w = np.abs(np.asarray(w, dtype=np.float64))
    E = np.zeros_like(w) if E is None else np.asarray(E, dtype=np.float64)
    ax = np.abs(val.astype(np.float64))
    A = np.bincount(rows, weights=ax * (w + E)[col], minlength=n)
    P = np.bincount(rows, weights=ax * E[col], minlength=n)
    nnz = np.diff(row_ptr).astype(np.float64)
    _, sl = slice_of(csr, len(w), g)
    per = np.bincount(rows * g + sl, minlength=n * g).reshape(n, g)
    m = np.ceil(per / float(L)).max(axis=1) if n else np.zeros(0)
    return lb.gamma(L + m + g) * A + P + nnz * (1e-20 + 2.0 ** -149)


def dsum(csr, w, idx, lam, E=None, g=G):
    """logistic_bound.dsum over this module's dz: (dsum_j, G_ref, reg_ref) of one worker's list."""
    row_ptr, col, val, _ = lb._csr(csr)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    w64 = np.asarray(w, dtype=np.float64)
    E = np.zeros_like(w64) if E is None else np.asarray(E, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    mult = np.bincount(idx, minlength=n).astype(np.float64)
    dci = lb.dc(dz(csr, w, E, g)) + lb.V
    ax = np.abs(val.astype(np.float64))
    t1 = np.bincount(col, weights=ax * (dci * mult)[rows], minlength=len(w64))
    cnt = np.bincount(col, weights=mult[rows], minlength=len(w64))
    unit = 2.0 ** (lb.vexp_of(val) - lb.shift(len(idx)) - 1)
    Gref, _ = ref.data_sum(csr, w64, idx)
    reg = 2.0 * lam * w64
    return t1 + cnt * unit + 2.0 * lam * E + 4.0 * lb.V * (np.abs(Gref) + np.abs(reg)), Gref, reg


def dw(csr, w, lists, lr, lam, E=None, g=G):
    """logistic_bound.dw over this module's dsum: E' >= |w' - w'_ref| after one step from weights that differ by at most E."""
    w64 = np.asarray(w, dtype=np.float64)
    E = np.zeros_like(w64) if E is None else np.asarray(E, dtype=np.float64)
    tot = np.zeros_like(w64)
    mean = np.zeros_like(w64)
    for idx in lists:
        ds, Gref, reg = dsum(csr, w, idx, lam, E, g)
        tot += ds
        mean += Gref + reg
    tot /= len(lists)
    mean /= len(lists)
    lr = float(lr)
    wn = w64 - lr * mean
    e = E + lr * tot + 2.0 * lb.V * (np.abs(w64) + lr * np.abs(mean))
    return e + lb.U * (np.abs(wn) + e) + 2.0 ** -150


# ---- the emulation: the kernel's own order, in numpy ---------------------------------------------------------------------
# The mistakes a kernel of this shape invites (tests/test_logistic_cs_bound.py):
#   slice_order_one_wg   workgroup 3 adds the G partials in descending slice order (its columns see another d)
#   shift_of_largest     the scatter scales with the shift of the step's LARGEST list (the cell header's rule), the finish with
#                        the worker's own
#   l2_listed_only       the finish visits the step's listed columns only (the SVM's sweep): no L2 term elsewhere
#   acc_not_cleared      worker 1's accumulators are not zeroed by the finish
#   padding_written_back the slices are written back with the stride of the widest slice's columns, not the padded stride: the
#                        padding of slice b lands on the first columns of slice b + 1
#   label_ignored        the label bit of row_first is not read: every row counts as y = +1
#   header_shift_finish  the finish scales with the SVM's 30-bit shift of the cell header
MUTATIONS = ("slice_order_one_wg", "shift_of_largest", "l2_listed_only", "acc_not_cleared", "padding_written_back", "label_ignored",
             "header_shift_finish")


def emu_dot(row_ptr, col, val, sl, w32, row, g=G, descending=False):
    """The slices' partials of one row and their sum in slice order (descending: the mistake)."""
    st, en = int(row_ptr[row]), int(row_ptr[row + 1])
    part = np.zeros(g, dtype=np.float32)
    zero = np.float32(0.0)
    for b in range(g):
        e = np.arange(st, en)[sl[st:en] == b]            # the slice's entries in the row's order
        t = zero
        for s0 in range(0, len(e), L):
            p = zero
            for q in e[s0:s0 + L]:
                pr = np.float32(val[q] * w32[col[q]])      # float32 * float32, rounded once
                p = np.float32(p + (pr if abs(pr) > np.float32(1e-20) else zero))
            t = np.float32(t + p)
        part[b] = t
    d = zero
    for b in (range(g - 1, -1, -1) if descending else range(g)):
        d = np.float32(d + part[b])
    return d


class Emu:
    """A context's state across steps: the weights and (for acc_not_cleared) what a finish left behind."""

    def __init__(self, csr, w32, g=G, mut=None):
        self.csr, self.g, self.mut = csr, g, mut
        self.w = np.asarray(w32, dtype=np.float32).copy()
        self.rank, self.sl = slice_of(csr, len(self.w), g)
        self.left = {}   # worker -> int64 sums the finish did not clear

    def step(self, lists, lr, lam):
        row_ptr, col, val, label = lb._csr(self.csr)
        g, mut, w32 = self.g, self.mut, self.w
        dp = len(w32)
        vexp = lb.vexp_of(val)
        listed = np.unique(np.concatenate([np.asarray(a, dtype=np.int64) for a in lists]))
        d = {int(r): emu_dot(row_ptr, col, val, self.sl, w32, int(r), g) for r in listed}
        d_bad = {int(r): emu_dot(row_ptr, col, val, self.sl, w32, int(r), g, True) for r in listed} if mut == "slice_order_one_wg" else d
        col_slice = self.rank % g                            # the slice of every KEY
        wj = w32.astype(np.float64)
        reg = (2.0 * lam) * wj
        total = np.zeros(dp)
        touched = np.zeros(dp, dtype=bool)
        largest = max(len(a) for a in lists)
        for k, idx in enumerate(lists):
            idx = np.asarray(idx, dtype=np.int64)
            S = lb.shift(len(idx))
            S_scatter = lb.shift(largest) if mut == "shift_of_largest" else S
            acc = self.left.pop(k, np.zeros(dp, dtype=np.int64)).copy()
            for r in idx:
                y = 1.0 if mut == "label_ignored" else float(label[r])
                st, en = int(row_ptr[r]), int(row_ptr[r + 1])
                for q in range(st, en):
                    dd = d_bad[int(r)] if col_slice[col[q]] == 3 else d[int(r)]
                    with np.errstate(over="ignore"):
                        c = -y / (1.0 + np.exp(y * float(dd)))
                    acc[col[q]] += int(np.rint(float(val[q]) * (c * 2.0 ** (S_scatter - vexp))))
                    touched[col[q]] = True
            S_fin = 30 - (largest - 1).bit_length() if mut == "header_shift_finish" else S
            Gk = acc.astype(np.float64) * 2.0 ** (vexp - S_fin)
            total = total + (Gk + reg)
            if mut == "acc_not_cleared" and k == 1:
                self.left[k] = acc
        mean = total / float(len(lists))
        wn = (wj - float(np.float32(lr)) * mean).astype(np.float32)
        if mut == "l2_listed_only":
            wn = np.where(touched, wn, w32)
        if mut == "padding_written_back":
            S_w = (dp + g - 1) // g                          # columns of the widest slice
            Sp = (S_w + 4) & ~3
            flat = np.zeros(g * S_w + Sp, dtype=np.float32)
            for b in range(g - 1, -1, -1):                   # (the last writer of an overlap: the slice below)
                piece = np.zeros(Sp, dtype=np.float32)
                keys = np.where(col_slice == b)[0]
                piece[self.rank[keys] // g] = wn[keys]
                flat[b * S_w:b * S_w + Sp] = piece
            wn = flat[(self.rank % g) * S_w + self.rank // g]
        self.w = wn
        return wn


# ---- designed inputs: rows whose place in the slices is known (CPU and GPU tests) --------------------------------------------

@functools.lru_cache(maxsize=None)
def designed(dp, n=48, k_lists=(4, 9, 30), n_steps=10, seed=2024):
    """(csr, steps, w0) over dp keys with rank == key.  Of the n listed rows, row 2 has 20 entries inside slice 5 (two slots; where
    dp < 16 * 20: every key of slice 5), row 3 lies in slice 9 whole, row 5 is empty; every step, worker 0 lists row 2 twice,
    workers 1 and 2 both list row 3, worker 2 lists the empty row.  Non-zero weights on every column."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        k = int(rng.integers(6, min(30, dp // 2)))
        rows.append(np.sort(rng.choice(dp, size=k, replace=False)))
    rows[5] = np.zeros(0, dtype=np.int64)                       # an empty row
    rows[2] = np.arange(5, min(dp, 5 + G * 20), G)              # keys that are 5 (mod 16): slots of slice 5 once rank == key
    rows[3] = np.arange(9, min(dp, 9 + G * 7), G)               # a row inside slice 9 alone
    # the ranking is by the count over all loaded rows, ties by ascending key: filler rows behind the n (never listed) raise
    # every key's count to the largest count at or above it, so the counts do not increase with the key and rank == key
    cnt = np.bincount(np.concatenate(rows), minlength=dp)
    deficit = np.maximum.accumulate(cnt[::-1])[::-1] - cnt
    for f in range(int(deficit.max())):
        rows.append(np.where(deficit > f)[0])
    col = np.concatenate(rows)
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    val = rng.uniform(-2.0, 2.0, size=len(col)).astype(np.float32)
    label = rng.choice(np.array([-1, 1], dtype=np.int8), size=len(rows))
    csr = (row_ptr, col.astype(np.int32), val, label)
    assert np.array_equal(slice_of(csr, dp)[0], np.arange(dp))
    steps = []
    for t in range(n_steps):
        lists = [rng.integers(0, n, size=m).astype(np.int32) for m in k_lists]
        lists[0][0], lists[0][1] = 2, 2                         # the long row, twice by one worker
        lists[1][0], lists[2][0] = 3, 3                         # the one-slice row, by two workers
        lists[2][1] = 5                                         # the empty row
        steps.append(lists)
    w0 = (rng.normal(size=dp) * 0.5).astype(np.float32)
    return csr, steps, w0
