"""Data, a float32 emulator and a derived per-row bound for the fp32 row-wise evaluation kernels at every lane-group width
-- test infrastructure, numpy and the C oracle, no GPU.  tests/test_lane_group_data.py shows that the bound holds for the
emulator and that seeded faults are caught; tests/test_gpu_lane_groups.py holds the kernels to the same comparison.

dsgd_load_csr gives a row to G = 8, 16, 32 or 64 lanes by the mean row length (csrc/dsgd_route.hpp: eval_group), and
dsgd_forward_kernel<G>, dsgd_eval_kernel<G>, dsgd_predict_kernel<G> and dsgd_eval_list_kernel<G> all take the row's dot from
row_dot<G, 4, LDSW> and group_sum<G> (csrc/dsgd_kernels.hpp).  Six matrices over D = 3,000 columns share ONE set of CORE
rows; FILLER rows of one fixed length per matrix follow them and move the mean, so the same CORE rows run at every width.

CORE (138 rows): six rows, three per label, of each length 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129,
255, 256, 257, 300, 515, 1,000 -- each G, each G x UNR and their neighbours, rows of many rounds of the tail loop.  Columns
are Zipfian (p ~ 1 / rank^1.1, without replacement, ascending within a row), so they fall on both sides of the 1,024-weight
LDS tile; values are normal, L2-normalised per row and rounded to float; weights are normal, rounded to float.  Exceptions:
  * TINY_ROWS hold nothing but 1e-25: every product falls under the 1e-20 filter, the dot is exactly 0 (without the filter
    it has a sign);
  * MIXED_ROWS have their first three entries replaced by 1e-25;
  * ZERO_W_ROW's only non-zero sits on ZERO_W_COL, whose weight is 0: its dot is exactly 0.

Matrices, as computed on the CPU by tests/test_lane_group_data.py (seed 20; `excluded`: rows the oracle alone leaves out
of the comparison, 0 < |x . w| <= bound -- the cap is 0.1 % of the rows; `zero`: rows whose oracle dot is exactly 0):

  name    lanes   rows     nnz    held   filler        mean   excluded  zero
  g8          8  2,538  29,568  29,574  2,400 x 4     11.65      0      10
  g16        16    738  43,968  43,974    600 x 40    59.59      0      10
  g32        32    438  58,968  58,974    300 x 130  134.64      0      10
  g64        64    438  97,968  97,974    300 x 260  223.68      0      10
  thr16      16    324  31,098  31,104    185 x 60    96          0      10     held = 96 rows exactly: the narrower group
  thr32      32    324  31,099  31,105    185 x 60    96 + 1/324  0      10     one entry more (the last row: 30 / 31 entries)

`held` is what the rule sees: dsgd_load_csr stores ONE explicit zero for a row without a non-zero (the streaming kernels rely
on every row owning a slot), dsgd_n_rows reports that count, and the mean is taken over it -- the six empty CORE rows count
six.  A matrix whose OWN nnz is 96 rows exactly would therefore get 32 lanes;
the two threshold matrices put the held count on the threshold.

The emulator (`emulate`) follows the kernel's order in float32: lane `sub` adds the filtered products of the positions sub,
sub + G, ... of the row one after the other from 0.0f (the unrolled part and the tail loop are one sequence), then group_sum's
stages in their order -- lane xor 1, lane xor 2, mirror within 8, (G >= 16) mirror within 16, (G >= 32) lane xor 16, (G >= 64)
lane xor 32 -- and lane 0's value is the row's.  It is no bit-for-bit claim about the device; it is an honest candidate
that the bound must admit, and the carrier of the seeded faults (MUTANTS) the comparison must catch.

The bound (`Matrix.bound`): with m = ceil(len / G) + log2 G additions on the longest path, one rounding of each product and
u = 2^-24, the computed dot differs from the exact one by at most  gamma_(m+1) * sum_j |x_j w_j|,  gamma_k = k u / (1 - k u)
(each product carries (1 + d) with |d| <= u, each addition another), plus len * 1e-20 for products that one side filters
and the other does not (such a product is within a rounding of 1e-20; the sum of |x_j w_j| runs over ALL products, which
pays for that rounding).  This is tighter than oracle/bounds.py's rel_gate_eps, (n_max + 2) u for the longest row of the
data whatever the order.  The fp64 oracle's own error, len * 2^-53 of the same sum, is not counted.  A row is compared where
the oracle's |x . w| exceeds the bound; rows whose oracle dot is exactly 0 are compared exactly (0 == 0).
"""

from __future__ import annotations

import numpy as np

from oracle import oracle as orc

U = 2.0 ** -24
UNR = 4
D = 3000
LAM = 1e-5
SEED = 20
EPS32 = np.float32(1e-20)      # DSGD_EPS as the kernels hold it
CORE_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 515, 1000)
PER_LENGTH = 6                 # three per label
N_CORE = PER_LENGTH * len(CORE_LENGTHS)
ZERO_W_COL = 1500              # (a feature id; beyond the 1,024-weight tile whatever its rank)
WIDTHS = (8, 16, 32, 64)
# name -> (intended lanes, filler rows, filler length, entries of one last row or None)
MATRICES = {"g8": (8, 2400, 4, None), "g16": (16, 600, 40, None), "g32": (32, 300, 130, None), "g64": (64, 300, 260, None),
            "thr16": (16, 185, 60, 30), "thr32": (32, 185, 60, 31)}
MUTANTS = ("tail_starts_late", "last_stage_missing", "stage_of_32_taken_at_16", "filter_dropped", "last_lane_skipped")
CAP = 0.001                    # excluded share per matrix (tests/test_gpu_predict.py)


def core_row(length, k=0):
    """the k-th CORE row of a length"""
    return CORE_LENGTHS.index(length) * PER_LENGTH + k


ZERO_W_ROW = core_row(1, 0)
TINY_ROWS = (core_row(7, 0), core_row(65, 3), core_row(300, 1))
MIXED_ROWS = (core_row(9, 0), core_row(33, 4), core_row(129, 2), core_row(257, 5), core_row(1000, 0))


def eval_group(nnz, n_rows):
    """csrc/dsgd_route.hpp: eval_group, restated (tests/cpp/route_test.cpp holds the header to the same expression)"""
    mean = float(nnz) / float(n_rows)
    return 64 if mean > 192.0 else 32 if mean > 96.0 else 16 if mean > 12.0 else 8


# ---- generation: vectorised ---------------------------------------------------------------------------------------------
def _zipf_rows(rng, lengths):
    """(row_ptr, col, val) of rows of the given lengths: per row, distinct Zipfian feature ids 1 .. D in ascending order (the
    Gumbel top-k form of sampling without replacement: the `length` largest of log p + Gumbel noise) and normal values of
    L2 norm 1."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    logp = -1.1 * np.log(np.arange(1, D + 1))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=row_ptr[1:])
    col = np.zeros(row_ptr[-1], dtype=np.int32)
    for length in np.unique(lengths):            # (per distinct LENGTH, not per row)
        rows = np.flatnonzero(lengths == length)
        if length == 0:
            continue
        key = logp[None, :] + rng.gumbel(size=(len(rows), D))
        top = np.argpartition(-key, length - 1, axis=1)[:, :length] if length < D else np.tile(np.arange(D), (len(rows), 1))
        ids = np.sort(top, axis=1).astype(np.int32) + 1
        at = row_ptr[rows][:, None] + np.arange(length)[None, :]
        col[at] = ids
    val = rng.normal(size=len(col))
    row_id = np.repeat(np.arange(n), lengths)
    norm = np.sqrt(np.bincount(row_id, weights=val * val, minlength=n))
    val /= norm[row_id]
    return row_ptr, col, val


_cache = {}


def core(seed=SEED):
    """(row_ptr, col, val, label, w): the shared CORE rows, their labels and the weights; values and weights are float32."""
    if ("core", seed) not in _cache:
        rng = np.random.default_rng(seed)
        lengths = np.repeat(np.asarray(CORE_LENGTHS, dtype=np.int64), PER_LENGTH)
        row_ptr, col, val = _zipf_rows(rng, lengths)
        label = np.tile(np.asarray([1, -1], dtype=np.int8), N_CORE // 2)        # three of each per length
        w = rng.normal(size=D + 1).astype(np.float32)
        w[ZERO_W_COL] = 0.0
        col[row_ptr[ZERO_W_ROW]] = ZERO_W_COL
        for r in TINY_ROWS:
            val[row_ptr[r]:row_ptr[r + 1]] = 1e-25
        for r in MIXED_ROWS:
            val[row_ptr[r]:row_ptr[r] + 3] = 1e-25
        _cache[("core", seed)] = (row_ptr, col, val.astype(np.float32), label, w)
    return _cache[("core", seed)]


class Matrix:
    """One matrix: CSR (float32 values), labels, weights, and the oracle side -- computed once, never changed."""

    def __init__(self, name, row_ptr, col, val, label, w, want_group):
        self.name, self.row_ptr, self.col, self.val, self.label, self.w, self.want_group = name, row_ptr, col, val, label, w, want_group
        self.n = len(row_ptr) - 1
        self.nnz = int(row_ptr[-1])
        self.lengths = np.diff(row_ptr)
        self.held_nnz = self.nnz + int((self.lengths == 0).sum())     # as the context holds it: an empty row owns one explicit zero
        self.row_id = np.repeat(np.arange(self.n), self.lengths)
        self.oracle = orc.Oracle(D, row_ptr, col, val.astype(np.float64), label, LAM)
        w64 = w.astype(np.float64)
        self.dot = np.asarray([self.oracle.row_dot(i, w64) for i in range(self.n)])
        self.pred = np.asarray(self.oracle.forward(w64, np.arange(self.n)), dtype=np.int64)
        self.abs_sum = np.bincount(self.row_id, weights=np.abs(val.astype(np.float64) * w64[col]), minlength=self.n)

    def bound(self, G):
        m = -(-self.lengths // G) + int(np.log2(G))
        k = (m + 1) * U
        return k * self.abs_sum / (1.0 - k) + self.lengths * 1e-20

    def zero(self):
        return self.dot == 0.0

    def compared(self, G):
        """rows whose prediction is held to the oracle's at G lanes: |x . w| beyond the bound, or exactly 0"""
        return (np.abs(self.dot) > self.bound(G)) | self.zero()

    def excluded(self, G):
        return ~self.compared(G)

    def tight_ranges(self, G):
        """maximal row ranges without an excluded row: their tallies are the oracle's, exactly"""
        cut = np.concatenate([[-1], np.flatnonzero(self.excluded(G)), [self.n]])
        return [(int(a) + 1, int(b)) for a, b in zip(cut[:-1], cut[1:]) if b - a > 1]

    def oracle_counts(self, lo, hi):
        return [int(c) for c in self.oracle.loss_acc(self.w.astype(np.float64), lo, hi)[2]]

    def line(self, G=None):
        """one line per matrix, in the style of the waivers table"""
        G = self.want_group if G is None else G
        return "%-6s lanes %2d  rows %6d  nnz %8d  held mean %8.3f  excluded %d  zero %d  smallest compared |x.w| / bound %.3g" % (
            self.name, G, self.n, self.nnz, self.held_nnz / self.n, int(self.excluded(G).sum()), int(self.zero().sum()),
            float((np.abs(self.dot) / np.maximum(self.bound(G), 1e-300))[self.compared(G) & ~self.zero()].min()))


def matrix(name, seed=SEED):
    if (name, seed) not in _cache:
        want, n_fill, fill_len, last = MATRICES[name]
        c_ptr, c_col, c_val, c_label, w = core(seed)
        # (thr16 / thr32 share their filler: the two differ in the last row's length alone)
        rng = np.random.default_rng([seed, n_fill, fill_len])
        f_ptr, f_col, f_val = _zipf_rows(rng, np.full(n_fill, fill_len, dtype=np.int64))
        f_label = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=n_fill)
        parts = [(c_ptr, c_col, c_val, c_label), (f_ptr, f_col, f_val.astype(np.float32), f_label)]
        if last is not None:
            l_ptr, l_col, l_val = _zipf_rows(rng, [last])
            parts.append((l_ptr, l_col, l_val.astype(np.float32), np.asarray([1], dtype=np.int8)))
        row_ptr = np.concatenate([[0]] + [p[0][1:] + off for p, off in zip(parts, np.cumsum([0] + [int(p[0][-1]) for p in parts[:-1]]))]).astype(np.int64)
        col = np.concatenate([p[1] for p in parts]).astype(np.int32)
        val = np.concatenate([p[2] for p in parts]).astype(np.float32)
        label = np.concatenate([p[3] for p in parts]).astype(np.int8)
        _cache[(name, seed)] = Matrix(name, row_ptr, col, val, label, w, want)
    return _cache[(name, seed)]


# ---- larger matrices: more rows than lane groups on 256 CUs (the persistent loop) ----------------------------------------
# name -> (intended lanes, rows, shortest row, longest row): lengths uniform in between
BIG = {"big8": (8, 40000, 0, 12), "big32": (32, 10000, 100, 140), "big64": (64, 6000, 200, 240)}


def big(name, seed=SEED):
    """(row_ptr, col, val float32, label, w float32): ascending distinct feature ids as running sums of uniform gaps (no
    Zipf: a 40,000 x 3,000 table of keys would take longer than the test), normal values of L2 norm 1."""
    _, n, lo, hi = BIG[name]
    rng = np.random.default_rng([seed, n])
    lengths = rng.integers(lo, hi + 1, size=n).astype(np.int64)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=row_ptr[1:])
    row_id = np.repeat(np.arange(n), lengths)
    gap_max = np.repeat(D // np.maximum(lengths, 1), lengths)           # length x gap_max <= D: the last id stays within 1 .. D
    gaps = 1 + (rng.random(len(row_id)) * gap_max).astype(np.int64)
    run = np.cumsum(gaps)
    before = np.concatenate([[0], run])[row_ptr[:-1]]                   # the running sum in front of each row
    col = (run - before[row_id]).astype(np.int32)
    val = rng.normal(size=len(col))
    val /= np.sqrt(np.bincount(row_id, weights=val * val, minlength=n))[row_id]
    label = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=n)
    return row_ptr, col, val.astype(np.float32), label, rng.normal(size=D + 1).astype(np.float32)


def big_matrix(name, seed=SEED):
    """big(name) with its oracle side (the C oracle: a second or less)"""
    if (name, seed) not in _cache:
        row_ptr, col, val, label, w = big(name, seed)
        _cache[(name, seed)] = Matrix(name, row_ptr, col, val, label, w, BIG[name][0])
    return _cache[(name, seed)]


def big_ranges(n):
    """Six ranges given out of row order, one of them empty, that cover every row once: lengths n/3, 5, 0, n/2 - 5, 3 and
    the rest, so the range-major order of the reply is not the row order.  With n_groups lane groups, the ordinals t and
    t + n_groups of a group fall in different ranges for every t below n - n_groups (the GPU test asserts it for its
    device's count)."""
    a, b = n // 2, n * 5 // 6
    return [(a, b), (0, 5), (7, 7), (5, a), (b, b + 3), (b + 3, n)]


def range_of_ordinal(ranges, t):
    off = 0
    for k, (b, e) in enumerate(ranges):
        if off <= t < off + (e - b):
            return k
        off += e - b
    raise IndexError(t)


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _partner(G, stage):
    lane = np.arange(G)
    if stage == 0:
        return lane ^ 1            # quad_perm [1,0,3,2]
    if stage == 1:
        return lane ^ 2            # quad_perm [2,3,0,1]
    if stage == 2:
        return (lane & ~7) | (7 - (lane & 7))      # row_half_mirror
    if stage == 3:
        return (lane & ~15) | (15 - (lane & 15))   # row_mirror
    return lane ^ (16 << (stage - 4))              # __shfl_xor 16, 32


def emulate(m, G, mutant=None, rows=None):
    """float32 dots of the listed rows (default: all, in order) as row_dot<G, 4> + group_sum<G> add them, optionally with one
    seeded fault.  `stage_of_32_taken_at_16` reaches into the neighbouring group of the wave: list position t takes the sum
    of position t ^ 1 on top (the launch gives position t to group t), which is why the rows are a list."""
    assert mutant is None or mutant in MUTANTS
    rows = np.arange(m.n) if rows is None else np.asarray(rows, dtype=np.int64)
    lengths = m.lengths[rows]
    K = max(1, -(-int(lengths.max()) // G)) + 1
    prod = np.zeros((len(rows), K * G), dtype=np.float32)
    pos = np.arange(int(lengths.sum())) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    src = np.repeat(m.row_ptr[rows], lengths) + pos
    p = m.val[src] * m.w[m.col[src]]                                   # float32 x float32, rounded once
    if mutant != "filter_dropped":
        p = np.where(np.abs(p) > EPS32, p, np.float32(0.0))
    prod[np.repeat(np.arange(len(rows)), lengths), pos] = p
    prod = prod.reshape(len(rows), K, G)
    acc = np.zeros((len(rows), G), dtype=np.float32)
    for k in range(K):                                                 # position sub + k G, in order (adding 0.0f changes nothing)
        if mutant == "tail_starts_late" and k == UNR:
            continue                                                   # the tail loop begins at (UNR + 1) G
        acc = acc + prod[:, k, :]
    if mutant == "last_lane_skipped":
        acc[:, G - 1] = 0.0
    n_stages = 3 + (G >= 16) + (G >= 32) + (G >= 64)
    if mutant == "last_stage_missing":
        n_stages -= 1
    for s in range(n_stages):
        acc = acc + acc[:, _partner(G, s)]
    d = acc[:, 0].copy()
    if mutant == "stage_of_32_taken_at_16" and G == 16:
        t = np.arange(len(rows))
        has = (t ^ 1) < len(rows)
        d[has] = d[has] + acc[(t ^ 1)[has], 0]
    return d


def predictions(d):
    """p = -signum(x . w)"""
    d = np.asarray(d)
    return np.where(d > 0, -1, np.where(d < 0, 1, 0)).astype(np.int64)


def host_counts(pred, label):
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    return [int(np.count_nonzero((pred != 0) & (pred == label))), int(np.count_nonzero(pred == 0)),
            int(np.count_nonzero((pred != 0) & (pred != label)))]


def agrees_with_oracle(m, G, pred):
    """The comparison of the GPU test, on predictions of all rows in order: every compared row's prediction is the oracle's
    (rows of dot 0 included: 0 == 0), and the tallies of every range without an excluded row are the oracle's."""
    pred = np.asarray(pred, dtype=np.int64)
    keep = m.compared(G)
    if not np.array_equal(pred[keep], m.pred[keep]):
        return False
    return all(host_counts(pred[lo:hi], m.label[lo:hi]) == m.oracle_counts(lo, hi) for lo, hi in m.tight_ranges(G))
