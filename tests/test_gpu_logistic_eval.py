"""The logistic model's distributed and sampled evaluation on the GPU (include/dsgd.h "THE LOGISTIC MODEL", DISTRIBUTED AND
SAMPLED EVALUATION: dsgd_lg_predict_ranges, dsgd_lg_loss_acc_list, dsgd_lg_loss_acc_sampled; csrc/dsgd_lg_eval.hpp), through the
C ABI via Engine.

The main guard is BIT EQUALITY with the calls the model already had: a range's loss and tallies against lg_loss_acc and
lg_loss_acc_ranges on that range, the probabilities against lg_predict_proba, the list form on arange(b, e) against
lg_loss_acc(b, e), the sampled form against the list form on the rows it drew, the rows against host.sampled_list on a
JavaRandom of the same seed.  Then everything against the fp64 reference tests/logistic_ref.py within the DERIVED bounds of
tests/logistic_bound.py:

  loss     lb.dloss of the range; for a list, lb.dloss of the CSR built of the listed rows, duplicates repeated.  The total over K
           ranges: the ranges' bounds weighted by their rows (the |w|^2 term enters once: the weights add up to one) plus the K
           additions of the ranges' sums, (K + 1) 2^-53 of the mean.
  proba    sigma has Lipschitz constant 1/4 and the fp32 d is within dz_i of the reference's, so before the rounding to float
           |p - p_ref| <= dz_i / 4 + 2^-49 (lb.dc: the 2^-49 covers the fp64 roundings of either side's expression on a value
           <= 1); the ONE rounding to float of a p <= 1 adds at most half an ulp of [0.5, 1], 2^-25:
               |p - p_ref| <= lb.dc(dz_i) + 2^-25.
  classes  exact on every row whose reference |d| exceeds its dz_i (the fp32 d then has the reference's sign), and on the rows
           whose every product is exactly zero -- empty rows, entries under zero weights only: class 0 on both sides; the
           other rows inside the margin are left out and must be at most 1 % of the rows.  Tallies: within the number of such rows of the reference's.

Uncertain rows counted on the CPU with logistic_ref alone before any GPU run, weights of logit standard deviation 1: 0 of the
28,400 rows of synth.generate(28400, seed=12); 0 of 4,096 of tests/logistic_cases.py; widths dim 1, 2,046, 2,047, 2,048: 0 of 600
each (dim 1: 203 rows have d == 0 exactly, class 0); hostile traits: 0, 0, 0, 0, 6 (zero_margin: three
of them sum to an exact 0 in fp64 from non-zero products) and 2 (ragged64) of 2,048; at most 1 of a list of 100.

Shapes: ranges of 1, 63, 64, 65 rows (64 rows per workgroup), 4,095 and 4,096 (the tile rule), 20,000 (more than n_cu * 64: the
stride wraps), an empty range between two others, all in ONE launch; 256 ranges of uneven lengths, empty ones among them.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import dsgd_amd
import hard_data as hd
import logistic_bound as lb
import logistic_cases as cases
import logistic_hard_cases as hc
import logistic_ref as ref
from dsgd_amd import _lib, host

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ESTATE, EUNSUPPORTED = _lib.EINVAL, _lib.ERANGE, _lib.ESTATE, _lib.EUNSUPPORTED
BIG_N, BIG_SEED = 28400, 12
MIX_LENGTHS = [1, 63, 64, 65, 0, 4095, 4096, 20000]   # (the empty range lies between two others)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ranges_of(lengths, at=0, gap=0):
    out = []
    for n in lengths:
        out.append((at, at + n))
        at += n + gap
    return out


MIX = ranges_of(MIX_LENGTHS, at=3, gap=1)
# 256 ranges: 1 .. 101 rows, every 25th one empty, in an order that is not the rows' (the halves trade places)
_R256 = ranges_of([0 if r % 25 == 24 else 1 + (r * 37) % 101 for r in range(256)], at=100, gap=2)
R256 = _R256[128:] + _R256[:128]
assert MIX[-1][1] <= BIG_N and max(e for _, e in R256) <= BIG_N and len(R256) == 256


class Ref:
    """The fp64 reference of one data set under one weight vector, computed once."""

    def __init__(self, csr, w, lam):
        self.csr, self.w, self.lam = csr, w, lam
        self.d = ref.dots(csr, w)
        self.dz = lb.dz(csr, w)
        self.y = np.asarray(csr[3], dtype=np.float64)
        self.certain = np.abs(self.d) > self.dz
        # a row whose every product x w is exactly zero (an empty row; entries on columns of zero weight only): the sum is +0 on
        # both sides, whatever the order
        self.certain |= ref.dots((csr[0], csr[1], np.abs(csr[2]), csr[3]), np.abs(np.asarray(w, dtype=np.float64))) == 0
        self.cls = np.sign(self.d).astype(np.int8)
        self.p = ref.proba(self.d)
        self.li = ref.row_loss(self.d, self.y)
        self.nsq = float(np.dot(np.asarray(w, np.float64), np.asarray(w, np.float64)))

    def rows_of(self, ranges):
        return np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in ranges]) if ranges else np.zeros(0, np.int64)

    def dloss(self, rows):
        """lb.dloss of the CSR built of `rows` (duplicates repeated), from the per-row terms computed once: its expression, term for
        term (test_the_cached_bound_is_lb_dloss holds the two together)"""
        li, n = self.li[rows], len(rows)
        per = float(np.mean(self.dz[rows] + 8.0 * lb.V * (1.0 + li)))
        return per + (n + 64) * lb.V * float(np.mean(li)) + self.lam * (len(self.w) + 8) * lb.V * self.nsq

    def tallies(self, rows):
        s, y = self.cls[rows].astype(np.float64), self.y[rows]
        return np.array([np.sum(s == y), np.sum(s == 0), np.sum(s == -y)], dtype=np.int64)

    def check_rows(self, rows, classes, proba, what):
        """classes and probabilities of `rows` (an array, duplicates allowed) against the reference"""
        sure = self.certain[rows]
        unsure = int(np.count_nonzero(~sure))
        assert unsure <= 0.01 * len(rows), (what, unsure, len(rows))
        assert np.array_equal(np.asarray(classes)[sure], self.cls[rows][sure]), what
        if proba is not None:
            err = np.abs(np.asarray(proba, dtype=np.float64) - self.p[rows])
            bound = lb.dc(self.dz[rows]) + 2.0 ** -25
            print("%s: proba max err/bound %.3f, %d uncertain rows" % (what, float(np.max(err / bound)), unsure))
            assert np.all(err <= bound), (what, float(np.max(err / bound)))
        return unsure

    def check_range(self, a, b, counts, loss, what):
        rows = np.arange(a, b)
        unsure = int(np.count_nonzero(~self.certain[rows]))
        assert int(np.sum(counts)) == b - a and np.all(np.abs(np.asarray(counts) - self.tallies(rows)) <= unsure), (what, counts)
        want = self.lam * self.nsq + float(np.mean(self.li[a:b]))
        bound = self.dloss(rows)
        print("%s: loss err/bound %.3f" % (what, abs(loss - want) / bound))
        assert abs(loss - want) <= bound, (what, loss, want, bound)


def sub_csr(csr, idx):
    """the CSR of the listed rows, duplicates repeated"""
    row_ptr, col, val, label = csr
    idx = np.asarray(idx, dtype=np.int64)
    lens = np.diff(row_ptr)[idx]
    take = np.concatenate([np.arange(row_ptr[i], row_ptr[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(col)[take], np.asarray(val)[take], np.asarray(label)[idx])


def check_list(R, idx, loss, acc, counts, what):
    idx = np.asarray(idx, dtype=np.int64)
    unsure = int(np.count_nonzero(~R.certain[idx]))
    assert unsure <= 0.01 * len(idx) or len(idx) < 100, (what, unsure)
    assert sum(counts) == len(idx) and np.all(np.abs(np.asarray(counts) - R.tallies(idx)) <= unsure), (what, counts, R.tallies(idx))
    assert acc == counts[0] / float(len(idx))
    want = R.lam * R.nsq + float(np.mean(R.li[idx]))
    bound = R.dloss(idx)
    print("%s: loss err/bound %.3f" % (what, abs(loss - want) / bound))
    assert abs(loss - want) <= bound, (what, loss, want, bound)


def engine_of(csr, dim, lam, w=None):
    eng = dsgd_amd.Engine(dim, lam)
    eng.load_csr(*csr)
    if w is not None:
        eng.set_weights(w)
    return eng


@functools.lru_cache(maxsize=None)
def big_data():
    d = dsgd_amd.synth.generate(BIG_N, seed=BIG_SEED)
    csr = (d.row_ptr, d.col, d.val, d.label)
    w = np.random.default_rng(3).standard_normal(d.dim + 1)
    w = (w * (1.0 / np.std(ref.dots(csr, w)))).astype(np.float32)   # (logits of standard deviation 1)
    w.setflags(write=False)
    return d, csr, w, Ref(csr, w, cases.LAM)


@pytest.fixture(scope="module")
def big():
    d, csr, w, R = big_data()
    with engine_of(csr, d.dim, cases.LAM, w) as eng:
        yield eng, R


@pytest.fixture(scope="module")
def synth():
    d = cases.data()
    w = cases.weights(1.0)
    with engine_of(cases.csr(d), d.dim, cases.LAM, w) as eng:
        yield eng, Ref(cases.csr(d), w, cases.LAM)


def check_predict_ranges(eng, R, ranges, what, twins=True):
    """One lg_predict_ranges call over `ranges` held to every contract; returns its outputs."""
    cls, proba, counts, range_loss, loss, acc = eng.lg_predict_ranges(ranges, want_proba=True)
    rows = R.rows_of(ranges)
    assert cls.dtype == np.int8 and proba.dtype == np.float32 and len(cls) == len(proba) == len(rows) and counts.shape == (len(ranges), 3)
    # the class is the sign of the d behind the probability
    assert set(np.unique(cls).tolist()) <= {-1, 0, 1}
    assert np.all(cls[proba > 0.5] == 1) and np.all(cls[proba < 0.5] == -1) and np.all(proba[cls == 0] == 0.5)
    assert np.all(proba[cls == 1] >= 0.5) and np.all(proba[cls == -1] <= 0.5)
    # ... and the bits of lg_predict_proba over the same rows
    assert np.array_equal(bits(proba), bits(eng.lg_predict_proba(rows.astype(np.int32)))), what
    # the tallies are those of the classes and the labels, range by range
    at = 0
    for r, (a, b) in enumerate(ranges):
        c, y = cls[at:at + b - a].astype(np.int64), R.y[a:b].astype(np.int64)
        assert counts[r].tolist() == [int(np.sum(c == y)), int(np.sum(c == 0)), int(np.sum(c == -y))], (what, r)
        at += b - a
    full = [(r, ab) for r, ab in enumerate(ranges) if ab[1] > ab[0]]
    for r, (a, b) in enumerate(ranges):
        if a == b:
            assert range_loss[r] == 0.0 and counts[r].tolist() == [0, 0, 0]
    if twins:
        # every range's loss and accuracy: the bits of lg_loss_acc on it alone and of lg_loss_acc_ranges, 16 ranges a call
        for r, (a, b) in full[:12] + full[-4:]:
            l1, a1 = eng.lg_loss_acc(a, b)
            assert (l1, a1) == (range_loss[r], counts[r][0] / float(b - a)), (what, r, a, b)
        for i in range(0, len(full), 16):
            chunk = full[i:i + 16]
            for (r, (a, b)), (l16, a16) in zip(chunk, eng.lg_loss_acc_ranges([ab for _, ab in chunk])):
                assert (l16, a16) == (range_loss[r], counts[r][0] / float(b - a)), (what, r, a, b)
    assert acc == int(counts[:, 0].sum()) / float(len(rows))
    # the same call gives the same bits
    again = eng.lg_predict_ranges(ranges, want_proba=True)
    assert np.array_equal(again[0], cls) and np.array_equal(bits(again[1]), bits(proba)) and np.array_equal(again[2], counts)
    assert np.array_equal(again[3], range_loss) and again[4:] == (loss, acc)
    # against the fp64 reference
    R.check_rows(rows, cls, proba, what)
    total_bound = 0.0
    for r, (a, b) in full:
        R.check_range(a, b, counts[r], range_loss[r], "%s range %d [%d, %d)" % (what, r, a, b))
        total_bound += (b - a) / float(len(rows)) * R.dloss(np.arange(a, b))
    want = R.lam * R.nsq + float(np.mean(R.li[rows]))
    total_bound += (len(ranges) + 1) * lb.V * float(np.mean(R.li[rows]))
    print("%s: total loss err/bound %.3f" % (what, abs(loss - want) / total_bound))
    assert abs(loss - want) <= total_bound, (what, loss, want, total_bound)
    return cls, proba, counts, range_loss, loss, acc


def test_the_cached_bound_is_lb_dloss(synth):
    _, R = synth
    idx = np.concatenate([np.random.default_rng(2).permutation(cases.N)[:300], [5, 5, 5]])
    assert np.isclose(R.dloss(idx), lb.dloss(sub_csr(R.csr, idx), R.w, 0, len(idx), R.lam), rtol=1e-9, atol=0.0)
    assert np.isclose(R.dloss(np.arange(1500, 2500)), lb.dloss(R.csr, R.w, 1500, 2500, R.lam), rtol=1e-9, atol=0.0)


# ---- 1. dsgd_lg_predict_ranges ----------------------------------------------------------------------------------------------
def test_every_shape_in_one_launch(big):
    eng, R = big
    check_predict_ranges(eng, R, MIX, "mixed")


def test_each_shape_alone_and_without_outputs(big):
    eng, R = big
    mixed = eng.lg_predict_ranges(MIX, want_proba=True)
    at = 0
    for r, (a, b) in enumerate(MIX):
        if b > a:   # a launch over the range alone: the same bytes, the same bits
            cls, proba, counts, range_loss, loss, acc = eng.lg_predict_ranges([(a, b)], want_proba=True)
            assert np.array_equal(cls, mixed[0][at:at + b - a]) and np.array_equal(bits(proba), bits(mixed[1][at:at + b - a]))
            assert np.array_equal(counts[0], mixed[2][r]) and range_loss[0] == mixed[3][r]
            assert (loss, acc) == eng.lg_loss_acc(a, b)     # one range: the total is the range's
        at += b - a
    # without the probabilities: the same classes; every output but one null: that one
    cls, none, counts, range_loss, loss, acc = eng.lg_predict_ranges(MIX)
    assert none is None and np.array_equal(cls, mixed[0]) and np.array_equal(counts, mixed[2]) and (loss, acc) == mixed[4:]
    k = len(MIX)
    rb, re_ = (C.c_int64 * k)(*[a for a, _ in MIX]), (C.c_int64 * k)(*[b for _, b in MIX])
    only = C.c_double(-1.0)
    assert eng._lib.dsgd_lg_predict_ranges(eng._ctx, None, rb, re_, k, None, None, None, None, C.byref(only), None) == 0
    assert only.value == mixed[4]
    assert eng._lib.dsgd_lg_predict_ranges(eng._ctx, None, rb, re_, k, None, None, None, None, None, None) == EINVAL


def test_256_ranges_of_uneven_lengths(big):
    eng, R = big
    check_predict_ranges(eng, R, R256, "256 ranges")


def test_all_zero_row_is_class_zero():
    # rows: empty; one entry under a zero weight; under -0.0; d > 0; d < 0 -- labels +1, -1, +1, -1, -1
    csr = (np.array([0, 0, 1, 2, 3, 4], np.int64), np.array([1, 2, 3, 4], np.int32), np.array([1.0, -2.0, 1.0, 1.0], np.float32),
           np.array([1, -1, 1, -1, -1], np.int8))
    w = np.array([0.0, 0.0, -0.0, 0.75, -0.75, 5.0, 0.0, 0.0], dtype=np.float32)
    with engine_of(csr, 7, 0.0, w) as eng:
        for ranges, want_cls, want_counts in (([(0, 5)], [0, 0, 0, 1, -1], [[1, 3, 1]]), ([(3, 5), (0, 1), (1, 3)], [1, -1, 0, 0, 0], [[1, 0, 1], [0, 1, 0], [0, 2, 0]])):
            cls, proba, counts, range_loss, loss, acc = eng.lg_predict_ranges(ranges, want_proba=True)
            assert cls.tolist() == want_cls and counts.tolist() == want_counts
            assert np.all(proba[np.array(want_cls) == 0] == 0.5)
            for r, (a, b) in enumerate(ranges):
                assert (range_loss[r], counts[r][0] / float(b - a)) == eng.lg_loss_acc(a, b)
        loss, acc, counts = eng.lg_loss_acc_list([0, 1, 2])
        # l = log1p(exp(-0)) = log 2 on every row: three additions, a division and the library's log1p, each within 2^-53 of a value < 1
        assert counts == [0, 3, 0] and acc == 0.0 and abs(loss - np.log(2.0)) <= 2.0 ** -50


# ---- 2. dsgd_lg_loss_acc_list -------------------------------------------------------------------------------------------------
LIST_RANGES = [(0, 1), (5, 68), (5, 69), (5, 70), (3, 4098), (3, 4099), (8400, 28400)]   # 1, 63, 64, 65, 4,095, 4,096 and 20,000 rows


def test_list_of_a_range_has_the_bits_of_lg_loss_acc(big):
    eng, R = big
    for a, b in LIST_RANGES:
        loss, acc, counts = eng.lg_loss_acc_list(np.arange(a, b, dtype=np.int32))
        assert (loss, acc) == eng.lg_loss_acc(a, b), (a, b)
        assert acc == counts[0] / float(b - a)
        R.check_range(a, b, counts, loss, "list of [%d, %d)" % (a, b))


def test_lists_with_duplicates_against_the_reference_and_themselves(big):
    eng, R = big
    rng = np.random.default_rng(31)
    p = rng.permutation(BIG_N).astype(np.int32)
    lists = {"1 entry": p[:1], "1,000 of a permutation": p[:1000], "row thrice": np.concatenate([p[:98], p[7:8], p[7:8]]),
             "4,097 with duplicates": rng.integers(0, 3000, size=4097).astype(np.int32), "one row 70 times": np.full(70, p[3], dtype=np.int32),
             "20,001 (longer than n_cu * 64, a row twice)": np.concatenate([p[:20000], p[11:12]])}
    for name, idx in lists.items():
        first = eng.lg_loss_acc_list(idx)
        assert eng.lg_loss_acc_list(idx) == first, name        # the same list, the same bits
        check_list(R, idx, *first, name)
    # a row named twice is counted twice
    one = eng.lg_loss_acc_list(p[3:4])
    many = eng.lg_loss_acc_list(np.full(70, p[3], dtype=np.int32))
    assert many[2] == [70 * c for c in one[2]] and many[1] == one[1]


# ---- 2b. ONE evaluation walk (csrc/dsgd_logistic.hpp: lg_eval_walk) behind every entry point -----------------------------------
def walk_data():
    """300 rows over 2,100 columns: ranks beyond LG_HOT (2,048) and beyond the 1,024-float tile of a short range.  Row 0 is empty,
    row 1 holds zeros only, row 2 has 150 non-zeros (the tail loop behind the LG_UNR * 16 = 64 in registers), row 3's two
    products are +0.5 and -0.5: d == 0 exactly."""
    rng = np.random.default_rng(77)
    n, dim = 300, 2100
    cols, vals = [], []
    for i in range(n):
        k = {0: 0, 1: 3, 2: 150, 3: 2}.get(i, int(rng.integers(20, 61)))
        c = np.sort(rng.choice(np.arange(3, dim + 1), size=k, replace=False)).astype(np.int32)
        v = (rng.standard_normal(k) + 0.25).astype(np.float32)
        if i == 1:
            v[:] = 0.0
        if i == 3:
            c, v = np.array([1, 2], np.int32), np.array([1.0, 1.0], np.float32)
        cols.append(c)
        vals.append(v)
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    label = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    csr = (row_ptr, np.concatenate(cols), np.concatenate(vals), label)
    w = rng.standard_normal(dim + 1)
    w[1], w[2] = 0.5, -0.5
    w = (w * np.where(np.arange(dim + 1) < 3, 1.0, 1.0 / np.std(ref.dots(csr, w)))).astype(np.float32)
    return csr, dim, w


def test_one_walk_behind_every_evaluation():
    csr, dim, w = walk_data()
    R = Ref(csr, w, cases.LAM)
    assert int(np.max(np.diff(csr[0]))) > 64 and R.d[3] == 0.0 and len(np.unique(csr[1])) > 2048
    with engine_of(csr, dim, cases.LAM, w) as eng:
        for a, b in ((0, 300), (1, 297)):
            rows = np.arange(a, b, dtype=np.int32)
            one = eng.lg_loss_acc(a, b)
            assert eng.lg_loss_acc_ranges([(a, b)]) == [one]
            assert eng.lg_loss_acc_ranges([(5, 50), (a, b), (a, b)])[1:] == [one, one]
            cls, proba, counts, range_loss, loss, acc = eng.lg_predict_ranges([(a, b)], want_proba=True)
            l_list, a_list, c_list = eng.lg_loss_acc_list(rows)
            assert (range_loss[0], loss, l_list) == (one[0],) * 3 and (acc, a_list) == (one[1],) * 2
            assert counts[0].tolist() == list(c_list) and sum(c_list) == b - a and one[1] == c_list[0] / float(b - a)
            # the class is the sign of the d behind the probability, which has the bits of lg_predict_proba
            assert np.array_equal(bits(proba), bits(eng.lg_predict_proba(rows)))
            assert np.array_equal(cls, np.sign(proba.astype(np.float64) - 0.5).astype(np.int8))
            y = R.y[a:b].astype(np.int64)
            assert counts[0].tolist() == [int(np.sum(cls == y)), int(np.sum(cls == 0)), int(np.sum(cls == -y))]
            zero = np.array([i - a for i in (0, 1, 3) if a <= i < b])
            assert np.all(cls[zero] == 0) and np.all(proba[zero] == 0.5)
            R.check_rows(rows.astype(np.int64), cls, proba, "walk [%d, %d)" % (a, b))
            R.check_range(a, b, counts[0], one[0], "walk [%d, %d)" % (a, b))
        # one topic whose plane is the labels: the single model
        eng.lg_topics_set(csr[3][None, :])
        eng.lg_topics_set_weights(w[None, :])
        for a, b in ((0, 300), (1, 297)):
            loss_t, acc_t = eng.lg_topics_loss_acc(a, b)
            assert (loss_t[0], acc_t[0]) == eng.lg_loss_acc(a, b)


# ---- 3. dsgd_lg_loss_acc_sampled ----------------------------------------------------------------------------------------------
def test_sampled_form_draws_the_reference_stream_and_has_the_bits_of_the_list_form(synth):
    eng, R = synth
    for seed, lo, hi, k in ((7, 0, 3000, 1000), (8, 3000, 4096, 5000), (9, 100, 165, 64), (10, 0, 4096, 1), (11, 77, 78, 5)):
        state = host.JavaRandom(seed).seed
        loss, acc, counts, st, draws, idx = eng.lg_loss_acc_sampled(state, lo, hi, k, want_idx=True)
        rnd = host.JavaRandom(seed)
        want = (host.sampled_list(rnd, hi - lo, k) + np.int32(lo)).astype(np.int32)
        assert np.array_equal(idx, want) and len(idx) == min(k, hi - lo) and st == rnd.seed, (seed, lo, hi, k)
        # the raw values a shuffle of the window consumes, rejections included (csrc/jrand.c)
        buf, st2 = np.arange(hi - lo, dtype=np.int32), C.c_uint64(state)
        assert draws == host._host_lib().dsgd_jrand_shuffle(C.byref(st2), buf.ctypes.data_as(C.c_void_p), C.c_int64(hi - lo)) and st == st2.value
        assert (loss, acc, counts) == eng.lg_loss_acc_list(idx), (seed, lo, hi, k)
        assert eng.lg_loss_acc_sampled(state, lo, hi, k)[:5] == (loss, acc, counts, st, draws)
        if hi - lo == 1:   # a window of one row draws nothing
            assert draws == 0 and st == state and idx.tolist() == [lo]
        if len(idx) >= 100:
            check_list(R, idx, loss, acc, counts, "sampled %d of [%d, %d)" % (k, lo, hi))


# ---- 4. refusals, with nothing written ------------------------------------------------------------------------------------------
def raw_ranges(eng, ranges, w=None):
    k = len(ranges)
    rb, re_ = (C.c_int64 * max(k, 1))(*[a for a, _ in ranges]), (C.c_int64 * max(k, 1))(*[b for _, b in ranges])
    total = max(64, sum(max(0, b - a) for a, b in ranges))
    cls, proba = np.full(total, 7, dtype=np.int8), np.full(total, 7.0, dtype=np.float32)
    counts, rl = np.full(3 * max(k, 1), -7, dtype=np.int64), np.full(max(k, 1), -7.0)
    loss, acc = C.c_double(-7.0), C.c_double(-7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = eng._lib.dsgd_lg_predict_ranges(eng._ctx, None if w is None else p(w), rb, re_, k, p(cls), p(proba), p(counts), p(rl), C.byref(loss), C.byref(acc))
    untouched = (cls == 7).all() and (proba == 7.0).all() and (counts == -7).all() and (rl == -7.0).all() and (loss.value, acc.value) == (-7.0, -7.0)
    return rc, bool(untouched)


def raw_list(eng, idx, n=None, w=None):
    idx = None if idx is None else np.asarray(idx, dtype=np.int32)
    loss, acc = C.c_double(-7.0), C.c_double(-7.0)
    counts = (C.c_int64 * 3)(-7, -7, -7)
    rc = eng._lib.dsgd_lg_loss_acc_list(eng._ctx, None if w is None else w.ctypes.data_as(C.c_void_p), None if idx is None else idx.ctypes.data_as(C.c_void_p),
                                        len(idx) if n is None else n, C.byref(loss), C.byref(acc), counts)
    return rc, (loss.value, acc.value, list(counts)) == (-7.0, -7.0, [-7] * 3)


def raw_sampled(eng, state, lo, hi, k, w=None, null_state=False):
    st = C.c_uint64(state)
    loss, acc = C.c_double(-7.0), C.c_double(-7.0)
    counts = (C.c_int64 * 3)(-7, -7, -7)
    idx = np.full(max(1, min(max(k, 1), 4096)), -7, dtype=np.int32)
    n, draws = C.c_int64(-7), C.c_int64(-7)
    rc = eng._lib.dsgd_lg_loss_acc_sampled(eng._ctx, None if w is None else w.ctypes.data_as(C.c_void_p), None if null_state else C.byref(st), lo, hi, k,
                                           C.byref(loss), C.byref(acc), counts, idx.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(draws))
    untouched = (loss.value, acc.value, list(counts), n.value, draws.value) == (-7.0, -7.0, [-7] * 3, -7, -7) and (idx == -7).all()
    return rc, int(st.value), bool(untouched)


def test_refused_arguments_write_nothing_and_leave_the_weights(synth):
    eng, R = synth
    n = cases.N
    other = (R.w * np.float32(0.5)).astype(np.float32)   # weights handed over with a refused call must not become resident
    state = host.JavaRandom(3).seed
    for ranges, code in (([(0, 10), (9, 20)], EINVAL), ([(0, 10), (30, 40), (5, 6)], EINVAL),   # overlapping
                         ([(i, i + 1) for i in range(257)], EINVAL),                             # 257 ranges
                         ([(0, 10), (20, 15)], EINVAL),                                         # reversed
                         ([(5, 5)], EINVAL), ([(5, 5), (9, 9)], EINVAL), ([], EINVAL),          # no rows at all
                         ([(0, 10), (n - 1, n + 1)], ERANGE), ([(-1, 5)], ERANGE)):             # a row outside the data
        assert raw_ranges(eng, ranges, other) == (code, True), ranges
    assert raw_ranges(eng, [(i, i + 1) for i in range(256)], None)[0] == 0
    for idx, code in (([0, n], ERANGE), ([3, -1, 4], ERANGE), ([], EINVAL)):
        assert raw_list(eng, idx, w=other) == (code, True), idx
    assert raw_list(eng, None, n=4) == (EINVAL, True) and raw_list(eng, [1, 2], n=0) == (EINVAL, True) and raw_list(eng, [1, 2], n=-5) == (EINVAL, True)
    for lo, hi, k, code in ((0, 100, 0, EINVAL), (0, 100, -1, EINVAL), (50, 50, 5, EINVAL), (60, 50, 5, EINVAL), (0, n + 1, 5, ERANGE), (-1, 50, 5, ERANGE)):
        assert raw_sampled(eng, state, lo, hi, k, other) == (code, state, True), (lo, hi, k)
    assert raw_sampled(eng, state, 0, 100, 10, null_state=True)[0] == EINVAL
    assert np.array_equal(bits(eng.get_weights()), bits(R.w))
    assert eng.lg_loss_acc_list(np.arange(100, dtype=np.int32))[:2] == eng.lg_loss_acc(0, 100)   # usable afterwards


def test_refused_contexts():
    d = cases.data()
    state = host.JavaRandom(3).seed
    with dsgd_amd.Engine(d.dim, cases.LAM, precision="fp64") as eng:    # an fp64 context
        eng.load_csr(*cases.csr(d))
        assert raw_ranges(eng, [(0, 10)]) == (EUNSUPPORTED, True)
        assert raw_list(eng, [1, 2, 3]) == (EUNSUPPORTED, True)
        assert raw_sampled(eng, state, 0, 100, 10) == (EUNSUPPORTED, state, True)
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:                      # no data loaded
        assert raw_ranges(eng, [(0, 10)]) == (ESTATE, True) and raw_list(eng, [1, 2, 3]) == (ESTATE, True)
        assert raw_sampled(eng, state, 0, 100, 10) == (ESTATE, state, True)
    with engine_of(cases.csr(d), d.dim, cases.LAM, cases.weights(1.0)) as eng:   # the lock-free engine running
        eng.build_dim_sparsity(cases.N)
        eng.async_start([(0, cases.N)], batch=100, lr=0.5, max_updates=1 << 40, seed=1, positional_bug=True)
        try:
            assert raw_ranges(eng, [(0, 10)]) == (ESTATE, True) and raw_list(eng, [1, 2, 3]) == (ESTATE, True)
            assert raw_sampled(eng, state, 0, 100, 10) == (ESTATE, state, True)
        finally:
            eng.async_stop()
        assert eng.lg_predict_ranges([(0, 10)])[2].sum() == 10          # usable afterwards


def test_window_beyond_the_device_form():
    n, d = (1 << 20) + 1, 1000      # rows of one entry each: one more than the longest window the device draws
    i = np.arange(n)
    csr = (np.arange(n + 1, dtype=np.int64), (i % d + 1).astype(np.int32), np.where(i % 3 == 0, -1.0, 1.0).astype(np.float32), np.where(i % 2 == 0, -1, 1).astype(np.int8))
    w = np.linspace(-1.0, 1.0, d + 1).astype(np.float32)
    with engine_of(csr, d, cases.LAM, w) as eng:
        state = host.JavaRandom(1).seed
        assert raw_sampled(eng, state, 0, n, 1000, (w * np.float32(2.0)).astype(np.float32)) == (EUNSUPPORTED, state, True)
        assert np.array_equal(bits(eng.get_weights()), bits(w))
        with pytest.raises(dsgd_amd.DsgdError) as e:
            eng.lg_loss_acc_sampled(state, 0, n, 1000)
        assert e.value.code == EUNSUPPORTED
        # 2^20 rows are served
        loss, acc, counts, st, dr, idx = eng.lg_loss_acc_sampled(state, 1, n, 1500, want_idx=True)
        rnd = host.JavaRandom(1)
        assert np.array_equal(idx, host.sampled_list(rnd, n - 1, 1500) + 1) and st == rnd.seed
        assert (loss, acc, counts) == eng.lg_loss_acc_list(idx)


# ---- 5. the context's state -------------------------------------------------------------------------------------------------
def test_new_calls_leave_the_context_as_they_found_it(synth):
    eng, R = synth
    w = R.w
    lists, lr = cases.step_cases()["3 workers 100/37/1"]
    glist = cases.gradient_lists()["100 (row thrice)"]
    state = host.JavaRandom(4).seed
    new_calls = {"predict_ranges": lambda: eng.lg_predict_ranges([(0, 100), (100, 100), (200, 4096)], want_proba=True),
                 "list": lambda: eng.lg_loss_acc_list(glist), "sampled": lambda: eng.lg_loss_acc_sampled(state, 0, 4096, 500)}

    def sequence(between):
        """gradient, evaluation, step, evaluation behind the step (on the |w'|^2 words the step left), step -- `between` in front of each"""
        eng.set_weights(w)
        out = []
        for f in (lambda: bits(eng.lg_gradient(glist)[0]), lambda: eng.lg_loss_acc(0, 4096), lambda: eng.lg_sync_step(lists, lr),
                  lambda: eng.lg_loss_acc(0, 4096), lambda: eng.lg_sync_step_ranges([(0, 1000), (1000, 4096)], 2.0 ** -6), lambda: bits(eng.get_weights())):
            between()
            out.append(f())
        return out

    base = sequence(lambda: None)
    for name, call in new_calls.items():
        got = sequence(call)
        for a, b in zip(base, got):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, name
    # weights handed over stay resident, and the figures are those of the resident form
    w2 = (w * np.float32(0.25)).astype(np.float32)
    for name, call_w, call in (("predict_ranges", lambda: eng.lg_predict_ranges([(0, 500)], w2), lambda: eng.lg_predict_ranges([(0, 500)])),
                               ("list", lambda: eng.lg_loss_acc_list(glist, w2), lambda: eng.lg_loss_acc_list(glist)),
                               ("sampled", lambda: eng.lg_loss_acc_sampled(state, 0, 4096, 500, w2), lambda: eng.lg_loss_acc_sampled(state, 0, 4096, 500))):
        eng.set_weights(w)
        a = call_w()
        assert np.array_equal(bits(eng.get_weights()), bits(w2)), name
        b = call()
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b) if x is not None), name
        assert eng.lg_loss_acc(0, 500) == eng.lg_loss_acc(0, 500, w2), name
    eng.set_weights(w)


# ---- 6. the mirror ----------------------------------------------------------------------------------------------------------
def test_logistic_sync_on_a_real_engine(synth, monkeypatch):
    eng, R = synth
    eng.set_weights(R.w)
    n_train = 3500
    m = host.LogisticSync(eng, n_train, cases.N, 3, rnd=host.JavaRandom(21))
    split = host.split_vanilla(n_train, 3)
    ranges = [(r.start, r.stop) for r in split]
    cls, _, counts, range_loss, loss, acc = eng.lg_predict_ranges(ranges)
    rows, classes = m.predict()
    assert np.array_equal(rows, np.arange(n_train)) and np.array_equal(classes, cls)
    assert m.distributed_loss_and_accuracy() == (loss, acc) and m.distributed_loss() == loss and m.distributed_accuracy() == acc
    w2 = (R.w * np.float32(0.5)).astype(np.float32)
    assert m.distributed_loss(w2) == eng.lg_predict_ranges(ranges, w2)[4]
    eng.set_weights(R.w)
    assert m.rnd.seed == host.JavaRandom(21).seed
    results = {}
    for env in ("0", "1"):
        monkeypatch.setenv("DSGD_SAMPLED_DEVICE", env)
        m = host.LogisticSync(eng, n_train, cases.N, 3, rnd=host.JavaRandom(21))
        results[env] = (m.local_sampled_loss(700), m.local_sampled_accuracy(300), m.local_sampled_loss(100, test=True), m.rnd.seed)
    assert results["0"] == results["1"]
    # ... and they are the direct Engine calls over the lists the host route draws, from where it leaves the stream
    rnd = host.JavaRandom(21)
    a = host.sampled_list(rnd, n_train, 700)
    b = host.sampled_list(rnd, n_train, 300)
    c = host.sampled_list(rnd, cases.N - n_train, 100) + np.int32(n_train)
    assert results["0"] == (eng.lg_loss_acc_list(a)[0], eng.lg_loss_acc_list(b)[1], eng.lg_loss_acc_list(c)[0], rnd.seed)
    m._pending = {"plan": None, "seed_before": 0}
    with pytest.raises(RuntimeError):
        m.local_sampled_loss(10)


# ---- 7. other widths, hostile values -----------------------------------------------------------------------------------------
def check_case(case, ranges, lists):
    R = Ref(case.csr, case.w, case.lam)
    with engine_of(case.csr, case.dim, case.lam, case.w) as eng:
        check_predict_ranges(eng, R, ranges, case.name)
        for a, b in ranges:
            if b > a:
                assert eng.lg_loss_acc_list(np.arange(a, b, dtype=np.int32))[:2] == eng.lg_loss_acc(a, b)
        for name, idx in lists.items():
            first = eng.lg_loss_acc_list(idx)
            assert first == eng.lg_loss_acc_list(idx)
            check_list(R, idx, *first, "%s list %s" % (case.name, name))
        n = len(case.csr[3])
        state = host.JavaRandom(6).seed
        loss, acc, counts, st, draws, idx = eng.lg_loss_acc_sampled(state, 0, n, 200, want_idx=True)
        assert (loss, acc, counts) == eng.lg_loss_acc_list(idx)


@pytest.mark.parametrize("dim", [1, 2046, 2047, 2048], ids=lambda d: "dp%d" % (d + 1))
def test_models_of_2_and_about_lg_hot_columns(dim):
    case = hc.width(dim)
    check_case(case, [(0, 300), (300, 300), (300, 599), (599, 600)], case.grad_lists)


@pytest.mark.parametrize("trait", hd.TRAITS)
def test_hostile_values(trait):
    case = hc.hostile(trait)
    check_case(case, hc.H_RANGES, case.grad_lists)
