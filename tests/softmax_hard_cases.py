"""The hard inputs that tests/test_softmax_bound.py (CPU) and tests/test_gpu_softmax_hard.py (GPU) share: tests/logistic_hard_cases.py's
counterpart for softmax regression (csrc/dsgd_lg_softmax.hpp).  Everything is built lazily and cached.  Five groups:

  hostile  logistic_hard_cases.hostile(trait)'s window of 2,048 rows, its three-worker lists and its ranges, for every trait of
           hard_data.TRAITS.  Class bytes from a seeded generator, every class present.  Class 0 carries the trait's own h.w (the
           planted rows keep their meaning for one class); every other class is dense: standard normal, scaled so that the class's
           fp64 logits over the window have standard deviation 2, rounded to float32.  C = 5 on every trait, 33 on scaled_m30 and
           signed (32-lane groups, idle lanes), 103 on wide and ragged64 (64-lane groups).
  width    600 rows built as logistic_hard_cases.width builds them, dense weights of unit-variance logits, lambda = 1e-3.  C = 128
           (the gradient's LDS head holds 4096 / TP = 32 ranks, groups of 64 lanes): dim 1, 30, 31, 32 -- narrower than the head,
           exactly as wide, one more -- and 62, 63, 64: the evaluation's tile min(hw_eval, dp) & ~63 goes from none to 64 ranks.
           C = 5 (the head holds 512 ranks): dim 510, 511, 512, and 255, 256: the finish's first and second workgroup.  W_EDGE_RANKS
           names the ranks on those edges; wherever the synthetic rows would leave one the regulariser alone, the row of every key
           (logistic_hard_cases.W_FULL_ROW) gives it data.
  small    the first 600 rows of logistic_cases.data() with the lists, classes and weights of tests/test_gpu_softmax.py's
           test_against_fp64, at the class counts on the group edges: C = 3, 4 (TP = 4, no padding class), 32 (16 lanes, all real)
           and 64 (32 lanes, all real).
  ties     hand-built rows of one entry on a private column: logits +40 on the tied classes and -40 elsewhere, EXACT on both
           sides, at C = 128, 64 and 32.  tie_rows says which classes tie, the row's class and the class every side must predict.
  exact    lambda = 0, every row saturated, the accumulators at full scale: see exact_case.  Every expectation is computed in
           Python integers and fractions and the fp64 reference softmax_bound.sync_step is REQUIRED to equal it here.
  long     20,000 synthetic rows for the evaluation's chains: more than twice 32 x 256 rows, so that chains carry two and three
           rows and the last pass is ragged.

A bounded case is a SimpleNamespace: group, name, csr, dim, C, cls (uint8), W (float32 [C, dp], read-only), lam, steps {name: (lists,
lr)}, range_sets {name: ranges}, lr_ranges, evals [(begin, end)].
"""

import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import hard_data as hd
import logistic_bound as lb
import logistic_hard_cases as lhc
import logistic_ref as ref
import softmax_bound as sm


def _frozen(a):
    a.setflags(write=False)
    return a


def classes_of(n, C, seed):
    """seeded class bytes, every class present"""
    cls = np.random.default_rng([seed, C]).integers(0, C, size=n).astype(np.uint8)
    cls[:C] = np.arange(C)
    return _frozen(cls)


def dense_weights(csr, dp, C, scale, seed, first=None):
    """float32 [C, dp]: per class standard normal, scaled so that its fp64 logits over the rows have standard deviation `scale`"""
    rng = np.random.default_rng(seed)
    W = np.empty((C, dp), dtype=np.float32)
    for c in range(C):
        w = rng.standard_normal(dp)
        W[c] = (w * (scale / np.std(ref.dots(csr, w)))).astype(np.float32)
    if first is not None:
        W[0] = first
    return _frozen(W)


# ---- hostile values ------------------------------------------------------------------------------------------------
H_CS = {t: (5,) for t in hd.TRAITS}
H_CS.update(scaled_m30=(5, 33), signed=(5, 33), wide=(5, 103), ragged64=(5, 103))
H_KEYS = [("hostile", t, C) for t in hd.TRAITS for C in H_CS[t]]


@functools.lru_cache(maxsize=None)
def hostile(trait, C):
    h = lhc.hostile(trait)   # (its window: logistic_hard_cases.H_WINDOW -- no softmax case needed a start of its own)
    dp = h.dim + 1
    W = dense_weights(h.csr, dp, C, 2.0, [51, hd.TRAITS.index(trait), C], first=h.w)
    return SimpleNamespace(group="hostile", name="%s C=%d" % (trait, C), csr=h.csr, dim=h.dim, C=C, cls=classes_of(lhc.H_ROWS, C, 52), W=W, lam=h.lam,
                           steps={"3 workers 100/37/1": h.step}, range_sets=h.range_sets, lr_ranges=h.lr_ranges, evals=h.evals)


# ---- model widths --------------------------------------------------------------------------------------------------
W_DIMS = {128: (1, 30, 31, 32, 62, 63, 64), 5: (255, 256, 510, 511, 512)}
W_KEYS = [("width", dim, C) for C in (128, 5) for dim in W_DIMS[C]]
# the ranks on an edge.  C = 128: the last rank of a model narrower than the LDS head of 32 ranks (30), the head's last word (31)
# and the first column beyond it (32); the last rank of a model without an evaluation tile (62), the tile's last rank (63) and
# the first rank read from global memory beside a tile (64).  C = 5: the head of 512 ranks in the same three positions (510, 511,
# 512); the last column of the finish's first workgroup (255) and the only one of its second (256).
W_EDGE_RANKS = {(128, 30): [30], (128, 31): [31], (128, 32): [31, 32], (128, 62): [62], (128, 63): [63], (128, 64): [63, 64],
                (5, 255): [255], (5, 256): [255, 256], (5, 510): [510], (5, 511): [511], (5, 512): [511, 512]}
W_LR_WHOLE = 2.0 ** -6   # the whole set as ONE worker: the step of the edge checks
# The three-worker step's lr.  C = 5 takes logistic_hard_cases.W_LR = 0.5.  At C = 128 the rows are the hand-built ones: up to dim + 1
# entries of magnitude up to 2, not normalised, so sum_j |x_ij| |w_cj| -- what dz_i grows with -- is many times the logit, and at
# lr = 0.5 the step lr G outweighs the weights it starts from: max |want| is then the gradient's size, and dw / max |want| the
# gradient's relative bound, above 1e-5 from dim 32 on.  At the ranges' lr, 2^-6, the weights carry max |want| and one step's bound
# is float precision at every width (tests/test_softmax_bound.py prints the ratio).
W_LR = {5: lhc.W_LR, 128: lhc.W_LR_RANGES}


@functools.lru_cache(maxsize=None)
def width(dim, C):
    if dim >= 255:
        from dsgd_amd import synth

        d = synth.generate(lhc.W_ROWS, seed=13, dim=dim)
        csr = lhc._with_full_row((d.row_ptr, d.col, d.val, d.label), dim)   # (the synthetic rows never use key 0)
    else:
        csr = lhc._hand_width(dim)
    assert np.all(np.bincount(csr[1], minlength=dim + 1) > 0)                # every rank has data
    W = dense_weights(csr, dim + 1, C, 1.0, [53, dim, C])
    rng = np.random.default_rng([54, dim])
    three = [rng.permutation(lhc.W_ROWS)[:n].astype(np.int32) for n in (100, 37, 1)]
    if dim >= 255 and not any(lhc.W_FULL_ROW in a for a in three):
        three[1][0] = lhc.W_FULL_ROW   # the row of every key steps with the 37-row worker
    return SimpleNamespace(group="width", name="dim %d C=%d" % (dim, C), csr=csr, dim=dim, C=C, cls=classes_of(lhc.W_ROWS, C, 55), W=W, lam=lhc.W_LAM,
                           steps={"3 workers 100/37/1": ([_frozen(a) for a in three], W_LR[C])}, range_sets=lhc.W_RANGE_SETS, lr_ranges=lhc.W_LR_RANGES,
                           evals=lhc.W_EVALS)


# ---- class counts on the group edges ---------------------------------------------------------------------------------
S_CS = (3, 4, 32, 64)
S_KEYS = [("small", C) for C in S_CS]


@functools.lru_cache(maxsize=None)
def small(C):
    """tests/test_gpu_softmax.py's `small` set and test_against_fp64's arguments at K = 1 and K = 3"""
    import logistic_cases as cases
    import test_gpu_softmax as t
    from test_gpu_logistic_topics import start_weights

    d, n = cases.data(), t.N_SMALL
    csr = (d.row_ptr[:n + 1], d.col[:d.row_ptr[n]], d.val[:d.row_ptr[n]], np.ones(n, np.int8))
    lists3 = [np.random.default_rng(6 + k).integers(0, n, size=k).astype(np.int32) for k in (100, 37, 1)]
    return SimpleNamespace(group="small", name="C=%d" % C, csr=csr, dim=d.dim, C=C, cls=_frozen(t.classes_of(n, C)), W=_frozen(start_weights(d.dim + 1, C)),
                           lam=cases.LAM, steps={"K=1": (lists3[:1], t.LR), "K=3": (lists3, t.LR)}, range_sets={}, lr_ranges=None, evals=list(t.RANGES))


# ---- ties ----------------------------------------------------------------------------------------------------------------
T_CS = (128, 64, 32)
T_KEYS = [("ties", C) for C in T_CS]
T_DIM = 255
T_LR = 0.25


def tie_rows(C):
    """[(the tied classes, the row's class, the class to predict)]: row 0 is EMPTY (every logit exactly 0: a tie of all classes);
    a tie across a ballot's far ends {1, C - 1}, at its top {C - 2, C - 1}, across the whole group {0, C - 1}, each also with the
    row's OWN class in the lowest slot (accuracy 1) and in the highest (accuracy 0); three tied; one row without a tie"""
    return [(tuple(range(C)), 0, 0),
            ((1, C - 1), 5, 1), ((1, C - 1), 1, 1), ((1, C - 1), C - 1, 1),
            ((C - 2, C - 1), 0, C - 2), ((C - 2, C - 1), C - 2, C - 2), ((C - 2, C - 1), C - 1, C - 2),
            ((0, C - 1), C - 1, 0), ((0, C - 1), 0, 0),
            ((2, C // 2, C - 3), C // 2, 2), ((3,), 3, 3)]


@functools.lru_cache(maxsize=None)
def ties(C):
    rows = tie_rows(C)
    n = len(rows)
    value = [np.float32(v) for v in (1.0, 0.5, 2.0)]
    W = np.zeros((C, T_DIM + 1), dtype=np.float32)
    csr_rows = [{}]
    for r in range(1, n):
        v = value[r % 3]
        W[:, 10 + r] = -40.0 / v            # (a power of two: every logit is exactly -40 ...)
        W[list(rows[r][0]), 10 + r] = 40.0 / v   # ... but the tied classes', exactly +40
        csr_rows.append({10 + r: v})
    csr = lhc._exact_csr(csr_rows, np.ones(n, np.int8))
    cls = _frozen(np.asarray([y for _, y, _ in rows], dtype=np.uint8))
    everything = np.arange(n, dtype=np.int32)
    # every row at every residue of four positions (and of two): a wave's lane groups other than its first vote too, and the 16- and
    # 32-lane forms take their ballot bits from a non-zero base
    blocks = [[0] * s + everything.tolist() for s in range(4)]   # (each filled up to a multiple of four positions with the empty row)
    predict = _frozen(np.asarray([r for b in blocks for r in b + [0] * (-len(b) % 4)], dtype=np.int32))
    assert all({int(p) % 4 for p in np.nonzero(predict == r)[0]} == {0, 1, 2, 3} for r in range(n)) and len(predict) >= 8
    return SimpleNamespace(group="ties", name="C=%d" % C, csr=csr, dim=T_DIM, C=C, cls=cls, W=_frozen(W), lam=0.0, rows=rows, predict=predict,
                           steps={"all rows, row 2 twice": ([_frozen(np.concatenate([everything, everything[2:3]]))], T_LR)}, range_sets={}, lr_ranges=None,
                           evals=[(0, n)] + [(r, r + 1) for r in range(n)])


# every case that is held to the derived bounds, on the CPU (emulated) and on the GPU: keys, so that collecting a test builds nothing
BOUND_KEYS = H_KEYS + W_KEYS + S_KEYS + T_KEYS
BOUND_IDS = ["-".join(str(x) for x in k) for k in BOUND_KEYS]


def bound_case(key):
    return {"hostile": hostile, "width": width, "small": small, "ties": ties}[key[0]](*key[1:])


def step_cases(case):
    """name -> (lists, lr): the list steps and every range set as np.arange lists"""
    out = dict(case.steps)
    for name, ranges in case.range_sets.items():
        out["ranges " + name] = ([np.arange(a, b, dtype=np.int32) for a, b in ranges], case.lr_ranges)
    return out


def reference(case):
    """(fp64 logits [n, C], dz_max [n]) of the case's weights, computed once"""
    if not hasattr(case, "_ref"):
        case._ref = (sm.logits(case.csr, case.W), sm.dz_max(case.csr, case.W))
    return case._ref


def step_reference(case, name):
    """(want, bound) of one step of step_cases: softmax_bound.sync_step and dw, computed once"""
    if not hasattr(case, "_steps"):
        case._steps = {}
    if name not in case._steps:
        lists, lr = step_cases(case)[name]
        case._steps[name] = (sm.sync_step(case.csr, case.W, case.cls, lists, lr, case.lam), sm.dw(case.csr, case.W, case.cls, lists, lr, case.lam))
    return case._steps[name]


def eval_reference(case, a, b):
    """(loss, dloss) of the case's weights over [a, b), computed once"""
    if not hasattr(case, "_evals"):
        case._evals = {}
    if (a, b) not in case._evals:
        Z, dzm = reference(case)
        case._evals[(a, b)] = (sm.loss_acc(case.csr, case.W, case.cls, a, b, case.lam, Z)[0], sm.dloss(case.csr, case.W, case.cls, a, b, case.lam, Z, dzm))
    return case._evals[(a, b)]


def expected_classes(case, a, b):
    """(the class every side must predict, which rows are compared): the reference's arg-max on the decided rows; a tie case's own table
    on every row"""
    if case.group == "ties":
        return np.asarray([p for _, _, p in case.rows[a:b]]), np.ones(b - a, dtype=bool)
    return np.argmax(reference(case)[0][a:b], axis=1), decided(case, a, b)


def decided(case, a, b):
    """bool [b - a]: the rows of [a, b) whose predicted class is compared (softmax_bound.decided)"""
    Z, dzm = reference(case)
    return sm.decided(Z[a:b], dzm[a:b])


def uncertain(case, a, b):
    return int(np.count_nonzero(~decided(case, a, b)))


# ---- full scale, exact ---------------------------------------------------------------------------------------------
# Every row has an entry 1.0 on column P (class 0) or M (class 1) beside the shared entries; the weights are 0 but on P -- -64 for
# class 0, +64 for class 1, -1000 for every class c >= 2 -- and, mirrored, on M.  For a class-0 row z - m is -128, 0 and -1064:
# exp(-1064) IS 0, exp(0) IS 1 and 1 + exp(-128) IS 1 whatever an exp or a division does in its last bits, so the coefficients
# p_c - [c == y] are EXACTLY -1, +1 and 0: class 0's sums are logistic_hard_cases._int_sums' (its label +1 = class 0, -1 = class
# 1), class 1's their negative, every other class's 0.  With all rows of class 0, n = 4,096 and vmax = 1, class 0's word on F
# reaches -2^62 and class 1's +2^62 in the same step.
E_CS = (2, 5, 65, 128)
E_W_OTHER = -1000.0
E_EXP_IS_ZERO = -746.0   # exp(x) is exactly 0.0 in fp64 below -745.14


def _assert_saturated(csr, cls, W):
    Z, dzm = sm.logits(csr, W), sm.dz_max(csr, W)   # (the GPU's fp32 logits are within dz_max of Z)
    y = np.asarray(cls, dtype=np.int64)
    i = np.arange(len(y))
    assert set(y.tolist()) <= {0, 1}
    assert float(np.max(Z[i, y] - Z[i, 1 - y] + 2.0 * dzm)) <= lhc.SATURATED, float(np.max(Z[i, y] - Z[i, 1 - y]))
    if Z.shape[1] > 2:
        assert float(np.max(Z[:, 2:] - Z[i, 1 - y][:, None] + 2.0 * dzm[:, None])) <= E_EXP_IS_ZERO


def exact_step(csr, cls, W, lists, lr):
    """float32 [C, dp]: np.float32 of the exact weights after one step from the float32 W.  Fractions; the exact value is required
    to BE a double (one rounding to float follows, as on the device) and the reference to give that double."""
    _assert_saturated(csr, cls, W)
    tot = sum(lhc._int_sums(csr, idx) for idx in lists)
    lrf = Fraction(float(lr))
    assert lrf.numerator == 1   # (a power of two)
    out = np.asarray(W, dtype=np.float64).copy()
    for j in np.nonzero(tot)[0]:
        for c, sign in ((0, 1), (1, -1)):
            exact = Fraction(float(W[c, j])) - sign * lrf * Fraction(int(tot[j]), (1 << lhc.E_UNIT) * len(lists))
            out[c, j] = float(exact)
            assert Fraction(out[c, j]) == exact, (c, int(j), exact)
    got = sm.sync_step(csr, W, cls, lists, lr, 0.0)
    assert np.array_equal(got, out), int(np.count_nonzero(got != out))
    return out.astype(np.float32)


def _start_weights(C):
    W = np.zeros((C, lhc.E_DIM + 1), dtype=np.float32)
    W[:, lhc.E_P] = W[:, lhc.E_M] = E_W_OTHER
    W[0, lhc.E_P], W[1, lhc.E_P], W[0, lhc.E_M], W[1, lhc.E_M] = -64.0, 64.0, 64.0, -64.0
    return W


@functools.lru_cache(maxsize=None)
def exact_case(shape, n, vmax_name, labels, C):
    """shape "tall" (one shared column F) or "broad" (2,100 shared columns); labels "zero" (every row of class 0) or "alt" (0, 1, 0,
    ...: F cancels to exactly +0.0 at even n).  expect: step {name: (lists, float32 W1)}, whole = (W1, W2): one and two steps over
    all rows as ONE worker -- what lists, the flat form and the ranges must all give; sums: class 0's integer column sums."""
    vmax = np.float32(hd.VMAX[vmax_name])
    y = [0 if labels == "zero" or i % 2 == 0 else 1 for i in range(n)]
    shared = {lhc.E_F: vmax} if shape == "tall" else {k: vmax for k in range(1, lhc.E_BROAD + 1)}
    csr = lhc._exact_csr([{**shared, (lhc.E_P if y[i] == 0 else lhc.E_M): np.float32(1.0)} for i in range(n)], [1 if c == 0 else -1 for c in y])
    assert lb.vexp_of(csr[2]) == (0 if vmax_name == "one" else 1)
    cls = _frozen(np.asarray(y, dtype=np.uint8))
    lr = lhc.E_LR_TALL if shape == "tall" else lhc.E_LR_BROAD
    W0 = _start_weights(C)
    everything = np.arange(n, dtype=np.int32)
    steps = {"all": [everything]}
    if shape == "tall" and n == 4096:
        steps["1 x 4097"] = [np.concatenate([everything[::-1], everything[1:2]])]   # 4,097 positions, row 1 twice: S = 49
        if labels == "zero":   # S = 50, 56 and 62 in one finish; 4,096 + 64 + 1 = 3 * 1,387: the mean over K = 3 is exact
            steps["3 workers 4096/64/1"] = [everything, np.arange(100, 164, dtype=np.int32), np.array([5], dtype=np.int32)]
    expect = SimpleNamespace(step={k: (v, exact_step(csr, cls, W0, v, lr)) for k, v in steps.items()})
    W1 = expect.step["all"][1]
    assert -64.0 < float(W1[0, lhc.E_P]) < -32.0 and 32.0 < float(W1[1, lhc.E_P]) < 64.0   # towards zero; still saturated: exact_step asserts it
    expect.whole = (W1, exact_step(csr, cls, W1, [everything], lr))
    expect.sums = lhc._int_sums(csr, everything)
    name = "%s n=%d vmax=%s labels=%s C=%d" % (shape, n, vmax_name, labels, C)
    return SimpleNamespace(group="exact", name=name, csr=csr, dim=lhc.E_DIM, C=C, cls=cls, W=_frozen(W0), lam=0.0, lr=lr, n=n, shape=shape, labels=labels,
                           vmax=float(vmax), expect=expect)


EXACT_KEYS = ([("tall", n, v, lab, C) for n in lhc.TALL_N for v in hd.VMAX for lab in ("zero", "alt") for C in E_CS] +
              [("broad", n, v, "zero", C) for n in lhc.BROAD_N for v in hd.VMAX for C in E_CS])
EXACT_IDS = ["-".join(str(x) for x in k) for k in EXACT_KEYS]


# ---- the long evaluation ---------------------------------------------------------------------------------------------------
# lgsm_eval_blocks gives one workgroup of 32 chains per 32 rows, at most one per compute unit: a chain serves a SECOND row -- the
# `ls = ls + l` over it and the stride `row += n_chains` -- only in a range of more than 32 n_cu rows, 8,192 on the MI355X's 256
# compute units.  20,000 rows give the chains two and three rows and a ragged last pass wherever rows > 2 * 32 * n_cu.
L_ROWS = 20000
L_CS = (5, 65)
L_LAM = 1e-5
L_N_CU = 256   # the MI355X; the shape assumes at most this many (the GPU test reads the device's own count and asserts the condition)
L_LONG = [(0, 20000), (3, 20000), (10000, 18193)]   # row_begin a multiple of nothing; 8,193 rows: ONE more than a row per chain
L_RANGES = L_LONG + [(0, 4095), (0, 4096)]          # ... and the two sides of the tile rule (rows >= 4096: the large LDS weight tile)


@functools.lru_cache(maxsize=None)
def _long_rows():
    from dsgd_amd import synth

    return synth.generate(L_ROWS, seed=29)


@functools.lru_cache(maxsize=None)
def long_case(C):
    d = _long_rows()
    csr = (d.row_ptr, d.col, d.val, d.label)
    return SimpleNamespace(group="long", name="C=%d" % C, csr=csr, dim=d.dim, C=C, cls=classes_of(L_ROWS, C, 57), W=dense_weights(csr, d.dim + 1, C, 2.0, [58, C]),
                           lam=L_LAM, evals=L_RANGES)
