"""The hard inputs that tests/test_logistic_hard_bound.py (CPU) and tests/test_gpu_logistic_hard.py (GPU) share, the pattern of
tests/logistic_cases.py.  Three groups:

  hostile    hard_data.build(trait) for every trait of hard_data.TRAITS: a window of 2,048 rows and the weights h.w as float32
             (the SVM's planted rows need no logistic meaning: the value ranges are what matters -- vexp 10, -30 and whatever
             the wide and ragged rows give, negative values, products under the 1e-20 filter, rows of 8,000 entries).
  exact      hand-built, lambda = 0, every row saturated: one entry 1.0 on column P (y = +1) or M (y = -1) with w[P] = -64 and
             w[M] = +64, every other weight 0, so y d = -64 and c = -y EXACTLY in fp64 (1 + exp(-64) rounds to 1).  `tall`: n rows
             with one more entry vmax on the shared column F -- the sum reaches n vmax 2^(S - vexp), 2^62 at n = 4,096 and
             vmax = 1; `broad`: 2,100 shared columns, those of rank 2,048 and beyond on the global-atomic path at full scale.
             Every expectation is computed here in Python integers and fractions and the fp64 reference is REQUIRED to equal
             it: a GPU mismatch cannot be blamed on the reference.
  width      models of dp = 2, 16, 256, 257, 2,048, 2,049 and 300,001 columns: fewer than the LDS head (LG_HOT = 2,048), exactly
             as many, one more; one and two workgroups of the finish; a model narrower than the evaluation's hot tile.  At dim 255,
             256, 2,047 and 2,048 one synthetic row is replaced by a row of EVERY key, so the columns on those edges carry data.

A case is a SimpleNamespace: group, name, csr, dim, w (float32, read-only), lam, grad_lists {name: list}, step (lists, lr),
range_sets {name: ranges}, lr_ranges, evals [(begin, end)].  The exact cases carry `expect` instead (see exact_case).
"""

import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import hard_data as hd
import logistic_bound as lb
import logistic_ref as ref

# ---- hostile values ------------------------------------------------------------------------------------------------
H_ROWS = 2048
H_LAM = 1e-5
H_LR = 0.5               # the three-worker step of 100 / 37 / 1 rows
H_LR_RANGES = 2.0 ** -6  # (a worker's gradient is a SUM over its rows: 1,500 of them)
H_RANGES = [(0, 1500), (1500, 2047), (2047, 2048)]
# the first row of every trait's window.  0 unless the window's evaluation ranges held more than 1 % uncertain rows
# (tests/test_logistic_hard_bound.py counts them); none does.
H_WINDOW = {t: 0 for t in hd.TRAITS}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def hostile(trait):
    h = hd.build(trait)
    a = H_WINDOW[trait]
    d = h.data.rows(a, a + H_ROWS)
    rng = np.random.default_rng([41, hd.TRAITS.index(trait)])
    p = rng.permutation(H_ROWS).astype(np.int32)
    three = [_frozen(rng.permutation(H_ROWS)[:n].astype(np.int32)) for n in (100, 37, 1)]
    return SimpleNamespace(group="hostile", name=trait, csr=(d.row_ptr, d.col, d.val, d.label), dim=d.dim, w=_frozen(h.w.astype(np.float32)), lam=H_LAM,
                           grad_lists={"100": _frozen(p[:100].copy()), "2049 (row twice)": _frozen(np.concatenate([p, p[3:4]]))},
                           step=(three, H_LR), range_sets={"1500/547/1": H_RANGES}, lr_ranges=H_LR_RANGES, evals=[(0, H_ROWS)] + H_RANGES)


# ---- model widths --------------------------------------------------------------------------------------------------
W_DIMS = (1, 15, 255, 256, 2047, 2048, 300000)
W_ROWS = 600   # (the hand-built sets too: the range sets and the evaluation over [0, 600) need 600 rows)
W_LAM = 1e-3
W_LR = 0.5
W_LR_RANGES = 2.0 ** -6
W_RANGE_SETS = {"300/299/1": [(0, 300), (300, 599), (599, 600)], "k16 x 37": [(37 * i, 37 * (i + 1)) for i in range(16)]}
W_EVALS = [(0, 600), (77, 78)]
BELOW2 = np.nextafter(np.float32(2.0), np.float32(0.0))


def _hand_width(dim):
    """600 rows over the keys 0 .. dim: 0 .. dim + 1 entries each (row 0 and whatever the seed gives: empty), values in
    +-[0.25, 2), labels +-1"""
    rng = np.random.default_rng([13, dim])
    row_ptr, col, val = [0], [], []
    for i in range(W_ROWS):
        k = 0 if i == 0 else int(rng.integers(0, dim + 2))
        keys = np.sort(rng.choice(dim + 1, size=k, replace=False))
        v = np.minimum((0.25 + 1.75 * rng.random(k)).astype(np.float32), BELOW2) * rng.choice(np.float32([-1.0, 1.0]), size=k)
        col += keys.tolist()
        val += v.tolist()
        row_ptr.append(len(col))
    label = rng.choice(np.int8([-1, 1]), size=W_ROWS)
    return (np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float32), label.astype(np.int8))


# The synthetic rows never use key 0, and 600 of them leave a few more keys of a narrow model without an entry: the columns of the
# last ranks -- at dim 2,047 and 2,048 the LDS head's last word (rank 2,047) and the first column beyond it (rank 2,048), at
# dim 256 the finish's second workgroup (rank 256) -- would hold the regulariser alone.  So at these widths row W_FULL_ROW is
# replaced by one that touches EVERY key 0 .. dim: every rank has data, the last ranks that row's entry alone.
W_FULL = (255, 256, 2047, 2048)
W_FULL_ROW = 1
# the ranks on an edge at each of these widths: the last column of the finish's first workgroup (255) and the only one of its
# second (256); the LDS head's last word (2,047) and the first column beyond it (2,048)
W_EDGE_RANKS = {255: [255], 256: [255, 256], 2047: [2047], 2048: [2047, 2048]}


def _with_full_row(csr, dim):
    row_ptr, col, val, label = csr
    rng = np.random.default_rng([17, dim])
    v = (0.5 + 0.5 * rng.random(dim + 1)) * rng.choice([-1.0, 1.0], size=dim + 1)
    v = (v / np.sqrt(np.sum(v * v))).astype(np.float32)   # (L2-normalised, as every synthetic row is: no entry above the others')
    b, e = int(row_ptr[W_FULL_ROW]), int(row_ptr[W_FULL_ROW + 1])
    lens = np.diff(row_ptr)
    lens[W_FULL_ROW] = dim + 1
    out = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([col[:b], np.arange(dim + 1, dtype=np.int32), col[e:]]).astype(np.int32),
           np.concatenate([val[:b], v, val[e:]]).astype(np.float32), label)
    assert np.all(np.bincount(out[1], minlength=dim + 1) > 0)
    return out


@functools.lru_cache(maxsize=None)
def width(dim):
    if dim >= 255:
        from dsgd_amd import synth

        d = synth.generate(W_ROWS, seed=13, dim=dim)
        csr = (d.row_ptr, d.col, d.val, d.label)
        if dim in W_FULL:
            csr = _with_full_row(csr, dim)
    else:
        csr = _hand_width(dim)
        assert np.any(np.diff(csr[0]) == 0) and np.all(np.abs(csr[2]) >= 0.25) and np.all(np.abs(csr[2]) < 2.0)
    w = np.random.default_rng(3).standard_normal(dim + 1)   # (logistic_cases.weights(1.0): logits of standard deviation 1)
    w = (w * (1.0 / np.std(ref.dots(csr, w)))).astype(np.float32)
    rng = np.random.default_rng([43, dim])
    p = rng.permutation(W_ROWS).astype(np.int32)
    three = [rng.permutation(W_ROWS)[:n].astype(np.int32) for n in (100, 37, 1)]
    if dim in W_FULL and not any(W_FULL_ROW in a for a in three):
        three[1][0] = W_FULL_ROW   # the row of every key steps with the 37-row worker
    three = [_frozen(a) for a in three]
    grads = {"17": _frozen(p[:17].copy()), "600 (the whole set)": _frozen(np.arange(W_ROWS, dtype=np.int32))}
    return SimpleNamespace(group="width", name="dim %d" % dim, csr=csr, dim=dim, w=_frozen(w), lam=W_LAM, grad_lists=grads,
                           step=(three, W_LR), range_sets=W_RANGE_SETS, lr_ranges=W_LR_RANGES, evals=W_EVALS)


# every case that is held to the derived bounds, on the CPU (emulated) and on the GPU: keys, so that collecting a test builds nothing
BOUND_KEYS = [("hostile", t) for t in hd.TRAITS] + [("width", d) for d in W_DIMS]
BOUND_IDS = ["%s-%s" % k for k in BOUND_KEYS]


def bound_case(key):
    return hostile(key[1]) if key[0] == "hostile" else width(key[1])


def bound_cases():
    return [bound_case(k) for k in BOUND_KEYS]


def step_cases(case):
    """name -> (lists, lr): the three-worker step and every range set as np.arange lists"""
    out = {"3 workers 100/37/1": case.step}
    for name, ranges in case.range_sets.items():
        out["ranges " + name] = ([np.arange(a, b, dtype=np.int32) for a, b in ranges], case.lr_ranges)
    return out


def uncertain(case, a, b):
    """how many rows of [a, b) have 0 < |d_ref| <= dz_i: their class may go either way"""
    d = ref.dots(case.csr, case.w)[a:b]
    return int(np.count_nonzero((np.abs(d) > 0) & (np.abs(d) <= lb.dz(case.csr, case.w)[a:b])))


# ---- full scale, exact ---------------------------------------------------------------------------------------------
E_DIM = 4095
E_P, E_M, E_F = 3000, 3001, 7     # broad: the keys 1 .. 2,100 tie on the count and rank by key (0 .. 2,099), P behind them
E_BROAD = 2100
E_LR_TALL = 2.0 ** -11            # n = 4,096: w[P] moves by 2, w[F] by 2 vmax -- y d stays below -40 for the second step
E_LR_BROAD = 2.0 ** -16           # n = 64: 2,100 columns move by 2^-10 vmax each; y d is still below -40 after TWO steps
E_UNIT = 23                       # every value is an integer multiple of 2^-23 (1.0, and the float below 2)
TALL_N = (4095, 4096, 4097)
BROAD_N = (63, 64, 65)
SATURATED = -40.0                 # exp(-40) < 2^-57: 1 + exp(y d) IS 1.0 in fp64 wherever y d <= -40, whatever the exp's last bits


def _exact_csr(rows, labels):
    row_ptr, col, val = [0], [], []
    for r in rows:
        for k in sorted(r):
            col.append(k)
            val.append(r[k])
        row_ptr.append(len(col))
    return (np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float32), np.asarray(labels, np.int8))


def _int_sums(csr, idx):
    """sum over the listed rows of -y x, per column, in units of 2^-E_UNIT: Python-exact integers (int64, far from its end)"""
    row_ptr, col, val, label = csr
    xi = np.ldexp(val.astype(np.float64), E_UNIT)
    assert np.array_equal(xi, np.rint(xi)) and float(np.abs(xi).max()) < 2.0 ** 25
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    mult = np.bincount(np.asarray(idx, dtype=np.int64), minlength=len(row_ptr) - 1)
    g = np.zeros(E_DIM + 1, dtype=np.int64)
    np.add.at(g, col, -label[rows].astype(np.int64) * xi.astype(np.int64) * mult[rows])
    assert int(np.abs(g).max()) < 2 ** 53   # (so g 2^-23 is a double)
    return g


def _assert_saturated(csr, w):
    d = ref.dots(csr, w)
    y = csr[3].astype(np.float64)
    assert float(np.max(y * d + lb.dz(csr, w))) <= SATURATED, float(np.max(y * d))   # (the GPU's fp32 dot is within dz of d)


def exact_gradient(csr, w, idx):
    """float64 [dp]: the gradient of the saturated rows, exact; the reference is required to give the same bits"""
    _assert_saturated(csr, w)
    g = np.ldexp(_int_sums(csr, idx).astype(np.float64), -E_UNIT)
    got = ref.gradient(csr, w, idx, 0.0)
    assert np.array_equal(got, g), int(np.count_nonzero(got != g))
    return g


def exact_step(csr, w, lists, lr):
    """float32 [dp]: np.float32 of the exact weights after one step from the float32 w.  Fractions; the exact value is
    required to BE a double (one rounding to float follows, as on the device) and the reference to give that double."""
    _assert_saturated(csr, w)
    tot = sum(_int_sums(csr, idx) for idx in lists)
    lrf = Fraction(float(lr))
    assert lrf.numerator == 1   # (a power of two)
    out = np.asarray(w, dtype=np.float64).copy()
    for j in np.nonzero(tot)[0]:
        exact = Fraction(float(w[j])) - lrf * Fraction(int(tot[j]), (1 << E_UNIT) * len(lists))
        out[j] = float(exact)
        assert Fraction(out[j]) == exact, (int(j), exact)
    got = ref.sync_step(csr, w, lists, lr, 0.0)
    assert np.array_equal(got, out), int(np.count_nonzero(got != out))
    return out.astype(np.float32)


def _start_weights():
    w = np.zeros(E_DIM + 1, dtype=np.float32)
    w[E_P], w[E_M] = -64.0, 64.0
    return w


@functools.lru_cache(maxsize=None)
def exact_case(shape, n, vmax_name, labels="plus"):
    """shape "tall" or "broad"; labels "plus" (all +1) or "alt" (+1, -1, +1, ...: F cancels to exactly 0 at even n).
    expect: gradient {name: (idx, float32 g)}, step {name: (lists, float32 w1)}, whole = (w1, w2): one and two steps over all
    rows as ONE worker -- what lists, ranges and the column lists must all give; one_row = (row, g of that row alone, on the weights of ANY step)."""
    vmax = np.float32(hd.VMAX[vmax_name])
    y = [1 if labels == "plus" or i % 2 == 0 else -1 for i in range(n)]
    shared = {E_F: vmax} if shape == "tall" else {k: vmax for k in range(1, E_BROAD + 1)}
    csr = _exact_csr([{**shared, (E_P if y[i] > 0 else E_M): np.float32(1.0)} for i in range(n)], y)
    assert lb.vexp_of(csr[2]) == (0 if vmax_name == "one" else 1)
    lr = E_LR_TALL if shape == "tall" else E_LR_BROAD
    w0 = _start_weights()
    everything = np.arange(n, dtype=np.int32)
    grads = {"all": everything}
    steps = {"all": [everything]}
    if shape == "tall" and n == 4096:
        twice = np.concatenate([everything[::-1], everything[1:2]])   # 4,097 positions, row 1 twice: S = 49
        grads["4097 (row twice)"] = twice
        steps["1 x 4097"] = [twice]
        if labels == "plus":   # S = 50, 56 and 62 in one finish; 4,096 + 64 + 1 = 3 * 1,387: the mean over K = 3 is exact
            steps["3 workers 4096/64/1"] = [everything, np.arange(100, 164, dtype=np.int32), np.array([5], dtype=np.int32)]
    expect = SimpleNamespace(gradient={k: (v, exact_gradient(csr, w0, v).astype(np.float32)) for k, v in grads.items()},
                             step={k: (v, exact_step(csr, w0, v, lr)) for k, v in steps.items()})
    w1 = expect.step["all"][1]
    # the step moves w[P] and w[M] TOWARDS zero (a saturated row is a wrong one) and the shared columns away from it; the
    # second step is still saturated: asserted inside exact_step, on the float32 weights the first one left
    assert 32.0 < abs(float(w1[E_P])) < 64.0
    expect.whole = (w1, exact_step(csr, w1, [everything], lr))
    # a saturated row's gradient is -y x whatever the weights are: the SAME one-row answer behind every step, on the weights
    # each step leaves (exact_gradient asserts the saturation and the reference's bits on each of them)
    row = n - 1
    after = [w for _, w in expect.step.values()] + [expect.whole[1]]
    g_rows = [exact_gradient(csr, w, [row]).astype(np.float32) for w in after]
    assert all(np.array_equal(g.view(np.uint32), g_rows[0].view(np.uint32)) for g in g_rows) and not np.signbit(g_rows[0][g_rows[0] == 0]).any()
    expect.one_row = (row, g_rows[0])
    expect.sums = _int_sums(csr, everything)
    name = "%s n=%d vmax=%s labels=%s" % (shape, n, vmax_name, labels)
    return SimpleNamespace(group="exact", name=name, csr=csr, dim=E_DIM, w=_frozen(w0), lam=0.0, lr=lr, n=n, shape=shape, labels=labels,
                           vmax=float(vmax), expect=expect)


EXACT_KEYS = ([("tall", n, v, lab) for n in TALL_N for v in hd.VMAX for lab in ("plus", "alt")] + [("broad", n, v, "plus") for n in BROAD_N for v in hd.VMAX])
EXACT_IDS = ["%s-%d-%s-%s" % k for k in EXACT_KEYS]
