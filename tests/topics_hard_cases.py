"""The hard inputs that tests/test_topics_hard_bound.py (CPU) and tests/test_gpu_topics_hard.py (GPU) share: tests/logistic_hard_cases.py's
counterpart for the one-vs-rest topic kernels (csrc/dsgd_lg_topics.hpp, _il.hpp, _wide.hpp, _cols.hpp).  Everything is built lazily and
cached.  A data set carries the planes and weights of the LARGEST topic count that uses it; a form at T topics takes the first T of
them, so one fp64 reference and one emulation per (data set, topic) serve every form.

  hostile  logistic_hard_cases.hostile(trait)'s window of 2,048 rows, its lists, ranges and learning rates.  Plane 0 is the window's
           own labels, plane 1 all +1, plane 2 all -1, the rest seeded +-1.  Topic 0 carries the trait's h.w, every other topic
           softmax_hard_cases.dense_weights at scale 2: a lane that reads its neighbour's topic changes the answer.
  width    600 rows built as logistic_hard_cases.width and softmax_hard_cases.width build them, every rank with data, dense weights:
           the models on either side of every LDS head (N_HOT) and of every evaluation tile (EVAL_TILES), and dim 1.
  exact    logistic_hard_cases.exact_case's saturated rows under a sign s_t per topic: plane t = s_t y, W[t][P] = -64 s_t and
           W[t][M] = +64 s_t, so y_t d_t = -64 for every row and topic and topic t's sums are the single model's times s_t: adjacent
           accumulator words hold +2^62 and -2^62.

A bounded case is a SimpleNamespace: group, name, csr, dim, T (the planes it carries), P (int8 [T, n]), W (float32 [T, dp], read-only),
lam, step (lists, lr), range_sets, lr_ranges, evals.
"""

import functools
from types import SimpleNamespace

import numpy as np

import hard_data as hd
import logistic_bound as lb
import logistic_hard_cases as lhc
import logistic_ref as ref
import softmax_hard_cases as shc

# ---- the forms -------------------------------------------------------------------------------------------------------------
FORMS = {"planar": (3, 8), "interleaved": (5, 9, 32), "wide": (33, 65, 103, 128)}
T_MAX = 128
SET_KW = {"planar": {}, "interleaved": {"interleaved": True}, "wide": {"wide": True}}
HOT_WORDS = {"planar": 2048, "interleaved": 2048, "wide": 4096}   # LGT_HOT_WORDS, LGTI_HOT_WORDS, LGTW_HOT_WORDS


def tp_of(form, T):
    """the topics stored per rank: T itself in the planar form, lgti_tp(T) -- T rounded up to a multiple of 4 -- in the others"""
    return T if form == "planar" else (T + 3) & ~3


def n_hot(form, T):
    """lgt_hot(T), lgti_hot(tp), lgtw_hot(tp): the ranks of the gradient kernel's LDS head"""
    return HOT_WORDS[form] // tp_of(form, T)


def acc_stride(dp):
    """lgt_acc_stride: ranks between two workers' column sums"""
    return (dp + 31) & ~31


# the head of every (form, T) the width group puts a model edge on (tests/cpp/lg_topics_*_host_test.cpp assert the host functions'
# values)
N_HOT = {("planar", 8): 256,        # 2048 / 8
         ("planar", 3): 682,        # 2048 / 3, rounded down
         ("interleaved", 32): 64,   # 2048 / 32
         ("interleaved", 9): 170,   # 2048 / 12 (TP = 12), rounded down
         ("wide", 128): 32,         # 4096 / 128
         ("wide", 103): 39,         # 4096 / 104 (TP = 104), rounded down
         ("wide", 33): 113}         # 4096 / 36 (TP = 36), rounded down
assert all(n_hot(f, T) == v for (f, T), v in N_HOT.items())
# The evaluation's tile of 600 rows: lg*_eval_hw(600, min(hw_eval, dp), T) = min(dp, 1024) & ~63, less what the carve refuses.  At
# 600 rows the carve leaves 128 ranks or more at every T above (the smallest: wide 128, (40960 - 16804) / 128 = 188 -> 128), so the
# tile goes from none to 64 ranks at dp = 64 and from 64 to 128 at dp = 128 in every form.
EVAL_TILES = (64, 128)


def _edge_dims(edge):
    """dim + 1 = edge - 1, edge, edge + 1"""
    return [edge - 2, edge - 1, edge]


def _edge_ranks(edge):
    """dim -> the ranks on the edge: the last rank of a model one narrower, the last word inside, that word and the first beyond"""
    return {edge - 2: [edge - 2], edge - 1: [edge - 1], edge: [edge - 1, edge]}


W_SETS = list(N_HOT)
W_DIMS = {ft: sorted({1} | set(_edge_dims(N_HOT[ft])) | {d for e in EVAL_TILES for d in _edge_dims(e)}) for ft in W_SETS}
W_KEYS = [("width", dim) for dim in sorted({d for ds in W_DIMS.values() for d in ds})]
# (form, T, dim) -> the named edge ranks, as logistic_hard_cases.W_EDGE_RANKS names them: the head's (dim = n_hot - 2: the last rank of
# a model narrower than the head; n_hot - 1: the head's last word; n_hot: that word and the first column beyond) and the tiles' (62:
# the last rank of a model without a tile; 63: the tile's last rank; 64: that rank and the first read from global memory beside a
# tile; 126, 127, 128: the same at the tile of 128 ranks)
W_EDGE_RANKS = {}
for _ft in W_SETS:
    for _edge in (N_HOT[_ft],) + EVAL_TILES:
        for _dim, _ranks in _edge_ranks(_edge).items():
            W_EDGE_RANKS[_ft + (_dim,)] = sorted(set(W_EDGE_RANKS.get(_ft + (_dim,), []) + _ranks))


def width_topics(dim):
    """the planes a width data set carries: the largest T of the forms that use it"""
    return max(T for (f, T) in W_SETS if dim in W_DIMS[(f, T)])


def _frozen(a):
    a.setflags(write=False)
    return a


def planes_of(labels, T, seed):
    """int8 [T, n]: the labels, all +1, all -1, then seeded +-1 (the first T of T_MAX: a prefix whatever T is)"""
    n = len(labels)
    rest = np.random.default_rng(seed).choice(np.array([-1, 1], dtype=np.int8), size=(T_MAX - 3, n))
    P = np.vstack([np.asarray(labels, dtype=np.int8)[None], np.ones((1, n), np.int8), -np.ones((1, n), np.int8), rest])
    return _frozen(np.ascontiguousarray(P[:T], dtype=np.int8))


# ---- hostile values ----------------------------------------------------------------------------------------------------------
H_FORMS = {t: [("planar", 8), ("interleaved", 32), ("wide", 128)] for t in hd.TRAITS}
for _t in ("wide", "ragged64"):
    H_FORMS[_t] += [("wide", 33), ("wide", 103)]
H_KEYS = [("hostile", t) for t in hd.TRAITS]
def H_BIT_TOPICS(T):
    """the topics held to a single-model engine's bits"""
    return sorted({0, 1, 2, T // 2, T - 2, T - 1})


@functools.lru_cache(maxsize=None)
def hostile(trait):
    h = lhc.hostile(trait)
    W = shc.dense_weights(h.csr, h.dim + 1, T_MAX, 2.0, [61, hd.TRAITS.index(trait)], first=h.w)
    return SimpleNamespace(group="hostile", name=trait, csr=h.csr, dim=h.dim, T=T_MAX, P=planes_of(h.csr[3], T_MAX, [62, hd.TRAITS.index(trait)]), W=W,
                           lam=h.lam, step=h.step, range_sets=h.range_sets, lr_ranges=h.lr_ranges, evals=h.evals)


# ---- model widths --------------------------------------------------------------------------------------------------------------
def width_lr(dim):
    """the three-worker step's lr: softmax_hard_cases.W_LR's reasoning -- the hand-built rows (dim < 255) are not normalised, and at
    lr = 0.5 their step outweighs the weights it starts from; at the ranges' lr one step's bound is float precision up to 64 keys (beyond:
    tests/test_topics_hard_bound.py's OWN_PRECISION)"""
    return lhc.W_LR if dim >= 255 else lhc.W_LR_RANGES


@functools.lru_cache(maxsize=None)
def width(dim):
    if dim >= 255:
        from dsgd_amd import synth

        d = synth.generate(lhc.W_ROWS, seed=13, dim=dim)
        csr = lhc._with_full_row((d.row_ptr, d.col, d.val, d.label), dim)   # (the synthetic rows never use key 0)
    else:
        csr = lhc._hand_width(dim)
    assert np.all(np.bincount(csr[1], minlength=dim + 1) > 0)                # every rank has data
    T = width_topics(dim)
    W = shc.dense_weights(csr, dim + 1, T, 1.0, [63, dim])
    rng = np.random.default_rng([64, dim])
    three = [rng.permutation(lhc.W_ROWS)[:n].astype(np.int32) for n in (100, 37, 1)]
    if dim >= 255 and not any(lhc.W_FULL_ROW in a for a in three):
        three[1][0] = lhc.W_FULL_ROW   # the row of every key steps with the 37-row worker
    return SimpleNamespace(group="width", name="dim %d" % dim, csr=csr, dim=dim, T=T, P=planes_of(csr[3], T, [65, dim]), W=W, lam=lhc.W_LAM,
                           step=([_frozen(a) for a in three], width_lr(dim)), range_sets=lhc.W_RANGE_SETS, lr_ranges=lhc.W_LR_RANGES, evals=lhc.W_EVALS)


BOUND_KEYS = H_KEYS + W_KEYS
BOUND_IDS = ["%s-%s" % k for k in BOUND_KEYS]


def bound_case(key):
    return hostile(key[1]) if key[0] == "hostile" else width(key[1])


def forms_of(key):
    """the (form, T) pairs that run a data set"""
    return H_FORMS[key[1]] if key[0] == "hostile" else [ft for ft in W_SETS if key[1] in W_DIMS[ft]]


def topic_csr(case, t):
    return (case.csr[0], case.csr[1], case.csr[2], case.P[t])


def step_cases(case):
    """name -> (lists, lr): the three-worker step and every range set as np.arange lists"""
    out = {"3 workers 100/37/1": case.step}
    for name, ranges in case.range_sets.items():
        out["ranges " + name] = ([np.arange(a, b, dtype=np.int32) for a, b in ranges], case.lr_ranges)
    return out


N_CHAIN = 3   # lg_topics_sync_steps: three steps of the three-worker lists in one call


def reference(case, t):
    """Everything tests/logistic_ref.py and tests/logistic_bound.py say about topic t, once: d, dz (all rows), steps {name: (want, dw)},
    chain (want, bound) after N_CHAIN three-worker steps (the bound carried from step to step as dw's E), evals {(a, b): (loss, dloss,
    tallies, uncertain rows)}"""
    if not hasattr(case, "_refs"):
        case._refs = {}
    if t not in case._refs:
        csr, w = topic_csr(case, t), case.W[t]
        d, dz = ref.dots(csr, w), lb.dz(csr, w)
        steps = {name: (ref.sync_step(csr, w, lists, lr, case.lam), lb.dw(csr, w, lists, lr, case.lam)) for name, (lists, lr) in step_cases(case).items()}
        lists, lr = case.step
        wk, E = w.astype(np.float64), None
        for _ in range(N_CHAIN):
            E = lb.dw(csr, wk, lists, lr, case.lam, E)
            wk = ref.sync_step(csr, wk, lists, lr, case.lam)
        evals = {}
        for a, b in case.evals:
            loss, _, tallies, _ = ref.loss_acc(csr, w, a, b, case.lam)
            unsure = int(np.count_nonzero((np.abs(d[a:b]) > 0) & (np.abs(d[a:b]) <= dz[a:b])))
            evals[(a, b)] = (loss, lb.dloss(csr, w, a, b, case.lam), tallies, unsure)
        case._refs[t] = SimpleNamespace(d=d, dz=dz, steps=steps, chain=(wk, E), evals=evals)
    return case._refs[t]


def forget(case):
    """drop a case's cached references (a hostile data set's 128 topics hold a few hundred MB)"""
    case.__dict__.pop("_refs", None)


# ---- full scale, exact ---------------------------------------------------------------------------------------------------------
def signs_of(T, pattern):
    """s_t: "alt" +1, -1, +1, ...; "run" the same with topics 3 .. 7 all -1 -- a run of equal signs across a quad (3 | 4) and two
    lane-pair boundaries (3 | 4, 5 | 6)"""
    s = np.where(np.arange(T) % 2 == 0, 1, -1)
    if pattern == "run":
        assert T >= 8
        s[3:7] = -1
    return s


@functools.lru_cache(maxsize=None)
def _exact_signed(shape, n, vmax_name, labels, sign):
    """logistic_hard_cases.exact_case under the sign: (csr with labels sign y, w0, expect) -- step {name: (lists, float32 w1)} and whole =
    (w1, w2).  Every expectation is exact_step's: Python integers and fractions, held against the fp64 reference there.  (Not the
    single model's times the sign: a column whose sum cancels keeps +0.0 under either sign.)"""
    base = lhc.exact_case(shape, n, vmax_name, labels)
    if sign > 0:
        return base.csr, base.w, SimpleNamespace(step=base.expect.step, whole=base.expect.whole)
    csr = (base.csr[0], base.csr[1], base.csr[2], _frozen((-base.csr[3]).astype(np.int8)))
    w0 = _frozen(np.where(base.w == 0.0, np.float32(0.0), -base.w).astype(np.float32))   # (+0.0, not -0.0, off P and M)
    assert not np.signbit(w0[w0 == 0.0]).any()
    step = {name: (lists, lhc.exact_step(csr, w0, lists, base.lr)) for name, (lists, _) in base.expect.step.items()}
    w1 = step["all"][1]
    whole = (w1, lhc.exact_step(csr, w1, [np.arange(n, dtype=np.int32)], base.lr))
    for (_, a), (_, b) in zip(step.values(), base.expect.step.values()):   # the single model's integers times s_t
        assert np.array_equal(a, -b)
    assert np.array_equal(whole[1], -base.expect.whole[1])
    return csr, w0, SimpleNamespace(step=step, whole=whole)


@functools.lru_cache(maxsize=None)
def exact_case(shape, n, vmax_name, labels, form, T, pattern):
    """expect: step {name: (lists, float32 W1 [T, dp])}, whole = (W1, W2): one and two steps over all rows as ONE worker"""
    base = lhc.exact_case(shape, n, vmax_name, labels)
    s = signs_of(T, pattern)
    side = {sg: _exact_signed(shape, n, vmax_name, labels, sg) for sg in (1, -1)}
    stack = lambda pick: _frozen(np.stack([pick(side[int(sg)]) for sg in s]))
    P = _frozen(np.ascontiguousarray(stack(lambda x: x[0][3]), dtype=np.int8))
    W0 = stack(lambda x: x[1])
    assert np.array_equal(P, s[:, None] * base.csr[3][None]) and np.all(W0[:, lhc.E_P] == -64.0 * s) and np.all(W0[:, lhc.E_M] == 64.0 * s)
    expect = SimpleNamespace(step={name: (lists, stack(lambda x: x[2].step[name][1])) for name, (lists, _) in base.expect.step.items()},
                             whole=(stack(lambda x: x[2].whole[0]), stack(lambda x: x[2].whole[1])), sums=base.expect.sums)
    name = "%s n=%d vmax=%s labels=%s %s T=%d signs=%s" % (shape, n, vmax_name, labels, form, T, pattern)
    return SimpleNamespace(group="exact", name=name, csr=base.csr, dim=lhc.E_DIM, form=form, T=T, signs=s, P=P, W=W0, lam=0.0, lr=base.lr, n=n, shape=shape,
                           labels=labels, vmax=base.vmax, expect=expect)


E_LARGEST = [("planar", 8), ("interleaved", 32), ("wide", 128)]
EXACT_KEYS = ([("tall", 4096, v, "plus", f, T, "alt") for f, T in E_LARGEST for v in hd.VMAX] +
              [("tall", n, v, "plus", f, T, "alt") for n in (4095, 4097) for f, T in E_LARGEST[1:] for v in hd.VMAX] +
              [("tall", 4096, "one", "alt", f, T, "alt") for f, T in E_LARGEST] +      # F cancels to +0.0 under either sign
              [("tall", 4096, "one", "plus", f, T, "run") for f, T in E_LARGEST] +
              [("broad", n, v, "plus", f, T, "alt") for n in lhc.BROAD_N for f, T in E_LARGEST + [("wide", 33)] for v in hd.VMAX])
EXACT_IDS = ["-".join(str(x) for x in k) for k in EXACT_KEYS]
