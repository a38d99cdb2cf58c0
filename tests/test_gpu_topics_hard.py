"""The one-vs-rest topic kernels on the GPU -- planar (csrc/dsgd_lg_topics.hpp), interleaved (_il.hpp), wide (_wide.hpp) and the column
lists (_cols.hpp) -- at hostile values, full-scale sums and model widths on every head and tile edge (tests/topics_hard_cases.py), against
the fp64 reference tests/logistic_ref.py on (csr, plane t).  Three kinds of comparison and no tolerance beyond them:

  within the DERIVED bounds of tests/logistic_bound.py (dw, dloss, dc + 2^-25), whose worth on exactly these inputs
      tests/test_topics_hard_bound.py shows on the CPU: ALL T topics of every hostile and width case, through lg_topics_sync_step,
      lg_topics_sync_steps (three steps in one call against three reference steps, the bound carried from step to step),
      lg_topics_loss_acc, lg_topics_predict and, interleaved and wide, lg_topics_sync_step_ranges and lg_topics_sync_steps_ranges;
  bit for bit, on the same inputs: topic t against a single-model engine loaded with plane t, wide against interleaved and interleaved
      against planar at a T both serve, ranges against arange lists, a list step behind a ranges step;
  exactly: the saturated full-scale cases, whose expectations are Python integers and fractions -- float32 bits with +2^62 and -2^62 in
      adjacent accumulator words, through lists, ranges and the column lists with one and two steps, each followed by a list step that
      must give the expected bits again: every word was zeroed.

Uncertain rows of the evaluation (0 < |d_ref| <= dz_i), counted on the CPU with the reference alone; tests/test_topics_hard_bound.py asserts
at most 1 % of each range for every topic and prints the counts.
"""

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_hard_cases as lhc
import logistic_ref as ref
import topics_hard_cases as tc

pytestmark = pytest.mark.gpu

COLS = "dsgd_lg_topics_cgrad_kernel"
RATIOS = {}   # (entry point, group) -> the largest error / bound seen


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def engine_of(case):
    eng = dsgd_amd.Engine(case.dim, case.lam)
    eng.load_csr(*case.csr)
    return eng


def within(entry, case, what, got, want, bound):
    """got, want, bound: [T, ...] -- every topic inside its own bound"""
    r = np.abs(np.asarray(got, dtype=np.float64) - want) / bound
    ratio = float(np.max(r))
    RATIOS[(entry, case.group)] = max(RATIOS.get((entry, case.group), 0.0), ratio)
    worst = int(np.argmax(np.max(r.reshape(len(r), -1), axis=1)))
    print("%s %s %s %s: max err/bound %.6f (topic %d)" % (entry, case.group, case.name, what, ratio, worst))
    assert ratio <= 1.0, (entry, case.name, what, ratio, worst)


def arange_lists(ranges):
    return [np.arange(a, b, dtype=np.int32) for a, b in ranges]


def flat_of(lists, n_steps):
    return np.concatenate(lists * n_steps), np.concatenate([[0], np.cumsum([len(a) for a in lists] * n_steps)])


def set_form(eng, case, form, T):
    eng.lg_topics_set(case.P[:T], **tc.SET_KW[form])
    eng.lg_topics_set_weights(case.W[:T])
    assert eng.n_topics == T


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (entry, group), ratio in sorted(RATIOS.items()):
        print("\nlargest error / bound, %s, %s: %.6f" % (entry, group, ratio))


@pytest.fixture(scope="module", params=tc.BOUND_KEYS, ids=tc.BOUND_IDS)
def ctx(request):
    """one context per data set: the topics' engine, a second one for the comparisons of two forms, a single-model engine"""
    case = tc.bound_case(request.param)
    with engine_of(case) as eng, engine_of(case) as other, engine_of(case) as one:
        yield request.param, case, eng, other, one
    tc.forget(case)


def stacked(case, T, pick):
    return np.stack([pick(tc.reference(case, t)) for t in range(T)])


# ---- against the reference, within the derived bounds: all T topics ----------------------------------------------------------------
def test_steps_within_dw(ctx):
    key, case, eng, other, _ = ctx
    lists, lr = case.step
    for form, T in tc.forms_of(key):
        tag = "%s T=%d " % (form, T)
        set_form(eng, case, form, T)
        st = eng.lg_topics_sync_step(lists, lr)
        assert st["n_samples"] == st["n_active"] == sum(len(a) for a in lists)
        W1 = eng.lg_topics_get_weights()
        within("lg_topics_sync_step", case, tag + "100/37/1", W1, *[stacked(case, T, lambda r: r.steps["3 workers 100/37/1"][i]) for i in (0, 1)])
        eng.lg_topics_set_weights(case.W[:T])
        flat, offs = flat_of(lists, tc.N_CHAIN)
        assert eng.lg_topics_sync_steps(flat, offs, tc.N_CHAIN, len(lists), lr)["n_samples"] == len(flat)
        W3 = eng.lg_topics_get_weights()
        assert np.isfinite(W3).all()
        within("lg_topics_sync_steps", case, tag + "3 x 100/37/1", W3, *[stacked(case, T, lambda r: r.chain[i]) for i in (0, 1)])
        if form == "planar":
            continue
        set_form(other, case, form, T)
        for name, ranges in case.range_sets.items():
            want, bound = [stacked(case, T, lambda r: r.steps["ranges " + name][i]) for i in (0, 1)]
            n = sum(b - a for a, b in ranges)
            eng.lg_topics_set_weights(case.W[:T])
            assert eng.lg_topics_sync_step_ranges(ranges, case.lr_ranges) == {"n_samples": n, "n_active": n} and eng.grad_kernel_name() == COLS
            Wr = eng.lg_topics_get_weights()
            within("lg_topics_sync_step_ranges", case, tag + name, Wr, want, bound)
            # a list step behind the ranges step reads every accumulator word: left clean -- the bits of the same two steps as lists
            eng.lg_topics_sync_step(lists, lr)
            other.lg_topics_set_weights(case.W[:T])
            other.lg_topics_sync_step(arange_lists(ranges), case.lr_ranges)
            assert np.array_equal(bits(other.lg_topics_get_weights()), bits(Wr)), (form, T, name)     # ranges against arange lists
            other.lg_topics_sync_step(lists, lr)
            assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(other.lg_topics_get_weights())), (form, T, name)
            eng.lg_topics_set_weights(case.W[:T])
            assert eng.lg_topics_sync_steps_ranges(ranges, 1, case.lr_ranges) == {"n_samples": n, "n_active": n} and eng.grad_kernel_name() == COLS
            Wc = eng.lg_topics_get_weights()
            within("lg_topics_sync_steps_ranges", case, tag + name, Wc, want, bound)
            assert np.array_equal(bits(Wc), bits(Wr)), (form, T, name)
            eng.lg_topics_set_weights(case.W[:T])                                                    # three steps in one call: three list steps
            eng.lg_topics_sync_steps_ranges(ranges, 3, case.lr_ranges)
            other.lg_topics_set_weights(case.W[:T])
            other.lg_topics_sync_steps(*flat_of(arange_lists(ranges), 3), 3, len(ranges), case.lr_ranges)
            assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(other.lg_topics_get_weights())), (form, T, name)


def test_evaluation_within_dloss_and_dc(ctx):
    key, case, eng, _, _ = ctx
    n = len(case.csr[3])
    for form, T in tc.forms_of(key):
        tag = "%s T=%d " % (form, T)
        set_form(eng, case, form, T)
        p = eng.lg_topics_predict(np.arange(n, dtype=np.int32))
        assert p.shape == (T, n)
        within("lg_topics_predict", case, tag + "all rows", p, stacked(case, T, lambda r: ref.proba(r.d)), stacked(case, T, lambda r: lb.dc(r.dz) + 2.0 ** -25))
        for a, b in case.evals:
            loss, acc = eng.lg_topics_loss_acc(a, b)
            ev = [tc.reference(case, t).evals[(a, b)] for t in range(T)]
            within("lg_topics_loss_acc", case, tag + "[%d, %d)" % (a, b), loss, np.asarray([e[0] for e in ev]), np.asarray([e[1] for e in ev]))
            for t in range(T):   # the tallies, within the rows whose class may go either way
                assert abs(acc[t] * (b - a) - ev[t][2][0]) <= ev[t][3] + 1e-9, (form, T, t, a, b, acc[t] * (b - a), ev[t][2], ev[t][3])


# ---- against each other, bit for bit -----------------------------------------------------------------------------------------------
def run_topics(eng, case, form, T):
    """what one form gives from the case's weights: one step, three in one call, every evaluation, the probabilities, the ranges' steps"""
    n = len(case.csr[3])
    lists, lr = case.step
    set_form(eng, case, form, T)
    ev = [eng.lg_topics_loss_acc(a, b) for a, b in case.evals]
    p = eng.lg_topics_predict(np.arange(n, dtype=np.int32))
    eng.lg_topics_sync_step(lists, lr)
    W1 = eng.lg_topics_get_weights()
    eng.lg_topics_set_weights(case.W[:T])
    eng.lg_topics_sync_steps(*flat_of(lists, tc.N_CHAIN), tc.N_CHAIN, len(lists), lr)
    W3 = eng.lg_topics_get_weights()
    ev3 = eng.lg_topics_loss_acc(0, n)   # (|w'|^2 from the finish's words)
    Wr = {}
    if form != "planar":
        for name, ranges in case.range_sets.items():
            eng.lg_topics_set_weights(case.W[:T])
            eng.lg_topics_sync_steps_ranges(ranges, 2, case.lr_ranges)
            Wr[name] = eng.lg_topics_get_weights()
    return SimpleResult(W1=W1, W3=W3, ev=ev, ev3=ev3, p=p, Wr=Wr)


class SimpleResult:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def run_single(one, case, t):
    """the same from a single-model engine loaded with plane t"""
    n = len(case.csr[3])
    lists, lr = case.step
    one.load_csr(*tc.topic_csr(case, t))
    one.set_weights(case.W[t])
    ev = [one.lg_loss_acc(a, b) for a, b in case.evals]
    p = one.lg_predict_proba(np.arange(n, dtype=np.int32))
    one.lg_sync_step(lists, lr)
    W1 = one.get_weights()
    one.set_weights(case.W[t])
    one.lg_sync_steps(*flat_of(lists, tc.N_CHAIN), tc.N_CHAIN, len(lists), lr)
    W3 = one.get_weights()
    ev3 = one.lg_loss_acc(0, n)
    Wr = {}
    for name, ranges in case.range_sets.items():
        one.set_weights(case.W[t])
        one.lg_sync_steps_ranges(ranges, 2, case.lr_ranges)
        Wr[name] = one.get_weights()
    return SimpleResult(W1=W1, W3=W3, ev=ev, ev3=ev3, p=p, Wr=Wr)


def test_topics_give_the_single_models_bits(ctx):
    key, case, eng, _, one = ctx
    singles = {}
    for form, T in tc.forms_of(key):
        got = run_topics(eng, case, form, T)
        for t in (range(T) if case.group == "width" else tc.H_BIT_TOPICS(T)):
            if t not in singles:
                singles[t] = run_single(one, case, t)
            s = singles[t]
            assert np.array_equal(bits(got.W1[t]), bits(s.W1)) and np.array_equal(bits(got.W3[t]), bits(s.W3)), (form, T, t)
            assert np.array_equal(bits(got.p[t]), bits(s.p)), (form, T, t)
            for (loss, acc), (lo, ac), ab in zip(got.ev + [got.ev3], s.ev + [s.ev3], case.evals + [("after", "steps")]):
                assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), (form, T, t, ab, loss[t], lo)
            for name in got.Wr:
                assert np.array_equal(bits(got.Wr[name][t]), bits(s.Wr[name])), (form, T, t, name)
    assert not np.array_equal(bits(got.W1), bits(case.W[:T]))


def test_the_forms_give_each_others_bits(ctx):
    """wide against interleaved and interleaved against planar, at a T both serve (32 and 8, or all the planes a narrow data set carries)"""
    key, case, eng, other, _ = ctx
    for (fa, fb), T in ((("wide", "interleaved"), min(case.T, 32)), (("interleaved", "planar"), min(case.T, 8))):
        a, b = run_topics(eng, case, fa, T), run_topics(other, case, fb, T)
        assert np.array_equal(bits(a.W1), bits(b.W1)) and np.array_equal(bits(a.W3), bits(b.W3)) and np.array_equal(bits(a.p), bits(b.p)), (fa, fb, T)
        assert np.array_equal(bits64(a.ev + [a.ev3]), bits64(b.ev + [b.ev3])), (fa, fb, T)
        for name in b.Wr:
            assert np.array_equal(bits(a.Wr[name]), bits(b.Wr[name])), (fa, fb, T, name)


# ---- the width edges, by name --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", tc.W_KEYS, ids=["dim-%d" % k[1] for k in tc.W_KEYS])
def test_width_edges(key):
    """test_gpu_logistic_hard.test_width_edges' three statements, per topic: a step changes every column that has an entry; every other
    column moves by the regulariser alone, to the bit; the named edge ranks (topics_hard_cases.W_EDGE_RANKS) differ from that"""
    case = tc.width(key[1])
    row_ptr, col, _, _ = case.csr
    n, dp, dim = len(row_ptr) - 1, case.dim + 1, case.dim
    everything = np.arange(n, dtype=np.int32)
    lr = 2.0 ** -6
    W64 = case.W.astype(np.float64)
    reg_only = (W64 - lr * ((2.0 * case.lam) * W64)).astype(np.float32)   # float32(w - lr 2 lambda w): the fp64 expression, rounded once
    one_row = int(np.argmax((np.diff(row_ptr) >= 1) & (np.diff(row_ptr) < dp))) if dim > 1 else int(np.argmax(np.diff(row_ptr) == 1))
    ranks = lb.ranks_of(case.csr, dp)
    with engine_of(case) as eng:
        assert np.array_equal(eng.column_ranks(), ranks)
        for form, T in tc.forms_of(key):
            set_form(eng, case, form, T)
            steps = [("lists", [everything]), ("lists", [np.array([one_row], dtype=np.int32)]), ("lists", [np.array([0], dtype=np.int32)])]   # (row 0 is empty where the rows are hand-built)
            if form != "planar":
                steps += [("ranges", [(0, n)]), ("cols", [(0, n)]), ("ranges", [(one_row, one_row + 1)])]
            none_seen = 0
            for how, arg in steps:
                eng.lg_topics_set_weights(case.W[:T])
                if how == "lists":
                    eng.lg_topics_sync_step(arg, lr)
                    used = np.concatenate([col[row_ptr[r]:row_ptr[r + 1]] for r in arg[0]] + [np.zeros(0, np.int32)])
                else:
                    eng.lg_topics_sync_step_ranges(arg, lr) if how == "ranges" else eng.lg_topics_sync_steps_ranges(arg, 1, lr)
                    used = col[row_ptr[arg[0][0]]:row_ptr[arg[0][1]]]
                W1 = eng.lg_topics_get_weights()
                has = np.bincount(used, minlength=dp) > 0
                assert np.all(bits(W1[:, has]) != bits(case.W[:T, has])), (form, T, how)                 # a step changes every column that has an entry
                assert np.array_equal(bits(W1[:, ~has]), bits(reg_only[:T, ~has])), (form, T, how)      # ... and lambda alone moves the others
                none_seen = max(none_seen, int(np.count_nonzero(~has)))
                if len(used) == int(row_ptr[-1]):   # the whole set: the named edge ranks carry data in every topic
                    for r in tc.W_EDGE_RANKS.get((form, T, dim), []):
                        k = int(np.where(ranks == r)[0][0])
                        assert has[k] and np.all(bits(W1[:, k]) != bits(reg_only[:T, k])), (form, T, how, r, k)
            assert none_seen >= 1   # (the second check is not an empty one at any width)


# ---- full scale, exactly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", tc.EXACT_KEYS, ids=tc.EXACT_IDS)
def test_full_scale_sums_are_exact(key):
    case = tc.exact_case(*key)
    ex, n, lr, T = case.expect, case.n, case.lr, case.T
    W1, W2 = ex.whole
    everything = np.arange(n, dtype=np.int32)
    first = {int(s): int(np.argmax(case.signs == s)) for s in (1, -1)}   # the loss of a topic is that of the first topic of its sign

    def after(eng, what, want):
        """the weights' bits, a finite loss within dloss on every topic, and the accumulators left clean: a list step from the expected
        weights gives the expected bits again -- both halves of every pair of words were zeroed"""
        got = eng.lg_topics_get_weights()
        assert np.array_equal(bits(got), bits(want)), (what, int(np.count_nonzero(bits(got) != bits(want))), np.nonzero(np.any(bits(got) != bits(want), axis=1))[0][:8])
        loss, _ = eng.lg_topics_loss_acc(0, n)
        assert np.isfinite(loss).all()
        by_sign = {s: (ref.loss_acc(tc.topic_csr(case, t), want[t], 0, n, 0.0)[0], lb.dloss(tc.topic_csr(case, t), want[t], 0, n, 0.0)) for s, t in first.items()}
        within("lg_topics_loss_acc", case, what, loss, np.asarray([by_sign[int(s)][0] for s in case.signs]), np.asarray([by_sign[int(s)][1] for s in case.signs]))
        eng.lg_topics_set_weights(W1)
        eng.lg_topics_sync_step([everything], lr)
        again = eng.lg_topics_get_weights()
        assert np.array_equal(bits(again), bits(W2)), (what, "the list step behind it", np.nonzero(np.any(bits(again) != bits(W2), axis=1))[0][:8])

    with engine_of(case) as eng, engine_of(case) as second:
        for e in (eng, second):
            e.lg_topics_set(case.P, **tc.SET_KW[case.form])
        for name, (lists, want) in ex.step.items():
            eng.lg_topics_set_weights(case.W)
            eng.lg_topics_sync_step(lists, lr)
            after(eng, "lg_topics_sync_step " + name, want)
        eng.lg_topics_set_weights(case.W)
        eng.lg_topics_sync_steps(*flat_of([everything], 2), 2, 1, lr)
        after(eng, "lg_topics_sync_steps x 2", W2)
        if case.form != "planar":
            eng.lg_topics_set_weights(case.W)
            eng.lg_topics_sync_step_ranges([(0, n)], lr)
            assert eng.grad_kernel_name() == COLS
            after(eng, "lg_topics_sync_step_ranges", W1)
            eng.lg_topics_set_weights(case.W)
            eng.lg_topics_sync_step_ranges([(0, n)], lr)
            eng.lg_topics_sync_step_ranges([(0, n)], lr)   # the second step, from the first one's weights
            after(eng, "lg_topics_sync_step_ranges twice", W2)
            for n_steps, want in ((1, W1), (2, W2)):
                second.lg_topics_set_weights(case.W)
                second.lg_topics_sync_steps_ranges([(0, n)], n_steps, lr)
                assert second.grad_kernel_name() == COLS
                after(second, "lg_topics_sync_steps_ranges x %d" % n_steps, want)
        if case.labels == "alt":   # F cancels: +0.0 under either sign
            eng.lg_topics_set_weights(case.W)
            eng.lg_topics_sync_step([everything], lr)
            f = eng.lg_topics_get_weights()[:, lhc.E_F]
            assert np.all(f == 0.0) and not np.signbit(f).any()
