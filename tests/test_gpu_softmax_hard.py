"""Softmax regression on the GPU (csrc/dsgd_lg_softmax.hpp) at hostile values, full-scale sums, odd model widths, class counts on the
group edges, ties across the ballots and a long evaluation (tests/softmax_hard_cases.py), against the fp64 reference of
tests/softmax_bound.py.  Three kinds of comparison and no tolerance beyond them:

  within the DERIVED bounds of tests/softmax_bound.py (dw, dloss, dc + 2^-25), whose worth on exactly these inputs
      tests/test_softmax_bound.py shows on the CPU: lg_softmax_sync_step, lg_softmax_sync_steps_ranges, lg_softmax_loss_acc and
      lg_softmax_predict on every hostile, width, small-class-count and tie case, lg_softmax_loss_acc on the long case;
  bit for bit: lg_softmax_sync_steps against lg_softmax_sync_step, the ranges against the lists over the same rows;
  exactly: the ties' predicted classes, and the saturated full-scale cases, whose expectations are Python integers and fractions --
      float32 bits through lists, the flat form and the ranges with one and two steps, the accumulators at +-2^62.

A predicted class is compared on every row the reference decides (softmax_bound.decided) and the correct count up to the uncertain
rows; tests/test_softmax_bound.py holds those to 1 % of each range and prints them: none in any evaluated range of any case here.

The long case's shape assumes at most 256 compute units: a chain of the evaluation serves a second row only in a range of more than
32 n_cu rows.  test_long_evaluation reads the device's count and asserts rows > 2 * 32 * n_cu on the whole-set ranges (three rows on
some chains, a ragged last pass) and rows > 32 * n_cu on [10000, 18193).
"""

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import softmax_bound as sm
import softmax_hard_cases as hc

pytestmark = pytest.mark.gpu

RATIOS = {}   # (entry point, group) -> the largest error / bound seen


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine_of(case):
    eng = dsgd_amd.Engine(case.dim, case.lam)
    eng.load_csr(*case.csr)
    eng.lg_softmax_set(case.cls, case.C)
    assert eng.n_classes == case.C
    return eng


def within(entry, case, what, got, want, bound):
    ratio = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / bound))
    RATIOS[(entry, case.group)] = max(RATIOS.get((entry, case.group), 0.0), ratio)
    print("%s %s %s %s: max err/bound %.6f" % (entry, case.group, case.name, what, ratio))
    assert ratio <= 1.0, (entry, case.name, what, ratio)


def flat(lists, n_steps):
    return np.concatenate(lists * n_steps), np.concatenate([[0], np.cumsum([len(a) for a in lists] * n_steps)])


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (entry, group), ratio in sorted(RATIOS.items()):
        print("\nlargest error / bound, %s, %s: %.6f" % (entry, group, ratio))


@pytest.fixture(scope="module", params=hc.BOUND_KEYS, ids=hc.BOUND_IDS)
def ctx(request):
    case = hc.bound_case(request.param)
    with engine_of(case) as eng:
        yield case, eng


# ---- against the reference, within the derived bounds ------------------------------------------------------------------
def test_steps_within_dw_and_the_forms_in_bits(ctx):
    case, eng = ctx
    for name, (lists, lr) in case.steps.items():
        want, bound = hc.step_reference(case, name)
        eng.lg_topics_set_weights(case.W)
        assert eng.lg_softmax_sync_step(lists, lr)["n_samples"] == sum(len(a) for a in lists)
        W1 = eng.lg_topics_get_weights()
        within("lg_softmax_sync_step", case, name, W1, want, bound)
        eng.lg_topics_set_weights(case.W)
        eng.lg_softmax_sync_steps(*flat(lists, 1), 1, len(lists), lr)
        assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(W1)), name
    for name, ranges in case.range_sets.items():
        want, bound = hc.step_reference(case, "ranges " + name)
        eng.lg_topics_set_weights(case.W)
        assert eng.lg_softmax_sync_steps_ranges(ranges, 1, case.lr_ranges)["n_samples"] == sum(b - a for a, b in ranges)
        W1 = eng.lg_topics_get_weights()
        within("lg_softmax_sync_steps_ranges", case, name, W1, want, bound)
        eng.lg_topics_set_weights(case.W)
        eng.lg_softmax_sync_step([np.arange(a, b, dtype=np.int32) for a, b in ranges], case.lr_ranges)
        assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(W1)), name


def test_evaluation_within_dloss_and_dc(ctx):
    case, eng = ctx
    n = len(case.cls)
    eng.lg_topics_set_weights(case.W)
    Z, dzm = hc.reference(case)
    idx = case.predict if case.group == "ties" else np.arange(n, dtype=np.int32)
    got_cls, p = eng.lg_softmax_predict(idx, proba=True)
    within("lg_softmax_predict", case, "%d positions" % len(idx), p, sm.probs(Z)[0][idx].T, (sm.dc(dzm, case.C) + 2.0 ** -25)[idx][None, :])
    expect, compared = hc.expected_classes(case, 0, n)
    assert np.array_equal(got_cls[compared[idx]], expect[idx][compared[idx]]) and np.array_equal(got_cls, eng.lg_softmax_predict(idx))
    for a, b in case.evals:
        loss, acc = eng.lg_softmax_loss_acc(a, b)
        want, bound = hc.eval_reference(case, a, b)
        within("lg_softmax_loss_acc", case, "[%d, %d)" % (a, b), loss, want, bound)
        correct_ref = int(np.count_nonzero(expect[a:b] == case.cls[a:b]))
        assert abs(acc * (b - a) - correct_ref) <= np.count_nonzero(~compared[a:b]) + 1e-9, (a, b, acc * (b - a), correct_ref)


@pytest.mark.parametrize("C", hc.T_CS)
def test_ties_across_the_ballots(C):
    """the lowest class of the largest logit, whichever lanes of the group tie and whichever group of the wave the row is in"""
    case = hc.ties(C)
    with engine_of(case) as eng:
        eng.lg_topics_set_weights(case.W)
        got = eng.lg_softmax_predict(case.predict)
        assert list(got) == [case.rows[r][2] for r in case.predict]
        for r, (tied, y, want) in enumerate(case.rows):
            loss, acc = eng.lg_softmax_loss_acc(r, r + 1)
            assert acc == float(want == y), (r, tied, y, acc)
            if tied == (0, C - 1):   # S = 2 exactly, z_y = m whichever of the two the row's class is
                assert abs(loss - np.log(2.0)) <= 1e-15, (r, loss)
        loss, acc = eng.lg_softmax_loss_acc(0, 1)   # the empty row: every logit 0, class 0, the loss log C
        assert acc == 1.0 and abs(loss - np.log(C)) <= 4e-16 * np.log(C)
        assert eng.lg_softmax_loss_acc(0, len(case.rows))[1] == sum(want == y for _, y, want in case.rows) / len(case.rows)


# ---- the width edges, by name ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, C", sorted((d, C) for C, d in hc.W_EDGE_RANKS))
def test_width_edges(dim, C):
    """the whole set as one worker: within dw, and every class's weight on every edge rank (softmax_hard_cases.W_EDGE_RANKS) moved,
    and by more than the regulariser alone -- tests/test_softmax_bound.py shows that each data sum there is more than 4 bounds from zero"""
    case = hc.width(dim, C)
    n, dp, lr = len(case.cls), dim + 1, hc.W_LR_WHOLE
    everything = [np.arange(n, dtype=np.int32)]
    W64 = case.W.astype(np.float64)
    reg_only = (W64 - lr * ((2.0 * case.lam) * W64)).astype(np.float32)
    want = sm.sync_step(case.csr, case.W, case.cls, everything, lr, case.lam)
    bound = sm.dw(case.csr, case.W, case.cls, everything, lr, case.lam)
    with engine_of(case) as eng:
        ranks = eng.column_ranks()
        assert np.array_equal(ranks, lb.ranks_of(case.csr, dp))
        for form in ("lists", "ranges"):
            eng.lg_topics_set_weights(case.W)
            if form == "lists":
                eng.lg_softmax_sync_step(everything, lr)
            else:
                eng.lg_softmax_sync_steps_ranges([(0, n)], 1, lr)
            W1 = eng.lg_topics_get_weights()
            within("lg_softmax_sync_step" if form == "lists" else "lg_softmax_sync_steps_ranges", case, "the whole set", W1, want, bound)
            for r in hc.W_EDGE_RANKS[(C, dim)]:
                key = int(np.where(ranks == r)[0][0])
                assert np.all(bits(W1[:, key]) != bits(case.W[:, key])) and np.all(bits(W1[:, key]) != bits(reg_only[:, key])), (form, r, key)


# ---- full scale, exactly -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", hc.EXACT_KEYS, ids=hc.EXACT_IDS)
def test_full_scale_sums_are_exact(key):
    case = hc.exact_case(*key)
    ex, n, lr = case.expect, case.n, case.lr
    W1, W2 = ex.whole
    everything = [np.arange(n, dtype=np.int32)]

    def after(eng, what, want):
        """the weights' bits, and a finite loss within dloss on them"""
        got = eng.lg_topics_get_weights()
        assert np.array_equal(bits(got), bits(want)), (what, int(np.count_nonzero(bits(got) != bits(want))))
        loss, _ = eng.lg_softmax_loss_acc(0, n)
        assert np.isfinite(loss)
        within("lg_softmax_loss_acc", case, what, loss, sm.loss_acc(case.csr, want, case.cls, 0, n, 0.0)[0], sm.dloss(case.csr, want, case.cls, 0, n, 0.0))

    with engine_of(case) as eng:
        for name, (lists, want) in ex.step.items():
            eng.lg_topics_set_weights(case.W)
            eng.lg_softmax_sync_step(lists, lr)
            after(eng, "lg_softmax_sync_step " + name, want)
            eng.lg_topics_set_weights(case.W)
            eng.lg_softmax_sync_steps(*flat(lists, 1), 1, len(lists), lr)
            after(eng, "lg_softmax_sync_steps " + name, want)
        eng.lg_topics_set_weights(case.W)
        eng.lg_softmax_sync_steps(*flat(everything, 2), 2, 1, lr)
        after(eng, "lg_softmax_sync_steps x 2", W2)
        for n_steps, want in ((1, W1), (2, W2)):
            eng.lg_topics_set_weights(case.W)
            eng.lg_softmax_sync_steps_ranges([(0, n)], n_steps, lr)
            after(eng, "lg_softmax_sync_steps_ranges x %d" % n_steps, want)
        if case.labels == "alt" and n % 2 == 0 and case.shape == "tall":   # F cancels: +0.0
            got = eng.lg_topics_get_weights()
            assert np.all(W2[:, hc.lhc.E_F] == 0.0) and not np.signbit(got[:, hc.lhc.E_F]).any()


# ---- the long evaluation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", hc.L_CS)
def test_long_evaluation(C):
    """chains with two and three rows, a ragged last pass, row_begin a multiple of nothing, 8,193 rows (one more than a row per chain),
    and the two sides of the tile rule.  The condition: rows > 2 * 32 * n_cu on the whole-set ranges, rows > 32 * n_cu on the third."""
    import torch

    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert all(b - a > 2 * 32 * n_cu for a, b in hc.L_LONG[:2]) and hc.L_LONG[2][1] - hc.L_LONG[2][0] > 32 * n_cu, n_cu
    case = hc.long_case(C)
    expect, compared = hc.expected_classes(case, 0, hc.L_ROWS)
    with engine_of(case) as eng:
        eng.lg_topics_set_weights(case.W)
        for a, b in case.evals:
            loss, acc = eng.lg_softmax_loss_acc(a, b)
            want, bound = hc.eval_reference(case, a, b)
            within("lg_softmax_loss_acc", case, "[%d, %d)" % (a, b), loss, want, bound)
            correct_ref = int(np.count_nonzero(expect[a:b] == case.cls[a:b]))
            assert abs(acc * (b - a) - correct_ref) <= np.count_nonzero(~compared[a:b]) + 1e-9, (a, b, acc * (b - a), correct_ref)
