"""The logistic family on the GPU at hostile values, full-scale sums and odd model widths (tests/logistic_hard_cases.py), against the
fp64 reference tests/logistic_ref.py.  Three kinds of comparison and no tolerance beyond them:

  within the DERIVED bounds of tests/logistic_bound.py (dg, dw, dloss, dc + 2^-25), whose worth on exactly these inputs
      tests/test_logistic_hard_bound.py shows on the CPU: every hostile and every width case, through lg_gradient, lg_sync_step,
      lg_loss_acc, lg_predict_proba, lg_sync_step_ranges and lg_sync_steps_ranges -- the column lists are held to the REFERENCE here,
      not only to the row form they share vexp, lg_shift, lg_coef and lg_add's expression with;
  bit for bit: ranges against lists, three column-list steps against three row-form steps in a second context, lg_loss_acc_ranges
      against single calls, a three-step lg_plan against lg_sync_steps;
  exactly: the saturated full-scale cases, whose expectations are Python integers and fractions -- float32 bits, through lists,
      ranges and the column lists with one and two steps, with the accumulators at +-2^62.

Uncertain rows of the evaluation (0 < |d_ref| <= dz_i: the class may go either way), counted on the CPU with logistic_ref alone
before any GPU run; the CPU test asserts <= 1 % of each range.  Over [0, 2048), [0, 1500), [1500, 2047), [2047, 2048):
scaled_p10, scaled_m30, signed and wide 0 / 0 / 0 / 0; zero_margin 3 / 1 / 2 / 0 (its rows of kind (b): every product under the
1e-20 filter); ragged64 2 / 2 / 0 / 0 (the 1e-25 entries).  Every width: 0 of [0, 600) and 0 of [77, 78).
"""

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_hard_cases as hc
import logistic_ref as ref

pytestmark = pytest.mark.gpu

COLS, ROWS, LIST = "dsgd_lg_cgrad_kernel", "dsgd_lg_grad_range_kernel", "dsgd_lg_grad_kernel"
RATIOS = {}   # (entry point, group) -> the largest error / bound seen


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f64bits(x):
    return np.float64(x).view(np.uint64)


def engine_of(case):
    eng = dsgd_amd.Engine(case.dim, case.lam)
    eng.load_csr(*case.csr)
    return eng


def within(entry, case, what, got, want, bound):
    ratio = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / bound))
    RATIOS[(entry, case.group)] = max(RATIOS.get((entry, case.group), 0.0), ratio)
    print("%s %s %s %s: max err/bound %.6f" % (entry, case.group, case.name, what, ratio))
    assert ratio <= 1.0, (entry, case.name, what, ratio)


def arange_lists(ranges):
    return [np.arange(a, b, dtype=np.int32) for a, b in ranges]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (entry, group), ratio in sorted(RATIOS.items()):
        print("\nlargest error / bound, %s, %s: %.6f" % (entry, group, ratio))


@pytest.fixture(scope="module", params=hc.BOUND_KEYS, ids=hc.BOUND_IDS)
def ctx(request):
    """one context per data set (and the second one of the column-list comparison)"""
    case = hc.bound_case(request.param)
    with engine_of(case) as eng, engine_of(case) as rows:
        yield case, eng, rows


# ---- against the reference, within the derived bounds ------------------------------------------------------------------
def test_gradient_and_step_within_dg_and_dw(ctx):
    case, eng, _ = ctx
    for name, idx in case.grad_lists.items():
        eng.set_weights(case.w)
        g, st = eng.lg_gradient(idx)
        assert st == {"n_samples": len(idx), "n_active": len(idx)} and eng.grad_kernel_name() == LIST
        within("lg_gradient", case, name, g, ref.gradient(case.csr, case.w, idx, case.lam), lb.dg(case.csr, case.w, idx, case.lam))
    assert np.array_equal(bits(eng.get_weights()), bits(case.w))
    lists, lr = case.step
    eng.lg_sync_step(lists, lr)
    within("lg_sync_step", case, "100/37/1", eng.get_weights(), ref.sync_step(case.csr, case.w, lists, lr, case.lam),
           lb.dw(case.csr, case.w, lists, lr, case.lam))


def test_evaluation_within_dloss_and_dc(ctx):
    case, eng, _ = ctx
    n = len(case.csr[3])
    eng.set_weights(case.w)
    dz = lb.dz(case.csr, case.w)
    p = eng.lg_predict_proba(np.arange(n))
    within("lg_predict_proba", case, "all rows", p, ref.proba(ref.dots(case.csr, case.w)), lb.dc(dz) + 2.0 ** -25)
    singles = []
    for a, b in case.evals:
        loss, acc = eng.lg_loss_acc(a, b)
        loss_ref, _, tallies, _ = ref.loss_acc(case.csr, case.w, a, b, case.lam)
        within("lg_loss_acc", case, "[%d, %d)" % (a, b), loss, loss_ref, lb.dloss(case.csr, case.w, a, b, case.lam))
        assert abs(acc * (b - a) - tallies[0]) <= hc.uncertain(case, a, b) + 1e-9, (a, b, acc * (b - a), tallies)
        singles.append((loss, acc))
    many = eng.lg_loss_acc_ranges(case.evals)
    assert [(f64bits(l), a) for l, a in many] == [(f64bits(l), a) for l, a in singles]


def test_ranges_and_column_lists_within_dw_and_the_bits_of_lists(ctx):
    case, eng, _ = ctx
    lr = case.lr_ranges
    for name, ranges in case.range_sets.items():
        lists = arange_lists(ranges)
        want = ref.sync_step(case.csr, case.w, lists, lr, case.lam)
        bound = lb.dw(case.csr, case.w, lists, lr, case.lam)
        n = sum(b - a for a, b in ranges)
        eng.set_weights(case.w)
        assert eng.lg_sync_step_ranges(ranges, lr) == {"n_samples": n, "n_active": n} and eng.grad_kernel_name() == ROWS
        w_ranges = eng.get_weights()
        within("lg_sync_step_ranges", case, name, w_ranges, want, bound)
        eng.set_weights(case.w)
        eng.lg_sync_step(lists, lr)
        assert eng.grad_kernel_name() == LIST and np.array_equal(bits(eng.get_weights()), bits(w_ranges)), name
        eng.set_weights(case.w)
        assert eng.lg_sync_steps_ranges(ranges, 1, lr) == {"n_samples": n, "n_active": n} and eng.grad_kernel_name() == COLS
        w_cols = eng.get_weights()
        within("lg_sync_steps_ranges", case, name, w_cols, want, bound)
        assert np.array_equal(bits(w_cols), bits(w_ranges)), name


# ---- against each other, bit for bit -----------------------------------------------------------------------------------
def test_three_column_list_steps_are_three_row_form_steps(ctx):
    case, cols, rows = ctx
    n = len(case.csr[3])
    for name, ranges in case.range_sets.items():
        cols.set_weights(case.w)
        rows.set_weights(case.w)
        cols.lg_sync_steps_ranges(ranges, 3, case.lr_ranges)
        assert cols.grad_kernel_name() == COLS
        for _ in range(3):
            rows.lg_sync_step_ranges(ranges, case.lr_ranges)
        assert rows.grad_kernel_name() == ROWS
        w_cols, w_rows = cols.get_weights(), rows.get_weights()
        assert np.isfinite(w_cols).all() and np.array_equal(bits(w_cols), bits(w_rows)), name
        got, want = cols.lg_loss_acc(0, n), rows.lg_loss_acc(0, n)   # the |w'|^2 words the last finish left
        assert f64bits(got[0]) == f64bits(want[0]) and got[1] == want[1], name


def test_a_three_step_plan_is_lg_sync_steps(ctx):
    case, eng, _ = ctx
    lists, lr = case.step
    plan = eng.lg_plan([lists] * 3)
    try:
        eng.set_weights(case.w)
        eng.plan_run(plan, 0, 3, lr)
        assert eng.synchronize()["n_samples"] == 3 * sum(len(a) for a in lists)
        w_plan = eng.get_weights()
    finally:
        plan.destroy()
    eng.set_weights(case.w)
    eng.lg_sync_steps(np.concatenate(lists * 3), np.concatenate([[0], np.cumsum([len(a) for a in lists] * 3)]), 3, len(lists), lr)
    assert eng.grad_kernel_name() == LIST
    assert np.isfinite(w_plan).all() and np.array_equal(bits(eng.get_weights()), bits(w_plan))


# ---- the width edges, by name ------------------------------------------------------------------------------------------
# logistic_hard_cases.W_EDGE_RANKS: the LDS head's last word (rank 2,047) and the first column beyond it (2,048); the last column of
# the finish's first workgroup (255) and the only one of its second (256).  The row of every key gives each of them data.
@pytest.mark.parametrize("dim", hc.W_DIMS)
def test_width_edges(dim):
    case = hc.width(dim)
    row_ptr, col, val, _ = case.csr
    n, dp = len(row_ptr) - 1, case.dim + 1
    everything = np.arange(n, dtype=np.int32)
    w64 = case.w.astype(np.float64)
    lr = 2.0 ** -6

    def reg_only(j):
        """float32(w - lr 2 lambda w): the fp64 expression, rounded once"""
        return (w64[j] - lr * ((2.0 * case.lam) * w64[j])).astype(np.float32)

    with engine_of(case) as eng:
        ranks = eng.column_ranks()
        assert np.array_equal(ranks, lb.ranks_of(case.csr, dp))
        eng.set_weights(case.w)
        g, _ = eng.lg_gradient(everything)
        bound = lb.dg(case.csr, case.w, everything, case.lam)
        within("lg_gradient", case, "the whole set", g, ref.gradient(case.csr, case.w, everything, case.lam), bound)
        data = ref.data_sum(case.csr, w64, everything)[0]
        count = np.bincount(col, minlength=dp)
        for r in hc.W_EDGE_RANKS.get(dim, []):
            key = int(np.where(ranks == r)[0][0])
            # the premise: the column has an entry, and its DATA sum is far above the bound -- a sum that were dropped, folded
            # into a neighbour or never flushed leaves dg; then the two plain statements of the same
            assert count[key] > 0 and abs(data[key]) > 4.0 * bound[key], (r, key)
            assert g[key] != 0.0 and g[key] != np.float32((2.0 * case.lam) * w64[key]), (r, key)
        if dim in (1, 15):
            rows = [int(np.argmax(np.diff(row_ptr) == 0)), int(np.argmax(np.diff(row_ptr) == 1)), int(np.argmax(np.diff(row_ptr) == dp))]
            steps = [("lists", [np.array([r], dtype=np.int32)]) for r in rows] + [("lists", [everything])]
        elif dim == 300000:
            steps = [("lists", [everything]), ("ranges", [(0, n)]), ("cols", [(0, n)])]
        else:   # (one ordinary row: the whole set leaves no column without an entry where the row of every key is)
            steps = [("lists", [everything]), ("lists", [np.array([0], dtype=np.int32)])]
        none_seen = 0
        for form, arg in steps:
            eng.set_weights(case.w)
            if form == "lists":
                eng.lg_sync_step(arg, lr)
                used = np.concatenate([col[row_ptr[r]:row_ptr[r + 1]] for r in arg[0]] + [np.zeros(0, np.int32)])
            else:
                eng.lg_sync_step_ranges(arg, lr) if form == "ranges" else eng.lg_sync_steps_ranges(arg, 1, lr)
                used = col[row_ptr[arg[0][0]]:row_ptr[arg[0][1]]]
            w1 = eng.get_weights()
            has = np.bincount(used, minlength=dp) > 0
            assert np.all(bits(w1[has]) != bits(case.w[has])), form                       # a step changes every column that has an entry
            assert np.array_equal(bits(w1[~has]), bits(reg_only(np.where(~has)[0]))), form   # ... and lambda alone moves the others
            none_seen = max(none_seen, int(np.count_nonzero(~has)))
            if dim == 300000:
                assert np.count_nonzero(~has) > 280000
        assert none_seen >= 1   # (the second check is not an empty one at any width)


# ---- full scale, exactly -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", hc.EXACT_KEYS, ids=hc.EXACT_IDS)
def test_full_scale_sums_are_exact(key):
    case = hc.exact_case(*key)
    ex, n, lr = case.expect, case.n, case.lr
    w1, w2 = ex.whole

    def after(eng, what, want):
        """the weights' bits, a finite loss within dloss on them, and the accumulators left clean: one row's own entries"""
        got = eng.get_weights()
        assert np.array_equal(bits(got), bits(want)), (what, int(np.count_nonzero(bits(got) != bits(want))))
        loss, _ = eng.lg_loss_acc(0, n)
        assert np.isfinite(loss)
        within("lg_loss_acc", case, what, loss, ref.loss_acc(case.csr, want, 0, n, 0.0)[0], lb.dloss(case.csr, want, 0, n, 0.0))
        row, g_row = ex.one_row   # (-y x on the row's columns and +0.0 elsewhere, whatever the saturated weights: float32 BITS)
        g, _ = eng.lg_gradient(np.array([row], dtype=np.int32))
        assert np.array_equal(bits(g), bits(g_row)) and np.count_nonzero(g) == case.csr[0][row + 1] - case.csr[0][row], what
        assert np.array_equal(bits(eng.get_weights()), bits(want)), what   # (a gradient changes no weight: the next step starts here)

    with engine_of(case) as eng, engine_of(case) as second:
        for name, (idx, want) in ex.gradient.items():
            eng.set_weights(case.w)
            g, _ = eng.lg_gradient(idx)
            assert np.array_equal(bits(g), bits(want)), (name, int(np.count_nonzero(bits(g) != bits(want))))
            if case.labels == "alt" and len(idx) % 2 == 0 and name == "all":   # F cancels: +0.0
                assert g[hc.E_F] == 0.0 and not np.signbit(g[hc.E_F])
        for name, (lists, want) in ex.step.items():
            eng.set_weights(case.w)
            eng.lg_sync_step(lists, lr)
            after(eng, "lg_sync_step " + name, want)
        eng.set_weights(case.w)
        eng.lg_sync_step_ranges([(0, n)], lr)
        assert eng.grad_kernel_name() == ROWS
        after(eng, "lg_sync_step_ranges", w1)
        eng.lg_sync_step_ranges([(0, n)], lr)   # the second step, from the first one's weights
        after(eng, "lg_sync_step_ranges twice", w2)
        for n_steps, want in ((1, w1), (2, w2)):
            second.set_weights(case.w)
            second.lg_sync_steps_ranges([(0, n)], n_steps, lr)
            assert second.grad_kernel_name() == COLS
            after(second, "lg_sync_steps_ranges x %d" % n_steps, want)
        if case.labels == "alt" and n % 2 == 0:
            assert w1[hc.E_F] == 0.0 and w2[hc.E_F] == 0.0 and not np.signbit(second.get_weights()[hc.E_F])
