"""tests/softmax_bound.py is worth something on the inputs tests/test_gpu_softmax_hard.py runs (CPU; the cases: tests/softmax_hard_cases.py).
For every hostile, width, small-class-count and tie case the honest emulation of the softmax step and of the evaluation stays inside
dw, dloss and dc + 2^-25, and these seeded mistakes -- the ones the inputs are there to catch -- leave the bound, or the exact
expectation:

  pad_in_S              the TP - C padding classes' zero logits join S            (applies where TP > C)
  drop_class_from_S     the last real class does not join S
  label_from_neighbour  [c == y] is taken from the lane's other class: y0 and y1 swapped
  highest_argmax        a tie gives the highest class, not the lowest            (applies where a range holds a tie: the hand-built
                        ones, and every EMPTY row -- all its logits are 0)
  loss_uses_pred        the loss takes z_pred where z_y belongs                   (applies where a row's predicted class is not its own)
  vexp_qscale, vexp_finish   vexp one too large where the entries are scaled / in the finish ONLY
  fold_head             the first rank beyond the gradient's LDS head is added to the head's last word, at 4096 / TP -- 32 ranks at
                        C = 128, 512 at C = 5 -- and not at the single model's 2,048  (applies where a list reaches that column)
  chain_skips           the evaluation drops each chain's second row              (the long case alone: test_long_evaluation)

A mutation of the STEP leaves dw on every step of every case where it applies (asserted); one of the EVALUATION need not -- scaled_m30's
loss is lambda |W|^2 of weights near 2^30, beside which dloss hides every row's loss -- so NAMED says on which cases each mutation must
show, and the test prints every case on which it does.  "Leaves" for an evaluation: the loss leaves dloss, a decided row's predicted
class differs from the reference's, or the correct count is off by more than the uncertain rows.

An UNCERTAIN row is one whose arg-max the reference does not decide (softmax_bound.decided); at most 1 % of every evaluated range may
be (printed per case and range).  The tie cases are held to their exact expectations instead: both sides compute +-40 exactly.

FLOAT_PRECISION: one step's bound is float precision and not a licence, max(bound) < 1e-5 max |want|, the single model's ratio.  One
trait has a ratio of its own.  On scaled_p10 the values are 2^10 times the base's and class 0's weights 2^-10 times: the step lr G
outweighs the weights it starts from by five orders of magnitude, so max |want| is the GRADIENT's size and the ratio is the gradient's
relative bound, dc_i = dz_i / 2 against coefficients of order 1 -- with dz_i = gamma(m_i + 4) sum_j |x_ij| |w_cj|, rows of up to 13
chunks and dense classes whose logits have standard deviation 2 (sum |x| |w| is several times that), dc_i reaches 2e-5.  4e-5 there.
"""

import functools

import numpy as np
import pytest

import logistic_bound as lb
import softmax_bound as sm
import softmax_hard_cases as hc

H3, HR, W3, WR3, WR16 = "3 workers 100/37/1", "ranges 1500/547/1", "3 workers 100/37/1", "ranges 300/299/1", "ranges k16 x 37"
TIE_STEP = "all rows, row 2 twice"
# mutation -> the (case key, "step" or "eval", its name) on which it must leave the bound or the exact expectation
NAMED = {
    "pad_in_S": [(("hostile", "wide", 103), "step", H3), (("hostile", "signed", 33), "step", HR), (("hostile", "scaled_p10", 5), "eval", "[0, 2048)"),
                 (("width", 512, 5), "step", W3), (("small", 3), "step", "K=3")],
    "drop_class_from_S": [(("hostile", "signed", 33), "step", HR), (("hostile", "ragged64", 103), "eval", "[0, 2048)"), (("width", 64, 128), "eval", "[0, 600)"),
                          (("small", 4), "step", "K=1"), (("small", 32), "step", "K=3"), (("small", 64), "step", "K=3"), (("ties", 32), "step", TIE_STEP)],
    "label_from_neighbour": [(("hostile", "ragged64", 103), "step", H3), (("hostile", "scaled_m30", 33), "step", HR), (("width", 1, 128), "step", W3),
                             (("small", 32), "step", "K=1"), (("small", 64), "step", "K=1"), (("ties", 64), "step", TIE_STEP)],
    "highest_argmax": [(("ties", 128), "eval", "[0, 11)"), (("ties", 64), "eval", "[1, 2)"), (("ties", 32), "eval", "[7, 8)"),
                       (("hostile", "ragged64", 5), "eval", "[0, 2048)"), (("width", 30, 128), "eval", "[0, 600)")],
    "loss_uses_pred": [(("hostile", "wide", 103), "eval", "[0, 2048)"), (("width", 63, 128), "eval", "[0, 600)"), (("small", 64), "eval", "[150, 250)"),
                       (("ties", 32), "eval", "[1, 2)")],
    "vexp_qscale": [(("hostile", "scaled_m30", 33), "step", H3), (("width", 1, 128), "step", W3)],
    "vexp_finish": [(("hostile", "scaled_p10", 5), "step", H3), (("width", 256, 5), "step", WR16)],
    "fold_head": [(("width", 32, 128), "step", W3), (("width", 32, 128), "step", WR3), (("width", 32, 128), "step", WR16), (("width", 512, 5), "step", W3),
                  (("width", 512, 5), "step", WR3), (("width", 512, 5), "step", WR16), (("hostile", "wide", 103), "step", HR), (("small", 64), "step", "K=3")],
}
FLOAT_PRECISION = 1e-5
OWN_PRECISION = {"scaled_p10": 4e-5}   # (the docstring's reason)


def emu_logits(case):
    if not hasattr(case, "_emu_Z"):
        case._emu_Z = sm.emu_logits(case.csr, case.W)
    return case._emu_Z


def applies(mut, case, form, name):
    row_ptr, col, _, _ = lb._csr(case.csr)
    C, dp = case.C, case.dim + 1
    if mut == "pad_in_S":
        return sm.tp_of(C) > C
    if mut == "drop_class_from_S":
        return True
    if form == "step":
        lists = hc.step_cases(case)[name][0]
        if mut in ("label_from_neighbour", "vexp_qscale", "vexp_finish"):
            return any(np.diff(row_ptr)[a].sum() > 0 for a in lists)
        if mut == "fold_head":
            if dp <= sm.hot_of(C):
                return False
            key = int(np.where(lb.ranks_of(case.csr, dp) == sm.hot_of(C))[0][0])
            return any(key in col[row_ptr[r]:row_ptr[r + 1]] for a in lists for r in a)
    else:
        a, b = eval_range(name)
        Z32 = emu_logits(case)[a:b]
        if mut == "highest_argmax":
            return bool(np.any(np.count_nonzero(Z32 == Z32.max(axis=1, keepdims=True), axis=1) > 1))
        if mut == "loss_uses_pred":
            return bool(np.any(np.argmax(Z32, axis=1) != case.cls[a:b]))
    raise ValueError((mut, form))


def eval_name(a, b):
    return "[%d, %d)" % (a, b)


def eval_range(name):
    a, b = name[1:-1].split(", ")
    return int(a), int(b)


def step_of(case, name, mut=None):
    """error / bound of the emulated step"""
    lists, lr = hc.step_cases(case)[name]
    want, bound = hc.step_reference(case, name)
    got = sm.emu_step(case.csr, case.W, case.cls, lists, lr, case.lam, mut, emu_logits(case)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - want) / bound
    return float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))


def eval_of(case, a, b, mut=None):
    """(loss error / dloss, whether the evaluation left its bound or an exact expectation)"""
    want, bound = hc.eval_reference(case, a, b)
    Z32 = emu_logits(case)
    loss, correct = sm.emu_loss_acc(case.W, case.cls, a, b, case.lam, Z32, mut)
    pred = sm.emu_eval(Z32[a:b], case.cls[a:b], mut)[1]
    expect, compared = hc.expected_classes(case, a, b)
    correct_ref = int(np.count_nonzero(expect == case.cls[a:b]))
    ratio = abs(loss - want) / bound if np.isfinite(loss) else np.inf
    out = ratio > 1.0 or bool(np.any(pred[compared] != expect[compared])) or abs(correct - correct_ref) > int(np.count_nonzero(~compared))
    return float(ratio), out


@functools.lru_cache(maxsize=None)
def survey(key):
    """One case, everything emulated once: (honest, mutated) -- honest: [(form, name, largest error / bound, left an exact expectation)];
    mutated: [(mutation, form, name, whether it left)] for every mutation that applies.  Cached: whichever test runs first builds it."""
    case = hc.bound_case(key)
    honest, mutated = [], []
    for name in hc.step_cases(case):
        honest.append(("step", name, step_of(case, name), False))
        for mut in sm.STEP_MUTATIONS:
            if applies(mut, case, "step", name):
                mutated.append((mut, "step", name, step_of(case, name, mut) > 1.0))
    for a, b in case.evals:
        name = eval_name(a, b)
        honest.append(("eval", name) + eval_of(case, a, b))
        for mut in sm.EVAL_MUTATIONS:
            if applies(mut, case, "eval", name):
                mutated.append((mut, "eval", name, eval_of(case, a, b, mut)[1]))
    Z, dzm = hc.reference(case)
    p = sm.emu_rows(emu_logits(case))[0].astype(np.float32).astype(np.float64)
    honest.append(("proba", "all rows", float(np.max(np.abs(p - sm.probs(Z)[0]) / (sm.dc(dzm, case.C) + 2.0 ** -25)[:, None])), False))
    return honest, mutated


@pytest.mark.parametrize("key", hc.BOUND_KEYS, ids=hc.BOUND_IDS)
def test_emulation_inside_and_step_mutations_outside(key):
    honest, mutated = survey(key)
    case = hc.bound_case(key)
    for form, name, ratio, out in honest:
        assert ratio <= 1.0 and not out, (form, name, ratio, out)
    assert len(honest) == len(hc.step_cases(case)) + len(case.evals) + 1
    for mut, form, name, out in mutated:
        if form == "step":
            assert out, (mut, name)
    assert {m for m, f, _, _ in mutated if f == "step"} >= {"drop_class_from_S", "label_from_neighbour", "vexp_qscale", "vexp_finish"}   # (these apply everywhere)


def test_mutations_leave_on_the_named_cases():
    surveys = {key: survey(key) for key in hc.BOUND_KEYS}
    for mut, named in NAMED.items():
        seen = [(key, form, name) for key, (_, mutated) in surveys.items() for m, form, name, out in mutated if m == mut and out]
        for entry in named:
            assert entry in seen, (mut, entry)
            print("%-20s leaves on %s / %s %s" % (mut, "-".join(str(x) for x in entry[0]), entry[1], entry[2]))
        print("    and on %d more (case, form, name)" % (len(seen) - len(named)))
    for group in ("hostile", "width", "small", "ties"):
        for form in ("step", "eval", "proba"):
            worst = max((ratio, hc.bound_case(key).name, name) for key, (honest, _) in surveys.items() if key[0] == group for f, name, ratio, _ in honest if f == form)
            print("honest emulation, %s, %s: largest error / bound %.6f (%s, %s)" % (form, group, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("key", hc.BOUND_KEYS, ids=hc.BOUND_IDS)
def test_uncertain_rows_and_float_precision(key):
    case = hc.bound_case(key)
    if case.group != "ties":   # (a tie is undecided by construction: those cases are held to their exact expectations)
        for a, b in case.evals:
            unsure = hc.uncertain(case, a, b)
            print("%s %s [%d, %d): %d uncertain rows" % (case.group, case.name, a, b, unsure))
            assert unsure <= 0.01 * (b - a)
    for name in hc.step_cases(case):
        want, bound = hc.step_reference(case, name)
        ratio = float(np.max(bound)) / float(np.max(np.abs(want)))
        print("%s %s %s: max bound / max |want| %.3e" % (case.group, case.name, name, ratio))
        assert ratio < (OWN_PRECISION.get(key[1], FLOAT_PRECISION) if key[0] == "hostile" else FLOAT_PRECISION)
        assert np.all(np.abs(want.astype(np.float32).astype(np.float64) - want) <= bound)   # (the reference, rounded to float, keeps its bound)


def test_ragged64_uncertain_rows_are_its_empty_rows():
    """under the plain gap rule top1 - top2 > 2 dz_max the window's uncertain rows are exactly its EMPTY rows (dz_max == 0 and every
    logit exactly 0: class 0 on both sides), which `decided` therefore compares; the rows with a 1e-25 entry are decided"""
    case = hc.hostile("ragged64", 5)
    Z, dzm = hc.reference(case)
    top = np.sort(Z, axis=1)
    plain = ~(top[:, -1] - top[:, -2] > 2.0 * dzm)
    empty = np.diff(case.csr[0]) == 0
    print("ragged64: %d rows fail the plain gap rule, %d rows are empty" % (np.count_nonzero(plain), np.count_nonzero(empty)))
    assert np.array_equal(plain, empty) and np.count_nonzero(empty) > 100 and np.all(Z[empty] == 0.0) and np.all(dzm[empty] == 0.0)
    assert np.all(emu_logits(case)[empty] == 0.0) and hc.uncertain(case, 0, len(empty)) == 0


def test_emu_logits_are_emu_dots_per_class():
    """softmax_bound.emu_logits takes all classes of a row at once; per class it is logistic_bound.emu_dots, in bits"""
    case = hc.hostile("ragged64", 5)
    nnz = np.diff(case.csr[0])
    rows = np.unique(np.concatenate([np.arange(64), np.argsort(nnz)[-3:]]))   # (the window's longest rows among them)
    assert nnz[rows].max() > 4 * 64 and nnz[rows].min() == 0                  # far beyond the four chunks kept in registers; an empty row
    Z32 = emu_logits(case)
    for c in (0, 1, case.C - 1):
        d = lb.emu_dots(case.csr, case.W[c], rows)
        assert all(np.float32(d[int(r)]).view(np.uint32) == Z32[r, c].view(np.uint32) for r in rows), c


@pytest.mark.parametrize("C", hc.T_CS)
def test_ties_are_exact(C):
    case = hc.ties(C)
    Z, dzm = hc.reference(case)
    Z32 = emu_logits(case)
    assert np.array_equal(Z32.astype(np.float64), Z) and np.all(Z[0] == 0.0) and np.all(np.abs(Z[1:]) == 40.0)
    li, pred = sm.emu_eval(Z32, case.cls)
    for r, (tied, y, want) in enumerate(case.rows):
        assert sorted(np.nonzero(Z[r] == Z[r].max())[0].tolist()) == sorted(tied) and pred[r] == want == min(tied), r
    assert [int(p == y) for p, y in zip(pred, case.cls)] == [1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1]
    for r in (7, 8):   # the tie of {0, C - 1}: S is 2 + (C - 2) exp(-80) = 2 in fp64, the loss log 2 whichever of the two the row's class is
        assert abs(li[r] - np.log(2.0)) <= 1e-15   # (log(S) - (z_y - m), the kernel's order: the reference's (log S + m) - z_y rounds at 40)
    assert len(case.predict) >= 8 and all({int(p) % 4 for p in np.nonzero(case.predict == r)[0]} == {0, 1, 2, 3} for r in range(len(case.rows)))


@pytest.mark.parametrize("key", hc.EXACT_KEYS, ids=hc.EXACT_IDS)
def test_exact_cases_are_exact(key):
    """exact_case itself holds every expectation against the fp64 reference; here: the scale the sums reach"""
    case = hc.exact_case(*key)
    S = lb.shift(case.n)
    top = max(abs(int(v)) for v in case.expect.sums) << (S - lb.vexp_of(case.csr[2]))   # in units of 2^-23: Python integers
    assert top <= 2 ** 62 << hc.lhc.E_UNIT
    if case.n in (4096, 64) and case.vmax == 1.0 and case.labels == "zero":
        assert top == 2 ** 62 << hc.lhc.E_UNIT          # the accumulator's whole range: class 0's word at -2^62, class 1's at +2^62
        assert int(case.expect.sums[hc.lhc.E_F if case.shape == "tall" else 1]) < 0
    if case.shape == "tall" and case.labels == "alt":
        assert (case.expect.sums[hc.lhc.E_F] == 0) == (case.n % 2 == 0)
    if "3 workers 4096/64/1" in case.expect.step:
        assert [lb.shift(len(a)) for a in case.expect.step["3 workers 4096/64/1"][0]] == [50, 56, 62]
    W1 = case.expect.whole[0]
    assert np.array_equal(W1[2:], case.W[2:]) and np.array_equal(W1[1] - case.W[1], -(W1[0] - case.W[0]))   # classes >= 2 stay; class 1 mirrors class 0
    if case.shape == "broad":   # the ranks beyond the LDS head take the global atomics, each with the full sum
        ranks = lb.ranks_of(case.csr, case.dim + 1)
        beyond = np.where((ranks >= sm.hot_of(case.C)) & (ranks < hc.lhc.E_BROAD))[0]
        assert len(beyond) == hc.lhc.E_BROAD - sm.hot_of(case.C) and np.all(np.abs(case.expect.sums[beyond]) == np.abs(case.expect.sums[1]))


@pytest.mark.parametrize("dim, C", sorted((d, C) for C, d in hc.W_EDGE_RANKS))
def test_edge_ranks_carry_data(dim, C):
    """the premise of the GPU module's edge checks: every class's data sum on the columns on the LDS head's, the finish's and the
    evaluation tile's edges stands more than 4 bounds from zero in the step over the whole set -- a sum dropped, folded or never
    flushed there cannot hide behind the regulariser"""
    case = hc.width(dim, C)
    everything = [np.arange(hc.lhc.W_ROWS, dtype=np.int32)]
    ranks = lb.ranks_of(case.csr, dim + 1)
    moved = hc.W_LR_WHOLE * np.abs(sm.data_sums(case.csr, case.W, case.cls, everything[0]))
    bound = sm.dw(case.csr, case.W, case.cls, everything, hc.W_LR_WHOLE, case.lam)
    count = np.bincount(case.csr[1], minlength=dim + 1)
    for r in hc.W_EDGE_RANKS[(C, dim)]:
        key = int(np.where(ranks == r)[0][0])
        assert count[key] > 0 and np.all(moved[:, key] > 4.0 * bound[:, key]), (r, key, count[key], float(np.min(moved[:, key] / bound[:, key])))


@pytest.mark.parametrize("C", hc.L_CS)
def test_long_evaluation(C):
    """the long case can see the mistake it is there for: on 256 compute units the three long ranges give chains a second and a third
    row, [10000, 18193) exactly ONE second row; dropping the chains' second rows leaves dloss on each; at most 1 % uncertain rows"""
    case = hc.long_case(C)
    Z, dzm = hc.reference(case)
    for a, b in case.evals:
        unsure = hc.uncertain(case, a, b)
        print("long %s [%d, %d): %d uncertain rows" % (case.name, a, b, unsure))
        assert unsure <= 0.01 * (b - a)
        chains, passes = sm.chain_rows(b - a, hc.L_N_CU)
        want, bound = hc.eval_reference(case, a, b)
        skipped = sm.loss_chain_skips(case.csr, case.W, case.cls, a, b, case.lam, hc.L_N_CU, Z)
        if (a, b) in hc.L_LONG:
            assert b - a > 32 * hc.L_N_CU and chains == 32 * hc.L_N_CU and passes.max() == (b - a - 1) // chains >= 1
            assert abs(skipped - want) > bound, (a, b, skipped, want, bound)
            print("long %s [%d, %d): chain_skips moves the loss by %.3e, dloss %.3e; %d second rows" % (case.name, a, b, abs(skipped - want), bound, np.count_nonzero(passes == 1)))
        else:
            assert passes.max() == 0 and skipped == want   # (one row per chain: the mutation does not apply)
    assert np.count_nonzero(sm.chain_rows(8193, hc.L_N_CU)[1] == 1) == 1 and (10000, 18193) in hc.L_LONG
    assert sm.chain_rows(20000, hc.L_N_CU)[1].max() == 2 and 20000 % (32 * hc.L_N_CU) != 0   # three rows on some chains, a ragged last pass
