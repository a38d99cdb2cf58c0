"""tests/logistic_bound.py is worth something on the HARD inputs too (CPU; tests/test_logistic_bound.py shows it for the synthetic
ones): for every hostile-values case and every width case of tests/logistic_hard_cases.py -- exactly what
tests/test_gpu_logistic_hard.py steps -- the honest fp32 emulation stays inside dw and dg, every existing mutation that applies
leaves them, and so do four new ones, the mistakes these inputs are there to catch:

  vexp_qscale        vexp one too large in qscale = 2^(S - vexp) ONLY
  vexp_finish        vexp one too large in the finish ONLY
  skip_last_column   the last column of the finish's ragged last workgroup is not written: rank dp - 1 of a step keeps its
                     weight, key dp - 1 of a gradient stays 0
  fold_2048          the first rank beyond the LDS head (2,048) is added to the head's last word (2,047)

A mutation "applies" where it changes anything at all (a forgotten 1/K needs K > 1, the regulariser on the support only needs a
weighted column without an entry, ...): `applies` below states each rule, from the data alone.  NAMED says on which case of each
group every new mutation must leave the bound; the test prints every case on which it does.

skip_last_column and the hostile group: the traits share hard_data.base_weights' support of 3,000 non-zero weights in 47,237,
and the column of rank dp - 1 of every window (key 47,234: no entry) has weight 0: a STEP that does not write it leaves the right
value, so no hostile step can show that mistake (asserted: it applies to none).  Key dp - 1 = 47,236 has entries in every window:
the GRADIENT of the 2,049-row list shows it, and is the named hostile case.  The width cases' weights are dense: every step of
every width shows it.

The exact cases' expectations are computed and held against the fp64 reference where they are built
(logistic_hard_cases.exact_case); test_exact_cases_are_exact builds every one and checks the scale they reach.
"""

import functools

import numpy as np
import pytest

import logistic_bound as lb
import logistic_hard_cases as hc
import logistic_ref as ref
from test_logistic_bound import MUTATIONS

NEW_MUTATIONS = ["vexp_qscale", "vexp_finish", "skip_last_column", "fold_2048"]
GRADIENT_MUTATIONS = ["drop_last", "label_by_position", "flip_sign", "vexp_qscale", "vexp_finish", "skip_last_column", "fold_2048"]
# new mutation -> group -> the (case, "step" or "gradient", its name) on which it must leave the bound.  fold_2048 is held to
# the model of EXACTLY one column more than the LDS head (dim 2,048, where the row of every key gives rank 2,048 its data), in
# every form that reaches that row, beside the wide one.
NAMED = {
    "vexp_qscale": {"hostile": [("scaled_m30", "step", "3 workers 100/37/1")], "width": [("dim 1", "step", "3 workers 100/37/1")]},
    "vexp_finish": {"hostile": [("scaled_p10", "step", "3 workers 100/37/1")], "width": [("dim 256", "step", "ranges k16 x 37")]},
    "skip_last_column": {"hostile": [("signed", "gradient", "2049 (row twice)")], "width": [("dim 256", "step", "3 workers 100/37/1")]},
    "fold_2048": {"hostile": [("wide", "step", "ranges 1500/547/1")],
                  "width": [("dim 2048", "step", "3 workers 100/37/1"), ("dim 2048", "step", "ranges 300/299/1"), ("dim 2048", "step", "ranges k16 x 37"),
                            ("dim 2048", "gradient", "600 (the whole set)"), ("dim 300000", "step", "ranges 300/299/1")]},
}
# One step's bound is float precision, not a licence: max(bound) < FLOAT_PRECISION * max |want| on every step case.  No hostile
# trait needs a ratio of its own: the largest of all cases is printed by test_uncertain_rows_and_float_precision.
FLOAT_PRECISION = 1e-5



def applies(mut, case, lists, form="step"):
    row_ptr, col, val, label = lb._csr(case.csr)
    nnz = np.diff(row_ptr)
    dp = case.dim + 1
    if mut == "drop_last":
        return any(nnz[a[-1]] > 0 for a in lists)
    if mut == "label_by_position":
        return any(nnz[r] > 0 and label[t % len(label)] != label[r] for a in lists for t, r in enumerate(a))
    if mut in ("flip_sign", "vexp_qscale", "vexp_finish"):
        return any(nnz[a].sum() > 0 for a in lists)
    if mut == "no_mean":
        return len(lists) > 1
    if mut == "wrong_worker_shift":
        return len({lb.shift(len(a)) for a in lists}) > 1
    touched = [np.bincount(np.concatenate([col[row_ptr[r]:row_ptr[r + 1]] for r in a] + [np.zeros(0, np.int64)]), minlength=dp) > 0 for a in lists]
    if mut == "support_only_reg":
        return case.lam > 0 and any(np.any((case.w != 0) & ~t) for t in touched)
    rank = lb.ranks_of(case.csr, dp)
    if mut == "skip_last_column":   # the column has a weight (the regulariser moves it) or an entry
        last = int(np.where(rank == dp - 1)[0][0]) if form == "step" else dp - 1
        return bool(case.w[last] != 0 or any(t[last] for t in touched))
    if mut == "fold_2048":
        return dp > 2048 and any(t[int(np.where(rank == 2048)[0][0])] for t in touched)
    raise ValueError(mut)


def all_dots(case):
    """the emulated fp32 dot of every row, once per case (no mutation touches it)"""
    if not hasattr(case, "_emu_d"):
        case._emu_d = lb.emu_dots(case.csr, case.w, np.arange(len(case.csr[3])))
    return case._emu_d


def step_of(case, name, mut=None):
    """(error / bound of the emulated step, whether the mutation applies)"""
    lists, lr = hc.step_cases(case)[name]
    want = ref.sync_step(case.csr, case.w, lists, lr, case.lam)
    got = lb.emu_step(case.csr, case.w, lists, lr, case.lam, mut, d=all_dots(case)).astype(np.float64)
    return np.abs(got - want) / lb.dw(case.csr, case.w, lists, lr, case.lam), mut is None or applies(mut, case, lists)


def gradient_of(case, name, mut=None):
    idx = case.grad_lists[name]
    want = ref.gradient(case.csr, case.w, idx, case.lam)
    got = lb.emu_gradient(case.csr, case.w, idx, case.lam, mut, d=all_dots(case)).astype(np.float64)
    return np.abs(got - want) / lb.dg(case.csr, case.w, idx, case.lam), mut is None or applies(mut, case, [idx], "gradient")


@functools.lru_cache(maxsize=None)
def survey(key):
    """One case, everything emulated once: (honest, mutated) -- honest: [(form, name, largest error / bound)]; mutated: [(mutation,
    form, name, whether it left the bound)] for every mutation that applies.  Cached: the tests below assert on it and
    test_new_mutations_leave_the_bound_on_the_named_cases reports from it, whichever of them runs, alone or in any order."""
    case = hc.bound_case(key)
    honest, mutated = [], []
    for name, (lists, _) in hc.step_cases(case).items():
        honest.append(("step", name, float(np.max(step_of(case, name)[0]))))
        for mut in MUTATIONS + NEW_MUTATIONS:
            if applies(mut, case, lists):
                mutated.append((mut, "step", name, bool(np.max(step_of(case, name, mut)[0]) > 1.0)))
    for name, idx in case.grad_lists.items():
        honest.append(("gradient", name, float(np.max(gradient_of(case, name)[0]))))
        for mut in GRADIENT_MUTATIONS:
            if applies(mut, case, [idx], "gradient"):
                mutated.append((mut, "gradient", name, bool(np.max(gradient_of(case, name, mut)[0]) > 1.0)))
    return honest, mutated


@pytest.mark.parametrize("key", hc.BOUND_KEYS, ids=hc.BOUND_IDS)
def test_emulation_inside_and_existing_mutations_outside(key):
    honest, mutated = survey(key)
    for form, name, ratio in honest:
        assert ratio <= 1.0, (form, name, ratio)
    assert len(honest) == len(hc.step_cases(hc.bound_case(key))) + len(hc.bound_case(key).grad_lists)
    for mut, form, name, out in mutated:
        if mut in MUTATIONS:
            assert out, (mut, form, name)
    assert {m for m, _, _, _ in mutated} >= {"drop_last", "flip_sign", "no_mean", "vexp_qscale", "vexp_finish"}   # (these apply everywhere)


def test_new_mutations_leave_the_bound_on_the_named_cases():
    surveys = {key: survey(key) for key in hc.BOUND_KEYS}
    for mut, groups in NAMED.items():
        for group, named in groups.items():
            seen = [(hc.bound_case(key).name, form, name) for key, (_, mutated) in surveys.items() if key[0] == group
                    for m, form, name, out in mutated if m == mut and out]
            for case_name, form, name in named:
                assert (case_name, form, name) in seen, (mut, group, case_name, form, name)
                print("%-17s %-8s leaves the bound on %s / %s %s" % (mut, group, case_name, form, name))
            print("    and on every one of: %s" % (seen,))
    for key in hc.BOUND_KEYS:   # the one blind spot, stated in the docstring
        if key[0] == "hostile":
            assert not any(applies("skip_last_column", hc.bound_case(key), lists) for lists, _ in hc.step_cases(hc.bound_case(key)).values()), key
    for group in ("hostile", "width"):
        for form in ("step", "gradient"):
            worst = max((ratio, hc.bound_case(key).name, name) for key, (honest, _) in surveys.items() if key[0] == group
                        for f, name, ratio in honest if f == form)
            print("honest emulation, %s, %s: largest error / bound %.6f (%s, %s)" % (form, group, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("key", hc.BOUND_KEYS, ids=hc.BOUND_IDS)
def test_uncertain_rows_and_float_precision(key):
    case = hc.bound_case(key)
    n_rows = len(case.csr[3])
    for a, b in case.evals + [(0, n_rows)]:
        unsure = hc.uncertain(case, a, b)
        print("%s %s [%d, %d): %d uncertain rows" % (case.group, case.name, a, b, unsure))
        assert unsure <= 0.01 * (b - a)
    for name, (lists, lr) in hc.step_cases(case).items():
        want = ref.sync_step(case.csr, case.w, lists, lr, case.lam)
        bound = lb.dw(case.csr, case.w, lists, lr, case.lam)
        ratio = float(np.max(bound)) / float(np.max(np.abs(want)))
        print("%s %s %s: max bound / max |want| %.3e" % (case.group, case.name, name, ratio))
        assert ratio < FLOAT_PRECISION


@pytest.mark.parametrize("key", hc.EXACT_KEYS, ids=hc.EXACT_IDS)
def test_exact_cases_are_exact(key):
    """exact_case itself holds every expectation against the fp64 reference; here: the scale the sums reach"""
    case = hc.exact_case(*key)
    S = lb.shift(case.n)
    top = max(abs(int(v)) for v in case.expect.sums) << (S - lb.vexp_of(case.csr[2]))   # in units of 2^-23: Python integers
    assert top <= 2 ** 62 << hc.E_UNIT
    if case.n in (4096, 64) and case.vmax == 1.0 and case.labels == "plus":
        assert top == 2 ** 62 << hc.E_UNIT          # the accumulator's whole range
    if case.shape == "tall" and case.labels == "alt":
        assert (case.expect.sums[hc.E_F] == 0) == (case.n % 2 == 0)
    if "3 workers 4096/64/1" in case.expect.step:
        assert [lb.shift(len(a)) for a in case.expect.step["3 workers 4096/64/1"][0]] == [50, 56, 62]
    ranks = lb.ranks_of(case.csr, case.dim + 1)
    if case.shape == "broad":   # ranks 2,048 .. 2,099 take the global atomics, each with the full sum
        beyond = np.where((ranks >= 2048) & (ranks < hc.E_BROAD))[0]
        assert len(beyond) == hc.E_BROAD - 2048 and np.all(np.abs(case.expect.sums[beyond]) == np.abs(case.expect.sums[1]))


@pytest.mark.parametrize("dim", hc.W_FULL)
def test_edge_ranks_carry_data(dim):
    """the premise of the GPU module's edge checks: the columns on the LDS head's and the finish's edges have entries, and their
    data sums stand far above dg -- a sum dropped, folded or never flushed there cannot hide behind the regulariser"""
    case = hc.width(dim)
    everything = np.arange(hc.W_ROWS)
    ranks = lb.ranks_of(case.csr, dim + 1)
    data = ref.data_sum(case.csr, case.w, everything)[0]
    bound = lb.dg(case.csr, case.w, everything, case.lam)
    count = np.bincount(case.csr[1], minlength=dim + 1)
    for r in hc.W_EDGE_RANKS[dim]:
        key = int(np.where(ranks == r)[0][0])
        assert count[key] > 0 and abs(data[key]) > 4.0 * bound[key], (r, key, count[key], data[key], bound[key])
