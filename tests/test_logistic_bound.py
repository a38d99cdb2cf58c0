"""tests/logistic_bound.py is worth something (CPU): for every list the GPU tests step, an honest fp32 emulation of the kernels
(the same lane assignment, the same sum order, the fp64 coefficient, the integer grid, the finish) stays inside the derived
bound, and each of six plausible mistakes leaves it.

The mistakes: a dropped last list position; the label taken by list position instead of by row; the residual's sign flipped;
a forgotten 1/K; the regulariser on the gradient's support only (the SVM's habit); S computed from the wrong worker's n.  On
the one-worker list the forgotten 1/K and the wrong worker's n change nothing (K = 1): they are asserted on the three-worker
step, the other four on both.
"""

import numpy as np
import pytest

import logistic_bound as lb
import logistic_cases as cases
import logistic_ref as ref

MUTATIONS = ["drop_last", "label_by_position", "flip_sign", "no_mean", "support_only_reg", "wrong_worker_shift"]


def test_shift_and_vexp_rules():
    assert [lb.shift(n) for n in (1, 2, 3, 4, 5, 100, 4096, 4097)] == [62, 61, 60, 60, 59, 55, 50, 49]
    assert lb.vexp_of(np.array([0.5], dtype=np.float32)) == -1 and lb.vexp_of(np.array([0.75, -1.0], dtype=np.float32)) == 0
    assert lb.vexp_of(np.array([1.5], dtype=np.float32)) == 1 and lb.vexp_of(np.array([0.0], dtype=np.float32)) == 1


def test_emulated_dot_follows_the_lane_order():
    """A row of 17 ones against weights that make the order visible: lane 0 adds entries 0 and 16 FIRST, the tree comes after."""
    row_ptr = np.array([0, 17], dtype=np.int64)
    col = np.arange(17, dtype=np.int32)
    val = np.ones(17, dtype=np.float32)
    w = np.full(17, np.float32(2.0 ** -24), dtype=np.float32)
    w[0] = 1.0
    # lane 0: 1 + 2^-24 (entry 16) is a tie and rounds to the even 1.0; the first pairing adds lane 1's 2^-24 to it: the same
    # tie, lost again; lanes 2..15 fold to 2^-23, 2^-22 and 2^-21 before they meet lane 0 and are all representable there:
    # fourteen of the sixteen small terms survive (a sequential sum would lose all of them, a pairwise one none)
    d = lb.emu_dot(row_ptr, col, val, w, 0)
    assert d == np.float32(1.0 + 14 * 2.0 ** -24)


@pytest.mark.parametrize("name", list(cases.step_cases()))
def test_emulation_inside_and_mutations_outside(name):
    csr = cases.csr()
    lists, lr = cases.step_cases()[name]
    w = cases.weights(1.0)
    want = ref.sync_step(csr, w, lists, lr, cases.LAM)
    bound = lb.dw(csr, w, lists, lr, cases.LAM)
    got = lb.emu_step(csr, w, lists, lr, cases.LAM).astype(np.float64)
    assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))
    assert float(np.max(bound)) < 1e-5 * float(np.max(np.abs(want)))   # (one step's bound is float precision, not a licence)
    for mut in MUTATIONS:
        if len(lists) == 1 and mut in ("no_mean", "wrong_worker_shift"):
            continue
        bad = lb.emu_step(csr, w, lists, lr, cases.LAM, mut).astype(np.float64)
        assert np.any(np.abs(bad - want) > bound), mut


@pytest.mark.parametrize("name", list(cases.step_cases()))
def test_five_emulated_steps_from_zero_stay_inside_the_accumulated_bound(name):
    csr = cases.csr()
    lists, lr = cases.step_cases()[name]
    w_ref = np.zeros(cases.data().dim + 1)
    w = np.zeros(cases.data().dim + 1, dtype=np.float32)
    E = np.zeros_like(w_ref)
    for _ in range(5):
        E = lb.dw(csr, w_ref, lists, lr, cases.LAM, E)
        w_ref = ref.sync_step(csr, w_ref, lists, lr, cases.LAM)
        w = lb.emu_step(csr, w, lists, lr, cases.LAM)
        assert np.all(np.abs(w.astype(np.float64) - w_ref) <= E)
    print("accumulated dw after five steps: max %.3e (max |w| %.3e)" % (float(np.max(E)), float(np.max(np.abs(w_ref)))))


@pytest.mark.parametrize("scale", [0.1, 10.0])
def test_emulated_gradient_inside_the_bound(scale):
    csr = cases.csr()
    w = cases.weights(scale)
    for name, idx in cases.gradient_lists().items():
        want = ref.gradient(csr, w, idx, cases.LAM)
        got = lb.emu_gradient(csr, w, idx, cases.LAM).astype(np.float64)
        bound = lb.dg(csr, w, idx, cases.LAM)
        assert np.all(np.abs(got - want) <= bound), (name, float(np.max(np.abs(got - want) / bound)))
        bad = lb.emu_gradient(csr, w, idx, cases.LAM, "flip_sign").astype(np.float64)
        assert np.any(np.abs(bad - want) > bound), name
