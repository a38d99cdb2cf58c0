"""No GPU: what tests/logistic_async_bound.py is worth.  An emulation of the kernels' order (logistic_bound.emu_acc + the asynchronous
finish) stays inside the bound on the lists tests/test_gpu_logistic_async.py runs and on the hard widths; the float64 reference
itself is inside; and each mistake this finish invites falls outside on at least one case."""

import numpy as np
import pytest

import logistic_async_bound as ab
import logistic_async_cases as ac
import logistic_async_ref as aref
import logistic_bound as lb
import logistic_cases as cases
import logistic_hard_cases as hard

LAM = cases.LAM


def inside(csr, w32, idx, lr, lam, mut=None, plan_batch=None, slices=False):
    dw, dd, wn, delta = ab.dstep(csr, w32, idx, lr, lam, slices=slices)
    w_emu, d_emu = ab.emu_step(csr, w32, idx, lr, lam, mut, plan_batch)
    return bool(np.all(np.abs(w_emu.astype(np.float64) - wn) <= dw)), bool(np.all(np.abs(d_emu - delta) <= dd))


@pytest.mark.parametrize("wname", list(ac.weight_sets()))
def test_emulation_and_reference_inside_on_the_shared_lists(wname):
    csr, w = cases.csr(), ac.weight_sets()[wname]
    for name, idx in ac.lists().items():
        assert inside(csr, w, idx, ac.LR, LAM) == (True, True), (wname, name)
        assert ab.reference_inside(csr, w, idx, ac.LR, LAM), (wname, name)
        assert ab.reference_inside(csr, w, idx, ac.LR, LAM, slices=True), (wname, name)


@pytest.mark.parametrize("dim", ac.WIDTHS)
def test_emulation_and_reference_inside_on_the_hard_widths(dim):
    c = hard.width(dim)
    for name, idx in ac.width_lists(dim).items():
        assert inside(c.csr, c.w, idx, ac.LR, c.lam) == (True, True), (dim, name)
        assert ab.reference_inside(c.csr, c.w, idx, ac.LR, c.lam), (dim, name)
    if dim in hard.W_FULL:
        assert np.diff(c.csr[0])[hard.W_FULL_ROW] > 64 and hard.W_FULL_ROW in ac.width_lists(dim)["37"]


def test_one_row_is_the_synchronous_step_of_one_worker():
    csr, w = cases.csr(), cases.weights(1.0)
    for r in (0, 7, 4095):
        idx = np.array([r], dtype=np.int32)
        a, _ = ab.emu_step(csr, w, idx, ac.LR, LAM)
        s = lb.emu_step(csr, w, [idx], ac.LR, LAM)
        assert np.array_equal(a.view(np.uint32), s.view(np.uint32)), r


def test_a_peer_that_applies_the_delta_has_the_bits():
    csr, w = cases.csr(), cases.weights(1.0)
    w1, delta = ab.emu_step(csr, w, ac.lists()["100"], ac.LR, LAM)
    peer = (w.astype(np.float64) - delta).astype(np.float32)
    assert np.array_equal(peer.view(np.uint32), w1.view(np.uint32))
    assert np.all(np.abs(peer.astype(np.float64) - aref.update_grad(w, np.arange(len(w)), delta)) <= ab.dupdate(w, delta))


# mutation -> the cases it is tried on: (weights, list, the plan's batch)
TRIALS = {"mean_over_K": [("logits 1", "100", None), ("logits 1", "2", None)],
          "reg_over_n": [("logits 1", "100", None), ("logits 8", "17", None)],
          "shift_from_batch": [("logits 1", "17", 100), ("logits 1", "2", 100)],
          "delta_float": [("tiny", "100", None), ("tiny", "1025", None)],
          "lr_data_only": [("logits 1", "100", None), ("logits 8", "1", None)]}


@pytest.mark.parametrize("mut", ab.MUTATIONS)
def test_each_mistake_leaves_the_bound(mut):
    csr = cases.csr()
    caught = []
    for wname, lname, batch in TRIALS[mut]:
        w, idx = ac.weight_sets()[wname], ac.lists()[lname]
        assert inside(csr, w, idx, ac.LR, LAM) == (True, True)          # (the honest emulation is inside on this very case)
        ok_w, ok_d = inside(csr, w, idx, ac.LR, LAM, mut, batch)
        caught.append(not ok_w)
    assert any(caught), (mut, caught)


def test_replay_of_the_master_on_the_zero_lag_schedule():
    """tests/logistic_async_ref.fit: checks at 0, check_every, 2 check_every, ..., the last one at max_steps; worker u mod K"""
    csr = cases.csr()
    seen = []
    out = aref.fit(csr, np.zeros(len(cases.weights(1.0))), 3000, cases.N, 3, 1, 16, ac.LR, LAM, lambda losses: False, 7, 0.5, seed=5,
                   max_steps=24, on_update=lambda u, w, idx: seen.append((u, idx.copy())))
    assert out["check_at"] == [0, 7, 14, 21, 24] and out["updates"] == 24 and out["checks"] == 5
    split = aref.split_vanilla(3000, 3)
    for u, idx in seen:   # positional_bug: positions inside the worker's OWN length, from row 0
        assert len(idx) == 16 and idx.min() >= 0 and idx.max() < split[u % 3][1] - split[u % 3][0]
    assert out["best_loss"] == min(out["test_losses"]) and out["test_losses"][0] < out["test_losses"][-1]
