"""No GPU needed: what tests/logistic_cs_bound.py is worth.  On inputs chosen here -- 400 columns (25 per slice of 16; filler rows make rank == key), 48 listed rows
of which one has 20 entries inside ONE slice (two slots), one sits in one slice whole and one is empty; three workers with lists
of 4, 9 and 30 rows (three different shifts; a row listed twice by one worker, a row listed by two), lambda = 0.05 and
non-zero weights on every column so that the L2 term matters everywhere -- the honest emulation of the slice order stays inside
the carried dw of the fp64 reference on EVERY coordinate of each of 10 chained steps, and each mistake a kernel of this shape
invites leaves it at some coordinate of some step:

    shift_of_largest, l2_listed_only, acc_not_cleared, padding_written_back, label_ignored, header_shift_finish.

slice_order_one_wg (one workgroup adds the partials in the other slice order) is different in kind: a reordering of a sum of
this depth is covered by gamma(k) sum |x||w| whatever the inputs, so NO input can take it outside a sound dz (the figure below
is printed: its worst err / bound stays under 1).  What it breaks is the promise that every workgroup holds the same d: the test
shows that on these inputs it changes bits of the weights, and on the GPU the determinism tests (one run against split runs,
caller lists against device-drawn ones: tests/test_gpu_logistic_cs.py) hold the kernel to one order."""

import functools

import numpy as np
import pytest

import logistic_cs_bound as cb
import logistic_ref as ref

DP, N, K_LISTS = 400, 48, (4, 9, 30)
LAM, LR, STEPS = 0.05, 0.25, 10


def inputs():
    return cb.designed(DP, N, K_LISTS, STEPS)


@functools.lru_cache(maxsize=None)
def reference():
    """(w_ref after every step, the carried bound E after every step) -- computed once, shared, never changed"""
    csr, steps, w0 = inputs()
    w, E = w0.astype(np.float64), np.zeros(DP)
    out = []
    for lists in steps:
        E = cb.dw(csr, w, lists, LR, LAM, E)
        w = ref.sync_step(csr, w, lists, LR, LAM)
        out.append((w, E))
    return out


def run(mut):
    """worst err / bound over all coordinates of every step, and the weights after every step"""
    csr, steps, w0 = inputs()
    emu = cb.Emu(csr, w0, mut=mut)
    worst, ws = 0.0, []
    for lists, (w_ref, E) in zip(steps, reference()):
        w = emu.step(lists, LR, LAM)
        assert np.all(np.isfinite(w))
        worst = max(worst, float(np.max(np.abs(w.astype(np.float64) - w_ref) / E)))   # every coordinate, none left out
        ws.append(w)
    return worst, ws


def test_the_inputs_have_the_shapes_they_claim():
    csr, steps, _ = inputs()
    row_ptr, col = csr[0], csr[1]
    rank, sl = cb.slice_of(csr, DP)
    per = lambda r: np.bincount(sl[row_ptr[r]:row_ptr[r + 1]], minlength=cb.G)
    assert per(2).max() == 20 and np.count_nonzero(per(2)) == 1          # more than 16 entries inside one slice: two slots
    assert np.count_nonzero(per(3)) == 1 and per(3).sum() == 7           # all entries in one slice
    assert row_ptr[6] == row_ptr[5]                                      # empty
    assert len({cb.lb.shift(n) for n in K_LISTS}) == 3
    assert all(list(l[0][:2]) == [2, 2] and l[1][0] == l[2][0] == 3 and l[2][1] == 5 for l in steps)


def test_the_honest_emulation_stays_inside_dw_over_ten_chained_steps():
    worst, _ = run(None)
    print("honest slice order: worst err / carried dw over %d steps x %d coordinates = %.3f" % (STEPS, DP, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("mut", [m for m in cb.MUTATIONS if m != "slice_order_one_wg"])
def test_a_mistake_leaves_dw(mut):
    worst, _ = run(mut)
    print("%s: worst err / carried dw = %.3g" % (mut, worst))
    assert worst > 1.0


def test_the_wrong_slice_order_moves_bits_but_no_sound_bound_can_see_it():
    worst, ws = run("slice_order_one_wg")
    _, honest = run(None)
    print("slice_order_one_wg: worst err / carried dw = %.3f" % worst)
    assert worst <= 1.0                                                   # (a reordering is inside gamma(k) sum |x||w|: the docstring)
    assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ws, honest))
