"""Softmax over few classes with the lanes across the non-zeros (csrc/dsgd_lg_softmax_il.hpp; Engine.lg_softmax_set(...,
interleaved=True)): every result carries the BITS of the wide softmax on the same rows, classes and weights -- at TP = 4, 8, 12, 16
and 32, with padding classes, idle lanes and a full group; on the long evaluation's chains and both sides of the tile rule; on hostile
values, the interleaved head's edge and ties across the lanes -- and, once, lies within tests/softmax_bound.py of plain fp64."""

import numpy as np
import pytest

import dsgd_amd
import logistic_cases as cases
import softmax_bound as sm
import softmax_hard_cases as hc
from dsgd_amd import _lib
from hard_data import TRAITS
from test_gpu_logistic_topics import bits, code_of, start_weights
from test_gpu_softmax import LR, N_SMALL, RANGES, classes_of, flat

pytestmark = pytest.mark.gpu

NEW, WIDE = "dsgd_lg_softmax_il_grad_kernel", "dsgd_lg_softmax_grad_kernel"
lists3 = lambda n: [np.random.default_rng(6 + k).integers(0, n, size=k).astype(np.int32) for k in (100, 37, 1)]   # (repeats included)


@pytest.fixture(scope="module")
def pair():
    d = cases.data()
    with dsgd_amd.Engine(d.dim, cases.LAM) as a, dsgd_amd.Engine(d.dim, cases.LAM) as b:
        for eng in (a, b):
            eng.load_csr(*cases.csr(d))
        yield a, b, d


def both(case):
    """(the new form, the wide form) on a hard case's rows, classes and weights"""
    out = []
    for il in (True, False):
        eng = dsgd_amd.Engine(case.dim, case.lam)
        eng.load_csr(*case.csr)
        eng.lg_softmax_set(case.cls, case.C, interleaved=il)
        eng.lg_topics_set_weights(case.W)
        out.append(eng)
    return out


def same_weights(a, b, start):
    Wa = a.lg_topics_get_weights()                                                    # (equal, and moved)
    assert np.array_equal(bits(Wa), bits(b.lg_topics_get_weights())) and not np.array_equal(bits(Wa), bits(start))


@pytest.mark.parametrize("C", (2, 3, 4, 5, 8, 9, 16, 29, 32))
def test_bits_of_the_wide_form(pair, C):
    a, b, d = pair
    cls, W0, lists = classes_of(cases.N, C), start_weights(d.dim + 1, C), lists3(N_SMALL)
    a.lg_softmax_set(cls, C, interleaved=True)
    b.lg_softmax_set(cls, C)

    def step(call):
        for eng in (a, b):
            eng.lg_topics_set_weights(W0)
            call(eng)
        same_weights(a, b, W0)

    step(lambda e: e.lg_softmax_sync_step(lists, LR))
    assert (a.grad_kernel_name(), b.grad_kernel_name()) == (NEW, WIDE)                # two paths, not one twice
    step(lambda e: e.lg_softmax_sync_steps(*flat(lists, 5), 5, 3, 2.0 ** -4))
    for ranges in ([(0, 4096)], [(0, 100), (100, 137), (4000, 4001)], [(77, 78)]):
        step(lambda e: e.lg_softmax_sync_steps_ranges(ranges, 2, 2.0 ** -10))          # (a worker's gradient is a SUM over its rows)
        assert a.lg_softmax_loss_acc(0, cases.N) == b.lg_softmax_loss_acc(0, cases.N)  # (|w_c|^2 from the finish)
    for eng in (a, b):
        eng.lg_topics_set_weights(W0)
    for lo, hi in RANGES:
        assert a.lg_softmax_loss_acc(lo, hi) == b.lg_softmax_loss_acc(lo, hi)         # (|w_c|^2 of weights the finish did not write)
    idx = np.random.default_rng(8).integers(0, cases.N, size=301).astype(np.int32)
    (ca, pa), (cb, pb) = a.lg_softmax_predict(idx, proba=True), b.lg_softmax_predict(idx, proba=True)
    assert np.array_equal(ca, cb) and np.array_equal(bits(pa), bits(pb)) and np.array_equal(ca, a.lg_softmax_predict(idx))


def test_long_chains_and_the_tile_rule():
    import torch

    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert all(b - a > 2 * 32 * n_cu for a, b in hc.L_LONG[:2]) and hc.L_LONG[2][1] - hc.L_LONG[2][0] > 32 * n_cu, n_cu
    a, b = both(hc.long_case(5))
    with a, b:
        for lo, hi in hc.L_RANGES:
            assert a.lg_softmax_loss_acc(lo, hi) == b.lg_softmax_loss_acc(lo, hi), (lo, hi)


@pytest.mark.parametrize("case", [("hostile", t, 5) for t in TRAITS] + [("width", 255, 5), ("width", 256, 5)], ids=lambda k: "-".join(map(str, k)))
def test_hostile_values_and_the_heads_edge(case):
    """(the interleaved head holds 2048 / 8 = 256 ranks at TP = 8: dim 255 fills it, dim 256 has one rank beyond)"""
    case = hc.bound_case(case)
    a, b = both(case)
    with a, b:
        n = len(case.cls)
        for lists, lr in case.steps.values():
            for eng in (a, b):
                eng.lg_topics_set_weights(case.W)
                eng.lg_softmax_sync_step(lists, lr)
            same_weights(a, b, case.W)
            assert a.lg_softmax_loss_acc(0, n) == b.lg_softmax_loss_acc(0, n)
        for ranges in case.range_sets.values():
            for eng in (a, b):
                eng.lg_topics_set_weights(case.W)
                eng.lg_softmax_sync_steps_ranges(ranges, 1, case.lr_ranges)
            same_weights(a, b, case.W)


def test_ties_across_the_lanes_of_one_group():
    case = hc.ties(32)
    a, b = both(case)
    with a, b:
        assert list(a.lg_softmax_predict(case.predict)) == [case.rows[r][2] for r in case.predict]
        for r, (_, y, want) in enumerate(case.rows):
            assert a.lg_softmax_loss_acc(r, r + 1) == b.lg_softmax_loss_acc(r, r + 1) and a.lg_softmax_loss_acc(r, r + 1)[1] == float(want == y)


@pytest.mark.parametrize("C", (5, 32))
def test_against_fp64(C):
    """test_gpu_softmax.test_against_fp64's inputs at K = 3: the module shows on the CPU what they are worth"""
    d = cases.data()
    csr = (d.row_ptr[:N_SMALL + 1], d.col[:d.row_ptr[N_SMALL]], d.val[:d.row_ptr[N_SMALL]], np.ones(N_SMALL, np.int8))
    cls, W0, lists = classes_of(N_SMALL, C), start_weights(d.dim + 1, C), lists3(N_SMALL)
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:
        eng.load_csr(*csr)
        eng.lg_softmax_set(cls, C, interleaved=True)
        eng.lg_topics_set_weights(W0)
        for lo, hi in RANGES:
            (loss, acc), (want_loss, want_acc, _) = eng.lg_softmax_loss_acc(lo, hi), sm.loss_acc(csr, W0, cls, lo, hi, cases.LAM)
            assert abs(loss - want_loss) <= sm.dloss(csr, W0, cls, lo, hi, cases.LAM) and acc == want_acc
        eng.lg_softmax_sync_step(lists, LR)
        assert eng.grad_kernel_name() == NEW
        assert np.all(np.abs(eng.lg_topics_get_weights() - sm.sync_step(csr, W0, cls, lists, LR, cases.LAM)) <= sm.dw(csr, W0, cls, lists, LR, cases.LAM))


def test_refusals(pair):
    a, b, d = pair
    cls, W0, lists = classes_of(cases.N, 9), start_weights(d.dim + 1, 9), [np.arange(50, dtype=np.int32), np.arange(50, 90, dtype=np.int32)]
    P = np.where(cls[None, :] == np.arange(9, dtype=np.uint8)[:, None], 1, -1).astype(np.int8)
    a.lg_softmax_set(cls, 9, interleaved=True)
    a.lg_topics_set_weights(W0)
    b.lg_topics_set(P, interleaved=True)                                              # the same planes WITHOUT the mark
    b.lg_topics_set_weights(W0)
    unchanged = lambda eng, C: eng.n_classes == C and eng.n_topics == 9 and np.array_equal(bits(eng.lg_topics_get_weights()), bits(W0))
    lib, ctx = a._lib, a._ctx
    for C in (1, 33, -1, 8):                                                          # C = 1, beyond 32, an entry >= C
        assert lib.dsgd_lg_softmax_set_il(ctx, C, _lib.ptr(cls)) == _lib.ERANGE and unchanged(a, 9), C
    assert lib.dsgd_lg_softmax_set_il(ctx, 9, None) == _lib.EINVAL and unchanged(a, 9)
    with dsgd_amd.Engine(d.dim, cases.LAM, precision="fp64") as e64:
        e64.load_csr(*cases.csr(d))
        assert e64._lib.dsgd_lg_softmax_set_il(e64._ctx, 9, _lib.ptr(cls)) == _lib.EUNSUPPORTED
    calls = (lambda: b.lg_softmax_sync_step(lists, LR), lambda: b.lg_softmax_sync_steps(*flat(lists, 1), 1, 2, LR),
             lambda: b.lg_softmax_sync_steps_ranges([(0, 10)], 1, LR), lambda: b.lg_softmax_loss_acc(0, 10), lambda: b.lg_softmax_predict(lists[0]))
    assert [code_of(c) for c in calls] == [_lib.ESTATE] * 5 and unchanged(b, 0)
    for eng in (a, b):                                                                # the topic calls keep serving the classes: interleaved topics' bits
        eng.lg_topics_sync_step(lists, LR)
    same_weights(a, b, W0)
    a.lg_softmax_set(None, interleaved=True)
    assert a.n_classes == 0 and a.n_topics == 0
