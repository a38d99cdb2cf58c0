"""Several topics over ROW RANGES on the GPU (csrc/dsgd_lg_topics_cols.hpp): every comparison but the fp64 one is of BITS -- against
lg_topics_sync_steps over the same rows as arange lists on a second engine in the same form, and against the single model on plane t."""
import ctypes as C

import numpy as np
import pytest
import dsgd_amd
import logistic_bound as lb
import logistic_cases as cases
import logistic_ref as ref
from dsgd_amd import _lib
from test_gpu_logistic import HD, _hand
from test_gpu_logistic_topics import bits, bits64, start_weights
from test_gpu_logistic_topics_wide import rig   # (three engines on the 4,096 shared rows, 128 planes)

pytestmark = pytest.mark.gpu

LR = 2.0 ** -6   # (a worker's gradient is a SUM over its rows)
# every group width (16: T <= 32, 32: <= 64, 64 beyond), idle lanes in the last pair (33, 65), padding topics (1, 5, 33, 65, 103)
FORMS = [("interleaved", 1), ("interleaved", 5), ("interleaved", 32), ("wide", 1), ("wide", 33), ("wide", 65), ("wide", 103), ("wide", 128)]
RANGE_SETS = {"whole": [(0, 4096)], "uneven": [(0, 100), (100, 137), (4000, 4001)], "overlap": [(0, 2000), (1000, 3000)],
              "k16": [(256 * i, 256 * (i + 1)) for i in range(16)], "one_row": [(77, 78)]}


def step_both(eng, oracle, ranges, n_steps, lr, W0):
    """n_steps over the ranges on `eng` (one step: the one-step call), over arange lists on `oracle`, from W0: equal bits, returned"""
    eng.lg_topics_set_weights(W0)
    oracle.lg_topics_set_weights(W0)
    st = eng.lg_topics_sync_step_ranges(ranges, lr) if n_steps == 1 else eng.lg_topics_sync_steps_ranges(ranges, n_steps, lr)
    rows = sum(b - a for a, b in ranges)
    assert st == {"n_samples": rows, "n_active": rows} and eng.grad_kernel_name() == "dsgd_lg_topics_cgrad_kernel"
    lists = [np.arange(a, b, dtype=np.int32) for a, b in ranges] * n_steps
    oracle.lg_topics_sync_steps(np.concatenate(lists), np.concatenate([[0], np.cumsum([len(a) for a in lists])]), n_steps, len(ranges), lr)
    assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(oracle.lg_topics_get_weights()))
    return eng.lg_topics_get_weights()


@pytest.mark.parametrize("name", list(RANGE_SETS))
@pytest.mark.parametrize("form,T", FORMS)
def test_ranges_give_the_list_forms_and_the_single_models_bits(rig, form, T, name):
    eng, oracle, one, P, d = rig
    ranges, W0 = RANGE_SETS[name], start_weights(d.dim + 1, T)
    for e in (eng, oracle):
        e.lg_topics_set(P[:T], **{form: True})
    assert not np.array_equal(bits(step_both(eng, oracle, ranges, 1, LR, W0)), bits(W0))
    W5 = step_both(eng, oracle, ranges, 5, LR, W0)
    assert np.array_equal(bits64(eng.lg_topics_loss_acc(0, cases.N)), bits64(oracle.lg_topics_loss_acc(0, cases.N)))   # the finish's |w_t'|^2 words
    lists = cases.step_cases()["3 workers 100/37/1"][0]          # a list step behind it reads every accumulator word: left clean
    assert eng.lg_topics_sync_step(lists, LR) == oracle.lg_topics_sync_step(lists, LR) and np.array_equal(bits(eng.lg_topics_get_weights()), bits(oracle.lg_topics_get_weights()))
    for t in (0, 51, 102) if (T, name) == (103, "uneven") else ():   # ... and the single model's column lists on plane t
        one.load_csr(d.row_ptr, d.col, d.val, P[t])
        one.set_weights(W0[t])
        one.lg_sync_steps_ranges(ranges, 5, LR)
        assert np.array_equal(bits(W5[t]), bits(one.get_weights())), t


@pytest.mark.parametrize("ranges", ([(0, 600)], [(0, 100), (100, 137), (599, 600)]), ids=("one", "three"))
def test_every_topic_against_the_fp64_reference(ranges):
    d = cases.data()
    rp, col, val = d.row_ptr[:601], d.col[:int(d.row_ptr[600])], d.val[:int(d.row_ptr[600])]
    P = np.random.default_rng(5).choice(np.array([-1, 1], dtype=np.int8), size=(128, 600))
    W0, lists = start_weights(d.dim + 1, 128), [np.arange(a, b, dtype=np.int32) for a, b in ranges]
    want = np.stack([ref.sync_step((rp, col, val, P[t]), W0[t], lists, LR, cases.LAM) for t in range(128)])
    bound = np.stack([lb.dw((rp, col, val, P[t]), W0[t], lists, LR, cases.LAM) for t in range(128)])
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:
        eng.load_csr(rp, col, val, P[0])
        for T in (33, 128):                                      # (no lane writes its neighbour's topic: ALL T topics)
            eng.lg_topics_set(P[:T], wide=True)
            eng.lg_topics_set_weights(W0[:T])
            eng.lg_topics_sync_step_ranges(ranges, LR)
            err = np.abs(eng.lg_topics_get_weights().astype(np.float64) - want[:T])
            print("T = %d, %d ranges: max err/bound %.3f" % (T, len(ranges), float(np.max(err / bound[:T]))))
            assert np.all(err <= bound[:T]), T


@pytest.mark.parametrize("workers", (1, 2))
@pytest.mark.parametrize("form,T", [("interleaved", 5), ("wide", 128)])
def test_hand_built_rows_bits(form, T, workers):
    csr, w, n_shape, sat0 = _hand()   # (empty, 64, 65, one crossing the head, saturation) and rows of 16 and 17, as test_gpu_logistic_topics_wide's
    rng = np.random.default_rng(T)
    more = [np.arange(300, 316), np.arange(400, 417)]
    row_ptr = np.concatenate([csr[0], csr[0][-1] + np.cumsum([len(r) for r in more])])
    col = np.concatenate([csr[1]] + more).astype(np.int32)
    val = np.concatenate([csr[2], rng.choice([-1.0, 1.0], size=33) * 2.0 ** rng.integers(-2, 3, size=33)]).astype(np.float32)
    label = np.concatenate([csr[3], [1, -1]]).astype(np.int8)
    n = len(label)
    P = np.ascontiguousarray(np.vstack([label[None], -label[None], rng.choice(np.array([-1, 1], dtype=np.int8), size=(T - 2, n))]), dtype=np.int8)
    ranges = [(0, n)] if workers == 1 else [(0, n_shape), (n_shape, n)]
    W0 = np.stack([np.roll(w, t) if t >= 3 else w for t in range(T)])
    with dsgd_amd.Engine(HD, 0.0) as eng, dsgd_amd.Engine(HD, 0.0) as one:
        eng.load_csr(row_ptr, col, val, label)
        eng.lg_topics_set(P, **{form: True})
        eng.lg_topics_set_weights(W0)
        eng.lg_topics_sync_step_ranges(ranges, 0.25)
        W1 = eng.lg_topics_get_weights()
        assert np.isfinite(W1).all() and not np.array_equal(bits(W1), bits(W0))
        for t in (0, T // 2, T - 1):
            one.load_csr(row_ptr, col, val, P[t])
            one.set_weights(W0[t])
            one.lg_sync_steps_ranges(ranges, 1, 0.25)
            assert np.array_equal(bits(W1[t]), bits(one.get_weights())), t


@pytest.mark.parametrize("form,T", [("interleaved", 8), ("wide", 33)])
def test_long_runs(form, T):
    d = dsgd_amd.synth.generate(50000, seed=5)   # shares of several fetches per lane group, columns cut by run and share boundaries
    P = np.random.default_rng(9).choice(np.array([-1, 1], dtype=np.int8), size=(T, 50000))
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng, dsgd_amd.Engine(d.dim, cases.LAM) as oracle:
        for e in (eng, oracle):
            e.load_csr(d.row_ptr, d.col, d.val, d.label)
            e.lg_topics_set(P, **{form: True})
        for ranges in ([(0, 50000)], [(0, 30000), (20000, 50000)]):
            step_both(eng, oracle, ranges, 2, 2.0 ** -10, start_weights(d.dim + 1, T))


def test_refusals_and_state(rig):
    eng, oracle, one, P, d = rig
    lib, ctx, z, W0 = eng._lib, eng._ctx, C.c_int64, start_weights(d.dim + 1, 5)
    def code(rb, re_, n_steps=1):
        return lib.dsgd_lg_topics_sync_steps_ranges(ctx, (z * len(rb))(*rb), (z * len(re_))(*re_), len(rb), z(n_steps), C.c_float(LR), None)

    eng.lg_topics_set(None)
    assert code([0], [10]) == _lib.ESTATE                        # no topics
    for form in ({}, {"interleaved": True}):
        eng.lg_topics_set(P[:5], **form)
        eng.lg_topics_set_weights(W0)
        if not form:                                             # the planar form: not served, and told which are
            assert code([0], [10]) == _lib.ESTATE and b"dsgd_lg_topics_set_il and dsgd_lg_topics_set_wide" in lib.dsgd_last_error()
        else:                                                    # lg_check_ranges' refusals with its codes, in front of the steps'
            assert code([0], [10], 0) == code([0], [10], -1) == code([5], [5]) == _lib.EINVAL and code([4000], [4097], 0) == _lib.ERANGE
            assert code([4000], [4097]) == lib.dsgd_lg_sync_step_ranges(ctx, (z * 1)(4000), (z * 1)(4097), 1, C.c_float(LR), None) == _lib.ERANGE
            assert lib.dsgd_lg_topics_sync_step_ranges(ctx, (z * 1)(9), (z * 1)(3), 1, C.c_float(LR), None) == _lib.EINVAL
        assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(W0))
    first = [(10, 900), (900, 2222)]                             # a configuration first laid out by the single model serves the topics
    assert eng.lg_sync_steps_ranges(first, 1, LR)["n_samples"] == 2212 and eng.grad_kernel_name() == "dsgd_lg_cgrad_kernel"
    oracle.lg_topics_set(P[:5], interleaved=True)
    step_both(eng, oracle, first, 2, LR, W0)
