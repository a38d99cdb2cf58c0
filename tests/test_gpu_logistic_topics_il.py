"""Several topics, INTERLEAVED, on the GPU (csrc/dsgd_lg_topics_il.hpp): the planar form's contract and oracle -- BITS of single-model
engines with label = plane t -- at T in {1, 5, 8, 9, 32}: three padding topics, a half-filled quad, the planar maximum, the first
size only this form serves, a full 128-byte line.  Planes: the data's labels, all +1, all -1, then seeded random ones."""

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_cases as cases
import logistic_ref as ref
from dsgd_amd import _lib
from test_gpu_logistic import HD, _hand
from test_gpu_logistic_topics import bits, bits64, lists_of, start_weights

pytestmark = pytest.mark.gpu

TS = (1, 5, 8, 9, 32)
LR = 0.5


@pytest.fixture(scope="module")
def rig():
    """the topics engine and the 32 single-model engines, one per plane"""
    d = cases.data()
    n = len(d.label)
    rest = np.random.default_rng(31).choice(np.array([-1, 1], dtype=np.int8), size=(29, n))
    P = np.ascontiguousarray(np.vstack([d.label.astype(np.int8)[None], np.ones((1, n), np.int8), -np.ones((1, n), np.int8), rest]))
    engines = [dsgd_amd.Engine(d.dim, cases.LAM) for _ in range(33)]
    engines[32].load_csr(*cases.csr(d))
    for t in range(32):
        engines[t].load_csr(d.row_ptr, d.col, d.val, P[t])
    yield engines[32], engines[:32], P, d
    for e in engines:
        e.close()


@pytest.mark.parametrize("T", TS)
def test_one_step_gives_every_topic_the_single_models_bits(rig, T):
    eng, oracle, P, d = rig
    W0 = start_weights(d.dim + 1, T)
    eng.lg_topics_set(P[:T], interleaved=True)
    assert eng.n_topics == T and np.all(eng.lg_topics_get_weights() == 0.0)
    steps = [lists_of(K, n, 100 * K + n) for K in (1, 3) for n in (1, 17, 100, 1025)]
    rep = lists_of(1, 50, 77)[0]
    steps.append([np.concatenate([rep, rep[:1], rep[:1]]), rep[::-1].copy()])   # a row named three times, and again by the peer
    for lists in steps:
        eng.lg_topics_set_weights(W0)
        assert eng.lg_topics_sync_step(lists, LR)["n_samples"] == sum(len(a) for a in lists)
        W1 = eng.lg_topics_get_weights()
        for t in range(T):
            oracle[t].set_weights(W0[t])
            oracle[t].lg_sync_step(lists, LR)
            assert np.array_equal(bits(W1[t]), bits(oracle[t].get_weights())), (T, [len(a) for a in lists], t)
    assert not np.array_equal(bits(W1[0]), bits(W0[0]))          # (the step moved something)


@pytest.mark.parametrize("T", TS)
def test_five_steps_evaluation_and_prediction_bits(rig, T):
    eng, oracle, P, d = rig
    lists = cases.step_cases()["3 workers 100/37/1"][0]
    flat = np.concatenate(lists * 5)
    offs = np.concatenate([[0], np.cumsum([len(a) for a in lists] * 5)])
    eng.lg_topics_set(P[:T], interleaved=True)                   # from zero weights
    for _ in range(5):
        eng.lg_topics_sync_step(lists, LR)
    W5 = eng.lg_topics_get_weights()
    eng.lg_topics_set_weights(np.zeros_like(W5))
    assert eng.lg_topics_sync_steps(flat, offs, 5, len(lists), LR)["n_samples"] == len(flat)
    W5b = eng.lg_topics_get_weights()
    assert np.array_equal(bits(W5), bits(W5b))                   # five steps in one call equal five calls ...
    for t in range(T):                                           # ... and the oracle
        oracle[t].set_weights(np.zeros(d.dim + 1, dtype=np.float32))
        oracle[t].lg_sync_steps(flat, offs, 5, len(lists), LR)
        assert np.array_equal(bits(W5b[t]), bits(oracle[t].get_weights())), t
    # the evaluation right behind the steps (|w|^2 from the finish) and behind weights the caller set (the |w|^2 kernel)
    for fresh in (True, False):
        if not fresh:
            eng.lg_topics_set_weights(W5b)
        for a, b in ((0, 4096), (1500, 2500), (77, 78)):
            loss, acc = eng.lg_topics_loss_acc(a, b)
            for t in range(T):
                if not fresh:
                    oracle[t].set_weights(W5b[t])
                lo, ac = oracle[t].lg_loss_acc(a, b)
                assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), (fresh, a, b, t, loss[t], lo)
    idx = np.random.default_rng(8).permutation(cases.N)[:300].astype(np.int32)
    idx[5] = idx[4]                                              # a row listed twice
    p = eng.lg_topics_predict(idx)
    assert p.shape == (T, 300)
    for t in range(T):
        assert np.array_equal(bits(p[t]), bits(oracle[t].lg_predict_proba(idx))), t


@pytest.mark.parametrize("T", (32, 5))
def test_hand_built_rows_bits(T):
    """every row shape, the 2,100-column row that crosses the head at every TP, saturation weights: one step, one evaluation"""
    csr, w, n_shape, sat0 = _hand()
    n = len(csr[3])
    rest = np.random.default_rng(T).choice(np.array([-1, 1], dtype=np.int8), size=(T - 3, n))
    P = np.ascontiguousarray(np.vstack([csr[3][None], -csr[3][None], np.ones((1, n), np.int8), rest]), dtype=np.int8)
    lists = [np.arange(n_shape, dtype=np.int32), np.arange(n_shape, n, dtype=np.int32)]
    W0 = np.stack([np.roll(w, t) if t >= 3 else w for t in range(T)])
    with dsgd_amd.Engine(HD, 0.0) as eng, dsgd_amd.Engine(HD, 0.0) as one:
        eng.load_csr(*csr)
        eng.lg_topics_set(P, interleaved=True)
        eng.lg_topics_set_weights(W0)
        eng.lg_topics_sync_step(lists, 0.25)
        W1 = eng.lg_topics_get_weights()
        loss, acc = eng.lg_topics_loss_acc(0, n)
        assert np.isfinite(W1).all() and np.isfinite(loss).all() and eng.column_ranks().max() >= 2048
        for t in range(T):
            one.load_csr(csr[0], csr[1], csr[2], P[t])
            one.set_weights(W0[t])
            one.lg_sync_step(lists, 0.25)
            assert np.array_equal(bits(W1[t]), bits(one.get_weights())), t
            lo, ac = one.lg_loss_acc(0, n)
            assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), t


def test_planar_and_interleaved_agree_at_eight_topics(rig):
    eng, oracle, P, d = rig
    lists, W0, got = cases.step_cases()["3 workers 100/37/1"][0], start_weights(d.dim + 1, 8), []
    for il in (False, True):
        eng.lg_topics_set(P[:8], interleaved=il)
        eng.lg_topics_set_weights(W0)
        for _ in range(3):
            eng.lg_topics_sync_step(lists, LR)
        got.append(eng.lg_topics_get_weights())
    assert np.array_equal(bits(got[0]), bits(got[1])) and not np.array_equal(bits(got[1]), bits(W0))


def test_one_of_nine_topics_against_the_fp64_reference(rig):
    eng, oracle, P, d = rig
    lists, lr = cases.step_cases()["3 workers 100/37/1"]
    w = cases.weights(1.0)
    eng.lg_topics_set(P[:9], interleaved=True)
    eng.lg_topics_set_weights(np.stack([w] * 9))
    eng.lg_topics_sync_step(lists, lr)
    W1 = eng.lg_topics_get_weights()
    loss, acc = eng.lg_topics_loss_acc(0, 4096)
    csr_t = (d.row_ptr, d.col, d.val, P[8])
    err = np.abs(W1[8].astype(np.float64) - ref.sync_step(csr_t, w, lists, lr, cases.LAM))
    bound = lb.dw(csr_t, w, lists, lr, cases.LAM)
    print("topic 8: max err/bound %.3f" % float(np.max(err / bound)))
    assert np.all(err <= bound)
    assert abs(loss[8] - ref.loss_acc(csr_t, W1[8], 0, 4096, cases.LAM)[0]) <= lb.dloss(csr_t, W1[8], 0, 4096, cases.LAM)


def test_refusals_leave_the_topics_as_they_were(rig):
    eng, oracle, P, d = rig
    lib, ctx = eng._lib, eng._ctx
    eng.lg_topics_set(P[:9], interleaved=True)
    W0 = start_weights(d.dim + 1, 9)
    eng.lg_topics_set_weights(W0)
    bad = P[:9].copy()
    bad[8, 4095] = 0
    assert lib.dsgd_lg_topics_set_il(ctx, 33, _lib.ptr(P)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_set_il(ctx, -1, _lib.ptr(P)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_set_il(ctx, 9, _lib.ptr(bad)) == _lib.EINVAL and b"plane 8, row 4095" in lib.dsgd_last_error()
    assert lib.dsgd_lg_topics_set(ctx, 9, _lib.ptr(P)) == _lib.EINVAL          # the planar call keeps its limit of 8
    assert eng.n_topics == 9 and np.array_equal(bits(eng.lg_topics_get_weights()), bits(W0))
    eng.lg_topics_set(None, interleaved=True)
    assert eng.n_topics == 0
