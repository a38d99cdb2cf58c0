"""Several topics, WIDE, on the GPU (csrc/dsgd_lg_topics_wide.hpp): BITS of the single model with label = plane t at every lane-group
width (T <= 32: 16 lanes, <= 64: 32, beyond: 64), with idle lanes in the last pair (T = 33, 65), RCV1's 103 and the full 128."""

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

WIDE_TS, LR = (33, 64, 65, 103, 128), 0.5
RANGES = ((0, 4096), (1500, 2500), (77, 78))
N_SMALL = 600   # rows of the fp64 comparison: more than two workgroups of the gradient at every width


@pytest.fixture(scope="module")
def rig():
    """the wide engine, an interleaved engine, one single-model engine (its labels loaded per topic) and the 128 planes"""
    d = cases.data()
    n = len(d.label)
    rest = np.random.default_rng(31).choice(np.array([-1, 1], dtype=np.int8), size=(125, n))
    P = np.ascontiguousarray(np.vstack([d.label.astype(np.int8)[None], np.ones((1, n), np.int8), -np.ones((1, n), np.int8), rest]))
    engines = [dsgd_amd.Engine(d.dim, cases.LAM) for _ in range(3)]
    for e in engines:
        e.load_csr(*cases.csr(d))
    yield engines[0], engines[1], engines[2], P, d
    for e in engines:
        e.close()


def run(eng, lists, W0, idx):
    """one step, then five steps in one call from W0: the weights after each, every range's loss and accuracy, the probabilities"""
    eng.lg_topics_set_weights(W0)
    eng.lg_topics_sync_step(lists, LR)
    W1 = eng.lg_topics_get_weights()
    eng.lg_topics_set_weights(W0)
    flat, offs = np.concatenate(lists * 5), np.concatenate([[0], np.cumsum([len(a) for a in lists] * 5)])
    assert eng.lg_topics_sync_steps(flat, offs, 5, len(lists), LR)["n_samples"] == len(flat)
    ev = [eng.lg_topics_loss_acc(a, b) for a, b in RANGES]
    return W1, eng.lg_topics_get_weights(), ev, eng.lg_topics_predict(idx)


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("T", (1, 5, 32))
def test_wide_gives_the_interleaved_forms_bits(rig, T, K):
    wide, il, one, P, d = rig
    lists, W0 = lists_of(K, 100, 10 * T + K), start_weights(d.dim + 1, T)
    idx = np.random.default_rng(8).permutation(cases.N)[:300].astype(np.int32)
    wide.lg_topics_set(P[:T], wide=True)
    il.lg_topics_set(P[:T], interleaved=True)
    assert wide.n_topics == T and np.all(wide.lg_topics_get_weights() == 0.0)
    a, b = run(wide, lists, W0, idx), run(il, lists, W0, idx)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and not np.array_equal(bits(a[0]), bits(W0))
    assert np.array_equal(bits64(a[2]), bits64(b[2])) and a[3].shape == (T, 300) and np.array_equal(bits(a[3]), bits(b[3]))


@pytest.mark.parametrize("T", WIDE_TS)
def test_wide_topics_give_the_single_models_bits(rig, T):
    wide, il, one, P, d = rig
    rep = lists_of(1, 1000, T)[0]
    lists = [rep[:1], rep[:16], rep[16:33], np.concatenate([rep, rep[:24], rep[:1]])]   # 1, 16, 17 and 1,025 rows, rows repeated
    W0 = start_weights(d.dim + 1, T)
    idx = np.random.default_rng(8).integers(0, cases.N, size=300).astype(np.int32)   # (rows listed twice among them)
    wide.lg_topics_set(P[:T], wide=True)
    W1, W5, ev, p = run(wide, lists, W0, idx)
    flat, offs = np.concatenate(lists * 5), np.concatenate([[0], np.cumsum([len(a) for a in lists] * 5)])
    for t in sorted({0, 1, T // 2, T - 2, T - 1}):
        one.load_csr(d.row_ptr, d.col, d.val, P[t])
        one.set_weights(W0[t])
        one.lg_sync_step(lists, LR)
        assert np.array_equal(bits(W1[t]), bits(one.get_weights())), t
        one.set_weights(W0[t])
        one.lg_sync_steps(flat, offs, 5, len(lists), LR)
        assert np.array_equal(bits(W5[t]), bits(one.get_weights())), t
        for (loss, acc), (a, b) in zip(ev, RANGES):
            lo, ac = one.lg_loss_acc(a, b)
            assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), (t, a, b, loss[t], lo)
        assert np.array_equal(bits(p[t]), bits(one.lg_predict_proba(idx))), t


@pytest.fixture(scope="module")
def small():
    """the first N_SMALL rows under all 128 planes: every topic's fp64 step (tests/logistic_ref.py) and its bound, computed once"""
    d = cases.data()
    nnz = int(d.row_ptr[N_SMALL])
    rp, col, val = d.row_ptr[:N_SMALL + 1], d.col[:nnz], d.val[:nnz]
    P = np.random.default_rng(5).choice(np.array([-1, 1], dtype=np.int8), size=(128, N_SMALL))
    lists = [np.random.default_rng(6 + n).integers(0, N_SMALL, size=n).astype(np.int32) for n in (100, 37, 1)]
    W0 = start_weights(d.dim + 1, 128)
    want = np.stack([ref.sync_step((rp, col, val, P[t]), W0[t], lists, LR, cases.LAM) for t in range(128)])
    bound = np.stack([lb.dw((rp, col, val, P[t]), W0[t], lists, LR, cases.LAM) for t in range(128)])
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:
        eng.load_csr(rp, col, val, P[0])
        yield eng, P, lists, W0, want, bound


@pytest.mark.parametrize("T", WIDE_TS)
def test_every_topic_against_the_fp64_reference(small, T):
    eng, P, lists, W0, want, bound = small                       # (no lane writes its neighbour's topic: ALL T topics)
    eng.lg_topics_set(P[:T], wide=True)
    eng.lg_topics_set_weights(W0[:T])
    eng.lg_topics_sync_step(lists, LR)
    err = np.abs(eng.lg_topics_get_weights().astype(np.float64) - want[:T])
    print("T = %d: max err/bound %.3f" % (T, float(np.max(err / bound[:T]))))
    assert np.all(err <= bound[:T])


@pytest.mark.parametrize("T", (5, 40, 128))
def test_hand_built_rows_bits(T):
    """test_gpu_logistic's rows (empty, 64 and 65 non-zeros, one crossing the head, saturation) and rows of 16 and 17: the walk's edges"""
    csr, w, n_shape, sat0 = _hand()
    rng = np.random.default_rng(T)
    more = [np.arange(300, 316), np.arange(400, 417)]
    row_ptr = np.concatenate([csr[0], csr[0][-1] + np.cumsum([len(r) for r in more])])
    col = np.concatenate([csr[1]] + more).astype(np.int32)
    val = np.concatenate([csr[2], rng.choice([-1.0, 1.0], size=33) * 2.0 ** rng.integers(-2, 3, size=33)]).astype(np.float32)
    label = np.concatenate([csr[3], [1, -1]]).astype(np.int8)
    n = len(label)                                               # (row lengths 0, 16, 17, 64, 65: the chunk and register edges)
    rest = rng.choice(np.array([-1, 1], dtype=np.int8), size=(T - 3, n))
    P = np.ascontiguousarray(np.vstack([label[None], -label[None], np.ones((1, n), np.int8), rest]), dtype=np.int8)
    lists = [np.arange(n_shape, dtype=np.int32), np.arange(n_shape, n, dtype=np.int32)]
    W0 = np.stack([np.roll(w, t) if t >= 3 else w for t in range(T)])
    with dsgd_amd.Engine(HD, 0.0) as eng, dsgd_amd.Engine(HD, 0.0) as one:
        eng.load_csr(row_ptr, col, val, label)
        eng.lg_topics_set(P, wide=True)
        eng.lg_topics_set_weights(W0)
        eng.lg_topics_sync_step(lists, 0.25)
        W1 = eng.lg_topics_get_weights()
        loss, acc = eng.lg_topics_loss_acc(0, n)
        assert np.isfinite(W1).all() and np.isfinite(loss).all() and eng.column_ranks().max() >= 2048
        for t in (0, T // 2, T - 1):
            one.load_csr(row_ptr, col, val, P[t])
            one.set_weights(W0[t])
            one.lg_sync_step(lists, 0.25)
            assert np.array_equal(bits(W1[t]), bits(one.get_weights())), t
            lo, ac = one.lg_loss_acc(0, n)
            assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), t


def test_refusals_and_the_form_that_is_set(rig):
    wide, il, one, P, d = rig
    lib, ctx = wide._lib, wide._ctx
    wide.lg_topics_set(P[:40], wide=True)
    W0 = start_weights(d.dim + 1, 40)
    wide.lg_topics_set_weights(W0)
    bad = np.ascontiguousarray(np.vstack([P, P[:1]]))
    assert lib.dsgd_lg_topics_set_wide(ctx, 129, _lib.ptr(bad)) == _lib.EINVAL
    bad[39, 4095] = 0
    assert lib.dsgd_lg_topics_set_wide(ctx, 40, _lib.ptr(bad)) == _lib.EINVAL and b"plane 39, row 4095" in lib.dsgd_last_error()
    assert lib.dsgd_lg_topics_set_il(ctx, 33, _lib.ptr(P)) == _lib.EINVAL        # the other setters keep their limits
    assert wide.n_topics == 40 and np.array_equal(bits(wide.lg_topics_get_weights()), bits(W0))
    with pytest.raises(ValueError):
        wide.lg_topics_set(P[:4], interleaved=True, wide=True)
    lists = lists_of(2, 50, 3)
    got = []
    for form in ({"interleaved": True}, {"wide": True}, {"interleaved": True}):   # each setter replaces the other's topics
        wide.lg_topics_set(P[:9 if "wide" in form else 7], **form)
        assert wide.n_topics == (9 if "wide" in form else 7) and np.all(wide.lg_topics_get_weights() == 0.0)
        wide.lg_topics_sync_step(lists, LR)
        got.append(wide.lg_topics_get_weights())
    assert np.array_equal(bits(got[0]), bits(got[1][:7])) and np.array_equal(bits(got[0]), bits(got[2]))
    wide.lg_topics_set(None, wide=True)
    assert wide.n_topics == 0 and wide.lg_topics_wide_max == 128
