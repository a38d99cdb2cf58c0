"""Softmax regression on the GPU (csrc/dsgd_lg_softmax.hpp) against a plain fp64 softmax within tests/softmax_bound.py at every
lane-group width, with padding classes, idle lanes (C = 33, 65), full groups without a padding class (C = 4, 32, 64) and the full 128; the forms in bits; the edges; the refusals."""

import numpy as np
import pytest

import dsgd_amd
import logistic_cases as cases
import softmax_bound as sm
from dsgd_amd import _lib
from test_gpu_logistic import HD, _hand
from test_gpu_logistic_topics import bits, code_of, start_weights

pytestmark = pytest.mark.gpu

CS, LR, N_SMALL, RANGES = (2, 3, 4, 5, 32, 33, 64, 65, 103, 128), 0.5, 600, ((0, 600), (150, 250), (77, 78))
flat = lambda lists, n: (np.concatenate(lists * n), np.concatenate([[0], np.cumsum([len(a) for a in lists] * n)]))   # n steps' flat lists


def classes_of(n, C, seed=17):   # fixed class bytes, every class present
    cls = np.random.default_rng(seed + C).integers(0, C, size=n).astype(np.uint8)
    cls[:C] = np.arange(C)
    return cls


@pytest.fixture(scope="module")
def small():
    """the first N_SMALL rows; on the CPU first: the reference, rounded to float, keeps its bound; padding classes let into S leave it"""
    d = cases.data()
    csr = (d.row_ptr[:N_SMALL + 1], d.col[:d.row_ptr[N_SMALL]], d.val[:d.row_ptr[N_SMALL]], np.ones(N_SMALL, np.int8))
    lists3 = [np.random.default_rng(6 + n).integers(0, N_SMALL, size=n).astype(np.int32) for n in (100, 37, 1)]
    cls, W0 = classes_of(N_SMALL, 5), start_weights(d.dim + 1, 5)
    want, bound = sm.sync_step(csr, W0, cls, lists3, LR, cases.LAM), sm.dw(csr, W0, cls, lists3, LR, cases.LAM)
    assert np.all(np.abs(want.astype(np.float32).astype(np.float64) - want) <= bound)
    assert np.any(np.abs(sm.sync_step(csr, W0, cls, lists3, LR, cases.LAM, pad=3) - want) > bound)
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:
        eng.load_csr(*csr)
        yield eng, csr, lists3, d.dim + 1


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("C", CS)
def test_against_fp64(small, C, K):
    eng, csr, lists3, dp = small
    lists, cls, W0 = lists3[:K], classes_of(N_SMALL, C), start_weights(dp, C)
    eng.lg_softmax_set(cls, C)
    assert eng.n_classes == C and eng.n_topics == C
    eng.lg_topics_set_weights(W0)
    dzm = sm.dz_max(csr, W0)
    for a, b in RANGES:
        (loss, acc), (want_loss, want_acc, Z) = eng.lg_softmax_loss_acc(a, b), sm.loss_acc(csr, W0, cls, a, b, cases.LAM)
        top = np.sort(Z, axis=1)
        assert np.all(top[:, -1] - top[:, -2] > 2.0 * dzm[a:b])                      # the reference's arg-max is decided on every row
        assert abs(loss - want_loss) <= sm.dloss(csr, W0, cls, a, b, cases.LAM) and acc == want_acc
    idx, Z = np.random.default_rng(8).integers(0, N_SMALL, size=300).astype(np.int32), sm.logits(csr, W0)
    got_cls, p = eng.lg_softmax_predict(idx, proba=True)
    assert np.array_equal(got_cls, np.argmax(Z, axis=1)[idx]) and np.array_equal(got_cls, eng.lg_softmax_predict(idx))
    assert np.all(np.abs(p.astype(np.float64) - sm.probs(Z)[0][idx].T) <= (sm.dc(dzm, C) + 2.0 ** -25)[idx][None, :])
    assert eng.lg_softmax_sync_step(lists, LR)["n_samples"] == sum(len(a) for a in lists)
    assert np.all(np.abs(eng.lg_topics_get_weights() - sm.sync_step(csr, W0, cls, lists, LR, cases.LAM)) <= sm.dw(csr, W0, cls, lists, LR, cases.LAM))


@pytest.fixture(scope="module")
def pair():
    d = cases.data()
    with dsgd_amd.Engine(d.dim, cases.LAM) as a, dsgd_amd.Engine(d.dim, cases.LAM) as b:
        yield a, b, d


@pytest.mark.parametrize("C, ranges, n", ((5, [(0, 4096)], 0), (103, [(0, 4096)], 0), (5, [(0, 100), (100, 137), (4000, 4001)], 0),
                                         (103, [(0, 100), (100, 137), (4000, 4001)], 0), (5, [(77, 78)], 0), (103, [(77, 78)], 0),
                                         (103, [(0, 30000), (30000, 50000)], 50000)))   # (50,000 rows: columns cut by run and share boundaries)
def test_forms_agree_in_bits(pair, C, ranges, n):
    a, b, d = pair
    d = dsgd_amd.synth.generate(n, seed=cases.SEED) if n else d
    cls, W0 = classes_of(len(d.label), C), start_weights(d.dim + 1, C)
    lists = [np.arange(lo, hi, dtype=np.int32) for lo, hi in ranges]
    lr, steps, out = 2.0 ** -10, 1 if n else 5, []                                    # (a worker's gradient is a SUM over its rows)
    for eng in (a, b):
        eng.load_csr(d.row_ptr, d.col, d.val, d.label)
        eng.lg_softmax_set(cls, C)
        eng.lg_topics_set_weights(W0)
    for _ in range(steps):
        a.lg_softmax_sync_step(lists, lr)
    b.lg_softmax_sync_steps(*flat(lists, steps), steps, len(lists), lr)
    five = a.lg_topics_get_weights()
    assert np.array_equal(bits(five), bits(b.lg_topics_get_weights())) and not np.array_equal(bits(five), bits(W0))
    for _ in range(2):                                                                # the same call twice from the same weights: the same bits
        a.lg_topics_set_weights(W0)
        assert a.lg_softmax_sync_steps_ranges(ranges, steps, lr)["n_samples"] == sum(len(x) for x in lists)
        out.append((a.lg_topics_get_weights(), a.lg_softmax_loss_acc(0, len(d.label))))
    assert np.array_equal(bits(out[0][0]), bits(five)) and np.array_equal(bits(out[1][0]), bits(five)) and out[0][1] == out[1][1]
    assert out[0][1] == b.lg_softmax_loss_acc(0, len(d.label))
    a.lg_softmax_sync_step(lists, lr)                                                 # a list step behind a ranges call equals the list engine's
    b.lg_softmax_sync_step(lists, lr)
    assert np.array_equal(bits(a.lg_topics_get_weights()), bits(b.lg_topics_get_weights()))


@pytest.mark.parametrize("C", (5, 40, 128))
def test_edges_on_hand_built_rows(C):
    csr, w, n_shape, sat0 = _hand()                                                  # row 0 is empty, row 1 = {column 7}, the last rows one private column each
    n = len(csr[3])
    cls = classes_of(n, C) if n >= C else (np.arange(n) % C).astype(np.uint8)
    cls[0], cls[1] = 0, 2
    W0 = np.stack([np.roll(w, 3 * c) for c in range(C)]).astype(np.float32)
    W0[:, 7] = -40.0 / csr[2][csr[0][1]]                                              # row 1 (a power of two on column 7): every logit -40 ...
    W0[[1, 2, 4], 7] *= -1.0                                                          # ... but classes 1, 2 and 4, which tie at +40
    W0[:, sat0], W0[0, sat0], W0[1, sat0] = 0.0, 80.0, -80.0                                            # row n_shape: logits +80, -80, 0, ...
    cls[n_shape] = 0
    with dsgd_amd.Engine(HD, 0.0) as eng:
        eng.load_csr(*csr)
        eng.lg_softmax_set(cls, C)
        eng.lg_topics_set_weights(W0)
        idx = np.array([0, 1, n_shape], dtype=np.int32)
        got, p = eng.lg_softmax_predict(idx, proba=True)
        want_p = sm.probs(sm.logits(csr, W0))[0][idx].T
        assert list(got) == [0, 1, 0]                                                 # the lowest class of the largest logit
        assert np.all(p[:, 0] == np.float32(1.0 / C)) and np.allclose(p, want_p.astype(np.float32), rtol=1e-6, atol=0.0)
        assert p[0, 2] == 1.0 and p[1, 2] == 0.0 and want_p[0, 2] == 1.0 and np.isfinite(p).all()   # exactly 1 and 0 where fp64 says so
        (l0, a0), (l1, a1), (l2, a2) = (eng.lg_softmax_loss_acc(r, r + 1) for r in idx)
        assert abs(l0 - np.log(C)) <= 4e-16 * np.log(C) and a0 == 1.0 and abs(l1 - np.log(3.0)) <= 1e-15 and a1 == 0.0 and np.isfinite(l2) and a2 == 1.0
        lists = [np.array([2, 2, 1, n_shape, 0], dtype=np.int32)]                      # a row listed twice counts twice
        eng.lg_softmax_sync_step(lists, 0.25)
        W1 = eng.lg_topics_get_weights()
        twice, once = (np.abs(W1 - sm.sync_step(csr, W0, cls, ls, 0.25, 0.0)) for ls in (lists, [lists[0][1:]]))
        assert np.isfinite(W1).all() and np.all(twice <= sm.dw(csr, W0, cls, lists, 0.25, 0.0)) and np.any(once > sm.dw(csr, W0, cls, lists, 0.25, 0.0))


def test_refusals(pair):
    a, b, d = pair
    cls, W0, lists = classes_of(cases.N, 9), start_weights(d.dim + 1, 9), [np.arange(50, dtype=np.int32), np.arange(50, 90, dtype=np.int32)]
    P = np.where(cls[None, :] == np.arange(9, dtype=np.uint8)[:, None], 1, -1).astype(np.int8)
    for eng in (a, b):
        eng.load_csr(*cases.csr(d))
    a.lg_softmax_set(cls, 9)
    a.lg_topics_set_weights(W0)
    b.lg_topics_set(P, wide=True)                                                     # the same planes WITHOUT the mark
    b.lg_topics_set_weights(W0)
    unchanged = lambda eng, C: eng.n_classes == C and eng.n_topics == 9 and np.array_equal(bits(eng.lg_topics_get_weights()), bits(W0))
    lib, ctx = a._lib, a._ctx
    for C in (1, 129, -1, 8):                                                         # C = 1, beyond 128, an entry >= C
        assert lib.dsgd_lg_softmax_set(ctx, C, _lib.ptr(cls)) == _lib.ERANGE and unchanged(a, 9), C
    assert lib.dsgd_lg_softmax_set(ctx, 9, None) == _lib.EINVAL and unchanged(a, 9)
    assert code_of(lambda: a.lg_softmax_sync_step([np.array([4096], np.int32)], LR)) == _lib.ERANGE
    assert code_of(lambda: a.lg_softmax_sync_steps_ranges([(5, 5)], 1, LR)) == _lib.EINVAL and unchanged(a, 9)
    calls = lambda e: (lambda: e.lg_softmax_sync_step(lists, LR), lambda: e.lg_softmax_sync_steps(*flat(lists, 1), 1, 2, LR),
                       lambda: e.lg_softmax_sync_steps_ranges([(0, 10)], 1, LR), lambda: e.lg_softmax_loss_acc(0, 10),
                       lambda: e.lg_softmax_predict(lists[0]))
    assert [code_of(c) for c in calls(b)] == [_lib.ESTATE] * 5 and unchanged(b, 0)    # topics without the mark
    a.build_dim_sparsity(cases.N)
    a.async_start([(0, cases.N)], batch=100, lr=0.5, max_updates=4000000, seed=1, positional_bug=True)   # the lock-free engine running
    try:
        assert [code_of(c) for c in calls(a)] == [_lib.EUNSUPPORTED] * 5
    finally:
        a.async_stop()
    assert unchanged(a, 9)
    with dsgd_amd.Engine(d.dim, cases.LAM, precision="fp64") as e64:                   # an fp64 context
        e64.load_csr(*cases.csr(d))
        assert e64._lib.dsgd_lg_softmax_set(e64._ctx, 9, _lib.ptr(cls)) == _lib.EUNSUPPORTED
    for eng in (a, b):                                                                # the topic calls keep serving the classes: the wide form's bits
        eng.lg_topics_sync_step(lists, LR)
    assert np.array_equal(bits(a.lg_topics_get_weights()), bits(b.lg_topics_get_weights())) and a.n_classes == 9
    a.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)                             # ANY communicator (the process's first loads the collective library)
    try:
        assert [code_of(c) for c in calls(a)] == [_lib.EUNSUPPORTED] * 5
    finally:
        a.comm_destroy()
    assert a.n_classes == 0 and a.n_topics == 0                                       # (the new ranking dropped the classes, as it drops any topics)
    a.lg_softmax_set(cls, 9)
    a.lg_topics_set(P[:4], wide=True)                                                 # any topics setter clears the mark
    assert a.n_classes == 0 and code_of(lambda: a.lg_softmax_loss_acc(0, 10)) == _lib.ESTATE
    a.lg_softmax_set(cls, 9)
    a.lg_softmax_set(None)                                                            # C = 0 frees the topics and the mark
    assert a.n_classes == 0 and a.n_topics == 0
