"""Several topics on the GPU (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS): one-vs-rest over T label planes on the same
rows, one launch pair per step.  The oracle is the code that is already bounded: T single-model engines over the same CSR with
label = plane t.  Topic t's weights, losses, accuracies and probabilities must be their BITS; one direct comparison against
the fp64 reference tests/logistic_ref.py within tests/logistic_bound.py stands beside that.

Data: logistic_cases.data() (4,096 synthetic rows, D = 47,236) and the hand-built CSR of tests/test_gpu_logistic.py (exact dots,
every row shape, a 2,100-column row crossing LG_HOT, saturation weights).  Planes for T in {1, 3, 8}: the data's labels, all +1,
all -1, then seeded random ones -- the planes of T are the first T of those eight."""

import ctypes as C

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_cases as cases
import logistic_ref as ref
from dsgd_amd import _lib
from test_gpu_logistic import HD, _hand

pytestmark = pytest.mark.gpu

TS = (1, 3, 8)
LR = 0.5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def code_of(fn):
    try:
        fn()
    except dsgd_amd.DsgdError as e:
        return e.code
    return _lib.OK


def planes8(labels, seed=31):
    n = len(labels)
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.array([-1, 1], dtype=np.int8), size=(5, n))
    return np.ascontiguousarray(np.vstack([labels.astype(np.int8)[None], np.ones((1, n), np.int8), -np.ones((1, n), np.int8), rest]), dtype=np.int8)


def start_weights(dp, T):
    """a different non-zero start per topic, float32 [T, dp]: the shared cases' weights at logit scales 1, 0.1 and 10, rolled
    by the topic's number from the fourth on"""
    base = [cases.weights(s) for s in (1.0, 0.1, 10.0)]
    return np.stack([np.roll(base[t % 3], 7 * (t // 3)) for t in range(T)]).astype(np.float32)


@pytest.fixture(scope="module")
def rig():
    """the topics engine and the eight single-model engines, one per plane"""
    d = cases.data()
    P = planes8(d.label)
    eng = dsgd_amd.Engine(d.dim, cases.LAM)
    eng.load_csr(*cases.csr(d))
    oracle = []
    for t in range(8):
        e = dsgd_amd.Engine(d.dim, cases.LAM)
        e.load_csr(d.row_ptr, d.col, d.val, P[t])
        oracle.append(e)
    yield eng, oracle, P, d
    for e in [eng] + oracle:
        e.close()


def lists_of(K, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(cases.N)[:n].astype(np.int32) if n <= cases.N else rng.integers(0, cases.N, size=n).astype(np.int32) for _ in range(K)]


@pytest.mark.parametrize("T", TS)
def test_one_step_gives_every_topic_the_single_models_bits(rig, T):
    eng, oracle, P, d = rig
    W0 = start_weights(d.dim + 1, T)
    eng.lg_topics_set(P[:T])
    assert np.all(eng.lg_topics_get_weights() == 0.0)            # topic weights start at zero
    steps = [(K, lists_of(K, n, 100 * K + n)) for K in (1, 3) for n in (1, 17, 100, 1025)]
    rep = lists_of(1, 50, 77)[0]
    steps.append((2, [np.concatenate([rep, rep[:1], rep[:1]]), rep[::-1].copy()]))   # a row named three times, and again by the peer
    for K, lists in steps:
        eng.lg_topics_set_weights(W0)
        st = eng.lg_topics_sync_step(lists, LR)
        assert st["n_samples"] == st["n_active"] == sum(len(a) for a in lists)
        W1 = eng.lg_topics_get_weights()
        for t in range(T):
            oracle[t].set_weights(W0[t])
            oracle[t].lg_sync_step(lists, LR)
            assert np.array_equal(bits(W1[t]), bits(oracle[t].get_weights())), (T, K, [len(a) for a in lists], t)
    assert not np.array_equal(bits(W1[0]), bits(W0[0]))          # (the step moved something)


@pytest.mark.parametrize("T", TS)
def test_five_steps_in_one_call_equal_five_calls_and_the_oracle(rig, T):
    eng, oracle, P, d = rig
    lists = cases.step_cases()["3 workers 100/37/1"][0]
    flat = np.concatenate(lists * 5)
    offs = np.concatenate([[0], np.cumsum([len(a) for a in lists] * 5)])
    eng.lg_topics_set(P[:T])                                     # from zero weights
    for _ in range(5):
        eng.lg_topics_sync_step(lists, LR)
    W5 = eng.lg_topics_get_weights()
    eng.lg_topics_set_weights(np.zeros_like(W5))
    st = eng.lg_topics_sync_steps(flat, offs, 5, len(lists), LR)
    assert st["n_samples"] == len(flat)
    W5b = eng.lg_topics_get_weights()
    assert np.array_equal(bits(W5), bits(W5b))
    for t in range(T):
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
        assert np.isfinite(loss).all() and np.all(loss > 0.0)


@pytest.mark.parametrize("T", TS)
def test_evaluation_and_prediction_bits(rig, T):
    eng, oracle, P, d = rig
    W = start_weights(d.dim + 1, T)
    eng.lg_topics_set(P[:T])
    eng.lg_topics_set_weights(W)
    idx = np.random.default_rng(8).permutation(cases.N)[:300].astype(np.int32)
    idx[5] = idx[4]                                              # a row listed twice
    p = eng.lg_topics_predict(idx)
    assert p.shape == (T, 300)
    res = [eng.lg_topics_loss_acc(a, b) for a, b in ((0, 4096), (1500, 2500), (77, 78))]
    for t in range(T):
        oracle[t].set_weights(W[t])
        assert np.array_equal(bits(p[t]), bits(oracle[t].lg_predict_proba(idx))), t
        for (loss, acc), (a, b) in zip(res, ((0, 4096), (1500, 2500), (77, 78))):
            lo, ac = oracle[t].lg_loss_acc(a, b)
            assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), (a, b, t)


def test_hand_built_rows_bits():
    """an empty row, 1, 64 and 65 non-zeros, the 2,100-column row crossing LG_HOT, saturation weights under both labels (the
    planes y and -y), all +1: exact dots, bits of the single model again -- steps of one and of two workers, then evaluation
    and probabilities from the stepped weights"""
    csr, w, n_shape, sat0 = _hand()
    n = len(csr[3])
    P = np.ascontiguousarray(np.stack([csr[3], -csr[3], np.ones(n, np.int8)]), dtype=np.int8)
    everything = np.arange(n, dtype=np.int32)
    with dsgd_amd.Engine(HD, 0.0) as eng:
        eng.load_csr(*csr)
        eng.lg_topics_set(P)
        for lists in ([everything], [everything[:n_shape], everything[n_shape:]], [np.array([0], np.int32)], [np.array([4], np.int32)]):
            eng.lg_topics_set_weights(np.stack([w, w, w]))
            eng.lg_topics_sync_step(lists, 0.25)
            W1 = eng.lg_topics_get_weights()
            loss, acc = eng.lg_topics_loss_acc(0, n)
            p = eng.lg_topics_predict(everything)
            assert np.isfinite(W1).all() and np.isfinite(loss).all()
            for t in range(3):
                with dsgd_amd.Engine(HD, 0.0) as one:
                    one.load_csr(csr[0], csr[1], csr[2], P[t])
                    one.set_weights(w)
                    one.lg_sync_step(lists, 0.25)
                    assert np.array_equal(bits(W1[t]), bits(one.get_weights())), (len(lists), t)
                    lo, ac = one.lg_loss_acc(0, n)
                    assert bits64(loss[t]) == bits64(lo) and bits64(acc[t]) == bits64(ac), t
                    assert np.array_equal(bits(p[t]), bits(one.lg_predict_proba(everything))), t
        ranks = eng.column_ranks()
        assert ranks.max() >= 2048     # (columns beyond the LDS head exist; with T = 3 the head's split falls inside the long row)


def test_three_topics_against_the_fp64_reference(rig):
    eng, oracle, P, d = rig
    T = 3
    lists, lr = cases.step_cases()["3 workers 100/37/1"]
    w = cases.weights(1.0)
    eng.lg_topics_set(P[:T])
    eng.lg_topics_set_weights(np.stack([w] * T))
    eng.lg_topics_sync_step(lists, lr)
    W1 = eng.lg_topics_get_weights()
    loss, acc = eng.lg_topics_loss_acc(0, 4096)
    for t in range(T):
        csr_t = (d.row_ptr, d.col, d.val, P[t])
        err = np.abs(W1[t].astype(np.float64) - ref.sync_step(csr_t, w, lists, lr, cases.LAM))
        bound = lb.dw(csr_t, w, lists, lr, cases.LAM)
        print("topic %d: max err/bound %.3f" % (t, float(np.max(err / bound))))
        assert np.all(err <= bound), t
        loss_ref = ref.loss_acc(csr_t, W1[t], 0, 4096, cases.LAM)[0]
        assert abs(loss[t] - loss_ref) <= lb.dloss(csr_t, W1[t], 0, 4096, cases.LAM), t


def test_state_and_refusals(rig):
    eng, oracle, P, d = rig
    dp = d.dim + 1
    lists = cases.step_cases()["3 workers 100/37/1"][0]
    w_own = cases.weights(1.0)
    eng.set_weights(w_own)
    own_before = eng.lg_loss_acc(0, 4096)
    eng.lg_topics_set(P[:3])
    W0 = start_weights(dp, 3)
    eng.lg_topics_set_weights(W0)
    eng.lg_topics_sync_step(lists, LR)
    eng.lg_topics_loss_acc(0, 4096)
    eng.lg_topics_predict(lists[0])
    # the context's own weights and evaluation are untouched
    assert np.array_equal(bits(eng.get_weights()), bits(w_own))
    assert eng.lg_loss_acc(0, 4096) == own_before
    # ... and the other way round
    W1 = eng.lg_topics_get_weights()
    eng.lg_sync_step(lists, LR)
    eng.set_weights(w_own)
    assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(W1))

    # refusals: nothing written
    lib, ctx = eng._lib, eng._ctx
    bad = P[:3].copy()
    bad[2, 4095] = 0
    assert lib.dsgd_lg_topics_set(ctx, 3, _lib.ptr(bad)) == _lib.EINVAL and b"plane 2, row 4095" in lib.dsgd_last_error()
    bad[2, 4095] = 2
    assert lib.dsgd_lg_topics_set(ctx, 3, _lib.ptr(bad)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_set(ctx, 9, _lib.ptr(P)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_set(ctx, -1, _lib.ptr(P)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_set(ctx, 3, None) == _lib.EINVAL
    out = [np.array([1, 2, 4096], dtype=np.int32)]
    assert code_of(lambda: eng.lg_topics_sync_step(out, LR)) == _lib.ERANGE
    assert code_of(lambda: eng.lg_topics_sync_step([np.array([-1], dtype=np.int32)], LR)) == _lib.ERANGE
    assert code_of(lambda: eng.lg_topics_sync_step([np.zeros(0, dtype=np.int32)], LR)) == _lib.EINVAL
    assert code_of(lambda: eng.lg_topics_sync_steps(np.array([1, 4096], np.int32), np.array([0, 1, 2]), 2, 1, LR)) == _lib.ERANGE
    assert code_of(lambda: eng.lg_topics_predict(np.array([4096], dtype=np.int32))) == _lib.ERANGE
    assert code_of(lambda: eng.lg_topics_loss_acc(0, 4097)) == _lib.ERANGE
    assert code_of(lambda: eng.lg_topics_loss_acc(10, 10)) == _lib.EINVAL
    assert np.array_equal(bits(eng.lg_topics_get_weights()), bits(W1))      # the topics are as they were: three of them, the same weights
    assert eng.lg_topics_loss_acc(0, 4096)[0].shape == (3,)

    # topics set through the raw handle: Engine sizes its arrays by the library's own count
    assert lib.dsgd_lg_topics_set(ctx, 5, _lib.ptr(P)) == _lib.OK and eng.n_topics == 5
    assert eng.lg_topics_loss_acc(0, 4096)[0].shape == (5,) and eng.lg_topics_predict(lists[0]).shape == (5, len(lists[0]))
    assert eng.lg_topics_get_weights().shape == (5, dp)

    # T = 0 drops the topics; a new set works
    eng.lg_topics_set(P[:3])
    eng.lg_topics_set(None)
    assert eng.n_topics == 0
    assert code_of(lambda: eng.lg_topics_sync_step(lists, LR)) == _lib.ESTATE
    assert code_of(lambda: eng.lg_topics_loss_acc(0, 10)) == _lib.ESTATE
    assert lib.dsgd_lg_topics_get_weights(ctx, _lib.ptr(np.zeros(dp, np.float32))) == _lib.ESTATE
    eng.lg_topics_set(P[:2])
    assert np.all(eng.lg_topics_get_weights() == 0.0) and eng.lg_topics_get_weights().shape == (2, dp)
    eng.lg_topics_sync_step(lists, LR)
    oracle[1].set_weights(np.zeros(dp, dtype=np.float32))
    oracle[1].lg_sync_step(lists, LR)
    assert np.array_equal(bits(eng.lg_topics_get_weights()[1]), bits(oracle[1].get_weights()))

    # a load drops the topics
    eng.load_csr(*cases.csr(d))
    assert eng.n_topics == 0
    assert code_of(lambda: eng.lg_topics_predict(lists[0])) == _lib.ESTATE
    st = _lib.BatchStats()
    ptrs = (C.c_void_p * 1)(_lib.ptr(lists[0]))
    ns = (C.c_int64 * 1)(len(lists[0]))
    assert lib.dsgd_lg_topics_sync_step(ctx, ptrs, ns, 1, C.c_float(LR), C.byref(st)) == _lib.ESTATE
    eng.lg_topics_set(P[:1])
    eng.lg_topics_sync_step(lists, LR)
    oracle[0].set_weights(np.zeros(dp, dtype=np.float32))
    oracle[0].lg_sync_step(lists, LR)
    assert np.array_equal(bits(eng.lg_topics_get_weights()[0]), bits(oracle[0].get_weights()))
    eng.lg_topics_set(None)


def test_refusals_by_mode():
    d = cases.data()
    P = planes8(d.label)
    with dsgd_amd.Engine(d.dim, cases.LAM, precision="fp64") as e64:       # an fp64 context
        e64.load_csr(*cases.csr(d))
        assert e64._lib.dsgd_lg_topics_set(e64._ctx, 2, _lib.ptr(P)) == _lib.EUNSUPPORTED
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:                          # no data
        assert eng._lib.dsgd_lg_topics_set(eng._ctx, 2, _lib.ptr(P)) == _lib.ESTATE
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:                          # the lock-free engine running
        eng.load_csr(*cases.csr(d))
        eng.lg_topics_set(P[:2])
        eng.build_dim_sparsity(cases.N)
        eng.async_start([(0, cases.N)], batch=100, lr=0.5, max_updates=4000000, seed=1, positional_bug=True)
        try:
            assert code_of(lambda: eng.lg_topics_sync_step([np.arange(10, dtype=np.int32)], LR)) == _lib.ESTATE
            assert eng._lib.dsgd_lg_topics_set(eng._ctx, 2, _lib.ptr(P)) == _lib.ESTATE
        finally:
            eng.async_stop()
        assert np.all(eng.lg_topics_get_weights() == 0.0)                   # nothing was written; usable afterwards
        eng.lg_topics_sync_step([np.arange(10, dtype=np.int32)], LR)


def test_any_communicator_is_refused():
    d = cases.data()
    P = planes8(d.label)
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:                          # dsgd_comm_init_lg's too
        eng.load_csr(*cases.csr(d))
        eng.lg_topics_set(P[:2])
        eng.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        try:
            assert eng._lib.dsgd_lg_topics_set(eng._ctx, 2, _lib.ptr(P)) == _lib.EUNSUPPORTED
            assert code_of(lambda: eng.lg_topics_sync_step([np.arange(10, dtype=np.int32)], LR)) == _lib.EUNSUPPORTED
        finally:
            eng.comm_destroy()
        # the columns were ranked again under the communicator: the topics went with the ranking they were stored in
        assert code_of(lambda: eng.lg_topics_get_weights()) == _lib.ESTATE
        eng.lg_topics_set(P[:2])
        assert np.all(eng.lg_topics_get_weights() == 0.0)
