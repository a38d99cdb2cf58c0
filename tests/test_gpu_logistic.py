"""The logistic model on the GPU (include/dsgd.h "THE LOGISTIC MODEL"), through the C ABI via Engine, against the fp64 reference
tests/logistic_ref.py within the DERIVED bounds of tests/logistic_bound.py (whose worth tests/test_logistic_bound.py shows on
the CPU for exactly the lists stepped here).  Data: synth.generate(4096, seed=11) at D = 47,236; where exact edges are needed,
a hand-built CSR of a few dozen rows whose dots are exact in fp32.

Uncertain rows of the evaluation (0 < |d_ref| <= dz_i, whose class may go either way), counted on the CPU with logistic_ref
alone before any GPU run: weights(1.0) -- 0 of 4,096 rows on [0, 4096), 0 of 1,000 on [1500, 2500), 0 of 1 on [77, 78); the
test asserts <= 1 % of each range.
"""

import ctypes as C

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_cases as cases
import logistic_ref as ref
from dsgd_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine_of(csr, dim, lam):
    eng = dsgd_amd.Engine(dim, lam)
    eng.load_csr(*csr)
    return eng


@pytest.fixture(scope="module")
def synth():
    d = cases.data()
    with engine_of(cases.csr(d), d.dim, cases.LAM) as eng:
        yield eng, cases.csr(d), d


# ---- the hand-built CSR: exact dots (values +-2^k, weights 2^-m), every row shape, sentinel and saturation columns ----
HD = 4095                      # keys 0 .. 4095
UNRG = 64                      # LG_UNR * 16
SAT_W = [0.0, -0.0, 1.0, -1.0, 16.0, -16.0, 128.0, -128.0, 1024.0, -1024.0]


def _hand():
    rng = np.random.default_rng(21)
    rows = [[], [7], list(range(100, 100 + UNRG)), list(range(200, 200 + UNRG + 1)), list(range(0, 2100))]
    for _ in range(20):
        rows.append(sorted(rng.choice(2100, size=int(rng.integers(2, 90)), replace=False)))
    n_shape = len(rows)
    sat0 = 3000
    for i in range(2 * len(SAT_W)):      # one non-zero, value 1, on a private column: d = that column's weight
        rows.append([sat0 + i])
    row_ptr, col, val = [0], [], []
    for i, r in enumerate(rows):
        col += list(r)
        val += [1.0] * len(r) if i >= n_shape else list(rng.choice([-1.0, 1.0], size=len(r)) * 2.0 ** rng.integers(-2, 3, size=len(r)))
        row_ptr.append(len(col))
    label = rng.choice([-1, 1], size=len(rows)).astype(np.int8)
    for i in range(len(SAT_W)):          # every saturation weight under both labels
        label[n_shape + 2 * i], label[n_shape + 2 * i + 1] = 1, -1
    w = np.zeros(HD + 1, dtype=np.float32)
    w[:2100] = 2.0 ** -rng.integers(0, 4, size=2100)
    for i, v in enumerate(SAT_W):
        w[sat0 + 2 * i] = w[sat0 + 2 * i + 1] = v
    csr = (np.array(row_ptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val, dtype=np.float32), label)
    return csr, w, n_shape, sat0


@pytest.mark.parametrize("scale", [0.1, 10.0])
def test_gradient_of_one_worker_within_dg(synth, scale):
    eng, csr, d = synth
    w = cases.weights(scale)
    eng.set_weights(w)
    for name, idx in cases.gradient_lists().items():
        g, st = eng.lg_gradient(idx)
        want = ref.gradient(csr, w, idx, cases.LAM)
        bound = lb.dg(csr, w, idx, cases.LAM)
        err = np.abs(g.astype(np.float64) - want)
        print("gradient %s scale %g: max err/bound %.3f" % (name, scale, float(np.max(err / bound))))
        assert np.all(err <= bound), (name, float(np.max(err / bound)))
        assert st == {"n_samples": len(idx), "n_active": len(idx)}
    assert np.array_equal(bits(eng.get_weights()), bits(w))   # a gradient changes no weight
    g2, _ = eng.lg_gradient(cases.gradient_lists()["17"], w=w)     # the weights handed over: the same bits
    g1, _ = eng.lg_gradient(cases.gradient_lists()["17"])
    assert np.array_equal(bits(g1), bits(g2))


def test_row_shapes_exact(synth):
    csr, w, n_shape, sat0 = _hand()
    n = len(csr[3])
    with engine_of(csr, HD, 0.0) as eng:
        eng.set_weights(w)
        ranks = eng.column_ranks()
        # the long row makes ranks beyond the LDS head exist: a column at the head's last rank and one at the first beyond it
        k_last, k_first = int(np.where(ranks == 2047)[0][0]), int(np.where(ranks == 2048)[0][0])
        d_ref = ref.dots(csr, w)
        assert np.array_equal(d_ref, d_ref.astype(np.float32).astype(np.float64))   # every dot is exact in fp32
        p = eng.lg_predict_proba(np.arange(n))
        p_ref = ref.proba(d_ref).astype(np.float32)
        assert np.all(np.abs(p.view(np.int32).astype(np.int64) - p_ref.view(np.int32).astype(np.int64)) <= 1)
        loss, acc = eng.lg_loss_acc(0, n)
        loss_ref, acc_ref, tallies, _ = ref.loss_acc(csr, w, 0, n, 0.0)
        assert acc == acc_ref and abs(loss - loss_ref) <= lb.dloss(csr, w, 0, n, 0.0)
        assert tallies[1] == 5   # the empty row, and the two rows each under the weights +0 and -0: class 0
        for idx in ([0], [1], [2], [3], [4], list(range(n_shape)), list(range(n))):
            g, _ = eng.lg_gradient(np.array(idx, dtype=np.int32))
            want = ref.gradient(csr, w, idx, 0.0)
            bound = lb.dg(csr, w, idx, 0.0)
            assert np.all(np.abs(g.astype(np.float64) - want) <= bound), idx
            if 4 in idx:
                assert g[k_last] != 0.0 and g[k_first] != 0.0
        assert np.all(eng.lg_gradient(np.array([0], dtype=np.int32))[0] == 0.0)   # the empty row adds nothing


def test_saturation(synth):
    csr, w, n_shape, sat0 = _hand()
    n = len(csr[3])
    with engine_of(csr, HD, 0.0) as eng:
        eng.set_weights(w)
        for i, wv in enumerate(SAT_W):
            for j, y in enumerate((1, -1)):
                row, key = n_shape + 2 * i + j, sat0 + 2 * i + j
                g, _ = eng.lg_gradient(np.array([row], dtype=np.int32))   # lambda = 0, x = 1: g[key] is c itself
                p = eng.lg_predict_proba(np.array([row], dtype=np.int32))[0]
                assert np.count_nonzero(g) == (0 if g[key] == 0 else 1) and not np.isnan(g).any()
                if abs(wv) >= 110:
                    assert p == (1.0 if wv > 0 else 0.0)
                    assert g[key] == (0.0 if y * wv > 0 else -float(y)), (wv, y, g[key])
                elif wv == 0:
                    assert p == 0.5 and g[key] == -y / 2.0
                else:
                    assert abs(float(g[key]) - float(ref.coef(float(wv), float(y)))) <= 2.0 ** -24
        loss, acc = eng.lg_loss_acc(0, n)
        assert np.isfinite(loss) and abs(loss - ref.loss_acc(csr, w, 0, n, 0.0)[0]) <= lb.dloss(csr, w, 0, n, 0.0)
        eng.lg_sync_step([np.arange(n, dtype=np.int32)], 0.25)
        w1 = eng.get_weights()
        assert np.isfinite(w1).all() and np.isfinite(eng.lg_loss_acc(0, n)[0])


@pytest.mark.parametrize("name", list(cases.step_cases()))
def test_five_steps_from_zero_and_the_bit_equalities(synth, name):
    eng, csr, d = synth
    lists, lr = cases.step_cases()[name]
    w_ref = np.zeros(d.dim + 1)
    E = np.zeros_like(w_ref)
    eng.set_weights(np.zeros(d.dim + 1, dtype=np.float32))
    for t in range(5):
        w_before = eng.get_weights()
        st = eng.lg_sync_step(lists, lr)
        assert st["n_samples"] == st["n_active"] == sum(len(a) for a in lists)
        w_gpu = eng.get_weights()
        # one step from the GPU's own weights: the single step's bound, nothing carried
        one = np.abs(w_gpu.astype(np.float64) - ref.sync_step(csr, w_before, lists, lr, cases.LAM))
        assert np.all(one <= lb.dw(csr, w_before, lists, lr, cases.LAM)), t
        # ... and the trajectory of the reference alone, within the accumulated bound
        E = lb.dw(csr, w_ref, lists, lr, cases.LAM, E)
        w_ref = ref.sync_step(csr, w_ref, lists, lr, cases.LAM)
        err = np.abs(w_gpu.astype(np.float64) - w_ref)
        print("step %d of %s: max err/accumulated bound %.3f" % (t, name, float(np.max(err / E))))
        assert np.all(err <= E), t
    w5 = eng.get_weights()
    # the same five steps in ONE call
    flat = np.concatenate(lists * 5)
    offs = np.concatenate([[0], np.cumsum([len(a) for a in lists] * 5)])
    eng.set_weights(np.zeros(d.dim + 1, dtype=np.float32))
    eng.lg_sync_steps(flat, offs, 5, len(lists), lr)
    assert np.array_equal(bits(eng.get_weights()), bits(w5))
    # one more step: as it is, twice from the same weights, and with every list reversed
    eng.lg_sync_step(lists, lr)
    w6 = eng.get_weights()
    for variant in (lists, [a[::-1].copy() for a in lists]):
        eng.set_weights(w5)
        eng.lg_sync_step(variant, lr)
        assert np.array_equal(bits(eng.get_weights()), bits(w6))


def test_ranges_give_the_bits_of_lists(synth):
    eng, csr, d = synth
    w = cases.weights(1.0)
    for ranges in ([(0, 4096)], [(5, 1000), (1000, 1017), (4095, 4096)]):
        eng.set_weights(w)
        eng.lg_sync_step_ranges(ranges, 2.0 ** -6)
        got = eng.get_weights()
        eng.set_weights(w)
        st = eng.lg_sync_step([np.arange(a, b, dtype=np.int32) for a, b in ranges], 2.0 ** -6)
        assert np.array_equal(bits(eng.get_weights()), bits(got)) and st["n_samples"] == sum(b - a for a, b in ranges)


def test_range_edges_with_sentinel_columns():
    """Row i owns the private column 100 + i (value 1) beside two shared ones.  lambda = 0, zero weights: every c is -y / 2, so a
    row inside [a, b) leaves lr * y / 2 on its column (within dw) and a row just outside leaves exactly 0.0."""
    n = 48
    row_ptr = np.arange(0, 3 * n + 1, 3, dtype=np.int64)
    col = np.array([[1, 2, 100 + i] for i in range(n)], dtype=np.int32).ravel()
    val = np.array([[0.5, -0.25, 1.0] for _ in range(n)], dtype=np.float32).ravel()
    label = np.where(np.arange(n) % 3 == 0, -1, 1).astype(np.int8)
    csr = (row_ptr, col, val, label)
    w0 = np.zeros(256, dtype=np.float32)
    with engine_of(csr, 255, 0.0) as eng:
        for a, b in ((0, n), (1, n - 1), (16, 33), (17, 18)):
            eng.set_weights(w0)
            eng.lg_sync_step_ranges([(a, b)], 0.5)
            w1 = eng.get_weights()
            want = ref.sync_step(csr, w0, [np.arange(a, b)], 0.5, 0.0)
            assert np.all(np.abs(w1.astype(np.float64) - want) <= lb.dw(csr, w0, [np.arange(a, b)], 0.5, 0.0))
            for i in range(n):
                if a <= i < b:
                    assert w1[100 + i] == 0.25 * label[i]
                else:
                    assert w1[100 + i] == 0.0 and not np.signbit(w1[100 + i])


def test_evaluation(synth):
    eng, csr, d = synth
    w = cases.weights(1.0)
    eng.set_weights(w)
    dz = lb.dz(csr, w)
    d_all = ref.dots(csr, w)
    p_all = eng.lg_predict_proba(np.arange(cases.N))
    assert np.all(np.abs(p_all.astype(np.float64) - ref.proba(d_all)) <= lb.dc(dz) + 2.0 ** -25)
    idx = np.array([4095, 0, 77, 77, 1234], dtype=np.int32)
    assert np.array_equal(bits(eng.lg_predict_proba(idx)), bits(p_all[idx]))
    for a, b in ((0, cases.N), (1500, 2500), (77, 78)):
        loss, acc = eng.lg_loss_acc(a, b)
        loss_ref, acc_ref, tallies, dr = ref.loss_acc(csr, w, a, b, cases.LAM)
        unsure = (np.abs(dr) > 0) & (np.abs(dr) <= dz[a:b])
        assert np.count_nonzero(unsure) <= 0.01 * (b - a)
        print("loss_acc [%d, %d): |loss - ref| / dloss %.3f, unsure rows %d" % (a, b, abs(loss - loss_ref) / lb.dloss(csr, w, a, b, cases.LAM),
                                                                                 np.count_nonzero(unsure)))
        assert abs(loss - loss_ref) <= lb.dloss(csr, w, a, b, cases.LAM)
        assert abs(acc * (b - a) - tallies[0]) <= np.count_nonzero(unsure) + 1e-9
        # row for row: the class a probability names (p > 1/2: +1, p < 1/2: -1) is the reference's on every sure row
        cls = np.sign(p_all[a:b].astype(np.float64) - 0.5)
        sure = ~unsure & (np.abs(dr) > 1e-6)
        assert np.array_equal(cls[sure], np.sign(dr[sure]))
        assert (loss, acc) == eng.lg_loss_acc(a, b)              # the same call: the same bits
        assert (loss, acc) == eng.lg_loss_acc(a, b, w=w)         # |w|^2 taken afresh: the same bits


def test_refusals_leave_the_weights_and_the_context(synth):
    eng, csr, d = synth
    w = cases.weights(1.0)
    eng.set_weights(w)
    ok = np.arange(10, dtype=np.int32)
    g = np.zeros(d.dim + 1, dtype=np.float32)
    p = np.zeros(10, dtype=np.float32)
    lib, ctx = eng._lib, eng._ctx
    one64 = (C.c_int64 * 1)(10)
    lists1 = (C.c_void_p * 1)(_lib.ptr(ok))
    offs = np.array([0, 10], dtype=np.int64)
    z = C.c_int64
    lo, hi = (z * 1)(5), (z * 1)(5)
    calls = {
        _lib.EINVAL: [
            lambda: lib.dsgd_lg_gradient(ctx, None, _lib.ptr(ok), z(10), None, None),          # null g_out
            lambda: lib.dsgd_lg_gradient(ctx, None, None, z(10), _lib.ptr(g), None),           # null list
            lambda: lib.dsgd_lg_gradient(ctx, None, _lib.ptr(ok), z(0), _lib.ptr(g), None),    # n < 1
            lambda: lib.dsgd_lg_predict(ctx, None, _lib.ptr(ok), z(0), _lib.ptr(p)),
            lambda: lib.dsgd_lg_predict(ctx, None, _lib.ptr(ok), z(10), None),
            lambda: lib.dsgd_lg_sync_step(ctx, lists1, one64, 0, 0.5, None),                   # no workers
            lambda: lib.dsgd_lg_sync_step(ctx, lists1, (z * 1)(0), 1, 0.5, None),              # an empty worker list
            lambda: lib.dsgd_lg_sync_step(ctx, (C.c_void_p * 1)(None), one64, 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_steps(ctx, _lib.ptr(ok), z(10), _lib.ptr(np.array([1, 10], dtype=np.int64)), z(1), 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_steps(ctx, _lib.ptr(ok), z(10), _lib.ptr(np.array([0, 9], dtype=np.int64)), z(1), 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_steps(ctx, _lib.ptr(ok), z(10), _lib.ptr(np.array([0, 10, 10], dtype=np.int64)), z(1), 2, 0.5, None),
            lambda: lib.dsgd_lg_sync_steps(ctx, _lib.ptr(ok), z(10), _lib.ptr(np.array([0, 11, 10], dtype=np.int64)), z(1), 2, 0.5, None),
            lambda: lib.dsgd_lg_sync_steps(ctx, _lib.ptr(ok), z(10), None, z(1), 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_step_ranges(ctx, lo, hi, 1, 0.5, None),                   # an empty range
            lambda: lib.dsgd_lg_sync_step_ranges(ctx, (z * 1)(9), (z * 1)(3), 1, 0.5, None),   # a reversed one
            lambda: lib.dsgd_lg_sync_step_ranges(ctx, lo, hi, 0, 0.5, None),
            lambda: lib.dsgd_lg_loss_acc(ctx, None, z(7), z(7), C.byref(C.c_double()), C.byref(C.c_double())),
            lambda: lib.dsgd_lg_loss_acc(ctx, None, z(0), z(7), None, None),
        ],
        _lib.ERANGE: [
            lambda: lib.dsgd_lg_gradient(ctx, None, _lib.ptr(np.array([0, cases.N], dtype=np.int32)), z(2), _lib.ptr(g), None),
            lambda: lib.dsgd_lg_gradient(ctx, _lib.ptr(np.ones(d.dim + 1, dtype=np.float32)), _lib.ptr(np.array([-1], dtype=np.int32)), z(1), _lib.ptr(g), None),
            lambda: lib.dsgd_lg_predict(ctx, None, _lib.ptr(np.array([cases.N], dtype=np.int32)), z(1), _lib.ptr(p)),
            lambda: lib.dsgd_lg_sync_step(ctx, (C.c_void_p * 1)(_lib.ptr(np.array([3, -2], dtype=np.int32))), (z * 1)(2), 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_steps(ctx, _lib.ptr(np.array([1, 2, 99999], dtype=np.int32)), z(3), _lib.ptr(np.array([0, 3], dtype=np.int64)), z(1), 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_step_ranges(ctx, (z * 1)(0), (z * 1)(cases.N + 1), 1, 0.5, None),
            lambda: lib.dsgd_lg_sync_step_ranges(ctx, (z * 1)(-1), (z * 1)(5), 1, 0.5, None),
            lambda: lib.dsgd_lg_loss_acc(ctx, None, z(0), z(cases.N + 1), C.byref(C.c_double()), C.byref(C.c_double())),
        ],
    }
    for code, fs in calls.items():
        for i, f in enumerate(fs):
            assert f() == code, (code, i, lib.dsgd_last_error())
            assert np.array_equal(bits(eng.get_weights()), bits(w)), (code, i)
    assert offs is not None and eng.lg_sync_step([ok], 0.5)["n_samples"] == 10     # a valid step follows
    assert not np.array_equal(bits(eng.get_weights()), bits(w))


def test_refused_states():
    d = cases.data()
    ok = np.arange(10, dtype=np.int32)
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:                      # no data loaded
        for f in (lambda: eng.lg_gradient(ok), lambda: eng.lg_sync_step([ok], 0.5), lambda: eng.lg_sync_step_ranges([(0, 5)], 0.5),
                  lambda: eng.lg_sync_steps(ok, [0, 10], 1, 1, 0.5), lambda: eng.lg_loss_acc(0, 5), lambda: eng.lg_predict_proba(ok)):
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                f()
            assert ei.value.code == _lib.ESTATE
    with dsgd_amd.Engine(d.dim, cases.LAM, precision="fp64") as eng:    # an fp64 context
        eng.load_csr(*cases.csr(d))
        for f in (lambda: eng.lg_gradient(ok), lambda: eng.lg_sync_step([ok], 0.5), lambda: eng.lg_sync_step_ranges([(0, 5)], 0.5),
                  lambda: eng.lg_sync_steps(ok, [0, 10], 1, 1, 0.5), lambda: eng.lg_loss_acc(0, 5), lambda: eng.lg_predict_proba(ok)):
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                f()
            assert ei.value.code == _lib.EUNSUPPORTED
    with engine_of(cases.csr(d), d.dim, cases.LAM) as eng:              # a communicator attached; then the engine running
        w = cases.weights(1.0)
        eng.set_weights(w)
        eng.comm_init(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        with pytest.raises(dsgd_amd.DsgdError) as ei:
            eng.lg_sync_step([ok], 0.5)
        assert ei.value.code == _lib.EUNSUPPORTED
        eng.comm_destroy()
        assert np.array_equal(bits(eng.get_weights()), bits(w))
        eng.build_dim_sparsity(cases.N)
        eng.async_start([(0, cases.N)], batch=100, lr=0.5, max_updates=4_000_000, seed=1, positional_bug=True)
        try:
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                eng.lg_sync_step([ok], 0.5)
            assert ei.value.code == _lib.ESTATE
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                eng.lg_loss_acc(0, 5)
            assert ei.value.code == _lib.ESTATE
        finally:
            eng.async_stop()
        assert eng.lg_sync_step([ok], 0.5)["n_active"] == 10            # usable afterwards


def test_svm_steps_around_logistic_calls_are_those_of_a_context_without():
    d = cases.data()
    lists, lr = cases.step_cases()["3 workers 100/37/1"]
    w = cases.weights(1.0)
    out = []
    for with_logistic in (False, True):
        with engine_of(cases.csr(d), d.dim, cases.LAM) as eng:
            eng.build_dim_sparsity(cases.N)
            eng.set_weights(w)
            eng.sync_step(lists, lr)
            w1 = eng.get_weights()
            if with_logistic:
                eng.lg_sync_step(lists, lr)
                eng.lg_sync_step_ranges([(0, 1000)], 2.0 ** -6)
                eng.lg_gradient(lists[0])
                eng.lg_loss_acc(0, cases.N)
                eng.lg_predict_proba(lists[1])
                eng.set_weights(w1)
            st = eng.sync_step(lists, lr)
            st2 = eng.sync_step_ranges([(0, 2000), (2000, 4096)], lr * 100 / 2048)
            out.append((w1, eng.get_weights(), st, st2, eng.loss_acc(0, cases.N)))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    assert out[0][2:] == out[1][2:]
