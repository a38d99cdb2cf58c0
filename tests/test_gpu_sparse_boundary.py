"""-m gpu: the reference's Sparse form at the boundary (include/dsgd.h "SPARSE VALUES"; csrc/dsgd_sparse.hpp).

Every sparse entry point is held to its dense twin: the pairs are the twin's vector compacted on the host -- keys
flatnonzero(|v| > 1e-20) ascending, values bit for bit -- with equal statistics, equal resident weights afterwards and the
twin's errors.  The compaction kernel takes tiles of 4,096 keys per workgroup, 4 per lane: 255 | 256 is a wave boundary,
4,095 | 4,096 a workgroup boundary."""

import ctypes as C

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, wire
from oracle import oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
EPS = 1e-20
N_ROWS, N_TRAIN = 20000, 16000
DIMS = [1, 63, 64, 65, 255, 256, 1023, 1024, 1025, 47236]
_DATA = {}


def _data():
    if "d" not in _DATA:
        _DATA["d"] = dsgd_amd.synth.generate(N_ROWS, seed=0)
    return _DATA["d"]


def _engine(precision="fp32"):
    d = _data()
    eng = dsgd_amd.Engine(d.dim, LAM, precision=precision)
    eng.load_csr(d.row_ptr, d.col, d.val, d.label)
    eng.build_dim_sparsity(N_TRAIN)
    return eng


def _dt(precision):
    return np.float64 if precision == "fp64" else np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _compact(v):
    k = np.flatnonzero(np.abs(v.astype(np.float64)) > EPS).astype(np.int32)
    return k, v[k]


def _check_pairs(keys, vals, dense):
    k, v = _compact(dense)
    assert keys.dtype == np.int32 and np.array_equal(keys, k)
    assert _same_bits(vals, v)


def _random_w(dim, dtype, seed=1, nnz=3000):
    rng = np.random.default_rng(seed)
    w = np.zeros(dim + 1, dtype=dtype)
    at = rng.choice(dim + 1, min(nnz, dim + 1), replace=False)
    w[at] = rng.normal(scale=0.1, size=len(at)).astype(dtype)
    return w


def _patterns(dim, dtype):
    dp = dim + 1
    rng = np.random.default_rng(dim)
    full = rng.normal(size=dp).astype(dtype)
    full[full == 0] = 1
    ends = np.zeros(dp, dtype=dtype)
    ends[0], ends[dim] = -1.5, 2.5
    sparse = np.zeros(dp, dtype=dtype)
    at = rng.random(dp) < 0.05
    sparse[at] = rng.normal(size=int(at.sum())).astype(dtype)
    return {"zero": np.zeros(dp, dtype=dtype), "full": full, "ends": ends, "5%": sparse}


# ---- 1. compaction and scatter-in at their edges, no data loaded ----
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("dim", DIMS)
def test_compaction_and_scatter_at_the_edges(dim, precision):
    dt = _dt(precision)
    with dsgd_amd.Engine(dim, LAM, precision=precision) as eng:
        for name, w in _patterns(dim, dt).items():
            eng.set_weights(w)
            keys, vals = eng.get_weights_sparse()
            assert vals.dtype == dt
            _check_pairs(keys, vals, w)
            assert len(keys) == {"zero": 0, "full": dim + 1}.get(name, len(keys))
            if name == "ends":
                assert keys.tolist() == sorted({0, dim})
            # ... and back in: the pairs in a shuffled order over weights that are not zero
            eng.set_weights(np.full(dim + 1, 7, dtype=dt))
            order = np.random.default_rng(3).permutation(len(keys))
            eng.set_weights_sparse(keys[order], vals[order])
            host_scatter = np.zeros(dim + 1, dtype=dt)
            host_scatter[keys] = vals
            assert _same_bits(eng.get_weights(), host_scatter), name


# ---- 2. the threshold ----
def test_threshold_fp64_across_wave_and_workgroup_boundaries():
    dim = 47236
    cases = [(1e-20, False), (np.nextafter(1e-20, 1), True), (-1e-19, True), (-0.0, False), (5e-324, False)]
    with dsgd_amd.Engine(dim, LAM, precision="fp64") as eng:
        for base in (255, 256, 4095, 4096):
            for shift in range(len(cases)):   # every value on either side of the boundary
                w = np.zeros(dim + 1)
                at = [base - 2 + (i + shift) % len(cases) for i in range(len(cases))]
                for k, (v, _) in zip(at, cases):
                    w[k] = v
                w[base + 3] = 1.0
                eng.set_weights(w)
                keys, vals = eng.get_weights_sparse()
                want = sorted([k for k, (_, kept) in zip(at, cases) if kept] + [base + 3])
                assert keys.tolist() == want
                assert _same_bits(vals, w[keys])


def test_threshold_fp32():
    dim = 47236
    lo = np.float32(1e-20)
    up = np.nextafter(lo, np.float32(1))
    assert float(lo) <= EPS < float(up)
    with dsgd_amd.Engine(dim, LAM) as eng:
        for base in (255, 4095):
            w = np.zeros(dim + 1, dtype=np.float32)
            w[base], w[base + 1], w[base + 2], w[base + 3] = lo, up, -lo, -up
            eng.set_weights(w)
            keys, vals = eng.get_weights_sparse()
            assert keys.tolist() == [base + 1, base + 3]
            assert _same_bits(vals, w[keys])


# ---- 3. gradient_sparse against gradient ----
def _lists():
    rng = np.random.default_rng(5)
    dup = rng.integers(0, N_TRAIN, size=100).astype(np.int32)
    dup[50:] = dup[:50]
    return [np.asarray([123], dtype=np.int32), dup, rng.permutation(N_TRAIN)[:4096].astype(np.int32)]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_gradient_sparse_against_the_dense_twin(precision):
    dt = _dt(precision)
    d = _data()
    w = _random_w(d.dim, dt)
    wk, wv = _compact(w)
    o = orc.Oracle(d.dim, d.row_ptr, d.col, d.val, d.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(N_TRAIN))
    with _engine(precision) as a, _engine(precision) as b:
        dense = b.gradient_f64 if precision == "fp64" else b.gradient
        for i, idx in enumerate(_lists()):
            a.set_weights(w)
            b.set_weights(w)
            for given in (False, True):   # the resident weights; then the same weights as pairs / dense
                keys, vals, st = a.gradient_sparse(idx, (wk, wv) if given else None)
                g, st_b = dense(idx, w if given else None)
                assert g.dtype == dt
                _check_pairs(keys, vals, g)
                assert st == st_b and st["n_samples"] == len(idx)
                assert _same_bits(a.get_weights(), b.get_weights())
            if i == 1:   # the oracle's support (orc_gradient)
                assert np.array_equal(keys, np.flatnonzero(o.gradient(w.astype(np.float64), idx)))
        # pairs that are NOT the resident weights replace them, as the dense w does
        w2 = _random_w(d.dim, dt, seed=2)
        keys, vals, _ = a.gradient_sparse(_lists()[1], _compact(w2))
        g, _ = dense(_lists()[1], w2)
        _check_pairs(keys, vals, g)
        assert _same_bits(a.get_weights(), w2) and _same_bits(b.get_weights(), w2)


def test_gradient_sparse_f64_with_slice_major_weights():
    """between plan runs the fp64 weights are slice-major on the device"""
    rng = np.random.default_rng(11)
    steps = [[rng.permutation(N_TRAIN)[:100].astype(np.int32)] for _ in range(3)]
    idx = _lists()[1]
    with _engine("fp64") as a, _engine("fp64") as b:
        for e in (a, b):
            p = e.plan(steps)
            e.plan_run(p, 0, len(steps), 0.5)
            p.destroy()
        keys, vals, st = a.gradient_sparse(idx)
        g, st_b = b.gradient_f64(idx)
        _check_pairs(keys, vals, g)
        assert st == st_b
        p = a.plan(steps)
        a.plan_run(p, 0, 1, 0.5)
        p.destroy()
        p = b.plan(steps)
        b.plan_run(p, 0, 1, 0.5)
        p.destroy()
        wk, wv = a.get_weights_sparse()
        _check_pairs(wk, wv, b.get_weights())


# ---- 4. the empty gradient ----
def test_empty_gradient():
    d = _data()
    row = 77
    lo, hi = d.row_ptr[row], d.row_ptr[row + 1]
    w = np.zeros(d.dim + 1, dtype=np.float32)
    w[d.col[lo:hi]] = -3.0 * float(d.label[row]) * d.val[lo:hi]   # y (x . w) = -3 |x|^2 < 0: the gate closes
    with _engine() as eng:
        keys, vals, st = eng.gradient_sparse(np.asarray([row], dtype=np.int32), _compact(w))
        assert len(keys) == 0 and len(vals) == 0
        assert st == {"n_samples": 1, "n_active": 0}
        g, _ = eng.gradient(np.asarray([row], dtype=np.int32))
        assert not g.any()


# ---- 5. async_step_sparse against async_step(want_delta=True) ----
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_async_step_sparse_against_the_dense_twin(precision):
    dt = _dt(precision)
    rng = np.random.default_rng(21)
    with _engine(precision) as a, _engine(precision) as b:
        w = _random_w(_data().dim, dt, seed=4)
        a.set_weights(w)
        b.set_weights(w)
        for _ in range(5):
            idx = rng.permutation(N_TRAIN)[:100].astype(np.int32)
            keys, vals, st = a.async_step_sparse(idx, 0.5)
            delta, st_b = b.async_step(idx, 0.5, want_delta=True)
            assert delta.dtype == dt and len(keys) > 0
            _check_pairs(keys, vals, delta)
            assert st == st_b
            assert _same_bits(a.get_weights(), b.get_weights())


# ---- 6. cap ----
def _raw_get(eng, cap, dt):
    k = np.full(max(cap, 1) + 2, -7, dtype=np.int32)
    v = np.full(max(cap, 1) + 2, 9.5, dtype=dt)
    nnz = C.c_int64(-1)
    fn = eng._lib.dsgd_get_weights_sparse_f64 if dt == np.float64 else eng._lib.dsgd_get_weights_sparse
    return fn(eng._ctx, _lib.ptr(k), _lib.ptr(v), C.c_int64(cap), C.byref(nnz)), nnz.value, k, v


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_cap_of_the_pure_forms(precision):
    dt = _dt(precision)
    idx = _lists()[1]
    with _engine(precision) as eng:
        w = _random_w(_data().dim, dt, seed=6)
        eng.set_weights(w)
        n_w = int(np.count_nonzero(w))
        rc, nnz, k, v = _raw_get(eng, n_w - 1, dt)
        assert rc == _lib.EINVAL and nnz == n_w
        assert (k == -7).all() and (v == 9.5).all()
        rc, nnz, k, v = _raw_get(eng, n_w, dt)
        assert rc == _lib.OK and nnz == n_w
        _check_pairs(k[:nnz], v[:nnz], w)
        assert (k[nnz:] == -7).all() and (v[nnz:] == 9.5).all()
        keys, vals, st = eng.gradient_sparse(idx)
        fn = eng._lib.dsgd_gradient_sparse_f64 if precision == "fp64" else eng._lib.dsgd_gradient_sparse
        for cap, want in ((len(keys) - 1, _lib.EINVAL), (len(keys), _lib.OK)):
            k = np.full(len(keys) + 2, -7, dtype=np.int32)
            v = np.full(len(keys) + 2, 9.5, dtype=dt)
            nnz = C.c_int64(-1)
            rc = fn(eng._ctx, None, None, C.c_int64(-1), _lib.ptr(idx), C.c_int64(len(idx)), _lib.ptr(k), _lib.ptr(v), C.c_int64(cap),
                    C.byref(nnz), None)
            assert rc == want and nnz.value == len(keys)
            if want == _lib.OK:
                assert np.array_equal(k[:len(keys)], keys) and _same_bits(v[:len(keys)], vals)
                assert (k[len(keys):] == -7).all()
            else:
                assert (k == -7).all() and (v == 9.5).all()
        assert _same_bits(eng.get_weights(), w)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_cap_of_the_async_form(precision):
    """the documented bound: min(D + 1, the listed rows' lengths summed)"""
    dt = _dt(precision)
    d = _data()
    idx = np.random.default_rng(8).permutation(N_TRAIN)[:100].astype(np.int32)
    bound = min(d.dim + 1, int(np.diff(d.row_ptr)[idx].sum()))
    assert 0 < bound < d.dim + 1   # (100 rows of 75 non-zeros on average)
    with _engine(precision) as a, _engine(precision) as b:
        w = _random_w(d.dim, dt, seed=9)
        a.set_weights(w)
        b.set_weights(w)
        k = np.full(d.dim + 1, -7, dtype=np.int32)
        v = np.full(d.dim + 1, 9.5, dtype=dt)
        nnz = C.c_int64(-1)
        st = _lib.BatchStats(-1, -1)

        def call(cap):
            if precision == "fp64":
                return a._lib.dsgd_async_step_sparse_f64(a._ctx, _lib.ptr(idx), C.c_int64(len(idx)), C.c_double(0.5), _lib.ptr(k), _lib.ptr(v),
                                                         C.c_int64(cap), C.byref(nnz), C.byref(st))
            return a._lib.dsgd_async_step_sparse(a._ctx, _lib.ptr(idx), C.c_int64(len(idx)), C.c_float(0.5), _lib.ptr(k), _lib.ptr(v),
                                                 C.c_int64(cap), C.byref(nnz), C.byref(st))

        assert call(bound - 1) == _lib.EINVAL
        assert (k == -7).all() and st.n_samples == -1      # nothing ran: no step counted
        assert _same_bits(a.get_weights(), w)
        good, idx = idx, np.asarray([0, N_ROWS], dtype=np.int32)   # a row outside the data: nothing runs either
        assert call(d.dim + 1) == _lib.ERANGE
        assert (k == -7).all() and _same_bits(a.get_weights(), w)
        idx = good
        for cap in (bound, d.dim + 1):
            assert call(cap) == _lib.OK
            delta, st_b = b.async_step(idx, 0.5, want_delta=True)
            _check_pairs(k[:nnz.value].copy(), v[:nnz.value].copy(), delta)
            assert (st.n_samples, st.n_active) == (st_b["n_samples"], st_b["n_active"])
            assert _same_bits(a.get_weights(), b.get_weights())


# ---- 7. errors change nothing ----
def _code(call):
    try:
        call()
    except _lib.DsgdError as e:
        return e.code
    return _lib.OK


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_errors_change_nothing(precision):
    dt = _dt(precision)
    d = _data()
    idx = _lists()[1]
    one = np.ones(2, dtype=dt)
    with _engine(precision) as eng:
        w = _random_w(d.dim, dt, seed=12)
        eng.set_weights(w)
        bad = [(lambda: eng.set_weights_sparse([5, 5], one), _lib.EINVAL),
               (lambda: eng.set_weights_sparse([3, -1], one), _lib.ERANGE),
               (lambda: eng.set_weights_sparse([3, d.dim + 1], one), _lib.ERANGE),
               (lambda: eng.gradient_sparse(idx, ([5, 5], one)), _lib.EINVAL),
               (lambda: eng.gradient_sparse(idx, ([-1, 5], one)), _lib.ERANGE),
               (lambda: eng.gradient_sparse(idx, ([d.dim + 1, 5], one)), _lib.ERANGE),
               (lambda: eng.gradient_sparse(np.zeros(0, dtype=np.int32)), _lib.EINVAL),
               (lambda: eng.async_step_sparse(np.zeros(0, dtype=np.int32), 0.5), _lib.EINVAL),
               (lambda: eng.gradient_sparse(np.asarray([0, N_ROWS], dtype=np.int32)), _lib.ERANGE),
               (lambda: eng.gradient_sparse(np.asarray([-1], dtype=np.int32)), _lib.ERANGE)]
        for call, want in bad:
            assert _code(call) == want
            assert _same_bits(eng.get_weights(), w)
        # the other precision's forms
        k = np.zeros(d.dim + 1, dtype=np.int32)
        nnz = C.c_int64(0)
        lib, ctx, n = eng._lib, eng._ctx, C.c_int64(len(idx))
        if precision == "fp64":
            v = np.zeros(d.dim + 1, dtype=np.float32)
            assert lib.dsgd_gradient_sparse(ctx, None, None, C.c_int64(-1), _lib.ptr(idx), n, _lib.ptr(k), _lib.ptr(v), C.c_int64(len(k)),
                                            C.byref(nnz), None) == _lib.EUNSUPPORTED
            assert lib.dsgd_async_step_sparse(ctx, _lib.ptr(idx), n, C.c_float(0.5), _lib.ptr(k), _lib.ptr(v), C.c_int64(len(k)),
                                              C.byref(nnz), None) == _lib.EUNSUPPORTED
            # (the float setter and getter serve an fp64 context as dsgd_set_weights / dsgd_get_weights do: promoted / rounded)
            assert lib.dsgd_get_weights_sparse(ctx, _lib.ptr(k), _lib.ptr(v), C.c_int64(len(k)), C.byref(nnz)) == _lib.OK
            _check_pairs(k[:nnz.value].copy(), v[:nnz.value].copy(), eng.get_weights_f32())
        else:
            v = np.zeros(d.dim + 1, dtype=np.float64)
            assert lib.dsgd_gradient_sparse_f64(ctx, None, None, C.c_int64(-1), _lib.ptr(idx), n, _lib.ptr(k), _lib.ptr(v), C.c_int64(len(k)),
                                                C.byref(nnz), None) == _lib.ESTATE
            assert lib.dsgd_async_step_sparse_f64(ctx, _lib.ptr(idx), n, C.c_double(0.5), _lib.ptr(k), _lib.ptr(v), C.c_int64(len(k)),
                                                  C.byref(nnz), None) == _lib.ESTATE
            assert lib.dsgd_get_weights_sparse_f64(ctx, _lib.ptr(k), _lib.ptr(v), C.c_int64(len(k)), C.byref(nnz)) == _lib.ESTATE
            assert lib.dsgd_set_weights_sparse_f64(ctx, _lib.ptr(k), _lib.ptr(v), C.c_int64(1)) == _lib.ESTATE
        assert _same_bits(eng.get_weights(), w)


def test_refused_while_the_lock_free_engine_runs():
    idx = _lists()[1]
    with _engine() as eng:
        w = _random_w(_data().dim, np.float32, seed=13)
        eng.set_weights(w)
        eng.async_start([(0, 8000), (8000, 16000)], batch=10, lr=0.5, max_updates=40, seed=1, positional_bug=False)
        try:
            twins = [(lambda: eng.set_weights_sparse(*_compact(w)), lambda: eng.set_weights(w)),
                     (lambda: eng.gradient_sparse(idx), lambda: eng.gradient(idx)),
                     (lambda: eng.async_step_sparse(idx, 0.5), lambda: eng.async_step(idx, 0.5))]
            for sparse, dense in twins:
                assert _code(sparse) == _code(dense) == _lib.ESTATE
            eng.get_weights_sparse()   # (allowed, as dsgd_get_weights is)
        finally:
            eng.async_wait()
        keys, vals = eng.get_weights_sparse()
        _check_pairs(keys, vals, eng.get_weights())


# ---- 8. the wire worker ----
class _DenseOnly:
    """the same engine without the sparse calls: the worker's dense path"""

    def __init__(self, eng):
        self._eng = eng
        self.dp, self.precision = eng.dp, eng.precision

    def gradient(self, idx, w=None):
        return self._eng.gradient(idx, w)


def test_wire_worker_serves_a_gradient_through_the_sparse_path():
    pytest.importorskip("grpc")
    d = _data()
    M = wire.messages()
    w = _random_w(d.dim, np.float64, seed=14)
    idx = _lists()[1]
    request = M["GradientRequest"](weights=wire.to_sparse(w, d.dim), samples=[int(i) for i in idx])
    with _engine() as eng:
        calls = []
        inner = eng.gradient_sparse
        eng.gradient_sparse = lambda *a: calls.append(1) or inner(*a)
        a = wire.SlaveWorker(eng, d.dim)
        b = wire.SlaveWorker(_DenseOnly(eng), d.dim)
        try:
            sparse_reply = a._rpc_Gradient(request)
            dense_reply = b._rpc_Gradient(request)
        finally:
            a.server.stop(grace=None)
            b.server.stop(grace=None)
        assert calls == [1]
        assert sparse_reply.gradUpdate.size == dense_reply.gradUpdate.size == d.dim
        got, want = dict(sparse_reply.gradUpdate.map), dict(dense_reply.gradUpdate.map)
        assert len(want) > 100 and got == want
