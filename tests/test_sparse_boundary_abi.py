"""Sparse values at the boundary (include/dsgd.h "SPARSE VALUES"), the parts that need no device: the new symbols and
their argument checks, the JNI natives through the stub JNIEnv, the wire module's pair conversions and its choice of the
backend's sparse calls, and the new kernels in the code object."""

import ctypes as C

import numpy as np
import pytest

from dsgd_amd import _lib, host, wire
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

NEW = ["dsgd_set_weights_sparse", "dsgd_set_weights_sparse_f64", "dsgd_get_weights_sparse", "dsgd_get_weights_sparse_f64",
       "dsgd_gradient_sparse", "dsgd_gradient_sparse_f64", "dsgd_async_step_sparse", "dsgd_async_step_sparse_f64"]


def test_new_entry_points_exported_and_reject_null_arguments_without_a_device():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    k = np.zeros(4, dtype=np.int32)
    nnz = C.c_int64(-5)
    n4 = C.c_int64(4)
    for sfx, v, lr in (("", np.zeros(4, dtype=np.float32), C.c_float(0.5)), ("_f64", np.zeros(4), C.c_double(0.5))):
        fn = lambda name: getattr(lib, name + sfx)
        # a null context
        assert fn("dsgd_set_weights_sparse")(None, _lib.ptr(k), _lib.ptr(v), n4) == _lib.EINVAL
        assert b"null" in lib.dsgd_last_error()
        assert fn("dsgd_get_weights_sparse")(None, _lib.ptr(k), _lib.ptr(v), n4, C.byref(nnz)) == _lib.EINVAL
        assert fn("dsgd_gradient_sparse")(None, None, None, C.c_int64(-1), _lib.ptr(k), n4, _lib.ptr(k), _lib.ptr(v), n4, C.byref(nnz),
                                          None) == _lib.EINVAL
        assert fn("dsgd_async_step_sparse")(None, _lib.ptr(k), n4, lr, _lib.ptr(k), _lib.ptr(v), n4, C.byref(nnz), None) == _lib.EINVAL
        assert nnz.value == -5
        # null arrays (with the null context: no context exists without a device)
        assert fn("dsgd_set_weights_sparse")(None, None, None, n4) == _lib.EINVAL
        assert fn("dsgd_get_weights_sparse")(None, None, None, n4, None) == _lib.EINVAL
        assert fn("dsgd_gradient_sparse")(None, None, None, n4, None, n4, None, None, n4, None, None) == _lib.EINVAL
        assert fn("dsgd_async_step_sparse")(None, None, n4, lr, None, None, n4, None, None) == _lib.EINVAL


def _natives(lib):
    from test_jni_shim import PREFIX

    def get(name, restype, argtypes):
        fn = getattr(lib, PREFIX + name)
        fn.restype = restype
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + argtypes
        return fn

    P = C.c_void_p
    out = {}
    for sfx, lr in (("", C.c_float), ("F64", C.c_double)):
        out["gradientSparse" + sfx] = get("gradientSparse" + sfx, C.c_int32, [P, P, P, P])
        out["asyncStepSparse" + sfx] = get("asyncStepSparse" + sfx, C.c_int32, [P, lr])
        out["getWeightsSparse" + sfx] = get("getWeightsSparse" + sfx, C.c_int32, [])
        out["setWeightsSparse" + sfx] = get("setWeightsSparse" + sfx, None, [P, P])
        out["takeSparse" + sfx] = get("takeSparse" + sfx, None, [P, P])
    return out


@pytest.mark.parametrize("sfx,dt", [("", np.float32), ("F64", np.float64)])
def test_jni_sparse_natives_through_the_stub_env(shim_lib, sfx, dt):
    from test_jni_shim import PREFIX, Env, jarr

    lib = C.CDLL(shim_lib)
    nat = _natives(lib)
    IAE = b"java/lang/IllegalArgumentException"
    (k, _k), (v, _v), (v3, _v3), (i, _i), (st, _st) = (jarr(np.arange(2, dtype=np.int32)), jarr(np.ones(2, dtype=dt)), jarr(np.ones(3, dtype=dt)),
                                                       jarr(np.arange(3, dtype=np.int32)), jarr(np.zeros(1, dtype=np.int64)))
    grad, step, getw, setw, take = (nat[n + sfx] for n in ("gradientSparse", "asyncStepSparse", "getWeightsSparse", "setWeightsSparse",
                                                            "takeSparse"))
    # null arrays and mismatched pairs: refused before any array is taken
    env = Env()
    assert grad(C.byref(env), None, 0, C.byref(k), C.byref(v), None, C.byref(st)) == -1
    assert env.thrown_class == IAE and env.n_get == 0
    for wk, wv in ((C.byref(k), None), (None, C.byref(v)), (C.byref(k), C.byref(v3))):
        env = Env()
        assert grad(C.byref(env), None, 0, wk, wv, C.byref(i), C.byref(st)) == -1
        assert env.thrown_class == IAE and env.n_get == 0
    env = Env()
    assert step(C.byref(env), None, 0, None, 0.5) == -1
    assert env.thrown_class == IAE and env.n_get == 0
    for a, b in ((None, C.byref(v)), (C.byref(k), None), (C.byref(k), C.byref(v3))):
        env = Env()
        setw(C.byref(env), None, 0, a, b)
        assert env.thrown_class == IAE and env.n_get == 0
        env = Env()
        take(C.byref(env), None, 0, a, b if b is None or a is None else C.byref(v))
        assert env.thrown_class == IAE and env.n_get == 0
    # a handle the shim did not create owns no scratch: IllegalArgumentException, nothing taken
    for call in (lambda e: grad(C.byref(e), None, 0, C.byref(k), C.byref(v), C.byref(i), C.byref(st)),
                 lambda e: step(C.byref(e), None, 0, C.byref(i), 0.5), lambda e: getw(C.byref(e), None, 0),
                 lambda e: take(C.byref(e), None, 0, C.byref(k), C.byref(v))):
        env = Env()
        call(env)
        assert env.thrown_class == IAE and env.n_get == 0 and env.n_critical == 0
    # the setter needs no scratch: a null context is DSGD_EINVAL from the library, both arrays taken and given back
    env = Env()
    setw(C.byref(env), None, 0, C.byref(k), C.byref(v))
    assert env.thrown_class == IAE and env.n_get == env.n_release == 2 and env.n_critical == 0
    from conftest import has_gpu

    if not has_gpu():   # no device: the context cannot be created, loudly
        create = getattr(lib, PREFIX + ("createF64" if sfx else "create"))
        create.restype = C.c_int64
        create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32]
        env = Env()
        assert create(C.byref(env), None, 47236, 1e-5, 0) == 0 and env.thrown_class == b"java/lang/RuntimeException"


@pytest.mark.gpu
@pytest.mark.parametrize("sfx,dt", [("", np.float32), ("F64", np.float64)])
def test_jni_sparse_natives_on_the_gpu(shim_lib, sfx, dt):
    """set -> get -> take through the natives: every array taken is released, the pairs are the ones set (ascending)"""
    from conftest import has_gpu
    from test_jni_shim import PREFIX, Env, jarr

    if not has_gpu():
        pytest.skip("no gfx950 device")
    lib = C.CDLL(shim_lib)
    nat = _natives(lib)
    create = getattr(lib, PREFIX + ("createF64" if sfx else "create"))
    create.restype = C.c_int64
    create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32]
    destroy = getattr(lib, PREFIX + "destroy")
    destroy.restype = None
    destroy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    env = Env()
    h = create(C.byref(env), None, 5000, 1e-5, 0)
    assert h != 0
    try:
        keys = np.asarray([4097, 3, 5000, 256, 0], dtype=np.int32)
        vals = np.asarray([1.5, -2.5, 3.25, 1e-21, -4.0], dtype=dt)   # (1e-21: at or under the threshold, not kept)
        (k, _k), (v, _v) = jarr(keys), jarr(vals)
        nat["setWeightsSparse" + sfx](C.byref(env), None, h, C.byref(k), C.byref(v))
        assert env.thrown_class == b"" and env.n_get == env.n_release == 2
        n = nat["getWeightsSparse" + sfx](C.byref(env), None, h)
        assert n == 4 and env.thrown_class == b""
        (ko, _ko), (vo, _vo) = jarr(np.zeros(n, dtype=np.int32)), jarr(np.zeros(n, dtype=dt))
        nat["takeSparse" + sfx](C.byref(env), None, h, C.byref(ko), C.byref(vo))
        assert env.thrown_class == b"" and env.n_critical == 0
        assert _ko.tolist() == [0, 3, 4097, 5000] and _vo.tolist() == [-4.0, -2.5, 1.5, 3.25]
        (kb, _kb) = jarr(np.zeros(n + 1, dtype=np.int32))
        nat["takeSparse" + sfx](C.byref(env), None, h, C.byref(kb), C.byref(vo))   # arrays of another length
        assert env.thrown_class == b"java/lang/IllegalArgumentException"
        env = Env()
        (i, _i) = jarr(np.arange(3, dtype=np.int32))
        assert nat["gradientSparse" + sfx](C.byref(env), None, h, None, None, C.byref(i), None) == -1   # no data loaded
        assert env.thrown_class == b"java/lang/RuntimeException" and env.n_get == env.n_release == 1
    finally:
        destroy(C.byref(env), None, h)


def test_pairs_round_trip_and_range_check():
    pytest.importorskip("google.protobuf")
    keys = np.asarray([7, 0, 3], dtype=np.int32)
    for dt, vals in ((np.float32, np.asarray([0.1, -2.0, 1e-19], dtype=np.float32)), (np.float64, np.asarray([0.1 + 1e-12, -2.0, 1e-19]))):
        sp = wire.sparse_from_pairs(keys, vals, 7)
        assert sp.size == 7 and dict(sp.map) == {int(k): float(v) for k, v in zip(keys, vals)}
        k2, v2 = wire.pairs_from_sparse(sp, 8, dt)
        assert k2.dtype == np.int32 and v2.dtype == dt
        order, back = np.argsort(keys), np.argsort(k2)
        assert np.array_equal(k2[back], keys[order]) and np.array_equal(v2[back], vals[order])
        # the same map as to_sparse builds from the dense vector
        dense = np.zeros(8, dtype=dt)
        dense[keys] = vals
        assert dict(wire.to_sparse(dense, 7).map) == dict(sp.map)
        assert np.array_equal(wire.from_sparse(sp, 8, dt)[k2], v2)
        with pytest.raises(IndexError):
            wire.pairs_from_sparse(sp, 7, dt)     # key 7 outside [0, 7)
    empty = wire.sparse_from_pairs(np.zeros(0, np.int32), np.zeros(0, np.float32), 7)
    assert len(empty.map) == 0 and empty.size == 7
    k0, v0 = wire.pairs_from_sparse(empty, 8)
    assert len(k0) == 0 and len(v0) == 0 and v0.dtype == np.float32
    bad = wire.messages()["Sparse"]()
    bad.map[-1] = 1.0
    with pytest.raises(IndexError):
        wire.pairs_from_sparse(bad, 8)


class _Dense:
    precision = "fp32"

    def __init__(self, dp):
        self.dp, self.calls = dp, []

    def gradient(self, idx, w=None):
        self.calls.append(("gradient", np.array(w, copy=True)))
        g = np.zeros(self.dp, dtype=np.float32)
        g[1], g[4] = 0.5, -0.25
        return g, {"n_samples": len(idx), "n_active": 1}

    def set_weights(self, w):
        self.calls.append(("set_weights", np.array(w, copy=True)))

    def async_step(self, idx, lr, want_delta=False):
        self.calls.append(("async_step", want_delta))
        raise RuntimeError("stop the loop")


class _Sparse(_Dense):
    def gradient_sparse(self, idx, w=None):
        self.calls.append(("gradient_sparse", w))
        return np.asarray([1, 4], dtype=np.int32), np.asarray([0.5, -0.25], dtype=np.float32), {"n_samples": len(idx), "n_active": 1}

    def set_weights_sparse(self, keys, vals):
        self.calls.append(("set_weights_sparse", (keys, vals)))

    def async_step_sparse(self, idx, lr):
        self.calls.append(("async_step_sparse", lr))
        raise RuntimeError("stop the loop")


def _worker(backend, dim, asynchronous=False):
    worker = wire.SlaveWorker.__new__(wire.SlaveWorker)   # (the handlers alone: no server)
    worker.backend, worker.size, worker.dp = backend, dim, dim + 1
    worker.metrics = host.Metrics()
    worker.asynchronous, worker.running_async = asynchronous, False
    worker.rnd = host.JavaRandom(0)
    worker.lock, worker.others, worker.master_stub = __import__("threading").Lock(), {}, None
    return worker


def test_wire_worker_uses_the_sparse_calls_when_the_backend_has_them():
    pytest.importorskip("google.protobuf")
    M = wire.messages()
    dim = 6
    w = np.asarray([0.0, 0.5, 0.0, 0.0, -1.5, 0.0, 2.0])
    req = M["GradientRequest"](weights=wire.to_sparse(w, dim), samples=[0, 1, 2])
    dense, sparse = _Dense(dim + 1), _Sparse(dim + 1)
    rep_d = _worker(dense, dim)._rpc_Gradient(req)
    rep_s = _worker(sparse, dim)._rpc_Gradient(req)
    assert [c[0] for c in dense.calls] == ["gradient"] and np.array_equal(dense.calls[0][1], w.astype(np.float32))
    assert [c[0] for c in sparse.calls] == ["gradient_sparse"]
    wk, wv = sparse.calls[0][1]
    assert wv.dtype == np.float32 and dict(zip(wk.tolist(), wv.tolist())) == {1: 0.5, 4: -1.5, 6: 2.0}
    assert dict(rep_s.gradUpdate.map) == dict(rep_d.gradUpdate.map) == {1: 0.5, 4: -0.25}
    assert rep_s.gradUpdate.size == rep_d.gradUpdate.size == dim
    with pytest.raises(ValueError):   # the empty batch fails on either path
        _worker(sparse, dim)._rpc_Gradient(M["GradientRequest"](weights=wire.to_sparse(w, dim), samples=[]))
    # startAsync: the weights go in as pairs, the iteration asks for a sparse delta
    start = M["StartAsyncRequest"](weights=wire.to_sparse(w, dim), samples=[0, 1, 2], batchSize=1, learningRate=0.5)
    for backend, names in ((_Dense(dim + 1), ["set_weights", "async_step"]), (_Sparse(dim + 1), ["set_weights_sparse", "async_step_sparse"])):
        wk_ = _worker(backend, dim, asynchronous=True)
        wk_._rpc_StartAsync(start)
        wk_._thread.join(timeout=10)
        assert [c[0] for c in backend.calls] == names
        assert isinstance(wk_._async_error, RuntimeError) and not wk_.running_async


def test_sparse_kernels_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    compact = {k: v for k, v in notes.items() if "dsgd_sparse_compact_kernel" in k}
    scatter = {k: v for k, v in notes.items() if "dsgd_sparse_scatter_kernel" in k}
    assert len(compact) == 4   # float, double, double -> float, and the fp32 gradient's regularising form
    assert len(scatter) == 3   # float, double, float -> double
    for k, v in {**compact, **scatter}.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    # the counts other tests pin are unchanged: no new instantiation of an existing kernel
    assert sum("dsgd_rp64_grad_kernel" in k for k in notes) == 1
    assert sum("dsgd_rp64_finish_kernel" in k for k in notes) == 2
    assert sum("dsgd_cs64_step_kernel" in k for k in notes) == 2
