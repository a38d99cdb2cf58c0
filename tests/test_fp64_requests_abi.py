"""CPU-side checks of the fp64 mode's request / response gradient and steps of any size (include/dsgd.h "THE FP64 MODE",
csrc/dsgd_rp64.hpp): the new entry points are exported and check their arguments without a device, the code object
carries the row-parallel fp64 kernels without spills or scratch, the JNI shim's new natives, host.MasterSync runs an
epoch whose plan an fp64 backend refuses through sync_step_f64 on the same lists, and the wire worker hands Double
weights to an fp64 backend and replies with its Double gradient."""

import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from dsgd_amd import _lib, host, wire
from oracle import oracle as orc
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

NEW = ["dsgd_gradient_f64", "dsgd_sync_step_f64", "dsgd_forward_f64"]


def test_new_entry_points_exported_and_reject_null_arguments_without_a_device():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    idx = np.zeros(4, dtype=np.int32)
    g = np.zeros(8)
    assert lib.dsgd_gradient_f64(None, None, _lib.ptr(idx), C.c_int64(4), _lib.ptr(g), None) == _lib.EINVAL
    assert b"null" in lib.dsgd_last_error()
    ptrs = (C.c_void_p * 1)(_lib.ptr(idx))
    ns = (C.c_int64 * 1)(4)
    assert lib.dsgd_sync_step_f64(None, ptrs, ns, C.c_int32(1), C.c_double(0.5), None) == _lib.EINVAL
    assert lib.dsgd_forward_f64(None, None, _lib.ptr(idx), C.c_int64(4), _lib.ptr(g)) == _lib.EINVAL
    assert b"null" in lib.dsgd_last_error()


def test_row_parallel_fp64_kernels_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    found = {k: v for k, v in notes.items() if "dsgd_rp64_" in k}
    assert sum("dsgd_rp64_grad_kernel" in k for k in found) == 1
    assert sum("dsgd_rp64_finish_kernel" in k for k in found) == 2   # the gradient and the step
    for k, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    assert sum("dsgd_cs64_step_kernel" in k for k in notes) == 2   # (no new instantiation of the plans' kernel)
    # the Double-value wrappers of the same bodies (csrc/dsgd_rp64.hpp, csrc/dsgd_cs64.hpp)
    twins = {k: v for k, v in notes.items()
             if any(n in k for n in ("dsgd_rp64v_grad_kernel", "dsgd_rp64v_finish_kernel", "dsgd_forward64v_kernel", "dsgd_eval64v_kernel"))}
    assert sum("dsgd_rp64v_grad_kernel" in k for k in twins) == 1
    assert sum("dsgd_rp64v_finish_kernel" in k for k in twins) == 3   # the gradient, the step and the asynchronous step
    assert sum("dsgd_forward64v_kernel" in k for k in twins) == 1 and sum("dsgd_eval64v_kernel" in k for k in twins) == 1
    for k, v in twins.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


def test_jni_fp64_request_natives_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr

    lib = C.CDLL(shim_lib)
    grad = getattr(lib, PREFIX + "gradientF64")
    grad.restype = C.c_int64
    grad.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    fwd = getattr(lib, PREFIX + "forwardF64")
    fwd.restype = None
    fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    (w, _w), (i, _i), (g, _g), (p, _p), (p2, _p2) = (jarr(np.zeros(8)), jarr(np.arange(3, dtype=np.int32)), jarr(np.zeros(8)),
                                                     jarr(np.zeros(3)), jarr(np.zeros(2)))
    for fn in (grad, fwd):
        out = g if fn is grad else p
        for args in ((None, C.byref(out)), (C.byref(i), None)):   # null arrays: refused before any array is taken
            env = Env()
            fn(C.byref(env), None, 0, C.byref(w), args[0], args[1])
            assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
        env = Env()
        fn(C.byref(env), None, 0, C.byref(w), C.byref(i), C.byref(out))   # null context -> DSGD_EINVAL, every array given back
        assert env.thrown_class == b"java/lang/IllegalArgumentException"
        assert env.n_get == env.n_release == 3 and env.n_critical == 0
        env = Env()
        fn(C.byref(env), None, 0, None, C.byref(i), C.byref(out))   # w = null: the resident weights (two arrays taken)
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == env.n_release == 2
    env = Env()
    fwd(C.byref(env), None, 0, None, C.byref(i), C.byref(p2))   # one prediction per sample
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    if not has_gpu():   # no device: the context cannot be created, loudly
        create = getattr(lib, PREFIX + "createF64")
        create.restype = C.c_int64
        create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32]
        env = Env()
        h = create(C.byref(env), None, 47236, 1e-5, 0)
        assert h == 0 and env.thrown_class == b"java/lang/RuntimeException"
        env = Env()
        grad(C.byref(env), None, h, C.byref(w), C.byref(i), C.byref(g))
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == env.n_release == 3


class _Unsupported(RuntimeError):
    code = _lib.EUNSUPPORTED


class _RefusingFp64Backend:
    """An fp64 backend whose plans are refused (as an fp64 engine refuses > 4 workers or > 1,024 rows per step)."""
    precision = "fp64"

    def __init__(self, dp):
        self.dp = dp
        self.steps, self.plans_tried, self.ranges_calls = [], 0, 0

    def set_weights(self, w):
        self.w = np.asarray(w, dtype=np.float64)

    def get_weights(self):
        return self.w

    def plan_from_seed(self, jstate, split, max_samples, batch_size):
        raise _Unsupported("device lists refused")

    def plan_flat(self, idx, offsets, n_steps, n_workers):
        self.plans_tried += 1
        raise _Unsupported("fp64 plans host at most 4 workers per step")

    def plan_run(self, plan, a, b, lr):
        raise AssertionError("no plan was made")

    def sync_step_f64(self, lists, lr):
        self.steps.append(([np.array(a, copy=True) for a in lists], lr))
        return {"n_samples": sum(len(a) for a in lists), "n_active": 0}

    def sync_step_ranges(self, ranges, lr):
        self.ranges_calls += 1

    def synchronize(self):
        return {"n_samples": 0, "n_active": 0}

    def loss_acc(self, lo, hi):
        return 1.0, 0.5, [0, 0, 0]


@pytest.mark.parametrize("k,batch,epochs", [(6, 7, 2), (3, 100, 2), (2, 3, 3)])
def test_master_sync_runs_a_refused_fp64_plan_through_sync_step_f64(k, batch, epochs):
    """Every step once, in order, with exactly the lists host.epoch_lists draws from the same JavaRandom(0) stream; the
    generator ends where the reference's ends; batch >= split stays off the range steps."""
    n_train, n_rows = 60, 75
    b = _RefusingFp64Backend(11)
    m = host.MasterSync(b, n_train, n_rows, node_count=k, rnd=host.JavaRandom(0))
    m.device_lists_min_draws = 0   # (the device form is tried first and refused)
    m.fit(np.zeros(11), epochs, batch, 0.25, lambda losses: False)
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(n_train, k)
    want = []
    for _ in range(epochs):
        idx, offs, n_steps = host.epoch_lists(rnd, split, max(len(r) for r in split), batch)
        want += [[idx[offs[s_ * k + j]:offs[s_ * k + j + 1]] for j in range(k)] for s_ in range(n_steps)]
    assert len(b.steps) == len(want) == m.steps_run
    for (got, lr), lists in zip(b.steps, want):
        assert lr == 0.25 and len(got) == k
        for a, e in zip(got, lists):
            assert np.array_equal(a, e)
    assert m.rnd.seed == rnd.seed
    assert b.ranges_calls == 0 and b.plans_tried >= epochs
    assert len(m.metrics.histograms["master.sync.batch.duration"]) == len(want)
    assert len(m.losses) == epochs


class _OracleGradFp64Backend:
    precision = "fp64"

    def __init__(self, o):
        self.o = o
        self.seen_w = []

    def gradient_f64(self, idx, w=None):
        self.seen_w.append(w)
        g = self.o.gradient(w, idx)
        return g, {"n_samples": len(idx), "n_active": self.o.last_stats["n_active"]}

    def forward_f64(self, idx, w=None):
        self.seen_w.append(w)
        return self.o.forward(w, idx)


def _small_oracle(dim=40, n_rows=200, seed=3):
    rng = np.random.default_rng(seed)
    row_ptr, cols, vals = [0], [], []
    for _ in range(n_rows):
        kk = int(rng.integers(3, 9))
        cols.append(np.sort(rng.choice(np.arange(1, dim + 1), size=kk, replace=False)))
        vals.append((rng.random(kk) + 0.05).astype(np.float32))
        row_ptr.append(row_ptr[-1] + kk)
    label = np.where(rng.random(n_rows) < 0.5, -1, 1).astype(np.int8)
    o = orc.Oracle(dim, np.asarray(row_ptr), np.concatenate(cols), np.concatenate(vals), label, 1e-3)
    o.set_dim_sparsity(o.dim_sparsity(n_rows))
    return o


def test_wire_gradient_and_forward_carry_doubles_for_an_fp64_backend():
    pytest.importorskip("google.protobuf")
    M = wire.messages()
    o = _small_oracle()
    dim = o.dim
    b = _OracleGradFp64Backend(o)
    worker = wire.SlaveWorker.__new__(wire.SlaveWorker)   # (the handler alone: no server)
    worker.backend, worker.size, worker.dp = b, dim, dim + 1
    worker.metrics = host.Metrics()
    rng = np.random.default_rng(1)
    w = np.zeros(dim + 1)
    keys = rng.choice(np.arange(dim + 1), size=25, replace=False)
    w[keys] = rng.normal(scale=0.1, size=25) + 1e-12   # Double values that no float32 holds
    assert not np.array_equal(w.astype(np.float32).astype(np.float64), w)
    idx = rng.integers(0, 200, size=60).astype(np.int32)
    rep = worker._rpc_Gradient(M["GradientRequest"](weights=wire.to_sparse(w, dim), samples=idx.tolist()))
    assert b.seen_w[-1].dtype == np.float64 and np.array_equal(b.seen_w[-1], w)
    g_ref = o.gradient(w, idx)
    got = dict(rep.gradUpdate.map)
    assert sorted(got) == np.flatnonzero(g_ref).tolist()   # zeros are not sent
    assert all(v != 0.0 for v in got.values())
    for kk, v in got.items():
        assert v == g_ref[kk]   # the Double values, no float32 rounding
    assert any(v != float(np.float32(v)) for v in got.values())
    rep = worker._rpc_Forward(M["ForwardRequest"](weights=wire.to_sparse(w, dim), samples=idx.tolist()))
    assert b.seen_w[-1].dtype == np.float64 and np.array_equal(b.seen_w[-1], w)
    assert list(rep.predictions) == o.forward(w, idx).tolist()


def test_from_sparse_keeps_float32_by_default():
    pytest.importorskip("google.protobuf")
    sp = wire.to_sparse(np.asarray([0.0, 0.1 + 1e-12, 0.0]), 2)
    assert wire.from_sparse(sp, 3).dtype == np.float32
    w64 = wire.from_sparse(sp, 3, np.float64)
    assert w64.dtype == np.float64 and w64[1] == 0.1 + 1e-12
