"""CPU-side checks of the fp64 asynchronous iteration (include/dsgd.h "THE FP64 MODE"): the new entry points are exported
and check their arguments without a device, the code object carries the new kernels within their register budget,
host.MasterAsync runs an fp64 backend on the zero-lag schedule (device plans in chunks, never the lock-free engine), the
wire worker hands Double updates to an fp64 backend, and the JNI shim's new natives."""

import ctypes as C
import re

import numpy as np
import pytest

import dsgd_amd
from dsgd_amd import _lib, host, wire
from oracle import oracle as orc
from oracle.hogwild_replay import hog_rows
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

NEW = ["dsgd_async_step_f64", "dsgd_update_grad_f64", "dsgd_async_plan_create", "dsgd_plan_run_async_f64"]


def test_new_entry_points_exported_and_reject_null_arguments_without_a_device():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    idx = np.zeros(4, dtype=np.int32)
    assert lib.dsgd_async_step_f64(None, _lib.ptr(idx), C.c_int64(4), C.c_double(0.5), None, None) == _lib.EINVAL
    assert lib.dsgd_update_grad_f64(None, None, None, C.c_int64(0)) == _lib.EINVAL
    rb = (C.c_int64 * 1)(0)
    re_ = (C.c_int64 * 1)(10)
    h = C.c_void_p()
    assert lib.dsgd_async_plan_create(None, rb, re_, C.c_int32(1), C.c_int32(1), C.c_uint64(0), C.c_int32(0), C.c_int64(0),
                                      C.c_int64(1), C.byref(h)) == _lib.EINVAL
    assert lib.dsgd_plan_run_async_f64(None, None, C.c_int64(0), C.c_int64(1), C.c_double(0.5)) == _lib.EINVAL
    assert b"null" in lib.dsgd_last_error()


def test_async_kernels_in_the_code_object_and_their_registers(tmp_path):
    """dsgd_cs64_async_kernel: 512 lanes (two waves per SIMD: 256 registers), no accumulation registers; its one-slot
    form (<= 512 rows per step: the reference's 100) spills nothing and uses no scratch; the lists and peer-update kernels
    are there, without scratch."""
    notes = _kernel_notes(tmp_path)
    steps = {k: v for k, v in notes.items() if "dsgd_cs64_async_kernel" in k}
    assert len(steps) == 2, sorted(steps)
    assert sum("dsgd_cs64_step_kernel" in k for k in notes) == 2
    for k, v in steps.items():
        assert int(re.search(r"ILi(\d+)E", k).group(1)) == 512
        assert v["vgpr_count"] <= 256 and v.get("agpr_count", 0) == 0, (k, v)
        if "ILi512ELi1ELi4E" in k:
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for name in ("dsgd_async_lists_kernel", "dsgd_update64_kernel", "dsgd_filter64_kernel"):
        found = [v for k, v in notes.items() if name in k]
        assert len(found) == 1, name
        assert found[0]["vgpr_spill_count"] == 0 and found[0]["private_segment_fixed_size"] == 0, name


def _data(n_rows=900, dim=60, seed=5):
    rng = np.random.default_rng(seed)
    row_ptr = [0]
    cols, vals = [], []
    for _ in range(n_rows):
        k = int(rng.integers(3, 9))
        c = np.sort(rng.choice(np.arange(1, dim + 1), size=k, replace=False))
        cols.append(c)
        vals.append(rng.random(k).astype(np.float32) + 0.05)
        row_ptr.append(row_ptr[-1] + k)
    label = np.where(rng.random(n_rows) < 0.5, -1, 1).astype(np.int8)
    return dim, np.asarray(row_ptr, np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(vals), label


class _OracleFp64Backend:
    """An fp64 backend whose plans are the oracle: async_plan draws hog_rows on the zero-lag schedule,
    plan_run_async applies orc_async_step; everything it is asked is recorded."""
    precision = "fp64"

    def __init__(self, o, n_train):
        self.o, self.n_train = o, n_train
        self.w = None
        self.chunks, self.runs, self.checks_at = [], [], []
        self.updates = 0
        self.async_start_calls = 0

    def set_weights(self, w):
        assert np.asarray(w).dtype == np.float64
        self.w = np.array(w, dtype=np.float64)

    def get_weights(self):
        return self.w.copy()

    def async_start(self, *a, **k):
        self.async_start_calls += 1
        raise AssertionError("the fp64 schedule never starts the lock-free engine")

    def loss_acc(self, lo, hi):
        self.checks_at.append(self.updates)
        loss, acc, counts, _ = self.o.loss_acc(self.w, lo, hi)
        return loss, acc, counts

    def async_plan(self, split, batch, seed, positional_bug, first_update, n_updates):
        self.chunks.append((first_update, n_updates))
        K = len(split)
        lists = [hog_rows(seed, u % K, u // K, split[u % K][0], split[u % K][1] - split[u % K][0], batch, positional_bug)
                 for u in range(first_update, first_update + n_updates)]
        return _Plan(first_update, lists)

    def plan_run_async(self, plan, b, e, lr):
        assert plan.first + b == self.updates, "updates run in order, each once"
        self.runs.append((plan.first + b, plan.first + e))
        for t in range(b, e):
            self.o.async_step(self.w, plan.lists[t], lr)
        self.updates = plan.first + e


class _Plan:
    def __init__(self, first, lists):
        self.first, self.lists, self.n_steps = first, lists, len(lists)
        self.destroyed = False

    def destroy(self):
        self.destroyed = True


@pytest.mark.parametrize("check_every,chunk", [(50, 120), (64, 64), (1000, 4096)])
def test_master_async_fp64_zero_lag_schedule(monkeypatch, check_every, chunk):
    dim, rp, col, val, label = _data()
    n_train, n_rows, K, batch, lr, seed, leak = 720, 900, 3, 10, 0.5, 11, 0.7
    o = orc.Oracle(dim, rp, col, val, label, 1e-3)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    b = _OracleFp64Backend(o, n_train)
    monkeypatch.setattr(host.MasterAsync, "FP64_CHUNK", chunk)
    m = host.MasterAsync(b, n_train, n_rows, K)
    state = m.fit(np.zeros(dim + 1), 1, batch, lr, lambda losses: False, check_every, leak, seed=seed, positional_bug=False)
    max_steps = n_train * 1
    assert b.async_start_calls == 0
    assert state.updates == max_steps
    # the chunks cover [0, max_steps) once, in order
    at = 0
    for first, n in b.chunks:
        assert first == at and n >= 1
        at += n
    assert at == max_steps
    assert [r for r in b.runs if r[0] == r[1]] == []
    assert b.runs[0][0] == 0 and b.runs[-1][1] == max_steps
    assert all(x[1] == y[0] for x, y in zip(b.runs, b.runs[1:]))
    # loss checks every check_every updates, and at the end
    want = list(range(0, max_steps, check_every)) + [max_steps]
    assert b.checks_at == want
    # the result: a plain replay of the same updates on the oracle
    w = np.zeros(dim + 1)
    split = [(r.start, r.stop) for r in host.split_vanilla(n_train, K)]
    losses, accs, best_l, best_w = [], [], float("inf"), w.copy()
    for u in range(max_steps + 1):
        if u % check_every == 0 or u == max_steps:
            l, a, _, _ = o.loss_acc(w, n_train, n_rows)
            pl = losses[0] if losses else l
            pa = accs[0] if accs else a
            l, a = leak * l + (1 - leak) * pl, leak * a + (1 - leak) * pa
            if best_l > l:
                best_l, best_w = l, w.copy()
            losses.insert(0, l)
            accs.insert(0, a)
        if u == max_steps:
            break
        k = u % K
        o.async_step(w, hog_rows(seed, k, u // K, split[k][0], split[k][1] - split[k][0], batch, False), lr)
    assert m.test_losses == losses and m.test_accs == accs
    assert state.loss == best_l
    assert np.array_equal(state.grad, best_w) and state.grad.dtype == np.float64


def test_master_async_fp64_stops_on_the_criterion():
    dim, rp, col, val, label = _data()
    o = orc.Oracle(dim, rp, col, val, label, 1e-3)
    o.set_dim_sparsity(o.dim_sparsity(720))
    b = _OracleFp64Backend(o, 720)
    m = host.MasterAsync(b, 720, 900, 2)
    state = m.fit(np.zeros(dim + 1), 1, 10, 0.5, lambda losses: len(losses) >= 3, 40, 1.0)
    assert b.checks_at == [0, 40, 80] and state.updates == 80 and b.async_start_calls == 0


class _RecordingBackend:
    def __init__(self, precision):
        self.precision = precision
        self.got = None

    def update_grad(self, keys, values):
        self.got = (np.asarray(keys), np.asarray(values))


@pytest.mark.parametrize("precision,dtype", [("fp64", np.float64), ("fp32", np.float32)])
def test_wire_update_grad_hands_doubles_to_an_fp64_backend(precision, dtype):
    pytest.importorskip("google.protobuf")
    M = wire.messages()
    b = _RecordingBackend(precision)
    worker = wire.SlaveWorker.__new__(wire.SlaveWorker)   # (the handler alone: no server)
    worker.backend, worker.asynchronous = b, True
    worker.metrics = host.Metrics()
    v = 0.1 + 1e-12   # not a float32
    req = M["GradUpdate"](gradUpdate=wire.to_sparse(np.asarray([0.0, v, 0.0, -3e-9]), 4))
    worker._rpc_UpdateGrad(req)
    keys, vals = b.got
    assert vals.dtype == dtype
    assert sorted(keys.tolist()) == [1, 3]
    got = dict(zip(keys.tolist(), vals.tolist()))
    if precision == "fp64":
        assert got[1] == v and got[3] == -3e-9
    else:
        assert got[1] == float(np.float32(v))


def test_jni_fp64_async_natives_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr

    lib = C.CDLL(shim_lib)
    step = getattr(lib, PREFIX + "asyncStepF64")
    step.restype = None
    step.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p]
    upd = getattr(lib, PREFIX + "updateGradF64")
    upd.restype = None
    upd.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    (i, _i), (d, _d) = jarr(np.arange(3, dtype=np.int32)), jarr(np.zeros(8, dtype=np.float64))
    for args in ((None, C.byref(d)), (C.byref(i), None)):   # null arrays: refused before any array is taken
        env = Env()
        step(C.byref(env), None, 0, args[0], 0.5, args[1])
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = Env()
    step(C.byref(env), None, 0, C.byref(i), 0.5, C.byref(d))   # null context -> DSGD_EINVAL
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == env.n_release == 2
    (k, _k), (v, _v), (v2, _v2) = jarr(np.arange(3, dtype=np.int32)), jarr(np.ones(3)), jarr(np.ones(2))
    for args in ((None, C.byref(v)), (C.byref(k), None)):
        env = Env()
        upd(C.byref(env), None, 0, args[0], args[1])
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = Env()
    upd(C.byref(env), None, 0, C.byref(k), C.byref(v2))   # length mismatch
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = Env()
    upd(C.byref(env), None, 0, C.byref(k), C.byref(v))     # null context -> DSGD_EINVAL
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == env.n_release == 2 and env.n_critical == 0
