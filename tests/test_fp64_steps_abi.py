"""CPU-side checks of an epoch's steps in one call (include/dsgd.h "AN EPOCH'S STEPS IN ONE CALL", csrc/dsgd_rp64.hpp): the
symbol is declared and exported and checks its arguments without a device, the fused kernels are in the code object
without spills or scratch, the JNI native runs against the stub jni.h, the C++ mirror compiles and forwards, and
host.MasterSync hands an epoch's refused fp64 plan over in ONE call where the backend has sync_steps_f64."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dsgd_amd import _lib, host
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_argument_checks_without_a_device():
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert "int dsgd_sync_steps_f64(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets" in header
    assert "#define DSGD_ABI_VERSION 1" in header
    lib = _lib.load()
    assert "dsgd_sync_steps_f64" in _lib.SYMBOLS and hasattr(lib, "dsgd_sync_steps_f64")
    assert lib.dsgd_abi_version() == 1
    idx = np.zeros(4, dtype=np.int32)
    offs = np.asarray([0, 4], dtype=np.int64)

    def call(ctx, i, o, n_steps, k):
        return lib.dsgd_sync_steps_f64(ctx, _lib.ptr(i), C.c_int64(4), _lib.ptr(o), C.c_int64(n_steps), C.c_int32(k), C.c_double(0.5), None, None)

    # no context exists without a device: every combination of null and invalid arguments comes back DSGD_EINVAL with the null
    # context (whichever check answers first; the checks on a live context are tests/test_gpu_fp64_steps.py's refusals)
    for ctx_args in ((idx, offs, 1, 1), (None, offs, 1, 1), (idx, None, 1, 1), (idx, offs, 0, 1), (idx, offs, -3, 1), (idx, offs, 1, 0),
                     (None, None, 0, 0)):
        assert call(None, *ctx_args) == _lib.EINVAL
        assert lib.dsgd_last_error()


def test_fused_step_kernels_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    for name, lds in (("dsgd_rp64_step_kernel", 8 * 1024), ("dsgd_rp64v_step_kernel", 16 * 1024)):
        found = {k: v for k, v in notes.items() if name in k}
        assert len(found) == 1, name
        v = next(iter(found.values()))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert lds <= v["group_segment_fixed_size"] <= lds + 64, (name, v)   # the hot ranks' words + the body's few scalars
    # the existing kernels: no new instantiation
    assert sum("dsgd_rp64_grad_kernel" in k for k in notes) == 1 and sum("dsgd_rp64v_grad_kernel" in k for k in notes) == 1
    assert sum("dsgd_rp64_finish_kernel" in k for k in notes) == 2 and sum("dsgd_rp64v_finish_kernel" in k for k in notes) == 3


def test_jni_native_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr, scala_natives, shim_signatures

    assert scala_natives()["syncStepsF64"] == (["Long", "Array[Int]", "Array[Long]", "Int", "Double", "Array[Long]"], "Long")
    assert shim_signatures()["syncStepsF64"][0][2:] == ["jlong", "jintArray", "jlongArray", "jint", "jdouble", "jlongArray"]
    patch = open(os.path.join(ROOT, "scala", "patch", "dsgd-hip-backend.diff")).read()
    assert "+  @native def syncStepsF64(" in patch
    lib = C.CDLL(shim_lib)
    fn = getattr(lib, PREFIX + "syncStepsF64")
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
    IAE = b"java/lang/IllegalArgumentException"
    (i, _i), (o, _o), (o5, _o5), (a2, _a2), (a3, _a3) = (jarr(np.arange(6, dtype=np.int32)), jarr(np.asarray([0, 1, 2, 3, 6], np.int64)),
                                                         jarr(np.asarray([0, 1, 2, 3, 5, 6], np.int64)), jarr(np.zeros(2, np.int64)),
                                                         jarr(np.zeros(3, np.int64)))
    # refused before any array is taken: null arrays, offsets that are not nSteps * nWorkers + 1, activeOut of another length
    for args in ((None, C.byref(o), 2, None), (C.byref(i), None, 2, None), (C.byref(i), C.byref(o5), 2, None), (C.byref(i), C.byref(o), 0, None),
                 (C.byref(i), C.byref(o), 2, C.byref(a3))):
        env = Env()
        assert fn(C.byref(env), None, 0, args[0], args[1], args[2], 0.5, args[3]) == 0
        assert env.thrown_class == IAE and env.n_get == 0
    # a null context: DSGD_EINVAL from the library, every array taken is given back
    for act, n in ((None, 2), (C.byref(a2), 3)):
        env = Env()
        assert fn(C.byref(env), None, 0, C.byref(i), C.byref(o), 2, 0.5, act) == 0
        assert env.thrown_class == IAE and env.n_get == env.n_release == n and env.n_critical == 0


def test_the_cpp_mirror_compiles_and_forwards(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text(r'''
#include "dsgd.hpp"
#include <cstdio>
// stand-ins for the library: the mirror's call must arrive with the flat lists as they are
static const int32_t* g_idx; static int64_t g_n_idx, g_n_steps; static const int64_t* g_offs; static int32_t g_k; static double g_lr;
extern "C" {
int dsgd_create(const dsgd_config*, dsgd_ctx** out) { *out = reinterpret_cast<dsgd_ctx*>(16); return 0; }
int dsgd_destroy(dsgd_ctx*) { return 0; }
const char* dsgd_last_error(void) { return "stub"; }
int dsgd_sync_steps_f64(dsgd_ctx*, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers, double lr,
                        int64_t* active, dsgd_batch_stats* st) {
  g_idx = idx; g_n_idx = n_idx; g_offs = offsets; g_n_steps = n_steps; g_k = n_workers; g_lr = lr;
  for (int64_t t = 0; active && t < n_steps; ++t) active[t] = 10 + t;
  st->n_samples = n_idx; st->n_active = 21;
  return 0;
}
}
int main() {
  dsgd::SparseSVM m(1e-5, 10, 0, DSGD_F_FP64);
  std::vector<int32_t> idx = {4, 5, 6, 7, 8, 9};
  std::vector<int64_t> offs = {0, 1, 3, 4, 6};
  std::vector<int64_t> act;
  const dsgd_batch_stats st = m.syncStepsF64(idx, offs, 2, 0.25, &act);
  bool ok = g_idx == idx.data() && g_n_idx == 6 && g_offs == offs.data() && g_n_steps == 2 && g_k == 2 && g_lr == 0.25;
  ok = ok && st.n_samples == 6 && st.n_active == 21 && act.size() == 2 && act[0] == 10 && act[1] == 11;
  bool threw = false;
  try { m.syncStepsF64(idx, offs, 3, 0.25); } catch (const std::exception&) { threw = true; }   // 4 lists are not n * 3
  std::printf("%d %d\n", ok ? 1 : 0, threw ? 1 : 0);
  return ok && threw ? 0 : 1;
}
''')
    exe = tmp_path / "mirror"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["1", "1"]


class _Unsupported(RuntimeError):
    code = _lib.EUNSUPPORTED


class _Fp64Backend:
    """An fp64 backend whose plans are refused; per-step calls only"""
    precision = "fp64"

    def __init__(self, dp):
        self.dp, self.steps, self.batched = dp, [], []

    def set_weights(self, w):
        self.w = np.asarray(w, dtype=np.float64)

    def get_weights(self):
        return self.w

    def plan_flat(self, idx, offsets, n_steps, n_workers):
        raise _Unsupported("fp64 plans host at most 4 workers per step")

    def sync_step_f64(self, lists, lr):
        self.steps.append(([np.array(a, copy=True) for a in lists], lr))
        return {"n_samples": sum(len(a) for a in lists), "n_active": 0}

    def synchronize(self):
        return {"n_samples": 0, "n_active": 0}

    def loss_acc(self, lo, hi):
        return 1.0, 0.5, [0, 0, 0]


class _BatchedBackend(_Fp64Backend):
    def sync_steps_f64(self, idx, offsets, n_steps, n_workers, lr, per_step=False):
        self.batched.append((np.array(idx, copy=True), np.array(offsets, copy=True), n_steps, n_workers, lr))
        return {"n_samples": len(idx), "n_active": 0}


class _CommBackend(_BatchedBackend):
    def sync_steps_f64(self, *a, **kw):
        super().sync_steps_f64(*a, **kw)
        raise _Unsupported("a communicator is attached")


def _fit(b, k=5, batch=7, epochs=2):
    m = host.MasterSync(b, 60, 75, node_count=k, rnd=host.JavaRandom(0), plans=True)
    m.device_lists = False
    m.fit(np.zeros(b.dp), epochs, batch, 0.25, lambda losses: False)
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(60, k)
    want = [host.epoch_lists(rnd, split, max(len(r) for r in split), batch) for _ in range(epochs)]
    assert m.rnd.seed == rnd.seed
    return m, want


def _per_step(want, k):
    return [[idx[offs[s * k + j]:offs[s * k + j + 1]] for j in range(k)] for idx, offs, n_steps in want for s in range(n_steps)]


def test_master_sync_hands_an_epoch_over_in_one_call(monkeypatch):
    monkeypatch.setenv("DSGD_F64_STEPS", "1")
    b = _BatchedBackend(11)
    m, want = _fit(b)
    assert len(b.batched) == 2 and not b.steps   # exactly one call per epoch, with the epoch's flat lists
    for (idx, offs, n_steps, k, lr), (w_idx, w_offs, w_steps) in zip(b.batched, want):
        assert (n_steps, k, lr) == (w_steps, 5, 0.25)
        assert np.array_equal(idx, w_idx) and np.array_equal(offs, w_offs)
    assert m.steps_run == sum(w[2] for w in want)
    assert len(m.metrics.histograms["master.sync.batch.duration"]) == m.steps_run


def _assert_per_step(b, want, k=5):
    steps = _per_step(want, k)
    assert len(b.steps) == len(steps)
    for (got, lr), lists in zip(b.steps, steps):
        assert lr == 0.25 and len(got) == k and all(np.array_equal(a, e) for a, e in zip(got, lists))


def test_master_sync_keeps_the_loop_where_the_call_is_missing_refused_or_switched_off(monkeypatch):
    monkeypatch.setenv("DSGD_F64_STEPS", "1")
    b = _Fp64Backend(11)              # no sync_steps_f64: today's loop
    _, want = _fit(b)
    _assert_per_step(b, want)
    c = _CommBackend(11)              # code -7 (a communicator): tried once per epoch, then the loop on the same lists
    _, want = _fit(c)
    assert len(c.batched) == 2
    _assert_per_step(c, want)
    monkeypatch.setenv("DSGD_F64_STEPS", "0")
    d = _BatchedBackend(11)           # the knob: the loop although the backend has the call
    _, want = _fit(d)
    assert not d.batched
    _assert_per_step(d, want)


def test_an_epoch_without_a_step_makes_no_call(monkeypatch):
    """lists with n_steps == 0 (a worker's slice empty from the first batch): the loop does nothing, and so does the batched form --
    fit then raises the reference's error instead of the library's DSGD_EINVAL"""
    for knob in ("1", "0"):
        monkeypatch.setenv("DSGD_F64_STEPS", knob)
        b = _BatchedBackend(11)
        m = host.MasterSync(b, 60, 75, node_count=5, rnd=host.JavaRandom(0), plans=True)
        lists = {"idx": np.zeros(0, np.int32), "offsets": np.zeros(1, np.int64), "n_steps": 0}
        assert m._run_steps_f64(lists, 5, 0.25) == 0
        assert not b.batched and not b.steps


def test_other_errors_of_the_call_are_raised(monkeypatch):
    monkeypatch.setenv("DSGD_F64_STEPS", "1")

    class _Broken(_BatchedBackend):
        def sync_steps_f64(self, *a, **kw):
            raise _lib.DsgdError(_lib.ESTATE, "gave up")

    with pytest.raises(_lib.DsgdError):
        _fit(_Broken(11))
