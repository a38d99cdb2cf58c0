"""CPU-side checks of the fp64 mode's row-parallel plans (include/dsgd.h "THE FP64 MODE", ROW-PARALLEL PLANS;
csrc/dsgd_rp64.hpp): the three creators are declared and exported and check their arguments without a device, the JNI
natives run against the stub jni.h, the C++ mirror compiles and forwards, the new kernels are in the code object without
spills or scratch, and the host mirrors take the plans only behind DSGD_F64_RP_PLANS=1."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dsgd_amd import _lib, host
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CREATORS = ("dsgd_plan_create_rp64_n", "dsgd_plan_create_from_seed_rp64", "dsgd_async_plan_create_rp64")


def test_declared_exported_and_argument_checks_without_a_device():
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert "ROW-PARALLEL PLANS" in header
    lib = _lib.load()
    for name in CREATORS:
        assert "int %s(dsgd_ctx* ctx, " % name in header
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    idx = np.zeros(4, dtype=np.int32)
    offs = np.asarray([0, 4], dtype=np.int64)
    b, e = np.asarray([0], np.int64), np.asarray([10], np.int64)
    sentinel = 0x1234
    out = C.c_void_p(sentinel)
    state = C.c_uint64(77)
    n_steps, draws = C.c_int64(-1), C.c_int64(-1)
    # no context exists without a device: null and invalid arguments come back DSGD_EINVAL with the null context, whichever check
    # answers first, and nothing is written (the checks on a live context are tests/test_gpu_fp64_rp_plans.py's refusals)
    for i, o, steps, k, po in ((idx, offs, 1, 1, C.byref(out)), (None, offs, 1, 1, C.byref(out)), (idx, None, 1, 1, C.byref(out)),
                               (idx, offs, 0, 1, C.byref(out)), (idx, offs, 1, 0, C.byref(out)), (idx, offs, 1, 1, None)):
        assert lib.dsgd_plan_create_rp64_n(None, _lib.ptr(i), C.c_int64(4), _lib.ptr(o), C.c_int64(steps), C.c_int32(k), po) == _lib.EINVAL
        assert lib.dsgd_last_error()
    for sp, sb, se, k, batch, po in ((C.byref(state), b, e, 1, 5, C.byref(out)), (None, b, e, 1, 5, C.byref(out)), (C.byref(state), None, e, 1, 5, C.byref(out)),
                                     (C.byref(state), b, e, 0, 5, C.byref(out)), (C.byref(state), b, e, 1, 0, C.byref(out)), (C.byref(state), b, e, 1, 5, None)):
        assert lib.dsgd_plan_create_from_seed_rp64(None, sp, _lib.ptr(sb), _lib.ptr(se), C.c_int32(k), C.c_int64(10), C.c_int32(batch), po,
                                                   C.byref(n_steps), C.byref(draws)) == _lib.EINVAL
    for sb, se, k, batch, first, n, po in ((b, e, 1, 5, 0, 1, C.byref(out)), (None, e, 1, 5, 0, 1, C.byref(out)), (b, e, 0, 5, 0, 1, C.byref(out)),
                                           (b, e, 1, 0, 0, 1, C.byref(out)), (b, e, 1, 5, -1, 1, C.byref(out)), (b, e, 1, 5, 0, 0, C.byref(out)),
                                           (b, e, 1, 5, 0, 1, None)):
        assert lib.dsgd_async_plan_create_rp64(None, _lib.ptr(sb), _lib.ptr(se), C.c_int32(k), C.c_int32(batch), C.c_uint64(3), C.c_int32(1),
                                               C.c_int64(first), C.c_int64(n), po) == _lib.EINVAL
    assert out.value == sentinel and state.value == 77 and n_steps.value == -1 and draws.value == -1


def test_new_kernels_in_the_code_object_without_spills_or_scratch(tmp_path):
    notes = _kernel_notes(tmp_path)
    for name, lds in (("dsgd_rp64_grad_rec_kernel", 8 * 1024), ("dsgd_rp64v_grad_rec_kernel", 16 * 1024), ("dsgd_rp64_finish_async_kernel", 0)):
        found = {k: v for k, v in notes.items() if name in k}
        assert len(found) == 1, name
        v = next(iter(found.values()))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert lds <= v["group_segment_fixed_size"] <= lds + 64, (name, v)   # the hot ranks' words + the body's few scalars
    # the record is a new instantiation beside the existing kernels, not a change of theirs
    assert sum("dsgd_rp64_grad_kernel" in k for k in notes) == 1 and sum("dsgd_rp64v_grad_kernel" in k for k in notes) == 1


def test_jni_natives_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr, scala_natives, shim_signatures

    natives, shim = scala_natives(), shim_signatures()
    assert natives["planCreateRp64"] == natives["planCreate"] and shim["planCreateRp64"] == shim["planCreate"]
    assert natives["planCreateFromSeedRp64"] == natives["planCreateFromSeed"] and shim["planCreateFromSeedRp64"] == shim["planCreateFromSeed"]
    assert natives["asyncPlanCreateRp64"] == (["Long", "Array[Long]", "Array[Long]", "Int", "Long", "Boolean", "Long", "Long"], "Long")
    patch = open(os.path.join(ROOT, "scala", "patch", "dsgd-hip-backend.diff")).read()
    for n in ("planCreateRp64", "planCreateFromSeedRp64", "asyncPlanCreateRp64"):
        assert "+  @native def %s(" % n in patch
    assert 'sys.props.get("dsgd.f64.rpPlans").contains("true")' in open(os.path.join(ROOT, "scala", "NativeSVM.scala")).read()
    lib = C.CDLL(shim_lib)
    IAE = b"java/lang/IllegalArgumentException"
    vp = C.c_void_p
    (i, _i), (o, _o), (o5, _o5) = jarr(np.arange(6, dtype=np.int32)), jarr(np.asarray([0, 1, 2, 3, 6], np.int64)), jarr(np.asarray([0, 1, 2, 3, 5, 6], np.int64))
    fn = getattr(lib, PREFIX + "planCreateRp64")
    fn.restype = C.c_int64
    fn.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int32]
    for offs, k in ((o5, 2), (o, 0)):   # offsets that are not nSteps * nWorkers + 1: refused before any array is taken
        env = Env()
        assert fn(C.byref(env), None, 0, C.byref(i), C.byref(offs), k) == 0
        assert env.thrown_class == IAE and env.n_get == 0
    env = Env()   # a null context: DSGD_EINVAL from the library, both arrays given back
    assert fn(C.byref(env), None, 0, C.byref(i), C.byref(o), 2) == 0
    assert env.thrown_class == IAE and env.n_get == env.n_release == 2 and env.n_critical == 0
    (st, _st), (st2, _st2), (b, _b), (e, _e), (e2, _e2) = (jarr(np.asarray([5, 0, 0], np.int64)), jarr(np.zeros(2, np.int64)), jarr(np.asarray([0, 10], np.int64)),
                                                           jarr(np.asarray([10, 20], np.int64)), jarr(np.asarray([10], np.int64)))
    fs = getattr(lib, PREFIX + "planCreateFromSeedRp64")
    fs.restype = C.c_int64
    fs.argtypes = [vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int32]
    for s_, e_ in ((st2, e), (st, e2)):   # a state of two entries; splitEnd of another length
        env = Env()
        assert fs(C.byref(env), None, 0, C.byref(s_), C.byref(b), C.byref(e_), 10, 5) == 0
        assert env.thrown_class == IAE and env.n_get == 0
    env = Env()
    assert fs(C.byref(env), None, 0, C.byref(st), C.byref(b), C.byref(e), 10, 5) == 0
    assert env.thrown_class == IAE and env.n_get == env.n_release == 3 and _st.tolist() == [5, 0, 0]   # the state untouched
    fa = getattr(lib, PREFIX + "asyncPlanCreateRp64")
    fa.restype = C.c_int64
    fa.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int32, C.c_int64, C.c_uint8, C.c_int64, C.c_int64]
    env = Env()
    assert fa(C.byref(env), None, 0, C.byref(b), C.byref(e2), 100, 1, 1, 0, 4) == 0
    assert env.thrown_class == IAE and env.n_get == 0
    env = Env()
    assert fa(C.byref(env), None, 0, C.byref(b), C.byref(e), 100, 1, 1, 0, 4) == 0
    assert env.thrown_class == IAE and env.n_get == env.n_release == 2


def test_the_cpp_mirror_compiles_and_forwards(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text(r'''
#include "dsgd.hpp"
#include <cstdio>
// stand-ins for the library: the mirror's calls must arrive with the caller's arrays and values as they are
static const int32_t* g_idx; static int64_t g_n_idx, g_n_steps, g_max, g_first, g_n_upd; static const int64_t* g_offs; static int32_t g_k, g_batch, g_bug;
static uint64_t g_seed; static int64_t g_b0, g_e1;
extern "C" {
int dsgd_create(const dsgd_config*, dsgd_ctx** out) { *out = reinterpret_cast<dsgd_ctx*>(16); return 0; }
int dsgd_destroy(dsgd_ctx*) { return 0; }
const char* dsgd_last_error(void) { return "stub"; }
int dsgd_plan_create_rp64_n(dsgd_ctx*, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers, dsgd_plan** out) {
  g_idx = idx; g_n_idx = n_idx; g_offs = offsets; g_n_steps = n_steps; g_k = n_workers;
  *out = reinterpret_cast<dsgd_plan*>(32);
  return 0;
}
int dsgd_plan_create_from_seed_rp64(dsgd_ctx*, uint64_t* jstate, const int64_t* sb, const int64_t* se, int32_t n_splits, int64_t max_samples,
                                    int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out) {
  g_b0 = sb[0]; g_e1 = se[1]; g_k = n_splits; g_max = max_samples; g_batch = batch_size;
  *jstate += 1; *n_steps_out = 7; *out = reinterpret_cast<dsgd_plan*>(48);
  return draws_out ? 1 : 0;
}
int dsgd_async_plan_create_rp64(dsgd_ctx*, const int64_t* ab, const int64_t* ae, int32_t n_workers, int32_t batch, uint64_t seed, int32_t bug,
                                int64_t first, int64_t n_updates, dsgd_plan** out) {
  g_b0 = ab[0]; g_e1 = ae[1]; g_k = n_workers; g_batch = batch; g_seed = seed; g_bug = bug; g_first = first; g_n_upd = n_updates;
  *out = reinterpret_cast<dsgd_plan*>(64);
  return 0;
}
}
int main() {
  dsgd::SparseSVM m(1e-5, 10, 0, DSGD_F_FP64);
  std::vector<int32_t> idx = {4, 5, 6, 7, 8, 9};
  std::vector<int64_t> offs = {0, 1, 3, 4, 6};
  bool ok = m.planRp64(idx, offs, 2) == reinterpret_cast<dsgd_plan*>(32);
  ok = ok && g_idx == idx.data() && g_n_idx == 6 && g_offs == offs.data() && g_n_steps == 2 && g_k == 2;
  bool threw = false;
  try { m.planRp64(idx, offs, 3); } catch (const std::exception&) { threw = true; }   // 4 lists are not n * 3
  dsgd::JavaRandom rnd(0);
  const uint64_t before = rnd.state();
  int64_t n = 0;
  ok = ok && m.planFromSeedRp64(rnd, {{0, 10}, {10, 19}}, 10, 5, &n) == reinterpret_cast<dsgd_plan*>(48);
  ok = ok && n == 7 && rnd.state() == before + 1 && g_b0 == 0 && g_e1 == 19 && g_k == 2 && g_max == 10 && g_batch == 5;
  ok = ok && m.asyncPlanRp64({{0, 10}, {10, 19}}, 100, 9, true, 3, 12) == reinterpret_cast<dsgd_plan*>(64);
  ok = ok && g_b0 == 0 && g_e1 == 19 && g_k == 2 && g_batch == 100 && g_seed == 9 && g_bug == 1 && g_first == 3 && g_n_upd == 12;
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


class _Plan:
    def __init__(self, kind, n_steps, n_samples):
        self.kind, self.n_steps, self.n_samples, self.destroyed = kind, n_steps, n_samples, False

    def destroy(self):
        self.destroyed = True


class _Backend:
    """An fp64 backend whose column-slice plans are refused; seed_ok: whether the device draws row-parallel plans' lists"""
    precision = "fp64"

    def __init__(self, dp, seed_ok=True):
        self.dp, self.seed_ok, self.calls, self.plans = dp, seed_ok, [], []

    def set_weights(self, w):
        self.w = np.asarray(w, dtype=np.float64)

    def get_weights(self):
        return self.w

    def plan_flat(self, idx, offsets, n_steps, n_workers, rp64=False):
        self.calls.append(("plan_flat", rp64))
        if not rp64:
            raise _Unsupported("fp64 plans host at most 4 workers per step")
        self.plans.append(_Plan("flat", n_steps, int(offsets[-1])))
        self.plans[-1].lists = (np.array(idx, copy=True), np.array(offsets, copy=True))
        return self.plans[-1]

    def plan_from_seed(self, jstate, split, max_samples, batch_size, rp64=False):
        self.calls.append(("plan_from_seed", rp64))
        if not rp64 or not self.seed_ok:
            raise _Unsupported("outside the device form")
        rnd = host.JavaRandom(0)
        rnd.seed = jstate
        idx, offs, n_steps = host.epoch_lists(rnd, split, max_samples, batch_size)
        self.plans.append(_Plan("seed", n_steps, int(offs[n_steps * len(split)])))
        return self.plans[-1], n_steps, rnd.seed, 0

    def plan_run(self, plan, a, b, lr):
        self.calls.append(("plan_run", plan.kind, a, b, lr))

    def sync_step_f64(self, lists, lr):
        self.calls.append(("sync_step_f64",))
        return {"n_samples": sum(len(a) for a in lists), "n_active": 0}

    def synchronize(self):
        return {"n_samples": 0, "n_active": 0}

    def loss_acc(self, lo, hi):
        return 1.0, 0.5, [0, 0, 0]


def _fit(b, epochs=3, k=5, batch=7):
    m = host.MasterSync(b, 60, 75, node_count=k, rnd=host.JavaRandom(0), plans=True)
    m.fit(np.zeros(b.dp), epochs, batch, 0.25, lambda losses: False)
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(60, k)
    want = [host.epoch_lists(rnd, split, max(len(r) for r in split), batch) for _ in range(epochs)]
    assert m.rnd.seed == rnd.seed   # the generator stands where the reference's would
    return m, want


def test_master_sync_takes_row_parallel_plans_only_behind_the_knob(monkeypatch):
    monkeypatch.delenv("DSGD_F64_STEPS", raising=False)
    monkeypatch.delenv("DSGD_F64_RP_PLANS", raising=False)
    b = _Backend(11)
    m, want = _fit(b)
    assert not b.plans and ("plan_flat", True) not in b.calls and ("plan_from_seed", True) not in b.calls   # unset: today's loop
    assert sum(c == ("sync_step_f64",) for c in b.calls) == m.steps_run == sum(w[2] for w in want)
    monkeypatch.setenv("DSGD_F64_RP_PLANS", "1")
    b = _Backend(11)
    m, want = _fit(b)
    # one device-drawn row-parallel plan per epoch, each run once and destroyed; the refused creator is asked once
    assert [p.kind for p in b.plans] == ["seed"] * 3 and all(p.destroyed for p in b.plans)
    assert b.calls.count(("plan_flat", False)) == 1 and ("sync_step_f64",) not in b.calls
    assert [c for c in b.calls if c[0] == "plan_run"] == [("plan_run", "seed", 0, w[2], 0.25) for w in want]
    assert m.steps_run == sum(w[2] for w in want)
    # the device refuses to draw: the host's lists go up as a row-parallel plan
    b = _Backend(11, seed_ok=False)
    m, want = _fit(b)
    assert [p.kind for p in b.plans] == ["flat"] * 3 and all(p.destroyed for p in b.plans)
    assert b.calls.count(("plan_from_seed", True)) == 1 and ("sync_step_f64",) not in b.calls
    for p, (w_idx, w_offs, w_steps) in zip(b.plans, want):
        assert p.n_steps == w_steps and np.array_equal(p.lists[0], w_idx) and np.array_equal(p.lists[1], w_offs)


def test_master_async_falls_back_only_behind_the_knob(monkeypatch):
    class _Async(_Backend):
        def value_bits(self):
            return 64

        def async_plan(self, split, batch, rp64=False, **kw):
            self.calls.append(("async_plan", rp64, kw["first_update"], kw["n_updates"]))
            if not rp64:
                raise _Unsupported("Double feature values")
            self.plans.append(_Plan("async", kw["n_updates"], kw["n_updates"] * batch))
            return self.plans[-1]

        def plan_run_async(self, plan, a, b, lr):
            self.calls.append(("plan_run_async", a, b))

    monkeypatch.delenv("DSGD_F64_RP_PLANS", raising=False)
    with pytest.raises(NotImplementedError, match="Double feature values"):
        host.MasterAsync(_Async(11), 60, 75, node_count=3).fit(np.zeros(11), 1, 5, 0.5, lambda l: False, 8, 0.9, max_steps=20)
    monkeypatch.setenv("DSGD_F64_RP_PLANS", "1")
    b = _Async(11)
    st = host.MasterAsync(b, 60, 75, node_count=3).fit(np.zeros(11), 1, 5, 0.5, lambda l: False, 8, 0.9, max_steps=20)
    assert st.updates == 20
    assert [c for c in b.calls if c[0] == "async_plan"] == [("async_plan", False, 0, 20), ("async_plan", True, 0, 20)]
    assert [c for c in b.calls if c[0] == "plan_run_async"] == [("plan_run_async", 0, 8), ("plan_run_async", 8, 16), ("plan_run_async", 16, 20)]
    assert all(p.destroyed for p in b.plans)
