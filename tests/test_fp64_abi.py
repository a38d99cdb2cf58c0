"""CPU-side checks of the fp64 mode (DSGD_F_FP64, include/dsgd.h "THE FP64 MODE"): the flag is known to the C ABI, the new
entry points check their arguments without a device, the code object carries the fp64 kernels within their register
budget, the JNI shim's fp64 natives, and host.MasterSync keeps an fp64 backend on its plans."""

import ctypes as C
import re

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

NEW = ["dsgd_set_weights_f64", "dsgd_get_weights_f64", "dsgd_set_dim_sparsity_f64", "dsgd_get_dim_sparsity_f64",
       "dsgd_plan_run_f64", "dsgd_precision"]


@pytest.mark.skipif(has_gpu(), reason="checks the no-device path")
def test_fp64_engine_without_a_device_is_unsupported_and_unknown_flags_stay_invalid():
    with pytest.raises(_lib.DsgdError) as ei:
        dsgd_amd.Engine(47236, 1e-5, precision="fp64")
    assert ei.value.code == _lib.EUNSUPPORTED
    with pytest.raises(_lib.DsgdError) as ei:
        dsgd_amd.Engine(47236, 1e-5, flags=0x2)
    assert ei.value.code == _lib.EINVAL and "flags" in str(ei.value)


def test_unknown_flag_is_invalid_before_the_device_check():
    lib = _lib.load()
    ctx = C.c_void_p()
    cfg = _lib.Config(47236, 0, 1e-5, _lib.F_FP64 | 0x2, 0)
    assert lib.dsgd_create(C.byref(cfg), C.byref(ctx)) == _lib.EINVAL
    with pytest.raises(ValueError):
        dsgd_amd.Engine(47236, 1e-5, precision="fp16")


def test_new_entry_points_reject_null_arguments_without_a_device():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.dsgd_set_weights_f64(None, None) == _lib.EINVAL
    assert lib.dsgd_get_weights_f64(None, None) == _lib.EINVAL
    assert lib.dsgd_set_dim_sparsity_f64(None, None) == _lib.EINVAL
    assert lib.dsgd_get_dim_sparsity_f64(None, None) == _lib.EINVAL
    assert lib.dsgd_plan_run_f64(None, None, C.c_int64(0), C.c_int64(1), C.c_double(0.5)) == _lib.EINVAL
    assert lib.dsgd_precision(None, None) == _lib.EINVAL
    assert b"null" in lib.dsgd_last_error()


def test_fp64_kernels_in_the_code_object_and_their_registers(tmp_path):
    """dsgd_cs64_step_kernel: 512 lanes, two waves per SIMD (256 registers), nothing in accumulation registers; the
    one-slot-per-lane form (the reference's 3 x 100) spills nothing and uses no scratch."""
    notes = _kernel_notes(tmp_path)
    steps = {k: v for k, v in notes.items() if "dsgd_cs64_step_kernel" in k}
    assert len(steps) == 2, sorted(steps)
    assert any("dsgd_eval64_kernel" in k for k in notes) and any("dsgd_forward64_kernel" in k for k in notes)
    for k, v in steps.items():
        assert int(re.search(r"ILi(\d+)E", k).group(1)) == 512
        assert v["vgpr_count"] <= 256 and v.get("agpr_count", 0) == 0, (k, v)
        if "ILi512ELi1ELi4E" in k:
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for k, v in notes.items():
        if "64_kernel" in k and "cs64_step" not in k:
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


class _FakeFp64Backend:
    precision = "fp64"

    def __init__(self, dp):
        self.dp = dp
        self.ranges_calls = 0
        self.plans_run = 0

    def set_weights(self, w):
        self.w = np.asarray(w, dtype=np.float64)

    def get_weights(self):
        return self.w

    def sync_step_ranges(self, ranges, lr):
        self.ranges_calls += 1

    def plan_flat(self, idx, offsets, n_steps, n_workers):
        return _FakePlan()

    def plan_run(self, plan, a, b, lr):
        self.plans_run += 1

    def synchronize(self):
        return {"n_samples": 0, "n_active": 0}

    def loss_acc(self, lo, hi):
        return 1.0, 0.5, [0, 0, 0]


class _FakePlan:
    def destroy(self):
        pass


def test_master_sync_keeps_an_fp64_backend_off_the_range_steps():
    """batch >= split: the fp32 path takes dsgd_sync_step_ranges; an fp64 backend runs the epoch through its plan."""
    b = _FakeFp64Backend(11)
    m = host.MasterSync(b, 40, 50, node_count=2, rnd=host.JavaRandom(0))
    m.fit(np.zeros(11), 2, 100, 0.5, lambda losses: False)
    assert b.ranges_calls == 0 and b.plans_run == 2


def test_jni_fp64_natives_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr

    lib = C.CDLL(shim_lib)
    create = getattr(lib, PREFIX + "createF64")
    create.restype = C.c_int64
    create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32]
    env = Env()
    assert create(C.byref(env), None, 0, 1e-5, 0) == 0
    assert env.thrown_class == b"java/lang/IllegalArgumentException"
    if not has_gpu():
        env = Env()
        assert create(C.byref(env), None, 47236, 1e-5, 0) == 0   # no device: loud failure
        assert env.thrown_class == b"java/lang/RuntimeException"
    for name in ("setWeightsF64", "getWeightsF64"):
        fn = getattr(lib, PREFIX + name)
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        env = Env()
        fn(C.byref(env), None, 0, None)   # null array
        assert env.thrown_class == b"java/lang/IllegalArgumentException", name
        env = Env()
        a, _keep = jarr(np.zeros(8, dtype=np.float64))
        fn(C.byref(env), None, 0, C.byref(a))
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == env.n_release == 1, name
    run = getattr(lib, PREFIX + "planRunF64")
    run.restype = None
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_double]
    env = Env()
    run(C.byref(env), None, 0, 0, 0, 1, 0.5)
    assert env.thrown_class == b"java/lang/IllegalArgumentException"
