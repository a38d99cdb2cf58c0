"""No GPU needed: the job form of the device-drawn epoch plans (dsgd_plan_create_from_seed_job / _rp64; include/dsgd.h) is
exported with its ctypes signature and checks what it can before it touches a device; the JNI native is paired with its
Scala declaration and the patch's copy; the C++ mirror compiles; and the bisection that finds the raw value of a draw
(csrc/dsgd_jr_bisect.hpp, the lines dsgd_jr_slice_job_kernel compiles) equals the linear walk of dsgd_jr_slice_kernel on
hand-made rejection lists."""

import ctypes as C
import os
import random
import subprocess

import numpy as np

from dsgd_amd import _lib
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")
NAMES = ("dsgd_plan_create_from_seed_job", "dsgd_plan_create_from_seed_job_rp64")


def test_exports_header_and_ctypes_signatures():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert "int %s(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first," % name in header
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        # (ctx, jstate*, job_len*, n_job, first, n_local, split_begin*, max_samples, batch_size, out*, n_steps_out*, draws_out*)
        assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    # what every rank must pass alike is said where the call is declared
    assert "EVERY RANK MUST PASS THE SAME *jstate, job_len, max_samples, batch_size AND n_local" in header


def test_argument_checks_without_a_device():
    lib = _lib.load()
    jl = np.asarray([10, 10], np.int64)
    sb = np.asarray([0, 10], np.int64)
    for name in NAMES:
        st, h, n, d = C.c_uint64(5), C.c_void_p(0x5A5A), C.c_int64(-1), C.c_int64(-1)
        rc = getattr(lib, name)(None, C.byref(st), _lib.ptr(jl), 2, 0, 2, _lib.ptr(sb), 100, 10, C.byref(h), C.byref(n), C.byref(d))
        assert rc == _lib.EINVAL and b"null context" in lib.dsgd_last_error()
        assert st.value == 5 and h.value == 0x5A5A and n.value == -1 and d.value == -1   # (nothing written)


def test_the_engine_binding_takes_flat_lists():
    import inspect

    import dsgd_amd

    sig = inspect.signature(dsgd_amd.Engine.plan_from_seed_job)
    assert list(sig.parameters) == ["self", "jstate", "job_lens", "first", "split_begins", "max_samples", "batch_size", "rp64"]
    assert sig.parameters["rp64"].default is False


def test_the_jni_native_is_paired_with_its_declaration(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr, scala_natives, shim_signatures

    want = (["Long", "Array[Long]", "Array[Long]", "Int", "Array[Long]", "Long", "Int", "Boolean"], "Long")
    assert scala_natives()["planCreateFromSeedJob"] == want
    assert shim_signatures()["planCreateFromSeedJob"][0][2:] == ["jlong", "jlongArray", "jlongArray", "jint", "jlongArray", "jlong", "jint", "jboolean"]
    patch = open(os.path.join(ROOT, "scala", "patch", "dsgd-hip-backend.diff")).read()
    assert "+  @native def planCreateFromSeedJob(ctx: Long, state: Array[Long], jobLen: Array[Long], first: Int," in patch
    lib = C.CDLL(shim_lib)
    fn = getattr(lib, PREFIX + "planCreateFromSeedJob")
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_uint8]
    (state, _s), (jl, _j), (sb, _b) = jarr(np.asarray([5, 0, 0], np.int64)), jarr(np.asarray([10, 10], np.int64)), jarr(np.asarray([0], np.int64))
    (state2, _s2), (sb3, _b3) = jarr(np.asarray([5, 0], np.int64)), jarr(np.asarray([0, 10, 20], np.int64))
    adr = lambda a: None if a is None else C.addressof(a)   # noqa: E731
    # null arrays, a short state, a window outside the job: refused before any array is taken
    for st_, jl_, first, sb_ in ((None, jl, 0, sb), (state, None, 0, sb), (state, jl, 0, None), (state2, jl, 0, sb), (state, jl, -1, sb),
                                 (state, jl, 2, sb), (state, jl, 0, sb3)):
        env = Env()
        assert fn(C.byref(env), None, 0, adr(st_), adr(jl_), first, adr(sb_), 100, 10, 0) == 0
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    for rp64 in (0, 1):   # a null context -> DSGD_EINVAL, every array given back, the state as it was
        env = Env()
        assert fn(C.byref(env), None, 0, adr(state), adr(jl), 1, adr(sb), 100, 10, rp64) == 0
        assert env.thrown_class == b"java/lang/IllegalArgumentException"
        assert env.n_get == env.n_release == 3 and env.n_critical == 0
        assert _s.tolist() == [5, 0, 0]


def test_the_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "dsgd.hpp"\n'
                   "dsgd_plan* use(dsgd::SparseSVM& m, dsgd::JavaRandom& rnd, const std::vector<int64_t>& jobLen, const std::vector<int64_t>& sb) {\n"
                   "  int64_t n = 0;\n  dsgd_plan* a = m.planCreateFromSeedJob(rnd, jobLen, 1, sb, 1000, 2500, false, &n);\n"
                   "  return n ? a : m.planCreateFromSeedJob(rnd, jobLen, 0, sb, 1000, 100, true, nullptr);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


SRC = r"""
#include <cstdio>
#include <vector>
#include "dsgd_jr_bisect.hpp"
// per line: n_rej, the rejections, m_lo, m_hi -> for every draw m in [m_lo, m_hi]: "bisect linear"
int main() {
  int n;
  while (std::scanf("%d", &n) == 1) {
    std::vector<int> rej((size_t)n);
    for (int i = 0; i < n; ++i) if (std::scanf("%d", &rej[(size_t)i]) != 1) return 1;
    long long lo, hi;
    if (std::scanf("%lld %lld", &lo, &hi) != 2) return 1;
    for (long long m = lo; m <= hi; ++m)
      std::printf("%lld %lld\n", dsgd_jr_raw_of_draw_bisect(m, rej.data(), n), dsgd_jr_raw_of_draw_linear(m, rej.data(), n));
  }
  return 0;
}
"""


def _raw_of_draw(m, rej):
    """by definition: the raw offset of the (m + 1)-th raw value that is not rejected"""
    rs, x, seen = set(rej), -1, -1
    while seen < m:
        x += 1
        if x not in rs:
            seen += 1
    return x


def test_the_bisection_is_the_linear_walk(tmp_path):
    src = tmp_path / "bisect.cpp"
    src.write_text(SRC)
    exe = tmp_path / "bisect"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    n_draws = 40
    cases = [[],                              # no rejection: draw m is raw value m
             [0],                             # the very first raw value rejected: every draw is one later
             [3, 4, 5],                       # consecutive raw values: one draw waits for three
             [0, 1, 2, 3],                    # ... from offset 0
             [n_draws - 1],                   # the raw value that would have served the LAST draw
             [n_draws - 1, n_draws],          # ... and the one behind it
             [2, 7, 8, 20, 21, 22, 39],
             list(range(0, 24, 2)),           # every other raw value: T_i = i, every draw from 0 to 11 has one
             [100]]                           # beyond every draw asked for
    rnd = random.Random(1)
    for n in (1, 2, 63, 64, 65, 511, 512):    # both sides of the old limit, the new limit itself
        cases.append(sorted(rnd.sample(range(0, 4 * n + 8), n)))
    inp = "".join("%d %s 0 %d\n" % (len(c), " ".join(map(str, c)), max(n_draws, 3 * len(c)) - 1) for c in cases)
    out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout.split()
    at = 0
    for c in cases:
        for m in range(max(n_draws, 3 * len(c))):
            bis, lin = int(out[at]), int(out[at + 1])
            at += 2
            assert bis == lin == _raw_of_draw(m, c), (c, m, bis, lin)
    assert at == len(out)
