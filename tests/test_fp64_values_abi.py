"""No GPU needed: the Double-feature-value entry points of the fp64 mode (dsgd_load_csr_f64, dsgd_value_bits; include/dsgd.h
"THE FP64 MODE") are exported and check their arguments before they touch a device; the hand-written rounding of the
two-word column sums (csrc/dsgd_round128.hpp) compiled for the host equals Python's correctly rounded float(int); the text
loader returns the parsed Doubles beside the floats."""

import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import dsgd_amd
from dsgd_amd import _lib
from oracle import ref_loader
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_exports_and_header():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    for name in ("dsgd_load_csr_f64", "dsgd_value_bits"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert "int %s(" % name in header


def test_argument_checks_without_a_device():
    lib = _lib.load()
    bits = C.c_int32(0)
    assert lib.dsgd_value_bits(None, C.byref(bits)) == _lib.EINVAL
    rp = np.zeros(2, np.int64)
    lab = np.ones(1, np.int8)
    assert lib.dsgd_load_csr_f64(None, C.c_int64(1), _lib.ptr(rp), None, None, _lib.ptr(lab)) == _lib.EINVAL
    assert b"null context" in lib.dsgd_last_error()


SRC = r"""
#include <cstdio>
#include "dsgd_round128.hpp"
int main() {
  long long hi; unsigned long long lo; int e;
  while (std::scanf("%lld %llu %d", &hi, &lo, &e) == 3) std::printf("%a\n", dsgd_round128(hi, lo, e));
  return 0;
}
"""


def test_round128_is_pythons_float_of_int(tmp_path):
    src = tmp_path / "r128.cpp"
    src.write_text(SRC)
    exe = tmp_path / "r128"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    rnd = random.Random(0)
    cases = [(0, 0, 0), (0, 0, -90), (1, 0, 0), (-1, 0, 0), (-1, 1 << 32, 0), (0, 1, -94), (0, (1 << 63) + 12345, -60)]
    for _ in range(10000):   # random (HI, LO) pairs of every magnitude, LO >= 2^32 included
        hb, lb = rnd.randrange(0, 63), rnd.randrange(0, 64)
        hi = rnd.randrange(-(1 << hb), (1 << hb) + 1)
        lo = rnd.randrange(0, 1 << lb)
        cases.append((hi, lo, rnd.randrange(-160, 40)))
    for k in range(53, 95):   # ties: the dropped bits exactly half a unit, an even and an odd neighbour, both signs
        for base in (1 << k, (1 << k) + (1 << (k - 52)), (3 << (k - 1)) + (1 << (k - 52))):
            for t in (base + (1 << (k - 53)), base + (1 << (k - 53)) + 1, base + (1 << (k - 53)) - 1, base - 1, (1 << (k + 1)) - 1):
                for sign in (1, -1):
                    tot = sign * t
                    for lo in (tot % (1 << 32), tot % (1 << 32) + (1 << 32) * 7):
                        hi = (tot - lo) >> 32
                        if (hi << 32) + lo == tot and -(1 << 63) <= hi < (1 << 63):
                            cases.append((hi, lo, -70))
    for t in (1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 94) + 1, -((1 << 94) + (1 << 41)), (1 << 62) << 32):
        lo = t % (1 << 32)
        cases.append(((t - lo) >> 32, lo, -10))
    inp = "".join("%d %d %d\n" % c for c in cases)
    out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(cases)
    # (two words hold |T| < 2^96: magnitudes above 2^100 come with the power of two)
    big = [c for c in cases if abs((c[0] << 32) + c[1]) > 1 << 90 and c[2] > 10]
    small = [c for c in cases if 0 < abs((c[0] << 32) + c[1]) < 1 << 53]
    assert big and small and any(c[1] >= 1 << 32 for c in cases) and any((c[0] << 32) + c[1] < 0 for c in cases)
    for (hi, lo, e), got in zip(cases, out):
        want = math_ldexp(float((hi << 32) + lo), e)
        assert float.fromhex(got) == want and (want != 0.0 or got.lstrip("-").startswith("0x0")), (hi, lo, e, got, want.hex())


def math_ldexp(x, e):
    import math
    return math.ldexp(x, e)   # (exact: the results are normal doubles)


def test_loader_returns_the_doubles():
    folder = os.path.join(ROOT, "tests", "golden", "lyrl2004_sample")
    data = dsgd_amd.rcv1.load(folder, full=True)
    assert data.val64 is not None and data.val64.dtype == np.float64 and data.val.dtype == np.float32
    want = []
    for name in dsgd_amd.rcv1.FILES:
        with open(os.path.join(folder, name)) as f:
            for line in f.read().split("\n")[:-1]:
                row = {}
                for tok in line.split(" ")[2:]:
                    if tok:
                        k, v = tok.split(":")[:2]
                        row[int(k)] = float(v)
                want.append(row)
    assert data.n_rows == len(want)
    n_inexact = 0
    for i, row in enumerate(want):
        b, e = int(data.row_ptr[i]), int(data.row_ptr[i + 1])
        got = dict(zip(data.col[b:e].tolist(), data.val64[b:e].tolist()))
        assert got == row   # entry for entry Python's float(text)
        n_inexact += sum(1 for v in row.values() if float(np.float32(v)) != v)
    assert n_inexact > 0   # (the sample's values are not float-representable: the doubles matter)
    assert np.array_equal(data.val, data.val64.astype(np.float32))   # the floats as they were: (float)strtod
    rp, col, val, lab, _ = ref_loader.rcv1(folder, full=True)
    assert np.array_equal(rp, data.row_ptr) and np.array_equal(lab, data.label)
    assert sorted(zip(col.tolist(), val.tolist())) == sorted(zip(data.col.tolist(), data.val64.tolist()))


def test_csr_rows_keeps_the_doubles():
    folder = os.path.join(ROOT, "tests", "golden", "lyrl2004_sample")
    data = dsgd_amd.rcv1.load(folder, full=False)
    part = data.rows(1, 3)
    b, e = int(data.row_ptr[1]), int(data.row_ptr[3])
    assert np.array_equal(part.val64, data.val64[b:e]) and np.array_equal(part.val, data.val[b:e])
    assert dsgd_amd.synth.generate(16, seed=1).val64 is None   # (the synthetic generator is float by construction)


def test_the_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "dsgd.hpp"\n'
                   "int use(dsgd::SparseSVM& m, const dsgd::Data& d, const std::vector<double>& v) {\n"
                   "  m.loadCsrF64(d, v);\n  return m.valueBits();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_jni_load_csr_f64_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr, scala_natives, shim_signatures

    assert scala_natives()["loadCsrF64"] == (["Long", "Array[Long]", "Array[Int]", "Array[Double]", "Array[Byte]"], "Unit")
    assert shim_signatures()["loadCsrF64"][0][2:] == ["jlong", "jlongArray", "jintArray", "jdoubleArray", "jbyteArray"]
    patch = open(os.path.join(ROOT, "scala", "patch", "dsgd-hip-backend.diff")).read()
    assert "+  @native def loadCsrF64(" in patch and "NativeSVM.loadCsrF64(ctx, rowPtr" in patch
    lib = C.CDLL(shim_lib)
    load = getattr(lib, PREFIX + "loadCsrF64")
    load.restype = None
    load.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    (rp, _rp), (col, _c), (val, _v), (lab, _l) = (jarr(np.asarray([0, 1, 2], np.int64)), jarr(np.asarray([1, 2], np.int32)),
                                                 jarr(np.asarray([0.1, 0.2])), jarr(np.asarray([1, -1], np.int8)))
    (val3, _v3) = jarr(np.asarray([0.1, 0.2, 0.3]))
    for args in ((None, col, val, lab), (rp, None, val, lab), (rp, col, None, lab), (rp, col, val, None), (rp, col, val3, lab),
                 (col, col, val, lab)):   # null arrays, lengths that do not fit: refused before any array is taken
        env = Env()
        load(C.byref(env), None, 0, *[None if a is None else C.addressof(a) for a in args])
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = Env()
    load(C.byref(env), None, 0, C.byref(rp), C.byref(col), C.byref(val), C.byref(lab))   # null context -> DSGD_EINVAL
    assert env.thrown_class == b"java/lang/IllegalArgumentException"
    assert env.n_get == env.n_release == 4 and env.n_critical == 0
