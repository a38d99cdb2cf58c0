"""The boundary of the distributed evaluation (dsgd_predict_ranges / _f64; core/Master.scala:61-98) without a GPU: the
library exports both entry points, the ctypes binding lists them, the argument checks need no device, and the JNI shim
compiles with its `predictRanges` native paired with the Scala declaration (the pattern of tests/test_jni_shim.py)."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dsgd_amd import _lib

SHIM = os.path.join(ROOT, "jni", "dsgd_jni.cpp")
SCALA = os.path.join(ROOT, "scala", "NativeSVM.scala")
PREFIX = "Java_epfl_distributed_core_ml_NativeSVM_00024_"
NAMES = ("dsgd_predict_ranges", "dsgd_predict_ranges_f64")


def test_library_exports_both_entry_points_and_the_binding_lists_them():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dsgd_\w+)", nm))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert "core/Master.scala:61-98" in header and "core/Slave.scala:129-140" in header
    assert lib.dsgd_abi_version() == 1


def test_a_null_context_is_refused_and_nothing_is_written():
    lib = _lib.load()
    rb, re_ = (C.c_int64 * 1)(0), (C.c_int64 * 1)(4)
    pred = np.full(4, 7, dtype=np.int8)
    loss, acc = C.c_double(-1), C.c_double(-1)
    for name in NAMES:
        rc = getattr(lib, name)(None, None, rb, re_, C.c_int32(1), pred.ctypes.data_as(C.c_void_p), None, C.byref(loss), C.byref(acc))
        assert rc == _lib.EINVAL
    assert (pred == 7).all() and loss.value == -1 and acc.value == -1


def test_engine_binding_has_predict_ranges():
    import dsgd_amd

    assert callable(getattr(dsgd_amd.Engine, "predict_ranges"))


# ---- the JNI shim -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_lib(tmp_path_factory):
    _lib.load()
    out = str(tmp_path_factory.mktemp("jni_predict") / "libdsgd_jni_predict_check.so")
    libdir = os.path.dirname(_lib.HIP_LIB)
    cmd = ["g++", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "tests", "jni_stub"), "-I" + os.path.join(ROOT, "include"), SHIM, "-o", out,
           "-L" + libdir, "-l:libdsgd_hip.so", "-Wl,-rpath," + libdir]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    return out


def test_predict_ranges_native_is_exported_and_paired_with_its_declaration(shim_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", shim_lib], stdout=subprocess.PIPE, text=True).stdout
    assert PREFIX + "predictRanges" in re.findall(r"\b(Java_\w+)", nm)
    scala = re.sub(r"//[^\n]*", "", open(SCALA).read())
    m = re.search(r"@native\s+def\s+predictRanges\s*\((.*?)\)\s*:\s*(\w+)", scala, flags=re.S)
    assert m, "NativeSVM.scala does not declare predictRanges"
    params = [p.split(":", 1)[1].strip() for p in re.split(r",\s*(?![^\[]*\])", m.group(1).replace("\n", " ")) if p.strip()]
    assert params == ["Long", "Array[Float]", "Array[Long]", "Array[Long]", "Array[Byte]", "Array[Double]"] and m.group(2) == "Unit"
    c = re.search(r"JNIEXPORT\s+(\w+)\s+JNICALL\s+NATIVE\(predictRanges\)\s*\((.*?)\)\s*\{", open(SHIM).read(), flags=re.S)
    assert c, "the shim does not define predictRanges"
    c_params = [p.strip().split()[0] for p in c.group(2).replace("\n", " ").split(",")]
    assert c.group(1) == "void"
    assert c_params == ["JNIEnv*", "jobject", "jlong", "jfloatArray", "jlongArray", "jlongArray", "jbyteArray", "jdoubleArray"]
    # HipSVM: predict(ranges): Array[Byte] and the two accessors over the native
    assert re.search(r"def\s+predict\s*\(\s*w:\s*Vec,\s*ranges:\s*Seq\[\(Int,\s*Int\)\]\)\s*:\s*Array\[Byte\]", scala)
    assert "def lastPredictLoss" in scala and "def lastPredictAccuracy" in scala and "NativeSVM.predictRanges(" in scala


class JArray(C.Structure):
    _fields_ = [("length", C.c_int32), ("elem_size", C.c_int32), ("data", C.c_void_p)]


class Env(C.Structure):
    _fields_ = [("thrown_class", C.c_char * 128), ("thrown_message", C.c_char * 512), ("n_get", C.c_int),
                ("n_release", C.c_int), ("n_critical", C.c_int)]


def jarr(a):
    a = np.ascontiguousarray(a)
    return JArray(len(a), a.itemsize, a.ctypes.data_as(C.c_void_p)), a


def test_predict_ranges_native_checks_lengths_before_it_takes_an_array(shim_lib):
    lib = C.CDLL(shim_lib)
    fn = getattr(lib, PREFIX + "predictRanges")
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5

    def call(rb, re_, n_pred, n_out=2):
        env = Env()
        (b, _b), (e, _e) = jarr(np.asarray(rb, dtype=np.int64)), jarr(np.asarray(re_, dtype=np.int64))
        (p, pa), (o, oa) = jarr(np.full(n_pred, 7, dtype=np.int8)), jarr(np.full(n_out, -1.0))
        fn(C.byref(env), None, 0, None, C.byref(b), C.byref(e), C.byref(p), C.byref(o))
        assert (pa == 7).all() and (oa == -1.0).all() and env.n_critical == 0
        return env

    env = call([0, 10], [10, 20], 19)                      # predOut one byte short of the ranges' 20 rows
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and b"predOut" in env.thrown_message and env.n_get == 0
    env = call([0, 10], [10], 20)                          # rowBegin / rowEnd of different lengths
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = call([0], [10], 10, n_out=1)                     # nowhere to put {loss, accuracy}
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = call([0, 10], [10, 20], 20)                      # well-formed: reaches the library, whose null context is DSGD_EINVAL
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and b"null context" in env.thrown_message
    assert env.n_get == env.n_release == 1                 # (w is null: only predOut was taken, and given back)
