"""The boundary of the sampled evaluation (dsgd_loss_acc_list / dsgd_loss_acc_sampled and their _f64 forms;
core/Master.scala:109-118) without a GPU: the library exports the four entry points, the ctypes binding lists them, the
argument checks need no device, and the JNI shim compiles with its `lossAccList` / `lossAccSampled` natives paired with the
Scala declarations (the pattern of tests/test_predict_abi.py)."""

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
LIST_NAMES = ("dsgd_loss_acc_list", "dsgd_loss_acc_list_f64")
SAMPLED_NAMES = ("dsgd_loss_acc_sampled", "dsgd_loss_acc_sampled_f64")


def test_library_exports_the_four_entry_points_and_the_binding_lists_them():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dsgd_\w+)", nm))
    for name in LIST_NAMES + SAMPLED_NAMES:
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert "core/Master.scala:109-118" in header
    for name in LIST_NAMES + SAMPLED_NAMES:
        assert re.search(r"\bint %s\(dsgd_ctx\* ctx," % name, header), name
    assert lib.dsgd_abi_version() == 1


def test_a_null_context_is_refused_and_nothing_is_written():
    lib = _lib.load()
    idx = np.arange(4, dtype=np.int32)
    out = np.full(4, 7, dtype=np.int32)
    loss, acc = C.c_double(-1), C.c_double(-1)
    counts = (C.c_int64 * 3)(-1, -1, -1)
    n, draws = C.c_int64(-1), C.c_int64(-1)
    state = C.c_uint64(0x1234567890AB)
    for name in LIST_NAMES:
        rc = getattr(lib, name)(None, None, idx.ctypes.data_as(C.c_void_p), 4, C.byref(loss), C.byref(acc), counts)
        assert rc == _lib.EINVAL, name
    for name in SAMPLED_NAMES:
        rc = getattr(lib, name)(None, None, C.byref(state), 0, 4, 2, C.byref(loss), C.byref(acc), counts, out.ctypes.data_as(C.c_void_p),
                                C.byref(n), C.byref(draws))
        assert rc == _lib.EINVAL, name
    assert loss.value == -1 and acc.value == -1 and list(counts) == [-1, -1, -1] and (n.value, draws.value) == (-1, -1)
    assert (out == 7).all() and state.value == 0x1234567890AB
    assert b"null context" in lib.dsgd_last_error()


def test_engine_binding_has_both_methods():
    import dsgd_amd

    assert callable(getattr(dsgd_amd.Engine, "loss_acc_list")) and callable(getattr(dsgd_amd.Engine, "loss_acc_sampled"))


# ---- the JNI shim -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_lib(tmp_path_factory):
    _lib.load()
    out = str(tmp_path_factory.mktemp("jni_sampled") / "libdsgd_jni_sampled_check.so")
    libdir = os.path.dirname(_lib.HIP_LIB)
    cmd = ["g++", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "tests", "jni_stub"), "-I" + os.path.join(ROOT, "include"), SHIM, "-o", out,
           "-L" + libdir, "-l:libdsgd_hip.so", "-Wl,-rpath," + libdir]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    return out


def paired(name, scala_params, scala_ret, c_ret, c_params):
    scala = re.sub(r"//[^\n]*", "", open(SCALA).read())
    m = re.search(r"@native\s+def\s+%s\s*\((.*?)\)\s*:\s*(\w+)" % name, scala, flags=re.S)
    assert m, "NativeSVM.scala does not declare %s" % name
    params = [p.split(":", 1)[1].strip() for p in re.split(r",\s*(?![^\[]*\])", m.group(1).replace("\n", " ")) if p.strip()]
    assert params == scala_params and m.group(2) == scala_ret
    c = re.search(r"JNIEXPORT\s+(\w+)\s+JNICALL\s+NATIVE\(%s\)\s*\((.*?)\)\s*\{" % name, open(SHIM).read(), flags=re.S)
    assert c, "the shim does not define %s" % name
    assert c.group(1) == c_ret
    assert [p.strip().split()[0] for p in c.group(2).replace("\n", " ").split(",")] == c_params


def test_both_natives_are_exported_and_paired_with_their_declarations(shim_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", shim_lib], stdout=subprocess.PIPE, text=True).stdout
    natives = re.findall(r"\b(Java_\w+)", nm)
    assert PREFIX + "lossAccList" in natives and PREFIX + "lossAccSampled" in natives
    paired("lossAccList", ["Long", "Array[Float]", "Array[Int]", "Array[Double]"], "Unit", "void",
           ["JNIEnv*", "jobject", "jlong", "jfloatArray", "jintArray", "jdoubleArray"])
    # the generator state goes in and comes back as a Long
    paired("lossAccSampled", ["Long", "Array[Float]", "Long", "Long", "Long", "Long", "Array[Double]"], "Long", "jlong",
           ["JNIEnv*", "jobject", "jlong", "jfloatArray", "jlong", "jlong", "jlong", "jlong", "jdoubleArray"])
    scala = re.sub(r"//[^\n]*", "", open(SCALA).read())
    assert re.search(r"def\s+sampledLossAndAccuracy\s*\(\s*w:\s*Vec,\s*state:\s*Long,", scala)
    assert "NativeSVM.lossAccSampled(" in scala and "NativeSVM.lossAccList(" in scala


class JArray(C.Structure):
    _fields_ = [("length", C.c_int32), ("elem_size", C.c_int32), ("data", C.c_void_p)]


class Env(C.Structure):
    _fields_ = [("thrown_class", C.c_char * 128), ("thrown_message", C.c_char * 512), ("n_get", C.c_int),
                ("n_release", C.c_int), ("n_critical", C.c_int)]


def jarr(a):
    a = np.ascontiguousarray(a)
    return JArray(len(a), a.itemsize, a.ctypes.data_as(C.c_void_p)), a


def test_natives_reach_the_library_and_leave_their_outputs_on_a_refusal(shim_lib):
    lib = C.CDLL(shim_lib)
    sampled = getattr(lib, PREFIX + "lossAccSampled")
    sampled.restype = C.c_int64
    sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    by_list = getattr(lib, PREFIX + "lossAccList")
    by_list.restype = None
    by_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    state = 0x1234567890AB
    # out too short: refused before the library is called
    env = Env()
    o, oa = jarr(np.full(3, -1.0))
    assert sampled(C.byref(env), None, 0, None, state, 0, 10, 5, C.byref(o)) == state
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and b"out" in env.thrown_message and (oa == -1.0).all()
    # well-formed: reaches the library, whose null context is DSGD_EINVAL; the state comes back as it went in
    env = Env()
    o, oa = jarr(np.full(4, -1.0))
    assert sampled(C.byref(env), None, 0, None, state, 0, 10, 5, C.byref(o)) == state
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and b"null context" in env.thrown_message and (oa == -1.0).all()
    env = Env()
    (i, _i), (o, oa) = jarr(np.arange(3, dtype=np.int32)), jarr(np.full(2, -1.0))
    by_list(C.byref(env), None, 0, None, C.byref(i), C.byref(o))
    assert env.thrown_class == b"java/lang/IllegalArgumentException" and b"null context" in env.thrown_message and (oa == -1.0).all()
    assert env.n_get == env.n_release == 1                 # (w is null: only idx was taken, and given back)
