"""CPU-side checks of the fp64 mode across ranks on Double feature values (include/dsgd.h "ACROSS RANKS",
csrc/dsgd_rp64_gather.hpp): dsgd_comm_init_f64v is declared, exported, listed and bound and refuses a null context without a
device; the JNI native and its Scala declaration are paired; the header names the call where it describes the ranks; the
two-plane gather kernel is in the code object without spills or scratch; and the layout helpers -- both planes and their
header positions inside a slot, no overlap, the rank word's (k, value type) round trip -- hold in a stand-alone host
program (tests/cpp/rp64_gather_test.cpp) at dp = 1, 62, 63 and RCV1's 47,237."""

import ctypes as C
import os
import re
import subprocess

import numpy as np

import dsgd_amd
from dsgd_amd import _lib
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dsgd.h")).read()
CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_comm_init_f64v_declared_exported_listed_and_bound():
    assert re.search(r"\bint\s+dsgd_comm_init_f64v\s*\(\s*dsgd_ctx\*\s*ctx,\s*const char\*\s*unique_id,\s*int32_t\s+world_size,\s*int32_t\s+rank\)\s*;", HEADER)
    assert "#define DSGD_ABI_VERSION 1" in HEADER
    lib = _lib.load()
    assert "dsgd_comm_init_f64v" in _lib.SYMBOLS and hasattr(lib, "dsgd_comm_init_f64v")
    assert lib.dsgd_comm_init_f64v.argtypes == [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]
    assert lib.dsgd_abi_version() == 1
    assert callable(getattr(dsgd_amd.Engine, "comm_init_f64v"))
    uid = b"\0" * _lib.UNIQUE_ID_BYTES
    assert lib.dsgd_comm_init_f64v(None, uid, 1, 0) == _lib.EINVAL   # null context
    assert b"null" in lib.dsgd_last_error()
    # (the first entry point is where it was)
    assert "dsgd_comm_init_f64" in _lib.SYMBOLS and lib.dsgd_comm_init_f64(None, C.c_char_p(uid), C.c_int32(1), C.c_int32(0)) == _lib.EINVAL


def test_the_header_names_the_call_under_across_ranks():
    mode = HEADER[HEADER.index("/* THE FP64 MODE"):HEADER.index("typedef struct dsgd_ctx dsgd_ctx;")]
    ranks = mode[mode.index("ACROSS RANKS"):mode.index("DOUBLE FEATURE VALUES (dsgd_load_csr_f64")]
    assert "dsgd_comm_init_f64v" in ranks and re.search(r"\bdsgd_comm_init_f64\b(?!v)", ranks)
    assert "K * 2 *" in ranks                      # the wire cost of a Double step is stated
    assert "DSGD_EINVAL" in ranks and "value type" in ranks
    # the refusals on Double data name the entry point that still refuses, and where to go instead
    refused = mode[mode.index("Refused on Double data"):mode.index("AN EPOCH'S STEPS IN ONE CALL")]
    assert re.search(r"\bdsgd_comm_init_f64\b(?!v)", refused) and "dsgd_comm_init_f64v" in refused


def test_jni_native_and_scala_declaration_are_paired(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr, scala_natives, shim_signatures

    assert scala_natives()["commInitF64v"] == (["Long", "Array[Byte]", "Int", "Int"], "Unit")
    assert shim_signatures()["commInitF64v"] == (["JNIEnv*", "jobject", "jlong", "jbyteArray", "jint", "jint"], "void")
    assert scala_natives()["commInitF64v"] == scala_natives()["commInitF64"]
    patch = open(os.path.join(ROOT, "scala", "patch", "dsgd-hip-backend.diff")).read()
    assert "+  @native def commInitF64v(ctx: Long, uniqueId: Array[Byte], worldSize: Int, rank: Int): Unit" in patch
    scala = open(os.path.join(ROOT, "scala", "NativeSVM.scala")).read()
    assert "NativeSVM.commInitF64v(ctx, uniqueId, worldSize, rank)" in scala      # HipSVM attaches through it
    lib = C.CDLL(shim_lib)
    init = getattr(lib, PREFIX + "commInitF64v")
    init.restype = None
    init.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32]
    short, _s = jarr(np.zeros(16, dtype=np.int8))
    full, _f = jarr(np.zeros(_lib.UNIQUE_ID_BYTES, dtype=np.int8))
    for ident in (None, C.byref(short)):   # a missing or short id: refused before any array is taken
        env = Env()
        init(C.byref(env), None, 0, ident, 1, 0)
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = Env()
    init(C.byref(env), None, 0, C.byref(full), 1, 0)   # null context -> DSGD_EINVAL, the array given back
    assert env.thrown_class == b"java/lang/IllegalArgumentException"
    assert env.n_get == env.n_release == 1 and env.n_critical == 0


def test_two_plane_gather_kernel_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    found = {k: v for k, v in notes.items() if "dsgd_rp64v_grad_gather_kernel" in k}
    assert len(found) == 1, sorted(found)
    v = next(iter(found.values()))
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    assert 16 * 1024 <= v["group_segment_fixed_size"] <= 16 * 1024 + 64, v   # both words of the hot ranks + the body's few scalars
    # the fold across the ranks is the single context's Double finish: no new instantiation, and none of the float family
    assert sum("dsgd_rp64v_finish_kernel" in k for k in notes) == 3
    assert sum("dsgd_rp64_finish_kernel" in k for k in notes) == 2 and sum("dsgd_rp64_header_kernel" in k for k in notes) == 1


def test_gather_layout_helpers_in_a_host_program(tmp_path):
    exe = str(tmp_path / "rp64_gather_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rp64_gather_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
