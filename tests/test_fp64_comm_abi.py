"""CPU-side checks of the fp64 mode across ranks (include/dsgd.h "ACROSS RANKS", csrc/dsgd_rp64.hpp): dsgd_comm_init_f64
is declared, exported and bound, checks its arguments without a device, the header's refusal list still names what is
not built, the gather's kernels are in the code object without spills or scratch -- and the single-context kernels are
still exactly the ones they were -- and the JNI shim's new natives."""

import ctypes as C
import os
import re

import numpy as np

import dsgd_amd
from dsgd_amd import _lib
from test_abi import _kernel_notes
from test_jni_shim import shim_lib  # noqa: F401  (the fixture: the shim compiled against the stub jni.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dsgd.h")).read()


def test_comm_init_f64_declared_exported_and_bound():
    assert re.search(r"\bint\s+dsgd_comm_init_f64\s*\(\s*dsgd_ctx\*\s*\w+,\s*const char\*\s*\w+,\s*int32_t\s+\w+,\s*int32_t\s+\w+\)\s*;", HEADER)
    lib = _lib.load()
    assert "dsgd_comm_init_f64" in _lib.SYMBOLS and hasattr(lib, "dsgd_comm_init_f64")
    assert callable(getattr(dsgd_amd.Engine, "comm_init_f64"))
    uid = b"\0" * _lib.UNIQUE_ID_BYTES
    assert lib.dsgd_comm_init_f64(None, C.c_char_p(uid), C.c_int32(1), C.c_int32(0)) == _lib.EINVAL   # null context
    assert b"null" in lib.dsgd_last_error()


def test_the_refusal_list_still_names_what_is_not_built():
    mode = HEADER[HEADER.index("/* THE FP64 MODE"):HEADER.index("typedef struct dsgd_ctx dsgd_ctx;")]
    refusals = mode[mode.index("everything else that would run an fp32 training kernel"):mode.index("The asynchronous iteration")]
    assert re.search(r"\bdsgd_comm_init\b(?!_f64)", refusals) and "dsgd_*_devices" in refusals
    assert "dsgd_comm_*" not in refusals           # (it shrank by exactly what is built)
    assert "ACROSS RANKS" in mode and "dsgd_comm_init_f64" in mode


def test_gather_kernels_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    found = {k: v for k, v in notes.items() if "dsgd_rp64_" in k}
    assert sum("dsgd_rp64_grad_gather_kernel" in k for k in found) == 1
    assert sum("dsgd_rp64_header_kernel" in k for k in found) == 1
    assert sum("dsgd_rp64_grad_kernel" in k for k in found) == 1      # (the single-context kernels: as they were; the
    assert sum("dsgd_rp64_finish_kernel" in k for k in found) == 2    #  fold over the ranks' workers IS finish<true>)
    for k, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)


def test_jni_comm_natives_through_the_stub_env(shim_lib):
    from test_jni_shim import PREFIX, Env, jarr

    lib = C.CDLL(shim_lib)
    uid_fn = getattr(lib, PREFIX + "commUniqueId")
    uid_fn.restype = None
    uid_fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    init = getattr(lib, PREFIX + "commInitF64")
    init.restype = None
    init.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32]
    destroy = getattr(lib, PREFIX + "commDestroy")
    destroy.restype = None
    destroy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    short, _s = jarr(np.zeros(16, dtype=np.int8))
    full, _f = jarr(np.zeros(_lib.UNIQUE_ID_BYTES, dtype=np.int8))
    for call in (lambda e: uid_fn(C.byref(e), None, None), lambda e: uid_fn(C.byref(e), None, C.byref(short)),
                 lambda e: init(C.byref(e), None, 0, None, 1, 0), lambda e: init(C.byref(e), None, 0, C.byref(short), 1, 0)):
        env = Env()
        call(env)   # a missing or short id: refused before any array is taken
        assert env.thrown_class == b"java/lang/IllegalArgumentException" and env.n_get == 0
    env = Env()
    init(C.byref(env), None, 0, C.byref(full), 1, 0)   # null context -> DSGD_EINVAL, the array given back
    assert env.thrown_class == b"java/lang/IllegalArgumentException"
    assert env.n_get == env.n_release == 1 and env.n_critical == 0
    env = Env()
    destroy(C.byref(env), None, 0)
    assert env.thrown_class == b"java/lang/IllegalArgumentException"
