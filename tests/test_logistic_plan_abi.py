"""No GPU needed: logistic plans and the several-ranges evaluation at the C ABI (include/dsgd.h "THE LOGISTIC MODEL": RESIDENT
PLANS, dsgd_lg_loss_acc_ranges) -- exported, declared with the prototypes distributed-sgd_amd/_lib.py binds, version 1 -- and the
refusals that need no device."""

import ctypes as C
import os
import re

import numpy as np

import dsgd_amd
from dsgd_amd import _lib, host
from conftest import ROOT

V, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
# name -> (the argument types _lib.py declares, the header's parameter list with the names taken out)
PROTOTYPES = {
    "dsgd_plan_create_lg_n": ([V, V, I64, V, I64, I32, V],
                              "dsgd_ctx*, const int32_t*, int64_t, const int64_t*, int64_t, int32_t, dsgd_plan**"),
    "dsgd_plan_create_from_seed_lg": ([V, V, V, V, I32, I64, I32, V, V, V],
                                      "dsgd_ctx*, uint64_t*, const int64_t*, const int64_t*, int32_t, int64_t, int32_t, dsgd_plan**, int64_t*, int64_t*"),
    "dsgd_lg_loss_acc_ranges": ([V, V, V, V, I32, V, V], "dsgd_ctx*, const float*, const int64_t*, const int64_t*, int32_t, double*, double*"),
}


def header_params(header, name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return ", ".join(re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(","))


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    for name, (argtypes, params) in PROTOTYPES.items():
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert header_params(header, name) == params, (name, header_params(header, name))
    # the from-seed form takes what dsgd_plan_create_from_seed takes, the list form what dsgd_plan_create_n takes
    assert header_params(header, "dsgd_plan_create_from_seed_lg") == header_params(header, "dsgd_plan_create_from_seed")
    assert header_params(header, "dsgd_plan_create_lg_n") == header_params(header, "dsgd_plan_create_n")
    assert lib.dsgd_abi_version() == 1 and "#define DSGD_ABI_VERSION 1" in header
    assert "7 a logistic plan" in header and "RESIDENT PLANS" in header
    for m in ("lg_plan", "lg_plan_flat", "lg_plan_from_seed", "lg_loss_acc_ranges"):
        assert callable(getattr(dsgd_amd.Engine, m)), m
    assert callable(host.LogisticSync)


def test_refusals_that_need_no_device():
    lib = _lib.load()
    idx = np.arange(4, dtype=np.int32)
    offs = np.array([0, 4], dtype=np.int64)
    sb, se = np.array([0], dtype=np.int64), np.array([4], dtype=np.int64)
    h, st, ns, dr = C.c_void_p(), C.c_uint64(5), C.c_int64(), C.c_int64()
    loss, acc = np.zeros(1), np.zeros(1)
    p = _lib.ptr
    # a null context, whatever else is passed: good arguments, null pointers, n < 1
    for args in ((p(idx), 4, p(offs), 1, 1, C.byref(h)), (None, 4, p(offs), 1, 1, C.byref(h)), (p(idx), 4, None, 1, 1, C.byref(h)),
                 (p(idx), 4, p(offs), 1, 1, None), (p(idx), 0, p(offs), 1, 1, C.byref(h)), (p(idx), 4, p(offs), 0, 1, C.byref(h)),
                 (p(idx), 4, p(offs), 1, 0, C.byref(h))):
        assert lib.dsgd_plan_create_lg_n(None, *args) == _lib.EINVAL
        assert b"null context" in lib.dsgd_last_error()
    for args in ((C.byref(st), p(sb), p(se), 1, 4, 2, C.byref(h), C.byref(ns), C.byref(dr)),
                 (None, p(sb), p(se), 1, 4, 2, C.byref(h), C.byref(ns), C.byref(dr)),
                 (C.byref(st), p(sb), p(se), 0, 4, 2, C.byref(h), C.byref(ns), C.byref(dr)),
                 (C.byref(st), p(sb), p(se), 1, 4, 0, C.byref(h), C.byref(ns), C.byref(dr))):
        assert lib.dsgd_plan_create_from_seed_lg(None, *args) == _lib.EINVAL
    assert st.value == 5 and not h.value
    for args in ((None, p(sb), p(se), 1, p(loss), p(acc)), (None, None, p(se), 1, p(loss), p(acc)), (None, p(sb), p(se), 0, p(loss), p(acc)),
                 (None, p(sb), p(se), 17, p(loss), p(acc)), (None, p(sb), p(se), 1, None, None)):
        assert lib.dsgd_lg_loss_acc_ranges(None, *args) == _lib.EINVAL
    # a null plan through the plan calls a logistic plan is carried by
    assert lib.dsgd_plan_run(None, None, I64(0), I64(1), C.c_float(0.5)) == _lib.EINVAL
