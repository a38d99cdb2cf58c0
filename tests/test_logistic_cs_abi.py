"""No GPU needed: the logistic column-slice plans at the C ABI (include/dsgd.h "THE LOGISTIC MODEL": COLUMN SLICES) -- the two entry
points exported, declared with the prototypes distributed-sgd_amd/_lib.py binds and with the parameter lists of the plain logistic
plans' creators, version 1, plan code 8 documented -- and the refusals that need no device."""

import ctypes as C
import inspect
import os

import numpy as np

import dsgd_amd
from dsgd_amd import _lib, host
from conftest import ROOT
from test_logistic_plan_abi import PROTOTYPES as LG_PROTOTYPES, header_params

PAIRS = {"dsgd_plan_create_lg_cs_n": "dsgd_plan_create_lg_n", "dsgd_plan_create_from_seed_lg_cs": "dsgd_plan_create_from_seed_lg"}


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    for name, plain in PAIRS.items():
        argtypes, params = LG_PROTOTYPES[plain]
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert header_params(header, name) == params == header_params(header, plain), name
    assert lib.dsgd_abi_version() == 1 and "#define DSGD_ABI_VERSION 1" in header
    assert "8 a logistic plan on column slices" in header and "COLUMN SLICES (opt-in)" in header and "7 a logistic plan" in header
    for fn in (dsgd_amd.Engine.lg_plan_flat, dsgd_amd.Engine.lg_plan_from_seed, dsgd_amd.Engine.lg_plan, host.LogisticSync.__init__):
        p = inspect.signature(fn).parameters["slices"]
        assert p.default is False, fn
    train = open(os.path.join(ROOT, "tools", "train.py")).read()
    assert '"--lg-slices"' in train and "a.lg_plans = a.lg_plans or a.lg_slices" in train


def test_refusals_that_need_no_device():
    lib = _lib.load()
    idx = np.arange(4, dtype=np.int32)
    offs = np.array([0, 4], dtype=np.int64)
    sb, se = np.array([0], dtype=np.int64), np.array([4], dtype=np.int64)
    h, st, ns, dr = C.c_void_p(), C.c_uint64(5), C.c_int64(), C.c_int64()
    p = _lib.ptr
    for args in ((p(idx), 4, p(offs), 1, 1, C.byref(h)), (None, 4, p(offs), 1, 1, C.byref(h)), (p(idx), 4, None, 1, 1, C.byref(h)),
                 (p(idx), 4, p(offs), 1, 1, None), (p(idx), 0, p(offs), 1, 1, C.byref(h)), (p(idx), 4, p(offs), 0, 1, C.byref(h)),
                 (p(idx), 4, p(offs), 1, 0, C.byref(h))):
        assert lib.dsgd_plan_create_lg_cs_n(None, *args) == _lib.EINVAL
        assert b"null context" in lib.dsgd_last_error()
    for args in ((C.byref(st), p(sb), p(se), 1, 4, 2, C.byref(h), C.byref(ns), C.byref(dr)),
                 (None, p(sb), p(se), 1, 4, 2, C.byref(h), C.byref(ns), C.byref(dr)),
                 (C.byref(st), p(sb), p(se), 0, 4, 2, C.byref(h), C.byref(ns), C.byref(dr)),
                 (C.byref(st), p(sb), p(se), 1, 4, 0, C.byref(h), C.byref(ns), C.byref(dr))):
        assert lib.dsgd_plan_create_from_seed_lg_cs(None, *args) == _lib.EINVAL
    assert st.value == 5 and not h.value


def test_the_mirror_passes_slices_to_both_constructors():
    calls = []

    class Backend:
        def lg_plan_from_seed(self, *a, **kw):
            calls.append(("seed", kw))
            raise _lib.DsgdError(-7, "not here")

        def lg_plan_flat(self, *a, **kw):
            calls.append(("flat", kw))
            return None

    for slices, want in ((True, {"slices": True}), (False, {})):
        del calls[:]
        m = host.LogisticSync(Backend(), 8, 10, 2, rnd=host.JavaRandom(0), device_lists=True, slices=slices)
        m._next_plan(host.split_vanilla(8, 2), 4, 2)
        assert calls == [("seed", want), ("flat", want)], calls
