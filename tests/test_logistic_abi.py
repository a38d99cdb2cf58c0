"""No GPU needed: the logistic model's entry points at the C ABI (include/dsgd.h "THE LOGISTIC MODEL") -- exported, declared,
bound, version 1 -- and failing cleanly where no context can be made."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import dsgd_amd
from dsgd_amd import _lib
from conftest import ROOT, has_gpu

NAMES = ["dsgd_lg_gradient", "dsgd_lg_sync_step", "dsgd_lg_sync_step_ranges", "dsgd_lg_sync_steps", "dsgd_lg_loss_acc", "dsgd_lg_predict"]


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint %s\(dsgd_ctx\* ctx" % name, header), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dsgd_abi_version() == 1 and "#define DSGD_ABI_VERSION 1" in header
    assert "THE LOGISTIC MODEL" in header and "signum(d)" in header
    for m in ("lg_gradient", "lg_sync_step", "lg_sync_step_ranges", "lg_sync_steps", "lg_loss_acc", "lg_predict_proba"):
        assert callable(getattr(dsgd_amd.Engine, m)), m


def test_a_null_context_is_refused_by_every_entry_point():
    lib = _lib.load()
    idx = np.arange(4, dtype=np.int32)
    out = np.zeros(8, dtype=np.float32)
    z = C.c_int64
    one = (z * 1)(4)
    lists = (C.c_void_p * 1)(_lib.ptr(idx))
    offs = np.array([0, 4], dtype=np.int64)
    loss, acc = C.c_double(), C.c_double()
    assert lib.dsgd_lg_gradient(None, None, _lib.ptr(idx), z(4), _lib.ptr(out), None) == _lib.EINVAL
    assert b"null context" in lib.dsgd_last_error()
    assert lib.dsgd_lg_sync_step(None, lists, one, 1, 0.5, None) == _lib.EINVAL
    assert lib.dsgd_lg_sync_step_ranges(None, (z * 1)(0), (z * 1)(4), 1, 0.5, None) == _lib.EINVAL
    assert lib.dsgd_lg_sync_steps(None, _lib.ptr(idx), z(4), _lib.ptr(offs), z(1), 1, 0.5, None) == _lib.EINVAL
    assert lib.dsgd_lg_loss_acc(None, None, z(0), z(4), C.byref(loss), C.byref(acc)) == _lib.EINVAL
    assert lib.dsgd_lg_predict(None, None, _lib.ptr(idx), z(4), _lib.ptr(out)) == _lib.EINVAL


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_no_context_without_a_device():
    with pytest.raises(dsgd_amd.DsgdError) as ei:
        dsgd_amd.Engine(47236, 1e-5)
    assert ei.value.code == _lib.EUNSUPPORTED
