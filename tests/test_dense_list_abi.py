"""The dense model's index lists, resident plans and per-row probabilities without a GPU: the seven entry points are
declared, exported and bound; and the lists that tests/test_gpu_dense_lists.py runs make its bit equalities mean
something -- with tests/dense_bound.py's `emulate` as an honest fp32 candidate, every seeded indexing fault moves at
least one weight away from the range step over the permuted data."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_lists as dl
import dsgd_amd
from conftest import ROOT
from dsgd_amd import _lib

NAMES = ("dsgd_dense_step_list", "dsgd_dense_loss_list", "dsgd_dense_predict", "dsgd_dense_predict_list",
         "dsgd_dense_plan_create", "dsgd_dense_plan_run", "dsgd_dense_plan_destroy")
N_CU = 4     # (the GPU test's big lengths follow the device: here the same formulas with a small count)


def test_the_seven_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert "#define DSGD_ABI_VERSION 1" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\bint\s+(dsgd_dense_\w+)\s*\(", code))
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dsgd_\w+)", nm))
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes, name
    assert "typedef struct dsgd_dense_plan dsgd_dense_plan;" in code
    assert "(pre-shuffled)" in header
    assert lib.dsgd_abi_version() == 1


def test_dense_logistic_has_the_new_methods():
    for name in ("step_list", "loss_list", "predict_proba", "plan", "plan_run"):
        assert callable(getattr(dsgd_amd.DenseLogistic, name)), name
    assert callable(dsgd_amd.DensePlan.destroy)


def test_null_handles_and_lists_need_no_device():
    lib = _lib.load()
    idx = np.zeros(4, dtype=np.int32)
    out = np.full(4, 7.0, dtype=np.float32)
    loss, acc = C.c_double(-1), C.c_double(-1)
    h = C.c_void_p()
    off = np.array([0, 4], dtype=np.int64)
    assert lib.dsgd_dense_step_list(None, _lib.ptr(idx), 4, 1.0) == _lib.EINVAL
    assert lib.dsgd_dense_loss_list(None, _lib.ptr(idx), 4, C.byref(loss), C.byref(acc)) == _lib.EINVAL
    assert lib.dsgd_dense_predict(None, 0, 4, _lib.ptr(out)) == _lib.EINVAL
    assert lib.dsgd_dense_predict_list(None, _lib.ptr(idx), 4, _lib.ptr(out)) == _lib.EINVAL
    assert lib.dsgd_dense_plan_create(None, _lib.ptr(idx), 4, _lib.ptr(off), 1, C.byref(h)) == _lib.EINVAL
    assert lib.dsgd_dense_plan_run(None, None, 0, 1, 1.0) == _lib.EINVAL
    assert lib.dsgd_dense_plan_destroy(None, None) == _lib.EINVAL
    assert (out == 7.0).all() and loss.value == -1 and acc.value == -1 and not h


def test_index_lists_are_checked_before_they_are_converted():
    from dsgd_amd.dense import _idx

    assert _idx([3, 1, 2]).dtype == np.int32
    assert len(_idx([])) == 0
    for bad in ([[1, 2]], [1.0, 2.0], 3):
        with pytest.raises(ValueError):
            _idx(bad)
    with pytest.raises(IndexError):
        _idx(np.array([2 ** 32 + 1]))          # would wrap onto row 1


def test_the_lists_are_what_their_names_say():
    for D, n_rows, kind, n in dl.cases(N_CU):
        idx = dl.make_list(kind, n, n_rows)
        assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < n_rows and idx[0] == n_rows - 1
        counts = np.bincount(idx, minlength=n_rows)
        if kind == "perm":
            assert len(idx) == n and counts.max() == 1
        elif kind == "reverse":
            assert (np.diff(idx) == -1).all() and len(idx) == n
        elif kind == "repeat":
            assert len(idx) == n and counts.max() == (5 if n >= 6 else max(1, n - 1)) and (counts > 1).sum() <= 1
        else:
            assert len(idx) == n_rows + n > n_rows and counts.max() > 1
    assert not np.array_equal(dl.step2_list(dl.SMALL_ROWS), dl.make_list("perm", 23, dl.SMALL_ROWS))


@pytest.mark.parametrize("variant", [0, 1])
def test_every_seeded_fault_moves_a_weight(variant):
    """The candidate is honest fp32 with the kernels' block structure; the reference is the same candidate over
    (X[idx], y[idx]) -- what engine B computes.  A fault that left every weight where it was would pass the GPU test's
    `==` as well.  (A list of ONE position has no second position for `first_of_block` to get wrong.)"""
    n_checked = 0
    for D, n_rows, kind, n in dl.cases(N_CU):
        if variant and D > 4096:
            continue
        X, y, w0 = dl.shard(D, n_rows)
        todo = [dl.make_list(kind, n, n_rows)]
        if n == dl.WIDE_N or n == 17:
            todo.append(dl.step2_list(n_rows))
        for idx in todo:
            assert dl.is_sensitive(X, y, w0, idx), (D, kind, n)
            grid = dl.db.launch_grid(variant, N_CU, len(idx))
            lr = 4.0
            ref = dl.db.emulate(X[idx], y[idx], w0, lr, 0, len(idx), variant, grid)[0]
            np.testing.assert_array_equal(dl.emulate_list(X, y, w0, lr, idx, variant, grid), ref)
            for fault in dl.LIST_FAULTS:
                if fault == "first_of_block" and len(idx) == 1:
                    continue
                got = dl.emulate_list(X, y, w0, lr, idx, variant, grid, fault=fault)
                assert (got != ref).any(), (D, kind, n, fault)
                n_checked += 1
    assert n_checked > 100
