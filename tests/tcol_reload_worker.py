"""Worker of tests/test_gpu_tcol.py::test_a_load_releases_the_column_lists_at_once: runs on the tests' seam build of the library
(DSGD_LIB_PATH = tests/rccl_stub/libdsgd_hip_seam.so), the only build that counts the bytes it holds (dsgd_test_live_bytes).
One context steps over two ranges through the column lists, loads other rows and steps again; a fresh context sees the second
rows only.  Reports the kernels, the comparisons of the weights' bits and the device bytes held as one JSON line "RELOAD {...}"."""

import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dsgd_amd  # noqa: E402
from dsgd_amd import _lib  # noqa: E402

N_ROWS, N_TRAIN, LAM, LR = 3000, 2400, 1e-5, 0.05
RANGES = [(0, 1000), (1000, 2000)]
lib = _lib.load()


def device_bytes():
    d, p = C.c_int64(-1), C.c_int64(-1)
    lib.dsgd_test_live_bytes(C.byref(d), C.byref(p))
    return d.value


def internal_nnz(d, rows=None):
    """entries the library holds for the rows: an empty row is stored as one explicit zero (dsgd_load_csr)"""
    n = d.n_rows if rows is None else rows
    return int(np.maximum(np.diff(d.row_ptr[:n + 1]), 1).sum())


def bits(w):
    return np.ascontiguousarray(w).view(np.uint32)


def step(eng, w):
    eng.build_dim_sparsity(N_TRAIN)
    eng.set_weights(w)
    eng.sync_step_ranges(RANGES, LR)
    return eng.grad_kernel_name(), eng.get_weights()


d1 = dsgd_amd.synth.generate(N_ROWS, seed=11)
d2 = dsgd_amd.synth.generate(N_ROWS, seed=12)
assert d1.dim == d2.dim and not np.array_equal(d1.col[:1000], d2.col[:1000])
rng = np.random.default_rng(5)
w = np.zeros(d1.dim + 1, dtype=np.float32)
hot = rng.choice(np.arange(1, d1.dim + 1), size=8000, replace=False)
w[hot] = rng.normal(scale=0.05, size=8000).astype(np.float32)

out = {"nnz": [internal_nnz(d1), internal_nnz(d2)], "n_ent": internal_nnz(d1, RANGES[-1][1])}
base = device_bytes()
with dsgd_amd.Engine(d1.dim, LAM) as eng:
    eng.load_csr(d1.row_ptr, d1.col, d1.val, d1.label)
    out["before_first_step"] = device_bytes() - base
    k1, w1 = step(eng, w)
    out["before_load"] = device_bytes() - base            # (the ranges' layout is cached)
    eng.load_csr(d2.row_ptr, d2.col, d2.val, d2.label)
    out["after_load"] = device_bytes() - base             # directly after the load
    k2, w2 = step(eng, w)
    out["after_second_step"] = device_bytes() - base
base = device_bytes()
with dsgd_amd.Engine(d2.dim, LAM) as fresh:
    fresh.load_csr(d2.row_ptr, d2.col, d2.val, d2.label)
    out["fresh_after_load"] = device_bytes() - base
    kf, wf = step(fresh, w)
    out["fresh_after_step"] = device_bytes() - base
out["kernels"] = [k1, k2, kf]
out["reloaded_equals_fresh"] = bool(np.array_equal(bits(w2), bits(wf)))
out["reloaded_equals_first"] = bool(np.array_equal(bits(w2), bits(w1)))
out["moved"] = bool(not np.array_equal(bits(w1), bits(w)))
print("RELOAD " + json.dumps(out), flush=True)
