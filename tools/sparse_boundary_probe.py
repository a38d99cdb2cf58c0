"""What the Sparse forms at the boundary cost against their dense twins (include/dsgd.h "SPARSE VALUES").

    python tools/sparse_boundary_probe.py [--out profiles/sparse_boundary_probe.json] [--rows 804414]
    python tools/sparse_boundary_probe.py --host-only      # the message-building part alone: needs no GPU
    python tools/sparse_boundary_probe.py --trace-loop     # 200 sparse gradient calls, for rocprofv3 --kernel-trace --stats

Through ctypes at the C ABI, synthetic data, per case: five medians of 50 calls after 20 warm-up calls; the reported figure
is the median of the five, the spread max - min of the five.  Dense and sparse calls of a case alternate block by block in
the same run.  Bytes copied per call are computed from the call's sizes (the sparse output is written by the kernel into
host-mapped memory: 16 bytes of header plus 4 + sizeof(value) per pair)."""

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dsgd_amd  # noqa: E402
from dsgd_amd import _lib, wire  # noqa: E402

LAM = 1e-5
WARM, CALLS, BLOCKS = 20, 50, 5


def _medians(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(BLOCKS):
        ts = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        out.append(statistics.median(ts))
    return out


def _pair(dense_fn, sparse_fn):
    """alternate the blocks of the two calls: both see the same machine state"""
    for _ in range(WARM):
        dense_fn()
        sparse_fn()
    d, s = [], []
    for _ in range(BLOCKS):
        for fn, acc in ((dense_fn, d), (sparse_fn, s)):
            ts = []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e6)
            acc.append(statistics.median(ts))
    rec = lambda m: {"us": round(statistics.median(m), 2), "spread_us": round(max(m) - min(m), 2), "medians_us": [round(x, 2) for x in m]}
    return rec(d), rec(s)


def host_part(dp=47237, nnz=3000):
    """building the GradUpdate message from a dense gradient (to_sparse) against building it from pairs"""
    rng = np.random.default_rng(0)
    g = np.zeros(dp, dtype=np.float32)
    keys = np.sort(rng.choice(dp, nnz, replace=False)).astype(np.int32)
    g[keys] = rng.normal(size=nnz).astype(np.float32)
    vals = g[keys]
    GradUpdate = wire.messages()["GradUpdate"]
    dense = _medians(lambda: GradUpdate(gradUpdate=wire.to_sparse(g, dp - 1)))
    pairs = _medians(lambda: GradUpdate(gradUpdate=wire.sparse_from_pairs(keys, vals, dp - 1)))
    a, b = GradUpdate(gradUpdate=wire.to_sparse(g, dp - 1)), GradUpdate(gradUpdate=wire.sparse_from_pairs(keys, vals, dp - 1))
    assert dict(a.gradUpdate.map) == dict(b.gradUpdate.map)
    sp = wire.to_sparse(g, dp - 1)
    d_in = _medians(lambda: wire.from_sparse(sp, dp))
    p_in = _medians(lambda: wire.pairs_from_sparse(sp, dp))
    rec = lambda m: {"us": round(statistics.median(m), 1), "spread_us": round(max(m) - min(m), 1)}
    return {"dp": dp, "nnz": nnz, "grad_update_from_dense_to_sparse": rec(dense), "grad_update_from_pairs": rec(pairs),
            "weights_from_sparse_dense": rec(d_in), "weights_pairs_from_sparse": rec(p_in)}


def _engine(data, n_train, precision):
    eng = dsgd_amd.Engine(data.dim, LAM, precision=precision)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(n_train)
    return eng


def gpu_part(n_rows):
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    n_train = int(n_rows * 0.8)
    dp = data.dim + 1
    rng = np.random.default_rng(1)
    out = {"n_rows": n_rows, "dp": dp, "cases": {}}
    lib = _lib.load()
    for precision, sizes in (("fp32", (100, 1024, 4096)), ("fp64", (100,))):
        f64 = precision == "fp64"
        dt, sz = (np.float64, 8) if f64 else (np.float32, 4)
        sfx = "_f64" if f64 else ""
        with _engine(data, n_train, precision) as eng:
            ctx = eng._ctx
            w = np.zeros(dp, dtype=dt)
            at = rng.choice(dp, 5000, replace=False)
            w[at] = rng.normal(scale=0.1, size=5000).astype(dt)
            wk = np.flatnonzero(w).astype(np.int32)
            wv = w[wk]
            eng.set_weights(w)
            g = np.zeros(dp, dtype=dt)
            gk, gv = np.zeros(dp, dtype=np.int32), np.zeros(dp, dtype=dt)
            nnz, st = C.c_int64(0), _lib.BatchStats()
            grad_d, grad_s = getattr(lib, "dsgd_gradient" + sfx), getattr(lib, "dsgd_gradient_sparse" + sfx)
            for n in sizes:
                idx = rng.permutation(n_train)[:n].astype(np.int32)
                cn = C.c_int64(n)
                for given in (False, True):
                    dense = lambda: _lib.check(grad_d(ctx, _lib.ptr(w) if given else None, _lib.ptr(idx), cn, _lib.ptr(g), C.byref(st)))
                    sparse = lambda: _lib.check(grad_s(ctx, _lib.ptr(wk) if given else None, _lib.ptr(wv) if given else None,
                                                       C.c_int64(len(wk) if given else -1), _lib.ptr(idx), cn, _lib.ptr(gk), _lib.ptr(gv),
                                                       C.c_int64(dp), C.byref(nnz), C.byref(st)))
                    d, s = _pair(dense, sparse)
                    k = int(nnz.value)
                    assert np.array_equal(gk[:k], np.flatnonzero(g)) and np.array_equal(gv[:k], g[gk[:k]])
                    out["cases"]["%s gradient %d rows, %s weights" % (precision, n, "given (5,000 non-zeros)" if given else "resident")] = {
                        "dense": d, "sparse": s, "nnz_out": k,
                        "bytes_dense": {"to_device": 4 * n + (sz * dp if given else 0), "to_host": sz * dp},
                        "bytes_sparse": {"to_device": 4 * n + ((4 + sz) * len(wk) if given else 0), "to_host": 16 + (4 + sz) * k}}
            # the asynchronous iteration with its delta, 100 rows (each call is a real step: the weights move on)
            idx = rng.permutation(n_train)[:100].astype(np.int32)
            cn = C.c_int64(100)
            lr = C.c_double(0.01) if f64 else C.c_float(0.01)
            step_d, step_s = getattr(lib, "dsgd_async_step" + sfx), getattr(lib, "dsgd_async_step_sparse" + sfx)
            dense = lambda: _lib.check(step_d(ctx, _lib.ptr(idx), cn, lr, _lib.ptr(g), C.byref(st)))
            sparse = lambda: _lib.check(step_s(ctx, _lib.ptr(idx), cn, lr, _lib.ptr(gk), _lib.ptr(gv), C.c_int64(dp), C.byref(nnz), C.byref(st)))
            d, s = _pair(dense, sparse)
            out["cases"]["%s async step 100 rows with its delta" % precision] = {
                "dense": d, "sparse": s, "nnz_out": int(nnz.value), "bytes_dense": {"to_device": 400, "to_host": sz * dp},
                "bytes_sparse": {"to_device": 400, "to_host": 16 + (4 + sz) * int(nnz.value)}}
    return out


def trace_loop(n_rows):
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    n_train = int(n_rows * 0.8)
    rng = np.random.default_rng(1)
    with _engine(data, n_train, "fp32") as eng:
        idx = rng.permutation(n_train)[:100].astype(np.int32)
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        for _ in range(200):
            eng.gradient_sparse(idx)
            eng.gradient(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_boundary_probe.json"))
    ap.add_argument("--rows", type=int, default=804414)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--trace-loop", action="store_true")
    a = ap.parse_args()
    if a.trace_loop:
        trace_loop(a.rows)
        return
    res = {"method": "ctypes at the C ABI; per case five medians of %d calls after %d warm-up calls, dense and sparse blocks "
                     "alternating; us = median of the five, spread_us = max - min of the five" % (CALLS, WARM),
           "host": host_part()}
    if not a.host_only:
        res["gpu"] = gpu_part(a.rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
