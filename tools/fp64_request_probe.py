"""The fp64 mode's request / response gradient and steps of any size (dsgd_gradient_f64, dsgd_sync_step_f64;
csrc/dsgd_rp64.hpp) against the fp32 engine and the fp64 plan path.

One GPU run, one JSON line, over N = 804,414 synthetic RCV1-like rows (80 % train, 3 workers' splits of 214,511 rows):
  gradient   us per call of gradient_f64 for n = 100, 4,096, 65,536 and one worker's whole split, next to the fp32
             dsgd_gradient on the same list (median over --reps calls, after one warm-up call)
  sync_step  us per call of sync_step_f64 for 3 x 100, 8 x 100, 4 x 4,096 and 3 x (whole split), next to the fp64 plan
             path (plan_run + synchronize of a --reps-step plan, per step) where the plans take the step

    python tools/fp64_request_probe.py [--rows 804414] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dsgd_amd
from dsgd_amd import _lib, host

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=804414)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
split = host.split_vanilla(n_train, 3)
rng = np.random.default_rng(0)


def engine(precision):
    eng = dsgd_amd.Engine(data.dim, LAM, precision=precision)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(n_train)
    return eng


def median_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1)


out = {"rows": a.rows, "n_train": n_train, "reps": a.reps, "gradient": {}, "sync_step": {}}
e32, e64 = engine("fp32"), engine("fp64")
with e32, e64:
    w = np.zeros(data.dim + 1)
    w[rng.choice(np.arange(1, data.dim + 1), 3000, replace=False)] = rng.normal(scale=0.1, size=3000)
    e32.set_weights(w.astype(np.float32))
    e64.set_weights(w)
    whole = np.asarray(split[0], dtype=np.int32)
    for name, idx in (("100", rng.permutation(whole)[:100]), ("4096", rng.permutation(whole)[:4096]),
                      ("65536", rng.permutation(whole)[:65536]), ("whole_split_%d" % len(whole), whole)):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        reps = a.reps if len(idx) <= 65536 else max(5, a.reps // 5)
        out["gradient"][name] = {"fp64_us": median_us(lambda: e64.gradient_f64(idx), reps),
                                 "fp32_us": median_us(lambda: e32.gradient(idx), reps)}
    for name, k, rows in (("3x100", 3, 100), ("8x100", 8, 100), ("4x4096", 4, 4096), ("3xwhole_split", 3, None)):
        sp = host.split_vanilla(n_train, k)
        lists = [np.ascontiguousarray(rng.permutation(np.asarray(r))[:rows], dtype=np.int32) for r in sp]
        reps = a.reps if rows is not None else max(5, a.reps // 5)
        e64.set_weights(np.zeros(data.dim + 1))
        rec = {"fp64_us": median_us(lambda: e64.sync_step_f64(lists, LR), reps)}
        try:
            p = e64.plan([lists] * a.reps)
        except _lib.DsgdError as e:
            if e.code != _lib.EUNSUPPORTED:
                raise
            rec["plan_fp64_us_per_step"] = None   # (beyond the column-slice plans)
        else:
            def run():
                e64.plan_run(p, 0, a.reps, LR)
                e64.synchronize()
            rec["plan_fp64_us_per_step"] = round(median_us(run, 5) / a.reps, 2)
            p.destroy()
        out["sync_step"][name] = rec
print(json.dumps(out))
