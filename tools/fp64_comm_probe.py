"""What a communicator costs the fp64 mode's synchronous step (dsgd_comm_init_f64; csrc/dsgd_rp64.hpp "across ranks").

One GPU run, one JSON line, over N = 23,149 synthetic RCV1-like rows (80 % train): us per call of sync_step_f64 for
3 x 100, 4 x 200 and one whole split (3 workers' splits of 6,173 rows),
  no_comm_us   without a communicator (the two row-parallel launches)
  world1_us    with real RCCL attached at world = 1: the gradient, 1 + K all-reduces of 64-bit integers, the headers, the
               finish -- RCCL's launches dominate it
(median over --reps calls, after one warm-up call).  RCCL may print its version banner first: the JSON is the last line.  Two ranks on one device run through the tests' stand-in only, which
stages through host memory: no timing of those is meaningful, none is taken.

    python tools/fp64_comm_probe.py [--rows 23149] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dsgd_amd
from dsgd_amd import host

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=23149)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
rng = np.random.default_rng(0)


def engine(attach):
    eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64")
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    if attach:
        eng.comm_init_f64(dsgd_amd.Engine.comm_unique_id(), 1, 0)
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


cases = []
for name, k, rows in (("3x100", 3, 100), ("4x200", 4, 200), ("3xwhole_split", 3, None)):
    sp = host.split_vanilla(n_train, k)
    cases.append((name, [np.ascontiguousarray(rng.permutation(np.asarray(r))[:rows], dtype=np.int32) for r in sp]))
out = {"rows": a.rows, "n_train": n_train, "reps": a.reps, "sync_step": {name: {} for name, _ in cases}}
for key, attach in (("no_comm_us", False), ("world1_us", True)):
    with engine(attach) as eng:
        for name, lists in cases:
            eng.set_weights(np.zeros(data.dim + 1))
            out["sync_step"][name][key] = median_us(lambda: eng.sync_step_f64(lists, LR), a.reps)
        if attach:
            eng.comm_destroy()
print(json.dumps(out))
