"""What a communicator costs the logistic model's steps (dsgd_comm_init_lg; csrc/dsgd_lg_gather.hpp).

One GPU run, one process, the product library over real RCCL at world = 1, N = 23,149 synthetic RCV1-like rows (80 % train).
Two engines on the same data, one with the communicator attached and one without, three shapes:
  3x100          one lg_sync_step call of 3 lists of 100 rows                       us per call (= per step)
  50x(3x100)     50 steps of 3 x 100 fresh lists in ONE lg_sync_steps call           us per step
  range_18519    one lg_sync_step_ranges call over the whole train range, 1 worker   us per call (= per step)
The legs are alternated (no_comm, world1, no_comm, ...) after one warm-up round; every figure is the median [min ... max] of
five.  With the communicator a call adds the agreement (one small all-reduce and one host read) and every step the header
kernel, the all-reduce of the slots and the gathered finish over k x 1 workers.  No speed is claimed and nothing is asserted:
the numbers are recorded as measured.  RCCL may print its version banner first: the JSON is the last line, and it is also
written to profiles/logistic_ranks_probe.json.  Two ranks on one device run through the tests' stand-in only, which stages
through host memory: no timing of those is meaningful, none is taken.

    python tools/logistic_ranks_probe.py [--rows 23149] [--runs 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import dsgd_amd

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=23149)
ap.add_argument("--runs", type=int, default=5)
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
rng = np.random.default_rng(0)
w0 = np.zeros(data.dim + 1, dtype=np.float32)


def engine(attach):
    eng = dsgd_amd.Engine(data.dim, LAM)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    if attach:
        eng.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)
    return eng


def pick(n):
    return rng.permutation(n_train)[:n].astype(np.int32)


one = [pick(100) for _ in range(3)]
epoch = [[pick(100) for _ in range(3)] for _ in range(50)]
flat = np.concatenate([l for s in epoch for l in s])
offs = np.concatenate([[0], np.cumsum([len(l) for s in epoch for l in s])]).astype(np.int64)
shapes = [("3x100", 1, lambda e: e.lg_sync_step(one, LR)),
          ("50x(3x100)", 50, lambda e: e.lg_sync_steps(flat, offs, 50, 3, LR)),
          ("range_%d" % n_train, 1, lambda e: e.lg_sync_step_ranges([(0, n_train)], LR * 100.0 / n_train))]


def spread(ts):
    return {"median": round(float(np.median(ts)), 1), "min": round(float(min(ts)), 1), "max": round(float(max(ts)), 1)}


out = {"rows": a.rows, "n_train": n_train, "runs": a.runs, "unit": "us per step", "shapes": {}}
with engine(False) as det, engine(True) as att:
    for name, steps, fn in shapes:
        ts = {"no_comm_us": [], "world1_us": []}
        for run in range(-1, a.runs):   # (run -1: the warm-up round)
            for key, eng in (("no_comm_us", det), ("world1_us", att)):
                eng.set_weights(w0)
                t0 = time.perf_counter()
                fn(eng)
                t = (time.perf_counter() - t0) * 1e6 / steps
                if run >= 0:
                    ts[key].append(t)
        out["shapes"][name] = {key: spread(t) for key, t in ts.items()}
        assert np.array_equal(det.get_weights().view(np.uint32), att.get_weights().view(np.uint32)), name   # (the same bits either way)
    att.comm_destroy()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "logistic_ranks_probe.json"), "w") as f:
    f.write(line + "\n")
print(line)
