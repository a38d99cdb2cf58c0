"""What the job forms cost on ONE rank (dsgd_lg_eval_job, dsgd_plan_create_from_seed_job_lg; csrc/dsgd_lg_eval_job.hpp).

The method of tools/logistic_ranks_probe.py: one GPU run, one process, the product library over real RCCL at world = 1, N =
23,149 synthetic RCV1-like rows (18,519 train rows, SplitStrategy.vanilla into 3 splits of 6,173).  Two engines on the same data,
one with the communicator attached and one without; after one warm-up round the legs are alternated, every figure is the median
[min ... max] of five runs, each run `--calls` calls back to back, host wall time (every call ends in its own synchronisation):
  eval       lg_eval_job over the 3 train splits (attached: the agreement, the evaluation launch, the fold kernel, the all-reduce
             of 64 words, one read-back) against lg_predict_ranges over the same splits on the engine without a communicator --
             the call of the parent commit                                                           us per call
  plan       an epoch's plan through lg_plan_from_seed_job (attached; batches of 100: 62 steps x 3 lists) against
             lg_plan_from_seed (no communicator), create + destroy                                   us per plan
These are ONE-RANK figures: what the gather costs between devices is not known -- real RCCL with more than one rank has not run.
No speed is claimed, no default depends on them and nothing is asserted but that both legs return the same bits / lists.  RCCL
may print its version banner first: the JSON is the last line, and it is also written to profiles/logistic_job_probe.json.

    python tools/logistic_job_probe.py [--rows 23149] [--runs 5] [--calls 200]
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
from dsgd_amd import host

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=23149)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
a = ap.parse_args()

LAM, K, BATCH = 1e-5, 3, 100
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
split = host.split_vanilla(n_train, K)
ranges = [(g.start, g.stop) for g in split]
lens, begins, max_samples = [len(g) for g in split], [g.start for g in split], max(len(g) for g in split)
w0 = (0.05 * np.random.default_rng(0).standard_normal(data.dim + 1)).astype(np.float32)
SEED = host.JavaRandom(3).seed


def engine(attach):
    eng = dsgd_amd.Engine(data.dim, LAM)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.set_weights(w0)
    if attach:
        eng.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)
    return eng


def eval_leg(eng, attached):
    return eng.lg_eval_job(ranges) if attached else eng.lg_predict_ranges(ranges)[2:]


def plan_leg(eng, attached):
    plan, n_steps, state, draws = (eng.lg_plan_from_seed_job(SEED, lens, 0, begins, max_samples, BATCH) if attached
                                   else eng.lg_plan_from_seed(SEED, ranges, max_samples, BATCH))
    plan.destroy()
    return n_steps, state, draws


def spread(ts):
    return {"median": round(float(np.median(ts)), 1), "min": round(float(min(ts)), 1), "max": round(float(max(ts)), 1)}


out = {"rows": a.rows, "n_train": n_train, "splits": K, "rows_per_split": lens, "batch": BATCH, "runs": a.runs, "calls_per_run": a.calls,
       "world": 1, "unit": "us per call, host wall time", "legs": {}}
with engine(False) as det, engine(True) as att:
    # the same bits and the same lists either way
    e0, e1 = eval_leg(det, False), eval_leg(att, True)
    assert np.array_equal(e0[0], e1[0]) and np.array_equal(e0[1].view(np.uint64), e1[1].view(np.uint64)) and tuple(e0[2:]) == tuple(e1[2:])
    assert plan_leg(det, False) == plan_leg(att, True)
    out["plan_steps"] = plan_leg(det, False)[0]
    for name, fn, calls in (("eval", eval_leg, a.calls), ("plan", plan_leg, max(1, a.calls // 10))):
        ts = {"no_comm_parent_call_us": [], "world1_job_form_us": []}
        for run in range(-1, a.runs):   # (run -1: the warm-up round)
            for key, eng, attached in (("no_comm_parent_call_us", det, False), ("world1_job_form_us", att, True)):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn(eng, attached)
                t = (time.perf_counter() - t0) * 1e6 / calls
                if run >= 0:
                    ts[key].append(t)
        out["legs"][name] = {key: spread(t) for key, t in ts.items()}
        out["legs"][name]["calls_per_run"] = calls
    att.comm_destroy()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "logistic_job_probe.json"), "w") as f:
    f.write(line + "\n")
print(line)
