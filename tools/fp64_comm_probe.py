"""What a communicator costs the fp64 mode's synchronous step (dsgd_comm_init_f64, dsgd_comm_init_f64v; csrc/dsgd_rp64.hpp
"across ranks").

One GPU run, one JSON line, over N = 23,149 synthetic RCV1-like rows (80 % train): us per call of sync_step_f64 for
3 x 100, 4 x 200 and one whole split (3 workers' splits of 6,173 rows),
  no_comm_us   without a communicator (the two row-parallel launches)
  world1_us    with real RCCL attached at world = 1: the gradient, 1 + K all-reduces of 64-bit integers, the headers, the
               finish -- RCCL's launches dominate it
and, on DOUBLE feature values (the same rows with full 53-bit mantissas; 3 x 100 and 4 x 200),
  f64v_double_us   real RCCL at world = 1 attached with dsgd_comm_init_f64v: two planes per slot, 1 + 2 K all-reduces
  f64_float_us     the same data rounded to float under dsgd_comm_init_f64: one plane per slot, 1 + K all-reduces
(--skip-double leaves that leg out: a library from before dsgd_comm_init_f64v, selected with DSGD_LIB_PATH for an A/B of the
calls that did not change)
and, for row-parallel plans under the communicator ("rank_plans": 3 x 100 and 4 x 200, float and Double data, a plan of
--plan-steps steps of fresh lists; us per STEP, three runs alternated in one process, median and min ... max),
  plan_world1_us   dsgd_plan_run_f64 on the plan with real RCCL attached at world = 1: one agreement and one host read per
                   call, the steps enqueued back to back, then dsgd_synchronize
  loop_world1_us   the loop of sync_step_f64 calls on the same lists under the same communicator: what the plan run replaces
  plan_no_comm_us  the same plan with no communicator: the floor the collectives sit on
(--skip-rank-plans leaves that leg out, for a library from before it)
(median over --reps calls, after one warm-up call).  RCCL may print its version banner first: the JSON is the last line.  Two ranks on one device run through the tests' stand-in only, which
stages through host memory: no timing of those is meaningful, none is taken.

    python tools/fp64_comm_probe.py [--rows 23149] [--reps 50] [--skip-double] [--skip-rank-plans] [--plan-steps 100]
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
ap.add_argument("--skip-double", action="store_true")
ap.add_argument("--skip-rank-plans", action="store_true")
ap.add_argument("--plan-steps", type=int, default=100)
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
rng = np.random.default_rng(0)


val64 = data.val.astype(np.float64) * (1.0 + np.random.default_rng(1).random(len(data.val)) * 2.0 ** -20)   # no float holds these


def engine(attach, val=None, v=False):
    eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64")
    eng.load_csr(data.row_ptr, data.col, data.val if val is None else val, data.label)
    if attach:
        (eng.comm_init_f64v if v else eng.comm_init_f64)(dsgd_amd.Engine.comm_unique_id(), 1, 0)
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
if not a.skip_double:
    out["sync_step_double"] = {name: {} for name, _ in cases[:2]}
    for key, val, v in (("f64v_double_us", val64, True), ("f64_float_us", val64.astype(np.float32), False)):
        with engine(True, val, v) as eng:
            assert eng.value_bits() == (64 if v else 32)
            for name, lists in cases[:2]:
                eng.set_weights(np.zeros(data.dim + 1))
                out["sync_step_double"][name][key] = median_us(lambda: eng.sync_step_f64(lists, LR), a.reps)
            eng.comm_destroy()


def per_step_us(fn, n_steps):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6 / n_steps


def spread(ts):
    return {"median": round(float(np.median(ts)), 1), "min": round(float(min(ts)), 1), "max": round(float(max(ts)), 1)}


if not a.skip_rank_plans:
    out["rank_plans"] = {"plan_steps": a.plan_steps, "runs": 3}
    w0 = np.zeros(data.dim + 1)
    for vname, val, v in (("float", data.val.astype(np.float32), False), ("double", val64, True)):
        for name, k, rows in (("3x100", 3, 100), ("4x200", 4, 200)):
            sp = host.split_vanilla(n_train, k)
            steps = [[np.ascontiguousarray(rng.permutation(np.asarray(r))[:rows], dtype=np.int32) for r in sp] for _ in range(a.plan_steps)]
            ts = {"plan_world1_us": [], "loop_world1_us": [], "plan_no_comm_us": []}
            with engine(True, val, v) as att, engine(False, val) as det:
                pa, pd = att.plan(steps, rp64=True), det.plan(steps, rp64=True)

                def run_plan(eng, p):
                    eng.plan_run(p, 0, a.plan_steps, LR)
                    eng.synchronize()

                def run_loop():
                    for lists in steps:
                        att.sync_step_f64(lists, LR)

                for warm in (True, False, False, False):   # one warm-up round, then three alternated runs
                    for key, fn in (("plan_world1_us", lambda: run_plan(att, pa)), ("loop_world1_us", run_loop), ("plan_no_comm_us", lambda: run_plan(det, pd))):
                        (att if key != "plan_no_comm_us" else det).set_weights(w0)
                        t = per_step_us(fn, a.plan_steps)
                        if not warm:
                            ts[key].append(t)
                pa.destroy()
                pd.destroy()
                att.comm_destroy()
            out["rank_plans"]["%s_%s" % (vname, name)] = {key: spread(t) for key, t in ts.items()}
print(json.dumps(out))
