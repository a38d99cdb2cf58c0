#!/usr/bin/env python3
"""What one EPOCH of Master.fit costs in the fp64 mode where the column-slice plans refuse it (DESIGN.md 3.8 "Row-parallel
plans"), one JSON line, us per step:

  a  the loop of Engine.sync_step_f64 calls over host-drawn lists (the draw is not timed: the path of DSGD_F64_STEPS=0)
  b  host.epoch_lists (csrc/jrand.c) + ONE Engine.sync_steps_f64 call: the draw and the upload are timed
  c  host.epoch_lists + Engine.plan_flat(rp64=True) + plan_run + synchronize: a row-parallel plan from host lists
  d  Engine.plan_from_seed(rp64=True) + plan_run + synchronize: the lists drawn by the device ("refused" where the device
     shuffle does not apply: batches beyond 1,024 rows)

at N = 804,414 synthetic rows (80 % train), from zero weights, one epoch of 3 x 100, 8 x 100 and 4 x 4,096, on Double and on
float data.  The four paths alternate inside each repetition, in one process, every one from the same generator state; the
first repetition is a warm-up and is dropped; --reps (>= 5) are kept.  Wall-clock time around calls that end behind their
own synchronisation; median with min and max.

    python tools/fp64_rp_plan_probe.py > profiles/fp64_rp_plans_probe.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dsgd_amd  # noqa: E402
from dsgd_amd import host  # noqa: E402

LAM, LR = 1e-5, 0.5


def summary(us):
    us = sorted(us)
    return {"median": round(us[len(us) // 2], 3), "min": round(us[0], 3), "max": round(us[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=804414)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if dsgd_amd.device_count() < 1:
        print(json.dumps({"status": "not run", "reason": "no gfx950 device"}))
        return 1
    data = dsgd_amd.synth.generate(args.rows, seed=7)
    n_train = int(args.rows * 0.8)
    val64 = data.val.astype(np.float64) * (1.0 + 1e-8 * np.random.default_rng(3).standard_normal(len(data.val)))
    out = {"status": "run", "rows": args.rows, "reps": args.reps, "unit": "us per step of one epoch", "cases": []}
    for values, val in (("double", val64), ("float", data.val)):
        with dsgd_amd.Engine(data.dim, LAM, precision="fp64") as eng:
            eng.load_csr(data.row_ptr, data.col, val, data.label)
            eng.build_dim_sparsity(n_train)
            for k, n in ((3, 100), (8, 100), (4, 4096)):
                split = host.split_vanilla(n_train, k)
                max_samples = max(len(r) for r in split)
                state0 = host.JavaRandom(0).seed
                times = {"a": [], "b": [], "c": [], "d": []}
                refused = None
                n_steps = 0
                for rep in range(args.reps + 1):
                    def lists():
                        rnd = host.JavaRandom(0)
                        rnd.seed = state0
                        return host.epoch_lists(rnd, split, max_samples, n)

                    zero = np.zeros(data.dim + 1)
                    # a: the per-call loop (lists drawn outside the clock)
                    idx, offs, n_steps = lists()
                    eng.set_weights(zero)
                    eng.synchronize()
                    t0 = time.perf_counter()
                    for s in range(n_steps):
                        o = offs[s * k:(s + 1) * k + 1]
                        eng.sync_step_f64([idx[o[j]:o[j + 1]] for j in range(k)], LR)
                    ta = time.perf_counter() - t0
                    # b: draw + one call
                    eng.set_weights(zero)
                    eng.synchronize()
                    t0 = time.perf_counter()
                    idx, offs, n_steps = lists()
                    eng.sync_steps_f64(idx[:offs[n_steps * k]], offs[:n_steps * k + 1], n_steps, k, LR)
                    tb = time.perf_counter() - t0
                    # c: draw + a row-parallel plan of the host's lists
                    eng.set_weights(zero)
                    eng.synchronize()
                    t0 = time.perf_counter()
                    idx, offs, n_steps = lists()
                    p = eng.plan_flat(idx[:offs[n_steps * k]], offs[:n_steps * k + 1], n_steps, k, rp64=True)
                    eng.plan_run(p, 0, n_steps, LR)
                    p.destroy()
                    eng.synchronize()
                    tc = time.perf_counter() - t0
                    # d: the lists drawn by the device
                    eng.set_weights(zero)
                    eng.synchronize()
                    td = None
                    t0 = time.perf_counter()
                    try:
                        p, n_d, _, _ = eng.plan_from_seed(state0, split, max_samples, n, rp64=True)
                        eng.plan_run(p, 0, n_d, LR)
                        p.destroy()
                        eng.synchronize()
                        td = time.perf_counter() - t0
                        assert n_d == n_steps
                    except dsgd_amd.DsgdError as e:
                        if e.code != -7:
                            raise
                        refused = str(e)
                    if rep == 0:
                        continue   # warm-up
                    for key, t in (("a", ta), ("b", tb), ("c", tc), ("d", td)):
                        if t is not None:
                            times[key].append(t * 1e6 / n_steps)
                case = {"values": values, "workers": k, "rows_per_worker": n, "steps_per_epoch": int(n_steps)}
                for key in "abcd":
                    case[key] = summary(times[key]) if times[key] else {"refused": refused}
                out["cases"].append(case)
    ref = next(c for c in out["cases"] if c["values"] == "double" and (c["workers"], c["rows_per_worker"]) == (3, 100))
    if "median" in ref["d"]:
        out["d_beats_b_at_3x100_double_by_more_than_b_spread"] = bool(ref["b"]["median"] - ref["d"]["median"] > ref["b"]["max"] - ref["b"]["min"])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
