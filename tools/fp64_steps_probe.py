#!/usr/bin/env python3
"""What an epoch's fp64 steps cost in three forms (DESIGN.md 3.8 "An epoch's steps in one call"), one JSON line:

  a  the loop of Engine.sync_step_f64 calls (the path before dsgd_sync_steps_f64; its code is unchanged)
  b  Engine.sync_steps_f64 with DSGD_RP64_FUSED=0 (the two-launch queue)
  c  Engine.sync_steps_f64 with DSGD_RP64_FUSED=1 (one fused launch per step)

at N = 804,414 synthetic rows, from zero weights, at 3 x 100, 8 x 100 and 4 x 4,096, on float and on Double data.  Every
form runs --steps steps per repetition (>= 2,000), --reps times (>= 5); the three forms alternate inside each repetition,
in one process; the first repetition is a warm-up and is dropped.  Wall-clock time around a call that returns behind its
own synchronisation; us per step as median with min and max.

    python tools/fp64_steps_probe.py > profiles/fp64_steps_probe.json
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


def engine(data, val, n_train, fused):
    os.environ["DSGD_RP64_FUSED"] = "1" if fused else "0"
    try:
        eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64")
    finally:
        os.environ.pop("DSGD_RP64_FUSED", None)
    eng.load_csr(data.row_ptr, data.col, val, data.label)
    eng.build_dim_sparsity(n_train)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=804414)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if dsgd_amd.device_count() < 1:
        print(json.dumps({"status": "not run", "reason": "no gfx950 device"}))
        return 1
    data = dsgd_amd.synth.generate(args.rows, seed=7)
    n_train = int(args.rows * 0.8)
    rng = np.random.default_rng(3)
    val64 = data.val.astype(np.float64) * (1.0 + 1e-8 * rng.standard_normal(len(data.val)))
    out = {"status": "run", "rows": args.rows, "steps_per_call": args.steps, "reps": args.reps, "unit": "us per step", "cases": []}
    for values, val in (("float", data.val), ("double", val64)):
        for k, n in ((3, 100), (8, 100), (4, 4096)):
            split = host.split_vanilla(n_train, k)
            lists = [[rng.integers(r.start, r.stop, size=n).astype(np.int32) for r in split] for _ in range(args.steps)]
            flat = np.concatenate([a for s in lists for a in s])
            offs = np.arange(args.steps * k + 1, dtype=np.int64) * n
            q, f = engine(data, val, n_train, False), engine(data, val, n_train, True)
            t = {"a": [], "b": [], "c": []}
            zero = np.zeros(data.dim + 1)
            for rep in range(args.reps + 1):
                for form in ("a", "b", "c"):
                    eng = f if form == "c" else q
                    eng.set_weights(zero)
                    eng.synchronize()
                    t0 = time.perf_counter_ns()
                    if form == "a":
                        for s in lists:
                            eng.sync_step_f64(s, LR)
                    else:
                        eng.sync_steps_f64(flat, offs, args.steps, k, LR)
                    dt = time.perf_counter_ns() - t0
                    if rep:
                        t[form].append(dt / 1e3 / args.steps)
            same = bool(np.array_equal(q.get_weights().view(np.uint64), f.get_weights().view(np.uint64)))
            out["cases"].append({"values": values, "workers": k, "rows_per_worker": n, "bits_equal_b_c": same,
                                 **{form: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for form, v in t.items()}})
            q.close()
            f.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
