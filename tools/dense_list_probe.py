#!/usr/bin/env python3
"""What reaching the rows of a dense mini-batch through an index list costs: wall time per step (host clock around
enqueued steps that end in a synchronise) of four legs, alternated in one process, three runs each.

    a  range       step(b, b + B) over contiguous ranges -- the code as it was: the baseline of the same run
    b  list        step_list over the slices of a random permutation of the shard
    c  plan        the same lists from a resident plan (one plan_run per run)
    d  list_arange step_list over arange slices: against (a) the indirection without the randomness

D = 4096 on a generated shard of 1,250,000 rows (20 GB: it streams past the caches), B = 4,096 and 65,536.  Prints one
JSON line (kept as profiles/dense_list_probe.json): per leg the median and [min, max] of the three runs in us per
step, and the median as a fraction of 8 TB/s for the B * (4 D + 4) bytes a step must read (lists: + 4 B).  Nothing
here is a threshold.

    python tools/dense_list_probe.py [rows]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsgd_amd  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1250000
dim = 4096
LR = 1e-3
PASSES = 8     # passes over the shard per timed window (a window of ~20 GB x 8)
out = {"rows": rows, "dim": dim, "variant": "mfma" if os.environ.get("DSGD_DENSE_MFMA", "0") not in ("", "0") else "valu",
       "clock": "host wall time around enqueued steps ending in dsgd_dense_synchronize", "runs": 3, "passes_per_run": PASSES, "cases": []}
rng = np.random.default_rng(0)
with dsgd_amd.DenseLogistic(dim) as eng:
    eng.generate(rows, seed=0)
    for B, steps in ((4096, 300), (65536, 19)):
        steps = min(steps, rows // B)
        starts = [i * B for i in range(steps)]
        perm = rng.permutation(rows).astype(np.int32)
        lists = [perm[s:s + B] for s in starts]
        aranges = [np.arange(s, s + B, dtype=np.int32) for s in starts]
        plan = eng.plan(lists)

        def leg_range():
            for s in starts:
                eng.step(s, s + B, LR)

        def leg_list():
            for idx in lists:
                eng.step_list(idx, LR)

        def leg_plan():
            eng.plan_run(plan, 0, steps, LR)

        def leg_arange():
            for idx in aranges:
                eng.step_list(idx, LR)

        legs = (("a_range", leg_range, 0), ("b_list", leg_list, 4), ("c_plan", leg_plan, 4), ("d_list_arange", leg_arange, 4))
        for _, fn, _ in legs:          # warm every leg at this shape
            fn()
        eng.synchronize()
        times = {name: [] for name, _, _ in legs}
        for rep in range(3):           # alternated: a b c d, a b c d, a b c d
            for name, fn, _ in legs:
                t0 = time.perf_counter()
                for _ in range(PASSES):
                    fn()
                eng.synchronize()
                times[name].append((time.perf_counter() - t0) / (steps * PASSES) * 1e6)
        plan.destroy()
        for name, _, extra in legs:
            t = sorted(times[name])
            out["cases"].append({"batch": B, "steps": steps, "leg": name, "us_per_step_median": round(t[1], 2),
                                 "us_per_step_min": round(t[0], 2), "us_per_step_max": round(t[2], 2),
                                 "frac_of_8TBps_median": round(B * (4 * dim + 4 + extra) / (t[1] * 1e-6) / 8e12, 4)})
    loss, acc = eng.loss(0, min(rows, 65536))
    out["final"] = {"loss": loss, "acc": acc, "weights_finite": bool(np.isfinite(eng.get_weights()).all())}
print(json.dumps(out))
