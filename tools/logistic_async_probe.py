"""The logistic model's asynchronous iteration against the parent commit's nearest call, in one process: one JSON line
(profiles/logistic_async_probe.json).

    python tools/logistic_async_probe.py [--repeat 5] [--rows 804414] [--updates 1200] > profiles/logistic_async_probe.json

The method of tools/logistic_plan_probe.py: per leg both sides are warmed up, then timed ALTERNATELY `--repeat` times -- host wall
time around work that ends in a device synchronise -- and reported as median [min .. max] microseconds PER UPDATE with the ratio of
the medians.  The shape: N = 804,414 synthetic rows (80 % of them train), 3 workers x 100 rows on the zero-lag schedule, the lists
drawn by the device (Engine.lg_async_plan).  The right-hand side of every leg is dsgd_lg_sync_steps with ONE worker on the same
lists -- what the parent commit had: the same gradient launch per update, only the finish differs.  Nothing here is a promise: the
figures are what came out.

  per call    lg_async_step, one call (one upload, two launches, one synchronisation) per update
  row plan    plan_run_async_lg on a plan of Engine.lg_async_plan + synchronize: two launches per update, nothing in between
  slice plan  the same on a plan made with slices=True: ONE persistent launch for all updates
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd
from dsgd_amd import host

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--rows", type=int, default=804414)
ap.add_argument("--updates", type=int, default=1200)
a = ap.parse_args()
LAM, K, BATCH, LR = 1e-5, 3, 100, 0.5
N_TRAIN = int(a.rows * 0.8)
T = a.updates


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def leg(name, new, old, before):
    runs = {"new": [], "parent": []}
    for fn in (new, old):   # warm-up: allocations, layouts, clocks
        for _ in range(3):
            before()
            fn()
    for _ in range(a.repeat):   # alternated
        for key, fn in (("new", new), ("parent", old)):
            before()
            runs[key].append(wall_us(fn) / T)
    out = {"leg": name, "unit": "us per update"}
    for key, v in runs.items():
        out[key] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    out["ratio_new_to_parent"] = round(float(np.median(runs["new"]) / np.median(runs["parent"])), 3)
    return out


res = {"tool": "tools/logistic_async_probe.py", "repeat": a.repeat, "rows": a.rows, "n_train": N_TRAIN, "workers": K, "batch": BATCH, "updates": T,
       "parent": "lg_sync_steps, one worker, the same lists", "legs": []}
data = dsgd_amd.synth.generate(a.rows, seed=1)
with dsgd_amd.Engine(data.dim, LAM) as eng:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    w0 = np.zeros(eng.dp, dtype=np.float32)
    split = [(r.start, r.stop) for r in host.split_vanilla(N_TRAIN, K)]
    rows_plan = eng.lg_async_plan(split, BATCH, seed=0, positional_bug=False, first_update=0, n_updates=T)
    slice_plan = eng.lg_async_plan(split, BATCH, seed=0, positional_bug=False, first_update=0, n_updates=T, slices=True)
    res["slice_plan_kind"] = slice_plan.info()["kind"]
    flat, offs = eng.plan_lists(rows_plan)
    lists = [flat[offs[t]:offs[t + 1]] for t in range(T)]
    reset = lambda: eng.set_weights(w0)
    parent = lambda: eng.lg_sync_steps(flat, offs, T, 1, LR)

    def per_call():
        for idx in lists:
            eng.lg_async_step(idx, LR)

    def run(plan):
        eng.plan_run_async_lg(plan, 0, T, LR)
        eng.synchronize()

    res["legs"].append(leg("per call: lg_async_step", per_call, parent, reset))
    res["legs"].append(leg("row plan: plan_run_async_lg + synchronize", lambda: run(rows_plan), parent, reset))
    res["legs"].append(leg("slice plan: plan_run_async_lg + synchronize, one persistent launch", lambda: run(slice_plan), parent, reset))
    reset()
    per_call()
    w_calls = eng.get_weights()
    reset()
    run(rows_plan)
    res["row_plan_bit_equal_to_calls"] = bool(np.array_equal(w_calls.view(np.uint32), eng.get_weights().view(np.uint32)))
    reset()
    run(slice_plan)
    res["slice_plan_max_abs_diff_to_calls"] = float(np.max(np.abs(eng.get_weights().astype(np.float64) - w_calls)))
    rows_plan.destroy()
    slice_plan.destroy()
print(json.dumps(res))
