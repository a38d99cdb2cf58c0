"""Logistic plans on column slices against the two-launch form the parent commit had, in one process: one JSON line
(profiles/logistic_slices_probe.json).

    python tools/logistic_slices_probe.py [--repeat 5] > profiles/logistic_slices_probe.json

The method of tools/logistic_plan_probe.py: per leg all sides are warmed up, then timed ALTERNATELY `--repeat` times -- host wall
time around plan_run + synchronize -- and reported as median [min .. max] microseconds per step.  Nothing here is a promise: the
figures are what came out.

  per shape (3 x 100, 4 x 200, 1 x 100; 50-step plans over 23,149 synthetic rows at RCV1's width, the same lists and the same
  weights before every run):
    slices   Engine.lg_plan_flat(slices=True): plan code 8, ONE launch of dsgd_lg_cs_step_kernel
    parent   Engine.lg_plan_flat(): plan code 7, two launches per step -- the parent commit's form
    svm      Engine.plan on the same lists (dsgd_cs_step_kernel, dimSparsity built): another model, beside it for scale
  create   plan creation alone (the upload; with slices: the layout's two passes too), ended by a device synchronise
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
a = ap.parse_args()
LAM, LR, ROWS, STEPS = 1e-5, 2.0 ** -3, 23149, 50
N_TRAIN = int(ROWS * 0.8)


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def stats(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def legs(sides, per, before):
    """every side warmed up three times, then all of them alternated `repeat` times; `before` runs untimed in front of every run"""
    runs = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(3):
            before()
            fn()
    for _ in range(a.repeat):
        for k, fn in sides.items():
            before()
            runs[k].append(wall_us(fn) / per)
    return {k: stats(v) for k, v in runs.items()}


res = {"tool": "tools/logistic_slices_probe.py", "repeat": a.repeat, "rows": ROWS, "steps": STEPS, "unit": "us per step (create: us per plan)",
       "shapes": []}
data = dsgd_amd.synth.generate(ROWS, seed=1)
with dsgd_amd.Engine(data.dim, LAM) as eng:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(N_TRAIN)
    w0 = np.zeros(eng.dp, dtype=np.float32)
    rng = np.random.default_rng(0)
    for K, B in ((3, 100), (4, 200), (1, 100)):
        steps = [[rng.integers(0, N_TRAIN, size=B).astype(np.int32) for _ in range(K)] for _ in range(STEPS)]
        idx = np.concatenate([l for s in steps for l in s])
        offs = np.arange(STEPS * K + 1, dtype=np.int64) * B
        plans = {"slices": eng.lg_plan_flat(idx, offs, STEPS, K, slices=True), "parent": eng.lg_plan_flat(idx, offs, STEPS, K), "svm": eng.plan(steps)}
        kinds = {k: p.info()["kind"] for k, p in plans.items()}

        def run(p):
            eng.plan_run(p, 0, STEPS, LR)
            eng.synchronize()

        def reset():
            eng.set_weights(w0)
            eng.synchronize()

        out = {"shape": "%d x %d" % (K, B), "plan_kinds": kinds}
        out["run"] = legs({k: (lambda p=p: run(p)) for k, p in plans.items()}, STEPS, reset)
        out["ratio_slices_to_parent"] = round(out["run"]["slices"]["median"] / out["run"]["parent"]["median"], 3)
        kernels = {}
        for k, p in plans.items():
            reset()
            run(p)
            kernels[k] = eng.grad_kernel_name()
        out["kernels"] = kernels
        for p in plans.values():
            p.destroy()

        def create(slices):
            p = eng.lg_plan_flat(idx, offs, STEPS, K, slices=slices)
            eng.plan_run(p, 0, 0, LR)      # (an empty range: the launch stream waits for the plan's set-up, nothing runs)
            eng.synchronize()
            p.destroy()

        out["create"] = legs({"slices": lambda: create(True), "parent": lambda: create(False)}, 1, lambda: None)
        res["shapes"].append(out)
print(json.dumps(res))
