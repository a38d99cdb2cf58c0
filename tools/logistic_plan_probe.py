"""Resident logistic plans, device-drawn lists and the several-ranges evaluation against the calls that were there, in one
process: one JSON line (profiles/logistic_plan_probe.json).

    python tools/logistic_plan_probe.py [--repeat 5] > profiles/logistic_plan_probe.json

The method of tools/logistic_probe.py: per leg both sides are warmed up, then timed ALTERNATELY `--repeat` times -- host wall
time around work that ends in a device synchronise -- and reported as median [min .. max] microseconds with the ratio of the
medians.  The right-hand side of every leg is code the parent commit had (dsgd_lg_sync_steps, host.epoch_lists + an upload,
two dsgd_lg_loss_acc calls): the baseline, in the same process.  Nothing here is a promise: the figures are what came out.

  steps       50 steps of 3 workers x 100 rows: plan_run + synchronize (the lists resident) against lg_sync_steps (the lists
              uploaded by the call), the same lists, the same weights before
  lists       an epoch's lists as a plan (18,519 train rows, 3 workers, batch 100: 62 steps): lg_plan_from_seed (the device
              draws) against epoch_lists (the host draws, csrc/jrand.c) + lg_plan_flat (the upload)
  evaluation  train and test in one lg_loss_acc_ranges call against two lg_loss_acc calls, at 18,519 and 4,630 rows
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd
from dsgd_amd import host

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
a = ap.parse_args()
LAM, ROWS = 1e-5, 23149
N_TRAIN = int(ROWS * 0.8)   # 18,519 train rows, 4,630 test rows


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def leg(name, new, old, per=1, before=lambda: None, unit="us"):
    """`new` against `old`, each a callable that returns behind its device work; `before` runs untimed in front of every run."""
    runs = {"new": [], "parent": []}
    for fn in (new, old):   # warm-up: allocations, layouts, clocks
        for _ in range(3):
            before()
            fn()
    for _ in range(a.repeat):   # alternated
        for key, fn in (("new", new), ("parent", old)):
            before()
            runs[key].append(wall_us(fn) / per)
    out = {"leg": name, "unit": unit}
    for key, v in runs.items():
        out[key] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    out["ratio_new_to_parent"] = round(float(np.median(runs["new"]) / np.median(runs["parent"])), 3)
    return out


res = {"tool": "tools/logistic_plan_probe.py", "repeat": a.repeat, "rows": ROWS, "n_train": N_TRAIN, "legs": []}
data = dsgd_amd.synth.generate(ROWS, seed=1)
with dsgd_amd.Engine(data.dim, LAM) as eng:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    w0 = np.zeros(eng.dp, dtype=np.float32)
    rng = np.random.default_rng(0)
    # ---- steps: 3 x 100 x 50 ----
    K, T, lr = 3, 50, 0.5
    lists = [rng.integers(0, N_TRAIN, size=100).astype(np.int32) for _ in range(K * T)]
    flat = np.concatenate(lists)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    plan = eng.lg_plan_flat(flat, offs, T, K)

    def run_plan():
        eng.plan_run(plan, 0, T, lr)
        eng.synchronize()

    res["legs"].append(leg("50 steps of 3 x 100 rows: plan_run + synchronize vs lg_sync_steps", run_plan, lambda: eng.lg_sync_steps(flat, offs, T, K, lr),
                           per=T, before=lambda: eng.set_weights(w0), unit="us per step"))
    eng.set_weights(w0)
    run_plan()
    w_plan = eng.get_weights()
    eng.set_weights(w0)
    eng.lg_sync_steps(flat, offs, T, K, lr)
    res["steps_bit_equal"] = bool(np.array_equal(w_plan.view(np.uint32), eng.get_weights().view(np.uint32)))
    plan.destroy()
    # ---- lists: an epoch's plan, drawn by the device against drawn by the host and uploaded ----
    split = host.split_vanilla(N_TRAIN, K)
    max_samples = max(len(r) for r in split)
    seed0 = host.JavaRandom(0).seed

    def from_seed():
        p, _, _, _ = eng.lg_plan_from_seed(seed0, split, max_samples, 100)
        eng.plan_lists(p)   # (ends behind the draw: the lists are read back)
        p.destroy()

    def from_host():
        idx, o, n = host.epoch_lists(host.JavaRandom(0), split, max_samples, 100)
        p = eng.lg_plan_flat(idx, o, n, K)
        eng.plan_lists(p)
        p.destroy()

    res["legs"].append(leg("an epoch's plan (3 x 6,173 rows, batch 100): lg_plan_from_seed vs epoch_lists + lg_plan_flat", from_seed, from_host,
                           unit="us per plan (creation + a read-back of the lists)"))
    # ---- evaluation: train and test ----
    eng.set_weights(w_plan)
    both = [(0, N_TRAIN), (N_TRAIN, ROWS)]

    def two_calls():
        eng.lg_loss_acc(0, N_TRAIN)
        eng.lg_loss_acc(N_TRAIN, ROWS)

    res["legs"].append(leg("train (18,519 rows) and test (4,630 rows): one lg_loss_acc_ranges vs two lg_loss_acc", lambda: eng.lg_loss_acc_ranges(both), two_calls,
                           unit="us per epoch's evaluation"))
    one = eng.lg_loss_acc_ranges(both)
    res["evaluation_bit_equal"] = bool(one == [eng.lg_loss_acc(0, N_TRAIN), eng.lg_loss_acc(N_TRAIN, ROWS)])
print(json.dumps(res))
