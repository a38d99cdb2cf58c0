"""The fp64 mode against the fp32 engine on the reference's shipped step sizes (include/dsgd.h "THE FP64 MODE").

One GPU run, one JSON line: for 3 x 100 (application.conf) and 4 x 200 (kube/config-sync.yaml) over N = 804,414 synthetic
RCV1-like rows (80 % train, lr 0.5, java.util.Random(0) lists), per precision
  us_per_step            median over 5 epochs of plan_run + synchronize (after one warm-up epoch), per step
  first_divergent_step   the oracle replaying the engine's recorded gate decisions (oracle/sync_replay.py): None = every
                         decision is the oracle's own
  epoch1_max_abs_diff    max |w - w_oracle| after the epoch (the oracle's own trajectory)
and the asynchronous iteration ("async", --async-updates updates of 3 workers x 100 on the zero-lag schedule):
  us_per_update          median over 5 runs of plan_run_async + synchronize of one resident plan, per update
  us_per_async_step_f64  / us_per_update_grad_f64: median per call of the per-call entries (their delta gossiped back)
  differing_decisions    the engine's recorded gate decisions against the oracle's sequential replay; max_abs_diff

    python tools/fp64_probe.py [--rows 804414] [--epochs 5] [--async-updates 20000] [--async-only]
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
from oracle import oracle as orc
from oracle import sync_replay

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=804414)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--async-updates", type=int, default=20000)
ap.add_argument("--async-only", action="store_true")
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
o.set_dim_sparsity(o.dim_sparsity(n_train))
out = {"rows": a.rows, "n_train": n_train, "lr": LR, "lambda": LAM}
for k, batch in (() if a.async_only else ((3, 100), (4, 200))):
    split = host.split_vanilla(n_train, k)
    idx, offsets, n_steps = host.epoch_lists(host.JavaRandom(0), split, max(len(r) for r in split), batch)
    steps = [[idx[offsets[s * k + j]:offsets[s * k + j + 1]] for j in range(k)] for s in range(n_steps)]
    w_oracle = np.zeros(data.dim + 1)
    for lists in steps:
        o.sync_step(w_oracle, lists, LR)
    cfg = {"steps": n_steps}
    for precision in ("fp32", "fp64"):
        with dsgd_amd.Engine(data.dim, LAM, precision=precision) as eng:
            eng.load_csr(data.row_ptr, data.col, data.val, data.label)
            eng.build_dim_sparsity(n_train)
            zeros = np.zeros(data.dim + 1, dtype=np.float64 if precision == "fp64" else np.float32)
            plan = eng.plan_flat(idx, offsets, n_steps, k)
            times = []
            for _ in range(a.epochs + 1):
                eng.set_weights(zeros)
                eng.synchronize()
                t0 = time.perf_counter()
                eng.plan_run(plan, 0, n_steps, LR)
                eng.synchronize()
                times.append(time.perf_counter() - t0)
            eng.set_weights(zeros)
            plan.record(True)
            eng.plan_run(plan, 0, n_steps, LR)
            eng.synchronize()
            mask, _ = plan.read_record()
            kernel = eng.grad_kernel_name()
            w = eng.get_weights().astype(np.float64)
            plan.destroy()
        w_replay = np.zeros(data.dim + 1)
        stats = sync_replay.replay(o, w_replay, steps, LR, mask)
        cfg[precision] = {"us_per_step": round(float(np.median(times[1:])) / n_steps * 1e6, 3), "kernel": kernel,
                          "first_divergent_step": stats["first_divergent_step"], "differing_decisions": stats["differing"],
                          "epoch1_max_abs_diff": float(np.abs(w - w_oracle).max())}
    cfg["fp64_over_fp32"] = round(cfg["fp64"]["us_per_step"] / cfg["fp32"]["us_per_step"], 3)
    out["%dx%d" % (k, batch)] = cfg

# ---- the asynchronous iteration (core/Slave.scala:79-111, 177-185) on the zero-lag schedule ----
from oracle.hogwild_replay import hog_rows, margins

K, B, SEED, n_up = 3, 100, 0, a.async_updates
split = [(r.start, r.stop) for r in host.split_vanilla(n_train, K)]
lists = [hog_rows(SEED, u % K, u // K, split[u % K][0], split[u % K][1] - split[u % K][0], B, True) for u in range(n_up)]
res = {"workers": K, "batch": B, "updates": n_up}
with dsgd_amd.Engine(data.dim, LAM, precision="fp64") as eng:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(n_train)
    zeros = np.zeros(data.dim + 1)
    plan = eng.async_plan(split, B, seed=SEED, positional_bug=True, first_update=0, n_updates=n_up)
    times = []
    for _ in range(6):
        eng.set_weights(zeros)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.plan_run_async(plan, 0, n_up, LR)
        eng.synchronize()
        times.append(time.perf_counter() - t0)
    eng.set_weights(zeros)
    plan.record(True)
    eng.plan_run_async(plan, 0, n_up, LR)
    mask, _ = plan.read_record()
    w = eng.get_weights()
    res["kernel"] = eng.grad_kernel_name()
    plan.destroy()
    t_step, t_upd = [], []
    for u in range(min(n_up, 600)):
        t0 = time.perf_counter()
        d, _ = eng.async_step(lists[u], LR, want_delta=True)
        t_step.append(time.perf_counter() - t0)
        nz = np.flatnonzero(d)
        t0 = time.perf_counter()
        eng.update_grad(nz, -d[nz])   # (the update undone: a peer's form of the same delta)
        t_upd.append(time.perf_counter() - t0)
res["us_per_update"] = round(float(np.median(times[1:])) / n_up * 1e6, 3)
res["us_per_async_step_f64"] = round(float(np.median(t_step)) * 1e6, 1)
res["us_per_update_grad_f64"] = round(float(np.median(t_upd)) * 1e6, 1)
w_o = np.zeros(data.dim + 1)
differing, first = 0, None
for t, rows in enumerate(lists):
    act = o.label[rows].astype(np.float64) * margins(o, w_o, rows) >= 0
    n_diff = int(np.count_nonzero(mask[t, :len(rows)] != act))
    if n_diff and first is None:
        first = t
    differing += n_diff
    o.async_step(w_o, rows, LR)
res["first_divergent_update"], res["differing_decisions"] = first, differing
res["max_abs_diff"] = float(np.abs(w - w_o).max())
out["async"] = res
print(json.dumps(out))
