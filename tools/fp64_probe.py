"""The fp64 mode against the fp32 engine on the reference's shipped step sizes (include/dsgd.h "THE FP64 MODE").

One GPU run, one JSON line: for 3 x 100 (application.conf) and 4 x 200 (kube/config-sync.yaml) over N = 804,414 synthetic
RCV1-like rows (80 % train, lr 0.5, java.util.Random(0) lists), per precision
  us_per_step            median over 5 epochs of plan_run + synchronize (after one warm-up epoch), per step
  first_divergent_step   the oracle replaying the engine's recorded gate decisions (oracle/sync_replay.py): None = every
                         decision is the oracle's own
  epoch1_max_abs_diff    max |w - w_oracle| after the epoch (the oracle's own trajectory)

    python tools/fp64_probe.py [--rows 804414] [--epochs 5]
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
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
o.set_dim_sparsity(o.dim_sparsity(n_train))
out = {"rows": a.rows, "n_train": n_train, "lr": LR, "lambda": LAM}
for k, batch in ((3, 100), (4, 200)):
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
print(json.dumps(out))
