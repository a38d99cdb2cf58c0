#!/usr/bin/env python3
"""What a loss check of MasterAsync costs while the lock-free engine runs, one JSON line, us per check at
the Python binding:

  loss_acc            Engine.loss_acc(n_train, n_rows): |w|^2 and the tallies on the moving weights
  loss_acc+weights    ... followed by Engine.get_weights(): what an IMPROVING check costs today (189 KB to the host)
  check               Engine.async_check(n_train, n_rows): snapshot, scalars and tallies of the snapshot, the update window
  check+keep          ... followed by Engine.async_check_keep(): an improving check with DSGD_ASYNC_SNAPSHOT=1

on the dev-mode synthetic size (23,149 rows, 80 % train), with 4 and with 256 workers running (batch 100, or the smallest
worker's whole split where that is smaller: 50 rows at 256 workers), from zero weights.  Three runs per worker count, each a fresh engine run; inside a run
the four routes alternate --reps times (after one untimed round) and the run's figure is the median of its repetitions;
reported: the median and the min ... max of the three runs, and the engine's updates per second over the run (the checks
share the device with it).  Wall-clock time around calls that end behind their own synchronisation.

    python tools/async_check_probe.py > profiles/async_check_probe.json
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

LAM = 1e-5
N_ROWS = 23149


def summary(runs):
    runs = sorted(runs)
    return {"median": round(runs[len(runs) // 2], 1), "min": round(runs[0], 1), "max": round(runs[-1], 1)}


def case(eng, dim, n_train, n_rows, workers, reps):
    split = [(r.start, r.stop) for r in host.split_vanilla(n_train, workers)]
    batch = min(100, min(e - b for b, e in split))

    def check_keep():
        eng.async_check(n_train, n_rows)
        eng.async_check_keep()

    def loss_acc_weights():
        eng.loss_acc(n_train, n_rows)
        eng.get_weights()

    calls = {"loss_acc": lambda: eng.loss_acc(n_train, n_rows), "loss_acc+weights": loss_acc_weights,
             "check": lambda: eng.async_check(n_train, n_rows), "check+keep": check_keep}
    runs = {name: [] for name in calls}
    rate = []
    for _ in range(3):
        eng.set_weights(np.zeros(dim + 1, dtype=np.float32))
        eng.async_start(split, batch=batch, lr=0.5, max_updates=1 << 40, seed=1, positional_bug=True)
        try:
            ts = {name: [] for name in calls}
            u0, t_start = eng.async_updates()[0], time.perf_counter()
            for rep in range(reps + 1):
                for name, fn in calls.items():
                    t0 = time.perf_counter()
                    fn()
                    if rep:
                        ts[name].append((time.perf_counter() - t0) * 1e6)
            u1, running = eng.async_updates()
            assert running, "the engine ended under the probe"
            rate.append((u1 - u0) / (time.perf_counter() - t_start))
        finally:
            eng.async_stop()
        for name in calls:
            runs[name].append(float(np.median(ts[name])))
    out = {name: summary(v) for name, v in runs.items()}
    out.update({"workers": workers, "batch": batch, "test_rows": n_rows - n_train,
                "engine_updates_per_s": round(sorted(rate)[1], 0)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, nargs="*", default=[4, 256])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if dsgd_amd.device_count() < 1:
        print(json.dumps({"status": "not run", "reason": "no gfx950 device"}))
        return 1
    n_train = int(N_ROWS * 0.8)
    data = dsgd_amd.synth.generate(N_ROWS, seed=0)
    out = {"status": "run", "reps": args.reps, "runs": 3, "precision": "fp32", "rows": N_ROWS, "n_train": n_train,
           "unit": "us per check (median of the runs' medians, min ... max of the runs)", "cases": []}
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        for workers in args.workers:
            out["cases"].append(case(eng, data.dim, n_train, N_ROWS, workers, args.reps))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
