#!/usr/bin/env python3
"""What the distributed evaluation costs, one JSON line, us per call at the Python binding:

  predict   ONE Engine.predict_ranges call over the three workers' splits of the train rows (dsgd_predict_ranges: one
            launch, one byte per prediction back, the tallies with it)
  forward   the three Engine.forward(arange(split)) calls it replaces (4 bytes per row up, 4 bytes per prediction back,
            no tallies)
  loss_acc  Engine.loss_acc over the same rows (the tallies alone; nothing per row crosses the boundary)

at N = 23,149 and N = 804,414 synthetic RCV1-like rows (80 % train, SplitStrategy.vanilla over 3 workers), from normal
weights, on an fp32 engine and on an fp64 engine (float values; --fp32-only leaves the second out).  Three runs in one
process; inside a run the three calls alternate --reps times (after one untimed round) and the run's figure is the median
of its repetitions; reported: the median and the min ... max of the three runs.  Wall-clock time around calls that end behind their own synchronisation.

    python tools/predict_probe.py > profiles/predict_probe.json
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


def summary(runs):
    runs = sorted(runs)
    return {"median": round(runs[len(runs) // 2], 1), "min": round(runs[0], 1), "max": round(runs[-1], 1)}


def case(eng, n_train, reps, fp64):
    split = host.split_vanilla(n_train, 3)
    ranges = [(r.start, r.stop) for r in split]
    lists = [np.arange(r.start, r.stop, dtype=np.int32) for r in split]
    fwd = eng.forward_f64 if fp64 else eng.forward
    calls = {"predict": lambda: eng.predict_ranges(ranges),
             "forward": lambda: [fwd(idx) for idx in lists],
             "loss_acc": lambda: eng.loss_acc(0, n_train)}
    # the three agree before anything is timed
    pred, counts, loss, acc = calls["predict"]()
    assert np.array_equal(pred.astype(np.float64), np.concatenate(calls["forward"]()).astype(np.float64))
    l_ref, a_ref, c_ref = calls["loss_acc"]()
    # (ranges of 4,096 rows and more: dsgd_loss_acc streams the split matrix in fixed point, another summation order of
    #  x . w than the row-wise kernels' -- rows a rounding away from the gate may be counted differently)
    tally_diff = int(np.abs(counts.sum(axis=0) - np.asarray(c_ref)).sum())
    runs = {k: [] for k in calls}
    for _ in range(3):
        ts = {k: [] for k in calls}
        for rep in range(reps + 1):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    ts[k].append((time.perf_counter() - t0) * 1e6)
        for k in calls:
            runs[k].append(float(np.median(ts[k])))
    out = {k: summary(v) for k, v in runs.items()}
    out.update({"n_train": n_train, "split": [len(r) for r in split], "tallies_differ_from_loss_acc_by": tally_diff,
                "predict_not_slower_than_forward": bool(out["predict"]["median"] <= out["forward"]["median"]),
                "predict_minus_loss_acc_us": round(out["predict"]["median"] - out["loss_acc"]["median"], 1),
                "loss_acc_spread_us": round(out["loss_acc"]["max"] - out["loss_acc"]["min"], 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[23149, 804414])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fp32-only", action="store_true", help="leave the fp64 engine out")
    args = ap.parse_args()
    if dsgd_amd.device_count() < 1:
        print(json.dumps({"status": "not run", "reason": "no gfx950 device"}))
        return 1
    out = {"status": "run", "reps": args.reps, "runs": 3, "unit": "us per call (median of the runs' medians, min ... max of the runs)",
           "cases": []}
    for rows in args.rows:
        data = dsgd_amd.synth.generate(rows, seed=0)
        n_train = int(rows * 0.8)
        w = np.random.default_rng(1).normal(size=data.dim + 1)
        for precision in ("fp32",) if args.fp32_only else ("fp32", "fp64"):
            with dsgd_amd.Engine(data.dim, LAM, precision=precision) as eng:
                eng.load_csr(data.row_ptr, data.col, data.val, data.label)
                eng.build_dim_sparsity(n_train)
                eng.set_weights(w if precision == "fp64" else w.astype(np.float32))
                c = case(eng, n_train, args.reps, precision == "fp64")
                c.update({"rows": rows, "precision": precision})
                out["cases"].append(c)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
