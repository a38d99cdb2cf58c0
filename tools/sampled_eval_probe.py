#!/usr/bin/env python3
"""What a sampled check costs, one JSON line, us per call at the Python binding:

  device    ONE Engine.loss_acc_sampled call: the device draws the sample and tallies it (dsgd_loss_acc_sampled)
  list      the host draws the sample (csrc/jrand.c: dsgd_jrand_shuffle), then ONE Engine.loss_acc_list call
  forward   the host draws the sample, Engine.forward over it, the tallies folded on the host -- what a user had to do
            before the list forms existed

for windows of len = 23,149 and len = 804,414 synthetic RCV1-like rows and samples_count in {1,000; 10,000; len}, from normal
weights on an fp32 engine.  Every figure comes with the draw's share of it: for `list` and `forward` the host shuffle timed
on its own, for `device` the call minus a loss_acc_list call over the same rows.  Three runs in one process; inside a run
the routes alternate --reps times (after one untimed round) and the run's figure is the median of its repetitions; reported:
the median and the min ... max of the three runs.  Wall-clock time around calls that end behind their own synchronisation.

    python tools/sampled_eval_probe.py > profiles/sampled_eval_probe.json
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


def case(eng, label, length, k, reps):
    state0 = host.JavaRandom(0).seed
    rnd = host.JavaRandom(0)
    label = np.asarray(label, dtype=np.float64)

    def draw():
        rnd.seed = state0
        return host.sampled_list(rnd, length, k)

    def by_forward():
        idx = draw()
        yp = label[idx] * eng.forward(idx)
        n = len(idx)
        c = [int(np.count_nonzero(yp > 0)), int(np.count_nonzero(yp == 0)), int(np.count_nonzero(yp < 0))]
        return c[0] / n, c

    idx0 = draw()
    calls = {"device": lambda: eng.loss_acc_sampled(state0, 0, length, k),
             "list": lambda: eng.loss_acc_list(draw()),
             "forward": by_forward,
             "draw_on_host": draw,
             "list_without_draw": lambda: eng.loss_acc_list(idx0)}
    # the routes agree before anything is timed
    loss_d, acc_d, counts_d, state_d, _ = calls["device"]()
    assert (loss_d, acc_d, counts_d) == calls["list"]() and state_d == rnd.seed
    assert calls["forward"]() == (acc_d, counts_d)
    runs = {name: [] for name in calls}
    for _ in range(3):
        ts = {name: [] for name in calls}
        for rep in range(reps + 1):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    ts[name].append((time.perf_counter() - t0) * 1e6)
        for name in calls:
            runs[name].append(float(np.median(ts[name])))
    out = {name: summary(v) for name, v in runs.items()}
    med = {name: out[name]["median"] for name in out}
    out.update({"len": length, "samples_count": k,
                "draw_share": {"device": round(max(0.0, med["device"] - med["list_without_draw"]) / med["device"], 3),
                               "list": round(med["draw_on_host"] / med["list"], 3),
                               "forward": round(med["draw_on_host"] / med["forward"], 3)}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", type=int, nargs="*", default=[23149, 804414])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if dsgd_amd.device_count() < 1:
        print(json.dumps({"status": "not run", "reason": "no gfx950 device"}))
        return 1
    out = {"status": "run", "reps": args.reps, "runs": 3, "precision": "fp32",
           "unit": "us per call (median of the runs' medians, min ... max of the runs)", "cases": []}
    for length in args.lens:
        data = dsgd_amd.synth.generate(length, seed=0)
        w = np.random.default_rng(1).normal(size=data.dim + 1).astype(np.float32)
        with dsgd_amd.Engine(data.dim, LAM) as eng:
            eng.load_csr(data.row_ptr, data.col, data.val, data.label)
            eng.build_dim_sparsity(length)
            eng.set_weights(w)
            for k in (1000, 10000, length):
                out["cases"].append(case(eng, data.label, length, k, args.reps))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
