"""The logistic model's whole-split steps by column lists beside its row form, in one process: one JSON
(profiles/logistic_cols_probe.json).

    python tools/logistic_cols_probe.py [--repeat 5] [--big-rows 804414] [--out profiles/logistic_cols_probe.json]

Per shape the FIRST lg_sync_steps_ranges call, which lays the ranges out, is timed on its own (one step, wall time around the
call).  Then both legs are warmed up and timed ALTERNATELY `--repeat` times: host wall time around `steps` steps ending in one
synchronise -- ONE lg_sync_steps_ranges call of `steps` steps against a loop of `steps` lg_sync_step_ranges calls (unchanged
code: the baseline; every call of it returns behind its kernels).  Reported: median [min .. max] microseconds per step, the
ratio of the medians, the bytes a step of the column form reads (8 per entry, the coefficient gathers and the dot's pass over
the CSR) as a fraction of 8 TB/s, and whether the two legs left bit-equal weights.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--big-rows", type=int, default=804414)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logistic_cols_probe.json"))
a = ap.parse_args()
LAM, PEAK = 1e-5, 8e12


def stat(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def legs(eng, data, ranges, steps):
    rows = sum(e - b for b, e in ranges)
    nnz = sum(int(data.row_ptr[e] - data.row_ptr[b]) for b, e in ranges)
    lr = 0.5 * 100 / rows
    w0 = np.zeros(eng.dp, dtype=np.float32)

    def cols():
        t0 = time.perf_counter()
        eng.lg_sync_steps_ranges(ranges, steps, lr)
        return (time.perf_counter() - t0) / steps * 1e6

    def rowform():
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.lg_sync_step_ranges(ranges, lr)
        return (time.perf_counter() - t0) / steps * 1e6

    eng.set_weights(w0)
    eng.lg_sync_step_ranges(ranges, lr)          # (the ranking, the accumulators: not the layout's cost)
    eng.set_weights(w0)
    t0 = time.perf_counter()
    eng.lg_sync_steps_ranges(ranges, 1, lr)      # the first call: the layout is built here
    first_us = (time.perf_counter() - t0) * 1e6
    kernel = eng.grad_kernel_name()
    runs, w_end = {"cols": [], "rows": []}, {}
    for fn in (cols, rowform):                   # warm-up
        eng.set_weights(w0)
        fn()
    for _ in range(a.repeat):                    # alternated
        for key, fn in (("cols", cols), ("rows", rowform)):
            eng.set_weights(w0)
            runs[key].append(fn())
            w_end[key] = eng.get_weights()
    col_bytes = nnz * 8 + nnz * 8 + nnz * 8 + (rows + 1) * 8 + rows + rows * 8   # entries, coefficient gathers, the dot's CSR pass, the table
    out = {"shape": "%d x %s rows" % (len(ranges), "/".join(str(e - b) for b, e in ranges[:3])), "workers": len(ranges), "rows": rows, "entries": nnz,
           "steps_per_run": steps, "kernel": kernel, "first_call_us": round(first_us, 1),
           "cols_us_per_step": stat(runs["cols"]), "rows_us_per_step": stat(runs["rows"]),
           "ratio_cols_to_rows": round(float(np.median(runs["cols"]) / np.median(runs["rows"])), 3),
           "cols_bytes_per_step": int(col_bytes),
           "cols_fraction_of_8TBps": round(col_bytes / (float(np.median(runs["cols"])) * 1e-6) / PEAK, 4),
           "weights_bit_equal": bool(np.array_equal(w_end["cols"].view(np.uint32), w_end["rows"].view(np.uint32)))}
    return out


res = {"tool": "tools/logistic_cols_probe.py", "repeat": a.repeat, "legs": [], "not_measured": []}
small = dsgd_amd.synth.generate(23149, seed=1)
n_train = int(23149 * 0.8)
with dsgd_amd.Engine(small.dim, LAM) as eng:
    eng.load_csr(small.row_ptr, small.col, small.val, small.label)
    res["legs"].append(legs(eng, small, [(0, n_train)], 50))
    third = n_train // 3
    res["legs"].append(legs(eng, small, [(i * third, (i + 1) * third) for i in range(3)], 50))
if a.big_rows > 0:
    big = dsgd_amd.synth.generate(a.big_rows, seed=2)
    n_train = int(a.big_rows * 0.8)
    with dsgd_amd.Engine(big.dim, LAM) as eng:
        eng.load_csr(big.row_ptr, big.col, big.val, big.label)
        res["legs"].append(legs(eng, big, [(0, n_train)], 10))
else:
    res["not_measured"].append("range of 643,531 rows")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
