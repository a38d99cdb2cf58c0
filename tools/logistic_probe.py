"""The logistic model's steps beside the SVM's, in one process: one JSON line (profiles/logistic_probe.json).

    python tools/logistic_probe.py [--repeat 5] [--big-rows 804414] > profiles/logistic_probe.json

Per shape both legs are warmed up, then timed ALTERNATELY `--repeat` times: host wall time around `steps` steps ending in one
synchronise (every call of either family returns behind its kernels).  Reported: median [min .. max] microseconds per step,
the ratio of the medians, and for the range shapes the algorithmic bytes of a step (CSR values and ranks, row starts, labels)
as a fraction of 8 TB/s.  The SVM legs are unchanged code: the baseline.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--big-rows", type=int, default=804414)
a = ap.parse_args()
LAM, PEAK = 1e-5, 8e12


def timed(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e6


def legs(eng, name, lg, svm, steps, bytes_per_step=None):
    w0 = np.zeros(eng.dp, dtype=np.float32)
    runs = {"logistic": [], "svm": []}
    for fn in (lg, svm):      # warm-up: allocations, layouts, clocks
        eng.set_weights(w0)
        timed(fn, 3)
    for _ in range(a.repeat):  # alternated
        for key, fn in (("logistic", lg), ("svm", svm)):
            eng.set_weights(w0)
            runs[key].append(timed(fn, steps))
    out = {"shape": name, "steps_per_run": steps}
    for key, v in runs.items():
        out[key + "_us_per_step"] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    out["ratio_logistic_to_svm"] = round(float(np.median(runs["logistic"]) / np.median(runs["svm"])), 3)
    if bytes_per_step is not None:
        out["algorithmic_bytes_per_step"] = int(bytes_per_step)
        for key in runs:
            out[key + "_fraction_of_8TBps"] = round(bytes_per_step / (float(np.median(runs[key])) * 1e-6) / PEAK, 4)
    return out


def range_bytes(data, b, e):
    nnz = int(data.row_ptr[e] - data.row_ptr[b])
    return nnz * 8 + (e - b + 1) * 8 + (e - b)


res = {"tool": "tools/logistic_probe.py", "repeat": a.repeat, "legs": [], "not_measured": []}
small = dsgd_amd.synth.generate(23149, seed=1)
n_train = int(23149 * 0.8)
with dsgd_amd.Engine(small.dim, LAM) as eng:
    eng.load_csr(small.row_ptr, small.col, small.val, small.label)
    eng.build_dim_sparsity(n_train)
    rng = np.random.default_rng(0)
    for k, n, steps in ((3, 100, 200), (1, 4096, 100), (1, 65536, 20)):
        lists = [rng.integers(0, n_train, size=n).astype(np.int32) for _ in range(k)]
        lr = 0.5 * 100 / n
        res["legs"].append(legs(eng, "lists %d x %d (lg_sync_step vs sync_step)" % (k, n), lambda: eng.lg_sync_step(lists, lr),
                                lambda: eng.sync_step(lists, lr), steps))
        if n == 100:   # an epoch's steps in one call against the same number of single calls
            T = 50
            flat = np.concatenate(lists * T)
            offs = np.concatenate([[0], np.cumsum([len(x) for x in lists] * T)])
            v = []
            for _ in range(a.repeat):
                eng.set_weights(np.zeros(eng.dp, dtype=np.float32))
                t0 = time.perf_counter()
                eng.lg_sync_steps(flat, offs, T, k, lr)
                v.append((time.perf_counter() - t0) / T * 1e6)
            res["legs"].append({"shape": "lists 3 x 100, %d steps in one lg_sync_steps call" % T,
                                "logistic_us_per_step": {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}})
    lr = 0.5 * 100 / n_train
    res["legs"].append(legs(eng, "range of %d rows (lg_sync_step_ranges vs sync_step_ranges)" % n_train, lambda: eng.lg_sync_step_ranges([(0, n_train)], lr),
                            lambda: eng.sync_step_ranges([(0, n_train)], lr), 50, range_bytes(small, 0, n_train)))
if a.big_rows > 0:
    big = dsgd_amd.synth.generate(a.big_rows, seed=2)
    n_train = int(a.big_rows * 0.8)
    with dsgd_amd.Engine(big.dim, LAM) as eng:
        eng.load_csr(big.row_ptr, big.col, big.val, big.label)
        eng.build_dim_sparsity(n_train)
        lr = 0.5 * 100 / n_train
        res["legs"].append(legs(eng, "range of %d rows (lg_sync_step_ranges vs sync_step_ranges)" % n_train, lambda: eng.lg_sync_step_ranges([(0, n_train)], lr),
                                lambda: eng.sync_step_ranges([(0, n_train)], lr), 10, range_bytes(big, 0, n_train)))
else:
    res["not_measured"].append("range of 643,531 rows")
print(json.dumps(res))
