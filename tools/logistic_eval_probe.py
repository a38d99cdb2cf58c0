"""The logistic model's distributed and sampled evaluation beside the calls that gave the same information before, in one
process: one JSON (profiles/logistic_eval_probe.json).

    python tools/logistic_eval_probe.py [--repeat 5] [--out profiles/logistic_eval_probe.json]

Data: synth.generate(23149, seed=1), the 18,519 train rows; standard normal weights (logits of standard deviation about 1).
Every leg is warmed up, then the new call and its baseline are timed ALTERNATELY `--repeat` times: host wall time around
`calls` calls, each of which returns behind its kernels (every call here ends in one synchronise).  Reported: median
[min .. max] microseconds per call and the ratio of the medians, new / baseline.

  predict_ranges  lg_predict_ranges(3 splits of the 18,519 rows, want_proba=True)      against lg_loss_acc_ranges(the 3 splits) +
                  lg_predict_proba(arange(18519)) -- the classes folded from the probabilities on the host are NOT timed
  list            lg_loss_acc_list(1,000 rows)         against lg_predict_proba(the 1,000 rows) + the fold on the host (labels, log)
  sampled         lg_loss_acc_sampled(1,000 of the 18,519)    against host.sampled_list + lg_loss_acc_list
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd
from dsgd_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logistic_eval_probe.json"))
a = ap.parse_args()
LAM = 1e-5


def stat(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def timed(fn):
    t0 = time.perf_counter()
    for _ in range(a.calls):
        fn()
    return (time.perf_counter() - t0) / a.calls * 1e6


def leg(name, new, base, same):
    for fn in (new, base):   # warm-up
        fn()
    runs = {"new": [], "base": []}
    for _ in range(a.repeat):   # alternated
        runs["new"].append(timed(new))
        runs["base"].append(timed(base))
    return {"leg": name, "calls_per_run": a.calls, "new_us_per_call": stat(runs["new"]), "baseline_us_per_call": stat(runs["base"]),
            "ratio_new_to_baseline": round(float(np.median(runs["new"]) / np.median(runs["base"])), 3), "same_figures": bool(same())}


data = dsgd_amd.synth.generate(23149, seed=1)
n_train = int(23149 * 0.8)
res = {"tool": "tools/logistic_eval_probe.py", "repeat": a.repeat, "rows": n_train, "legs": [],
       "not_measured": ["kernel time alone (every figure is host wall time around calls that synchronise)", "256 ranges", "lists beyond 1,000 rows",
                        "windows that reject inside the shuffle", "a second process or a busy device", "the host fold of classes from probabilities"]}
with dsgd_amd.Engine(data.dim, LAM) as eng:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    w = np.random.default_rng(3).standard_normal(eng.dp).astype(np.float32)
    eng.set_weights(w)   # (the rows are L2-normalised: logits of standard deviation about 1)
    ranges = [(r.start, r.stop) for r in host.split_vanilla(n_train, 3)]
    every = np.arange(n_train, dtype=np.int32)
    y = np.asarray(data.label, dtype=np.float64)

    def base_ranges():
        return eng.lg_loss_acc_ranges(ranges), eng.lg_predict_proba(every)

    def same_ranges():
        cls, proba, counts, range_loss, _, _ = eng.lg_predict_ranges(ranges, want_proba=True)
        la, pb = base_ranges()
        return (np.array_equal(proba.view(np.uint32), pb.view(np.uint32)) and
                all(la[r] == (range_loss[r], counts[r][0] / float(e - b)) for r, (b, e) in enumerate(ranges)))

    res["legs"].append(leg("predict_ranges: 3 splits of %d rows" % n_train, lambda: eng.lg_predict_ranges(ranges, want_proba=True), base_ranges, same_ranges))

    idx = np.random.default_rng(5).permutation(n_train)[:1000].astype(np.int32)

    def base_list():   # what a user had: the probabilities, and the loss and the tallies folded here
        pr = eng.lg_predict_proba(idx).astype(np.float64)
        yy = y[idx]
        cls = np.sign(pr - 0.5)
        with np.errstate(divide="ignore"):
            li = -np.log(np.where(yy > 0, pr, 1.0 - pr))
        return float(np.mean(li)), float(np.count_nonzero(cls == yy)) / len(idx)

    def same_list():   # (the host fold works from the ROUNDED probability: the same accuracy, a loss within float rounding)
        loss, acc, _ = eng.lg_loss_acc_list(idx)
        bl, ba = base_list()
        return acc == ba and abs(loss - LAM * float(np.dot(w.astype(np.float64), w.astype(np.float64))) - bl) < 1e-4

    res["legs"].append(leg("list: 1,000 rows", lambda: eng.lg_loss_acc_list(idx), base_list, same_list))

    state = host.JavaRandom(7).seed

    def base_sampled():
        rnd = host.JavaRandom(0)
        rnd.seed = state
        return eng.lg_loss_acc_list(host.sampled_list(rnd, n_train, 1000)), rnd.seed

    def same_sampled():
        loss, acc, counts, st, _ = eng.lg_loss_acc_sampled(state, 0, n_train, 1000)
        return ((loss, acc, counts), st) == base_sampled()

    res["legs"].append(leg("sampled: 1,000 of %d rows" % n_train, lambda: eng.lg_loss_acc_sampled(state, 0, n_train, 1000), base_sampled, same_sampled))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
