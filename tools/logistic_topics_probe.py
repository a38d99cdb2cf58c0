"""Several topics against the parent's way: microseconds per step of ONE dsgd_lg_topics_sync_steps call over T topics, and of T
single-model contexts (each holding its own copy of the matrix) stepped one after the other by dsgd_lg_sync_steps -- at the
reference's batch sizes 3 x 100 and at 4 x 4,096, for T = 1, 2, 4, 8.

    python tools/logistic_topics_probe.py [--rows 23149] [--steps 1000] [--calls 10] [--repeats 5] [--out profiles/logistic_topics_probe.json]

Every figure is host wall time around a WINDOW of `calls` calls of `steps` steps each, every call ending in its own
synchronisation (both entry points return behind their kernels): uploads of the lists included on both sides, kernel time alone
not separated.  The defaults make the shortest window (3 x 100, T = 1: 10,000 steps) about 0.4 s and the longest about 6 s, so
that no figure rests on a window of milliseconds; each window's length in seconds is reported beside its figure.  Both sides
are warmed with one call of the timed shape; the two are alternated `repeats` times and the median and the spread (min, max)
are reported.  The weights are compared bit for bit after the warm-up pair.  A run without a gfx950 device fails:
there is no fallback.  One JSON line goes to stdout and to --out."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=23149)
ap.add_argument("--steps", type=int, default=1000, help="steps per call")
ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--lam", type=float, default=1e-5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "logistic_topics_probe.json"))
a = ap.parse_args()
if dsgd_amd.device_count() < 1:
    sys.exit("logistic_topics_probe: no gfx950 device (nothing is measured without one)")

data = dsgd_amd.synth.generate(a.rows, seed=0)
rng = np.random.default_rng(1)
planes = np.ascontiguousarray(np.vstack([data.label[None].astype(np.int8), rng.choice(np.array([-1, 1], np.int8), size=(7, data.n_rows))]))
LR = 2.0 ** -10


def lists_for(k, batch):
    r = np.random.default_rng(100 * k + batch)
    flat = r.integers(0, data.n_rows, size=a.steps * k * batch).astype(np.int32)
    offs = np.arange(0, a.steps * k * batch + 1, batch, dtype=np.int64)
    return flat, offs


def timed(fn):
    t0 = time.perf_counter()
    for _ in range(a.calls):
        fn()
    return (time.perf_counter() - t0) * 1e6 / (a.steps * a.calls)


result = {"rows": data.n_rows, "steps_per_call": a.steps, "calls_per_window": a.calls, "repeats": a.repeats, "unit": "us per step, host wall time around synchronising calls",
          "shapes": []}
singles = []
for t in range(8):
    e = dsgd_amd.Engine(data.dim, a.lam)
    e.load_csr(data.row_ptr, data.col, data.val, planes[t])
    singles.append(e)
with dsgd_amd.Engine(data.dim, a.lam) as eng:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    for k, batch in ((3, 100), (4, 4096)):
        flat, offs = lists_for(k, batch)
        for T in (1, 2, 4, 8):
            eng.lg_topics_set(planes[:T])
            zero = np.zeros(data.dim + 1, dtype=np.float32)

            def run_topics():
                eng.lg_topics_sync_steps(flat, offs, a.steps, k, LR)

            def run_singles():
                for t in range(T):
                    singles[t].lg_sync_steps(flat, offs, a.steps, k, LR)

            for t in range(T):
                singles[t].set_weights(zero)
            run_topics(), run_singles()                                   # warm-up of the timed shape; then the bits
            W = eng.lg_topics_get_weights()
            same = all(np.array_equal(W[t].view(np.uint32), singles[t].get_weights().view(np.uint32)) for t in range(T))
            tt, ts = [], []
            for _ in range(a.repeats):                                    # alternated
                tt.append(timed(run_topics))
                ts.append(timed(run_singles))
            result["shapes"].append({"workers": k, "batch": batch, "T": T, "bits_equal": bool(same),
                                     "shortest_window_s": min(tt + ts) * a.steps * a.calls * 1e-6,
                                     "topics_us": {"median": float(np.median(tt)), "min": min(tt), "max": max(tt)},
                                     "singles_us": {"median": float(np.median(ts)), "min": min(ts), "max": max(ts)}})
for e in singles:
    e.close()
line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
