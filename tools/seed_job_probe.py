"""Milliseconds per epoch of plan creation, the lists drawn by the device in its two forms and by the host's generator.

One JSON line (kept as profiles/seed_job_probe.json).  N = 804,414 rows of which 643,531 train (RCV1's sizes; the lists do
not depend on the rows' contents: cheap rows).  One process, one engine; after a warm-up round the legs ALTERNATE for
5 rounds, and each leg reports the median and min .. max of its 5 creations (the plan is destroyed outside the timing):
  a  Engine.plan_from_seed, 3 workers x 100 rows                       (the existing form)
  b  Engine.plan_from_seed_job, the same job hosted whole
  c  the job form for one rank's window of an 8-worker job, n_local = 1, batch 100
  d  the job form at 4 workers x 4,096 rows
  e  the job form on ONE worker over all 643,531 train rows, batch 100  (the existing form refuses: > 64 rejections)
  f  host.epoch_lists(native=True) over the jobs of c, d and e          (csrc/jrand.c on this machine's threads)
A leg the library refuses reports "refused" and its code.  No default depends on these figures."""

import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dsgd_amd  # noqa: E402
from dsgd_amd import host  # noqa: E402

N_ROWS, N_TRAIN = 804414, 643531
ROUNDS = 5


def main():
    state0 = host.JavaRandom(0).seed
    data = dsgd_amd.synth.generate(N_ROWS, seed=3, dim=1000, nnz_mean=4)
    jobs = {name: host.split_vanilla(N_TRAIN, k) for name, k in (("a", 3), ("c", 8), ("d", 4), ("e", 1))}
    batch = {"a": 100, "c": 100, "d": 4096, "e": 100}
    with dsgd_amd.Engine(data.dim, 1e-5) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(N_TRAIN)

        def device(form, name, first=0, n_local=None):
            split = jobs[name]
            max_samples = max(len(r) for r in split)

            def leg():
                t0 = time.perf_counter()
                if form == "old":
                    plan = eng.plan_from_seed(state0, split, max_samples, batch[name])[0]
                else:
                    mine = split[first:first + (n_local or len(split))]
                    plan = eng.plan_from_seed_job(state0, [len(r) for r in split], first, [r.start for r in mine], max_samples, batch[name])[0]
                dt = time.perf_counter() - t0
                if plan is not None:
                    plan.destroy()
                eng.synchronize()
                return dt
            return leg

        def on_host(name):
            split = jobs[name]

            def leg():
                rnd = host.JavaRandom(0)
                t0 = time.perf_counter()
                host.epoch_lists(rnd, split, max(len(r) for r in split), batch[name], native=True)
                return time.perf_counter() - t0
            return leg

        legs = {"a_plan_from_seed_3x100": device("old", "a"), "b_job_form_3x100_whole": device("job", "a"),
                "c_job_form_window_1_of_8_x100": device("job", "c", 0, 1), "d_job_form_4x4096": device("job", "d"),
                "e_job_form_1x100_643531_rows": device("job", "e"), "e_old_form_1x100_643531_rows": device("old", "e"),
                "f_host_8x100": on_host("c"), "f_host_4x4096": on_host("d"), "f_host_1x100_643531_rows": on_host("e")}
        times = {k: [] for k in legs}
        refused = {}
        for rnd_ in range(ROUNDS + 1):   # (round 0: the warm-up)
            for k, leg in legs.items():
                if k in refused:
                    continue
                try:
                    dt = leg()
                except dsgd_amd.DsgdError as e:
                    refused[k] = e.code
                    continue
                if rnd_:
                    times[k].append(dt * 1e3)
    out = {"probe": "seed_job_probe", "n_rows": N_ROWS, "n_train": N_TRAIN, "rounds": ROUNDS, "host_threads": os.environ.get("DSGD_HOST_THREADS", "online CPUs capped at 32"),"unit": "ms per epoch of plan creation",
           "legs": {k: ({"refused": refused[k]} if k in refused else
                        {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}) for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
