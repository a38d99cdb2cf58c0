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
there is no fallback.  One JSON line goes to stdout and to --out.

--interleaved: the interleaved form (Engine.lg_topics_set(planes, interleaved=True)) under the same protocol -- for T = 1, 2, 4, 8
against the planar dsgd_lg_topics_sync_steps on the same engine, for T = 16, 32 against T single-model contexts stepped one
after the other; the default --out becomes profiles/logistic_topics_il_probe.json.

--wide: the wide form (Engine.lg_topics_set(planes, wide=True)) under the same protocol -- for T = 1, 8, 32 against the interleaved
form on a second context, for T = 64, 103, 128 against ceil(T / 32) interleaved contexts (each with its own copy of the matrix)
stepped one after the other, which is what serves that many topics without the wide form; --T picks the topic counts of one
run; the default --out becomes profiles/logistic_topics_wide_probe.json.

--ranges: whole-split steps (Engine.lg_topics_sync_steps_ranges: the column lists with the lanes across the topics) -- K = 1 and
K = 4 equal ranges over all rows, T = 8, 32 interleaved and T = 103, 128 wide (--T picks others), against what serves such a step
without them: Engine.lg_topics_sync_steps over arange lists in the same form on a second context.  The same protocol; the
defaults become 50 steps per call and 4 calls per window (a step is milliseconds); the layout of the ranges is built by the
warm-up call and is not in any window; the default --out becomes profiles/logistic_topics_ranges_probe.json.

--softmax: softmax regression over C exclusive classes (Engine.lg_softmax_sync_steps, Engine.lg_softmax_sync_steps_ranges) against
the closest thing there is without it, the wide one-vs-rest step of T = C topics on a second context -- C = 8, 53, 103, 128
(--T picks others) at 3 x 100 and 4 x 4,096 rows per list step and at all rows as ONE range per ranges step.  The same
protocol (the sides alternated `repeats` times, the median and the spread); the two sides compute different models, so no
bits are compared; the ranges windows run steps / 20 steps per call; the default --out becomes
profiles/logistic_softmax_probe.json.

--by-columns: the list steps by the whole matrix's column lists (Engine.lg_topics_sync_steps / lg_softmax_sync_steps with
by_columns=True) on one context against the same call without it on a second, the same lists -- wide topics T = 32 and 103, wide
softmax C = 103, softmax over few classes C = 5, 16 and 32, at 3 x 100 and 4 x 4,096 rows per step, at --rows and at --rows-large
(where the lists are a small share of the matrix and the whole-matrix walk is expected to lose).  No step names a row twice (a
step that does is served by the list launches).  The same protocol; 1000 steps per call at 3 x 100 and 40 at 4 x 4,096 unless
--steps is given, 3 calls per window, the sides alternated `repeats` times (default here 3); the matrix's layout is built by the
warm-up call and is in no window; the weights are compared bit for bit after every warm-up pair; the default --out becomes
profiles/logistic_lists_cols_probe.json."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=23149)
ap.add_argument("--steps", type=int, help="steps per call (default 1000; --ranges: 50)")
ap.add_argument("--calls", type=int, help="calls per timed window (default 10; --ranges: 4)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--lam", type=float, default=1e-5)
ap.add_argument("--interleaved", action="store_true", help="time the interleaved form: against the planar form up to T = 8, against T single models at 16 and 32")
ap.add_argument("--wide", action="store_true", help="time the wide form: against the interleaved form up to T = 32, against ceil(T / 32) interleaved contexts beyond")
ap.add_argument("--ranges", action="store_true", help="time whole-split steps over row ranges against the same rows as arange lists in the same form")
ap.add_argument("--softmax", action="store_true", help="time the softmax list and ranges steps against the wide one-vs-rest step of the same C; "
                                                       "with --interleaved: softmax over 2 to 32 classes with the lanes across the non-zeros against the wide softmax")
ap.add_argument("--by-columns", action="store_true", help="time the list steps by the whole matrix's column lists against the list form on a second context")
ap.add_argument("--rows-large", type=int, default=185192, help="--by-columns: the second, larger matrix")
ap.add_argument("--T", help="--softmax: comma-separated class counts (default 8,53,103,128); --wide / --ranges: comma-separated topic counts (default 1,8,32,64,103,128 / 8,32,103,128)")
ap.add_argument("--out")
a = ap.parse_args()
if a.by_columns:
    if a.wide or a.interleaved or a.ranges or a.softmax:
        sys.exit("logistic_topics_probe: --by-columns is a run of its own")
    if dsgd_amd.device_count() < 1:
        sys.exit("logistic_topics_probe: no gfx950 device (nothing is measured without one)")
    a.calls = a.calls or 3
    a.repeats = 3 if a.repeats == 5 else a.repeats
    a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "logistic_lists_cols_probe.json")
    LR = 2.0 ** -10
    result = {"steps_per_call": {"3x100": a.steps or 1000, "4x4096": a.steps or 40}, "calls_per_window": a.calls, "repeats": a.repeats,
              "unit": "us per step, host wall time around synchronising calls", "shapes": []}
    for n_rows in (a.rows, a.rows_large):
        data = dsgd_amd.synth.generate(n_rows, seed=0)
        rng = np.random.default_rng(1)
        planes = np.ascontiguousarray(np.vstack([data.label[None].astype(np.int8), rng.choice(np.array([-1, 1], np.int8), size=(102, n_rows))]))
        with dsgd_amd.Engine(data.dim, a.lam) as eng, dsgd_amd.Engine(data.dim, a.lam) as other:
            for e in (eng, other):
                e.load_csr(data.row_ptr, data.col, data.val, data.label)
            for k, batch in ((3, 100), (4, 4096)):
                steps = a.steps or (1000 if batch == 100 else 40)
                flat = np.concatenate([rng.permutation(n_rows)[:k * batch] for _ in range(steps)]).astype(np.int32)   # no row twice in a step
                offs = np.arange(0, steps * k * batch + 1, batch, dtype=np.int64)
                for model, n in (("wide topics", 32), ("wide topics", 103), ("wide softmax", 103), ("few-classes softmax", 5), ("few-classes softmax", 16),
                                 ("few-classes softmax", 32)):
                    for e in (eng, other):                                # (from zero weights on both sides)
                        if model == "wide topics":
                            e.lg_topics_set(planes[:n], wide=True)
                        else:
                            e.lg_softmax_set(np.random.default_rng(n).integers(0, n, size=n_rows).astype(np.uint8), n, interleaved=model != "wide softmax")
                    call = (lambda e, **kw: e.lg_topics_sync_steps(flat, offs, steps, k, LR, **kw)) if model == "wide topics" else \
                           (lambda e, **kw: e.lg_softmax_sync_steps(flat, offs, steps, k, LR, **kw))
                    call(eng, by_columns=True), call(other)               # warm-up of the timed shape (and the matrix's layout); then the bits
                    same = bool(np.array_equal(eng.lg_topics_get_weights().view(np.uint32), other.lg_topics_get_weights().view(np.uint32)))
                    tc, tl = [], []
                    for _ in range(a.repeats):                            # alternated
                        for side, fn in ((tc, lambda: call(eng, by_columns=True)), (tl, lambda: call(other))):
                            t0 = time.perf_counter()
                            for _ in range(a.calls):
                                fn()
                            side.append((time.perf_counter() - t0) * 1e6 / (steps * a.calls))
                    result["shapes"].append({"rows": n_rows, "workers": k, "batch": batch, "share_of_rows": k * batch / n_rows, "model": model, "T_or_C": n,
                                             "bits_equal": same, "kernel": eng.grad_kernel_name(), "shortest_window_s": min(tc + tl) * steps * a.calls * 1e-6,
                                             "by_columns_us": {"median": float(np.median(tc)), "min": min(tc), "max": max(tc)},
                                             "lists_us": {"median": float(np.median(tl)), "min": min(tl), "max": max(tl)}})
                    print(json.dumps(result["shapes"][-1]), flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    sys.exit(0)
a.steps = a.steps or (50 if a.ranges else 1000)
a.calls = a.calls or (4 if a.ranges else 10)
a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                              "logistic_softmax_il_probe.json" if a.softmax and a.interleaved else "logistic_softmax_probe.json" if a.softmax else "logistic_topics_ranges_probe.json" if a.ranges else "logistic_topics_wide_probe.json" if a.wide else "logistic_topics_il_probe.json" if a.interleaved else "logistic_topics_probe.json")
softmax_il = a.softmax and a.interleaved   # softmax over few classes, the lanes across the non-zeros, against the wide softmax
if a.wide + a.interleaved + a.ranges + a.softmax > 1 and not (softmax_il and not a.wide and not a.ranges):
    sys.exit("logistic_topics_probe: --wide, --interleaved, --ranges and --softmax are separate runs (--softmax --interleaved is one)")
if dsgd_amd.device_count() < 1:
    sys.exit("logistic_topics_probe: no gfx950 device (nothing is measured without one)")

data = dsgd_amd.synth.generate(a.rows, seed=0)
rng = np.random.default_rng(1)
planes = np.ascontiguousarray(np.vstack([data.label[None].astype(np.int8), rng.choice(np.array([-1, 1], np.int8), size=(127 if a.wide or a.ranges or a.softmax else 31 if a.interleaved else 7, data.n_rows))]))
LR = 2.0 ** -10
wide_T = tuple(int(t) for t in (a.T or "1,8,32,64,103,128").split(","))


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


def write(result):
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


result = {"rows": data.n_rows, "steps_per_call": a.steps, "calls_per_window": a.calls, "repeats": a.repeats, "unit": "us per step, host wall time around synchronising calls",
          "shapes": []}
if softmax_il:
    # the new form on one context, the wide softmax on a second, the same classes; alternated windows, medians with min and max;
    # after the warm-up of every shape the two contexts' weights are compared bit for bit
    with dsgd_amd.Engine(data.dim, a.lam) as eng, dsgd_amd.Engine(data.dim, a.lam) as other:
        for e in (eng, other):
            e.load_csr(data.row_ptr, data.col, data.val, data.label)
        whole, r_steps = [(0, data.n_rows)], max(1, a.steps // 20)
        for C in (int(t) for t in (a.T or "2,5,8,16,32").split(",")):
            cls = rng.integers(0, C, size=data.n_rows).astype(np.uint8)
            eng.lg_softmax_set(cls, C, interleaved=True)
            other.lg_softmax_set(cls, C)
            for k, batch in ((3, 100), (4, 4096), (1, data.n_rows), (0, 0)):
                per_call = a.steps if batch not in (0, data.n_rows) else r_steps
                flat, offs = lists_for(k, batch) if batch not in (0, data.n_rows) else (None, None)

                def run(e):
                    if batch == 0:
                        for _ in range(per_call):
                            e.lg_softmax_loss_acc(0, data.n_rows)
                    elif flat is None:
                        e.lg_softmax_sync_steps_ranges(whole, per_call, LR)
                    else:
                        e.lg_softmax_sync_steps(flat, offs, per_call, k, LR)

                run(eng), run(other)                                      # warm-up of the timed shape (and the ranges' layout)
                same = bool(np.array_equal(eng.lg_topics_get_weights().view(np.uint32), other.lg_topics_get_weights().view(np.uint32)))
                same = same and eng.lg_softmax_loss_acc(0, data.n_rows) == other.lg_softmax_loss_acc(0, data.n_rows)
                til, tw = [], []
                for _ in range(a.repeats):                                # alternated
                    til.append(timed(lambda: run(eng)) * a.steps / per_call)
                    tw.append(timed(lambda: run(other)) * a.steps / per_call)
                result["shapes"].append({"workers": k, "batch": batch, "C": C, "form": "loss_acc" if batch == 0 else "ranges" if flat is None else "lists",
                                         "steps_per_call": per_call, "shortest_window_s": min(til + tw) * per_call * a.calls * 1e-6, "same_bits": same,
                                         "interleaved_us": {"median": float(np.median(til)), "min": min(til), "max": max(til)},
                                         "wide_us": {"median": float(np.median(tw)), "min": min(tw), "max": max(tw)}})
    write(result)
    sys.exit(0)
if a.softmax:
    with dsgd_amd.Engine(data.dim, a.lam) as eng, dsgd_amd.Engine(data.dim, a.lam) as other:
        for e in (eng, other):
            e.load_csr(data.row_ptr, data.col, data.val, data.label)
        whole, r_steps = [(0, data.n_rows)], max(1, a.steps // 20)
        for C in (int(t) for t in (a.T or "8,53,103,128").split(",")):
            eng.lg_softmax_set(rng.integers(0, C, size=data.n_rows).astype(np.uint8), C)   # (from zero weights on both sides)
            other.lg_topics_set(planes[:C], wide=True)
            for k, batch in ((3, 100), (4, 4096), (1, data.n_rows)):
                per_call = r_steps if batch == data.n_rows else a.steps
                flat, offs = (None, None) if batch == data.n_rows else lists_for(k, batch)

                def run_softmax():
                    if flat is None:
                        eng.lg_softmax_sync_steps_ranges(whole, per_call, LR)
                    else:
                        eng.lg_softmax_sync_steps(flat, offs, per_call, k, LR)

                def run_wide():
                    if flat is None:
                        other.lg_topics_sync_steps_ranges(whole, per_call, LR)
                    else:
                        other.lg_topics_sync_steps(flat, offs, per_call, k, LR)

                run_softmax(), run_wide()                                 # warm-up of the timed shape (and the ranges' layout)
                tsm, tw = [], []
                for _ in range(a.repeats):                                # alternated
                    tsm.append(timed(run_softmax) * a.steps / per_call)
                    tw.append(timed(run_wide) * a.steps / per_call)
                result["shapes"].append({"workers": k, "batch": batch, "C": C, "form": "ranges" if flat is None else "lists", "steps_per_call": per_call,
                                         "shortest_window_s": min(tsm + tw) * per_call * a.calls * 1e-6,
                                         "softmax_us": {"median": float(np.median(tsm)), "min": min(tsm), "max": max(tsm)},
                                         "wide_one_vs_rest_us": {"median": float(np.median(tw)), "min": min(tw), "max": max(tw)}})
    write(result)
    sys.exit(0)
if a.ranges:
    with dsgd_amd.Engine(data.dim, a.lam) as eng, dsgd_amd.Engine(data.dim, a.lam) as other:
        for e in (eng, other):
            e.load_csr(data.row_ptr, data.col, data.val, data.label)
        for k in (1, 4):
            cuts = [data.n_rows * i // k for i in range(k + 1)]
            ranges = list(zip(cuts[:-1], cuts[1:]))
            flat = np.tile(np.arange(data.n_rows, dtype=np.int32), a.steps)
            offs = np.concatenate([[0], np.cumsum([e - b for b, e in ranges] * a.steps)]).astype(np.int64)
            for T in (int(t) for t in (a.T or "8,32,103,128").split(",")):
                form = {"interleaved": True} if T <= 32 else {"wide": True}
                for e in (eng, other):
                    e.lg_topics_set(planes[:T], **form)               # (from zero weights on both sides)

                def run_ranges():
                    eng.lg_topics_sync_steps_ranges(ranges, a.steps, LR)

                def run_lists():
                    other.lg_topics_sync_steps(flat, offs, a.steps, k, LR)

                run_ranges(), run_lists()                                 # warm-up of the timed shape (and the layout); then the bits
                same = np.array_equal(eng.lg_topics_get_weights().view(np.uint32), other.lg_topics_get_weights().view(np.uint32))
                tr, tl = [], []
                for _ in range(a.repeats):                                # alternated
                    tr.append(timed(run_ranges))
                    tl.append(timed(run_lists))
                result["shapes"].append({"workers": k, "rows_per_step": data.n_rows, "T": T, "bits_equal": bool(same), "form": next(iter(form)),
                                         "kernel": eng.grad_kernel_name(), "shortest_window_s": min(tr + tl) * a.steps * a.calls * 1e-6,
                                         "ranges_us": {"median": float(np.median(tr)), "min": min(tr), "max": max(tr)},
                                         "lists_us": {"median": float(np.median(tl)), "min": min(tl), "max": max(tl)}})
    write(result)
    sys.exit(0)
singles = []
for t in range(0 if a.wide else 32 if a.interleaved else 8):
    e = dsgd_amd.Engine(data.dim, a.lam)
    e.load_csr(data.row_ptr, data.col, data.val, planes[t])
    singles.append(e)
with dsgd_amd.Engine(data.dim, a.lam) as eng, dsgd_amd.Engine(data.dim, a.lam) as other:
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    other.load_csr(data.row_ptr, data.col, data.val, data.label)      # (--interleaved: the planar form's engine)
    il_parts = [other]                                                # (--wide: the interleaved contexts, 32 topics each)
    for _ in range(-(-max(wide_T) // 32) - 1 if a.wide else 0):
        il_parts.append(dsgd_amd.Engine(data.dim, a.lam))
        il_parts[-1].load_csr(data.row_ptr, data.col, data.val, data.label)
    for k, batch in ((3, 100), (4, 4096)):
        flat, offs = lists_for(k, batch)
        for T in (wide_T if a.wide else (1, 2, 4, 8, 16, 32) if a.interleaved else (1, 2, 4, 8)):
            planar_side = a.interleaved and T <= 8                       # --interleaved: the other side is the planar form while it can be
            eng.lg_topics_set(planes[:T], interleaved=a.interleaved, wide=a.wide)
            zero = np.zeros(data.dim + 1, dtype=np.float32)

            def run_topics():
                eng.lg_topics_sync_steps(flat, offs, a.steps, k, LR)

            def run_singles():
                for t in range(T):
                    singles[t].lg_sync_steps(flat, offs, a.steps, k, LR)

            def run_planar():
                other.lg_topics_sync_steps(flat, offs, a.steps, k, LR)

            def run_il_parts():
                for e in il_parts[:-(-T // 32)]:
                    e.lg_topics_sync_steps(flat, offs, a.steps, k, LR)

            for t in range(0 if a.wide else T):
                singles[t].set_weights(zero)
            if a.wide:
                for i, e in enumerate(il_parts[:-(-T // 32)]):
                    e.lg_topics_set(planes[32 * i:min(32 * i + 32, T)], interleaved=True)
                run_singles = run_il_parts
            if planar_side:
                other.lg_topics_set(planes[:T])
                run_singles = run_planar
            run_topics(), run_singles()                                   # warm-up of the timed shape; then the bits
            W = eng.lg_topics_get_weights()
            if a.wide:
                same = np.array_equal(W.view(np.uint32), np.vstack([e.lg_topics_get_weights() for e in il_parts[:-(-T // 32)]]).view(np.uint32))
            elif planar_side:
                same = np.array_equal(W.view(np.uint32), other.lg_topics_get_weights().view(np.uint32))
            else:
                same = all(np.array_equal(W[t].view(np.uint32), singles[t].get_weights().view(np.uint32)) for t in range(T))
            tt, ts = [], []
            for _ in range(a.repeats):                                    # alternated
                tt.append(timed(run_topics))
                ts.append(timed(run_singles))
            result["shapes"].append({"workers": k, "batch": batch, "T": T, "bits_equal": bool(same),
                                     "topics_side": "wide" if a.wide else "interleaved" if a.interleaved else "planar",
                                     "other_side": "%d interleaved" % -(-T // 32) if a.wide else "planar" if planar_side else "singles",
                                     "shortest_window_s": min(tt + ts) * a.steps * a.calls * 1e-6,
                                     "topics_us": {"median": float(np.median(tt)), "min": min(tt), "max": max(tt)},
                                     "singles_us": {"median": float(np.median(ts)), "min": min(ts), "max": max(ts)}})
for e in singles + il_parts[1:]:
    e.close()
write(result)
