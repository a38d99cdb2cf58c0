"""The "dev" role of the reference's Main (Main.scala:32-118, 153-159: master and node-count slaves in one process) on
one MI355X: same `dsgd { ... }` keys / DSGD_* variables, same scenario -- load, 80/20 split, dimSparsity, initial
loss and accuracy, fit (sync or async, early stopping by patience / conv-delta), final weights, final test loss and
accuracy -- with the HIP engine hosting all the workers.

    DSGD_DATA_PATH=/data/rcv1 python tools/train.py [--conf application.conf] [--synthetic ROWS] [--device 0] [--weights-out w.txt]
                                                    [--precision fp64] [--f64-rp-plans] [--model logistic [--lg-plans | --lg-slices] [--lg-async]]

--precision fp64: the engine keeps the reference's Double weights (include/dsgd.h "THE FP64 MODE"); an async fit runs the
zero-lag schedule of host.MasterAsync (one update at a time, every update seen by every worker).
--f64-rp-plans (or DSGD_F64_RP_PLANS=1; with --precision fp64): what the column-slice plans refuse -- real files' Double
feature values, more than 4 workers, batches beyond 1,024 rows -- runs as resident row-parallel plans (include/dsgd.h
"THE FP64 MODE", ROW-PARALLEL PLANS); the asynchronous fit then keeps the files' Doubles too.  With a communicator attached
(one process per GPU, comm_init_f64 / comm_init_f64v) a synchronous epoch then runs as ONE row-parallel plan run per rank on
host-drawn lists, one agreement between the ranks per epoch, instead of one sync_step_f64 per step.  Off by default.
--model logistic: the logistic model on the same rows (include/dsgd.h "THE LOGISTIC MODEL"; fp32; synchronous unless --lg-async): per epoch every
worker's split is shuffled on the host and cut into batches, the epoch's steps run as ONE lg_sync_steps call, and lg_loss_acc
reports train and test log-loss and accuracy.  The default model is the SVM, and nothing changes on its path.
--lg-plans (with --model logistic): Master.fit's flow instead (host.LogisticSync) -- the lists drawn from the reference's random
stream, by the device where it can; an epoch as ONE resident logistic plan, the next one created while it runs; train and test
evaluated in one launch; the reference's early stopping (patience / conv-delta) over the test losses.
--lg-slices (implies --lg-plans): the plans additionally get their column slices -- an epoch is ONE persistent launch where they
apply (include/dsgd.h "THE LOGISTIC MODEL", COLUMN SLICES; up to 6 workers at RCV1's width, batches up to 1,024 rows in all).
--lg-async (with --model logistic): MasterAsync.fit's flow on the zero-lag schedule (host.LogisticAsync; include/dsgd.h "THE
LOGISTIC MODEL", ASYNCHRONOUS): device-drawn one-worker plans, a loss check every check-every updates with the leaky average,
best weights kept, maxSteps = train rows x max-epochs.  With --lg-slices a window of updates is ONE persistent launch.
--topics CCAT,ECAT,GCAT,MCAT (with --model logistic; up to 8 names): one-vs-rest over the named topics on the same rows
(include/dsgd.h "THE LOGISTIC MODEL", SEVERAL TOPICS) -- rcv1.load_topics' planes (+1 iff ANY qrels line tags the document),
host.LogisticTopics: Master.fit's flow with the lists shared, one launch pair per step whatever the number of topics, the early
stopping applied per topic.  With --synthetic plane 0 is the data's labels and the others are the signs of seeded planted directions.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsgd_amd
from dsgd_amd import host, rcv1

ap = argparse.ArgumentParser()
ap.add_argument("--conf", help="application.conf to read the dsgd{...} block from (DSGD_* variables override)")
ap.add_argument("--synthetic", type=int, default=0, help="use N synthetic RCV1-like rows instead of data-path")
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--weights-out", help="write the `idx:value` line of Main.scala:114 here instead of logging it")
ap.add_argument("--precision", choices=("fp32", "fp64"), default="fp32", help="fp64: the reference's Double arithmetic")
ap.add_argument("--f64-rp-plans", action="store_true", help="fp64: refused plans run as row-parallel plans, under a communicator too: one plan run per epoch and rank (DSGD_F64_RP_PLANS=1)")
ap.add_argument("--model", choices=("svm", "logistic"), default="svm", help="logistic: log-loss, probabilities, plain L2 (fp32; synchronous unless --lg-async)")
ap.add_argument("--lg-plans", action="store_true", help="logistic: Master.fit's flow on resident logistic plans (host.LogisticSync)")
ap.add_argument("--lg-slices", action="store_true", help="logistic: --lg-plans on column slices, one persistent launch per epoch (host.LogisticSync(slices=True))")
ap.add_argument("--lg-async", action="store_true", help="logistic: MasterAsync.fit's flow on the zero-lag schedule (host.LogisticAsync); honours --lg-slices")
ap.add_argument("--topics", help="logistic: comma-separated topic names, one-vs-rest in one launch pair per step (host.LogisticTopics)")
a = ap.parse_args()
topics = [t for t in (a.topics or "").split(",") if t]
if topics and (a.model != "logistic" or a.lg_plans or a.lg_slices or a.lg_async):
    ap.error("--topics goes with --model logistic alone (no plans, slices or asynchronous fit over several topics)")
if len(topics) > dsgd_amd.Engine.lg_topics_max:
    ap.error("--topics takes at most %d names" % dsgd_amd.Engine.lg_topics_max)
if a.lg_async and a.lg_plans:
    ap.error("--lg-plans and --lg-async are two fits: give one (--lg-slices goes with either)")
a.lg_plans = a.lg_plans or a.lg_slices
if a.lg_async and a.model != "logistic":
    ap.error("--lg-async goes with --model logistic")
if a.lg_plans and a.model != "logistic":
    ap.error("--lg-plans goes with --model logistic")
if a.model == "logistic" and a.precision != "fp32":
    ap.error("--model logistic runs on the fp32 engine")
if a.f64_rp_plans:
    os.environ["DSGD_F64_RP_PLANS"] = "1"   # (host.MasterSync / host.MasterAsync read it at every fit)
rp_plans = a.precision == "fp64" and os.environ.get("DSGD_F64_RP_PLANS", host.F64_RP_PLANS_DEFAULT) == "1"


def log(msg, *args):  # logback's pattern is not reproduced; the messages are
    print(time.strftime("%H:%M:%S"), msg.replace("{}", "%s") % args if args else msg, flush=True)


def fit_logistic(eng, cfg, n_train, n_rows):
    """A plain loop: host-drawn lists, one lg_sync_steps call per epoch, lg_loss_acc on train and test after each."""
    split = host.split_vanilla(n_train, cfg.node_count)
    k = len(split)
    n_steps = max(1, min(len(r) for r in split) // cfg.batch_size)
    rng = np.random.default_rng(0)
    log("logistic: {} workers, {} steps of {} rows per epoch, lr {}", k, n_steps, cfg.batch_size, cfg.learning_rate)
    l0, a0 = eng.lg_loss_acc(0, n_train)
    log("initial loss: {}", l0)
    log("initial accuracy: {}", a0)
    for epoch in range(cfg.max_epochs):
        perms = [rng.permutation(len(r)).astype(np.int32) + r.start for r in split]
        lists = [perms[w][t * cfg.batch_size:(t + 1) * cfg.batch_size] for t in range(n_steps) for w in range(k)]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
        t0 = time.time()
        eng.lg_sync_steps(np.concatenate(lists), offs, n_steps, k, cfg.learning_rate)
        dt = time.time() - t0
        ltr, atr = eng.lg_loss_acc(0, n_train)
        lte, ate = eng.lg_loss_acc(n_train, n_rows)
        log("epoch {}: train loss {} acc {}, test loss {} acc {} ({}s)", epoch, round(ltr, 6), round(atr, 4), round(lte, 6), round(ate, 4), round(dt, 3))
    log("final test loss: {}", lte)
    log("final test accuracy: {}", ate)


def synthetic_planes(data, n_topics, seed=1):
    """plane 0: the data's labels; plane t >= 1: the sign of x . u_t for a seeded planted direction u_t (a zero dot counts as -1)"""
    rng = np.random.default_rng(seed)
    planes = [np.asarray(data.label, dtype=np.int8)]
    rows = np.repeat(np.arange(data.n_rows), np.diff(data.row_ptr))
    for _ in range(1, n_topics):
        u = rng.standard_normal(data.dim + 1)
        d = np.bincount(rows, weights=data.val.astype(np.float64) * u[data.col], minlength=data.n_rows)
        planes.append(np.where(d > 0, 1, -1).astype(np.int8))
    return np.ascontiguousarray(np.stack(planes), dtype=np.int8)


def fit_topics(eng, cfg, planes, names, n_train, n_rows):
    eng.lg_topics_set(planes)
    master = host.LogisticTopics(eng, n_train, n_rows, cfg.node_count, rnd=host.JavaRandom(0), log=log)
    l0, a0 = eng.lg_topics_loss_acc(0, n_train)
    for t, name in enumerate(names):
        log("{}: {} of {} rows tagged, initial loss {}, initial accuracy {}", name, int((planes[t] > 0).sum()), n_rows, l0[t], a0[t])
    t0 = time.time()
    states = master.fit(np.zeros((len(names), eng.dp), dtype=np.float32), cfg.max_epochs, cfg.batch_size, cfg.learning_rate,
                        host.EarlyStopping.no_improvement(cfg.patience, cfg.conv_delta, None))
    log("fit ({}s, {} steps of {} topics)", round(time.time() - t0, 3), master.steps_run, len(names))
    eng.lg_topics_set_weights(np.stack([s.grad for s in states]))     # every topic at the weights its own rule kept
    lte, ate = eng.lg_topics_loss_acc(n_train, n_rows)
    for t, name in enumerate(names):
        log("{}: {} epochs, train loss {}, final test loss {}, final test accuracy {}", name, states[t].updates, states[t].loss, lte[t], ate[t])


cfg = host.Config.load(open(a.conf).read() if a.conf else None)
log("config: {}", cfg)
log("loading data in: {}", "synthetic(%d)" % a.synthetic if a.synthetic else cfg.data_path)
t0 = time.time()
planes = None
if a.synthetic:
    data = dsgd_amd.synth.generate(a.synthetic, seed=0)
    if topics:
        planes = synthetic_planes(data, len(topics))
elif topics:
    data, planes = rcv1.load_topics(cfg.data_path, topics, full=cfg.full)
else:
    data = rcv1.load(cfg.data_path, full=cfg.full)
log("data loaded: {} ({}s)", data.n_rows, round(time.time() - t0, 2))
n_train = int(data.n_rows * 0.8)                                              # Main.scala:52
metrics = host.Metrics()
with dsgd_amd.Engine(data.dim, cfg.lambda_, device=a.device, precision=a.precision) as eng:
    # fp64 on real files: the parsed Doubles as the reference holds them (--synthetic is float by construction; the
    # asynchronous fit runs resident column-slice plans, which hold float values -- unless row-parallel plans are on)
    values = data.val64 if a.precision == "fp64" and (rp_plans or not cfg.async_) and getattr(data, "val64", None) is not None else data.val
    eng.load_csr(data.row_ptr, data.col, values, data.label)
    log("feature values: {} bits{}", eng.value_bits() if a.precision == "fp64" else 32,
        " (fp64 asynchronous fit: resident plans hold float values, NOT the Double feature values)"
        if a.precision == "fp64" and cfg.async_ and not rp_plans and getattr(data, "val64", None) is not None else "")
    if a.model == "logistic":   # (its own loop; dimSparsity plays no part)
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        if topics:
            fit_topics(eng, cfg, planes, topics, n_train, data.n_rows)
            sys.exit(0)
        if a.lg_async:
            master = host.LogisticAsync(eng, n_train, data.n_rows, cfg.node_count, log=log, slices=a.lg_slices)
            l0, a0 = eng.lg_loss_acc(0, n_train)
            log("initial loss: {}", l0)
            log("initial accuracy: {}", a0)
            t0 = time.time()
            state = master.fit(np.zeros(data.dim + 1, dtype=np.float32), cfg.max_epochs, cfg.batch_size, cfg.learning_rate,
                               host.EarlyStopping.no_improvement(cfg.patience, cfg.conv_delta, None), cfg.check_every, cfg.leaky_loss)
            log("fit ({}s, {} updates, {} loss checks, best leaky test loss {})", round(time.time() - t0, 3), state.updates, master.checks, state.loss)
            lte, ate = eng.lg_loss_acc(n_train, data.n_rows, w=state.grad)
            log("final test loss: {}", lte)
            log("final test accuracy: {}", ate)
            sys.exit(0)
        if a.lg_plans:
            master = host.LogisticSync(eng, n_train, data.n_rows, cfg.node_count, rnd=host.JavaRandom(0), log=log, metrics=metrics, slices=a.lg_slices)
            log("initial loss: {}", master.local_loss())
            log("initial accuracy: {}", master.local_accuracy())
            t0 = time.time()
            state = master.fit(np.zeros(data.dim + 1, dtype=np.float32), cfg.max_epochs, cfg.batch_size, cfg.learning_rate,
                               host.EarlyStopping.no_improvement(cfg.patience, cfg.conv_delta, None))
            log("fit ({}s, {} epochs, {} of them on device-drawn lists)", round(time.time() - t0, 3), state.updates, master.device_drawn_epochs)
            log("final test loss: {}", master.local_loss(test=True))
            log("final test accuracy: {}", master.local_accuracy(test=True))
            sys.exit(0)
        fit_logistic(eng, cfg, n_train, data.n_rows)
        sys.exit(0)
    t0 = time.time()
    eng.build_dim_sparsity(n_train)                                            # Main.scala:54-65
    log("dim sparsity ({}s)", round(time.time() - t0, 3))
    w0 = np.zeros(data.dim + 1, dtype=np.float32)
    eng.set_weights(w0)
    # Main.scala:74-78: master.distributedLoss(w0, ss) / distributedAccuracy(w0, ss) -- the train rows split over the workers,
    # one forward pass per split, folded: ONE launch for all splits and both figures (Engine.predict_ranges).  Beyond its 256
    # ranges the tallies of the whole train range are the same numbers (dsgd_loss_acc).
    split = host.split_vanilla(n_train, cfg.node_count)
    if len(split) <= eng.predict_max_ranges:
        _, _, l0, a0 = eng.predict_ranges([(r.start, r.stop) for r in split])
    else:
        l0, a0, _ = eng.loss_acc(0, n_train)
    log("initial loss: {}", l0)
    log("initial accuracy: {}", a0)
    stop = host.EarlyStopping.no_improvement(cfg.patience, cfg.conv_delta, None)
    t0 = time.time()
    if cfg.async_:
        master = host.MasterAsync(eng, n_train, data.n_rows, cfg.node_count, log=log, poll_s=0.001)
        state = master.fit(w0, cfg.max_epochs, cfg.batch_size, cfg.learning_rate, stop, cfg.check_every, cfg.leaky_loss)
    else:
        master = host.MasterSync(eng, n_train, data.n_rows, cfg.node_count, rnd=host.JavaRandom(0), log=log, metrics=metrics)
        state = master.fit(w0, cfg.max_epochs, cfg.batch_size, cfg.learning_rate, stop)
    log("fit ({}s)", round(time.time() - t0, 3))
    w1 = np.asarray(state.grad, dtype=np.float64 if a.precision == "fp64" else np.float32)
    line = host.format_final_weights(w1)
    if a.weights_out:
        open(a.weights_out, "w").write(line + "\n")
        log("final weights: {} entries written to {}", int(np.count_nonzero(w1)), a.weights_out)
    else:
        log("final weights: {}", line)
    if a.precision == "fp64":   # (the fp64 weights are the engine's own: no float copy replaces them)
        if cfg.async_:          # (the best weights of the async fit, as they are)
            eng.set_weights(w1)
        l1, a1, _ = eng.loss_acc(n_train, data.n_rows)
    else:
        l1, a1, _ = eng.loss_acc(n_train, data.n_rows, w=w1)                   # localLoss / localAccuracy on testData
    log("final test loss: {}", l1)
    log("final test accuracy: {}", a1)
    if cfg.record:
        for ln in metrics.influx_lines():
            print(ln)
