"""Host-side mirror of the reference's coordination layer for the hot path.

Same names, argument meaning and stopping behaviour as the Scala classes, so that parity tests read like
the reference.  Citations are relative to /root/reference/src/main/scala/epfl/distributed/.

    Config            utils/Config.scala:3-21 + resources/application.conf:1-52 (DSGD_* overrides)
    SplitStrategy     core/ml/SplitStrategy.scala:13-14
    EarlyStopping     core/ml/EarlyStopping.scala:11-46
    GradState         core/ml/GradState.scala:6-24  (`grad` holds the WEIGHTS)
    JavaRandom        java.util.Random (the generator behind scala.util.Random, seeded 0 at Main.scala:32)
    scala_shuffle     scala.util.Random.shuffle (2.12): the per-batch reshuffle of Master.scala:184
    MasterSync.fit    core/Master.scala:120-218
    predict, distributed_loss, distributed_accuracy (both masters)   core/Master.scala:61-98
    local_sampled_loss, local_sampled_accuracy (both masters)        core/Master.scala:109-118
    MasterAsync.fit   core/MasterAsync.scala:32-62, 96-177
    LogisticSync.fit  core/Master.scala:120-218 with the logistic model of one engine (resident logistic plans)
    Metrics           the Kamon instruments of the path, same names (core/Slave.scala:90-181, core/Master.scala:150-183)
    format_final_weights   the `final weights: idx:val ...` log line (Main.scala:114)

All arithmetic happens behind a *backend* (the HIP `Engine`); this module only orchestrates.  A backend
offers: sync_step(idx_lists, lr), gradient(idx) -> (g, stats), apply(g_mean, lr), loss_acc(lo, hi),
get_weights(), set_weights(w), optionally resident plans (plan_flat(idx, offsets, n_steps, n_workers) -> plan with
.destroy(), plan_run(plan, step_begin, step_end, lr), synchronize()): an epoch of Master.fit then runs as ONE plan; and for
the asynchronous mode async_start/async_updates/async_stop.
"""

from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np


SPARSE_EPSILON = 1e-20  # math/Sparse.scala:104: entries with abs(v) <= epsilon are not stored


# ---- instruments (Kamon names, so dashboards such as kube/monitor.yaml keep working) ----------------------
class Metrics:
    """Counters / histograms / timers under the reference's instrument names:
    counters `slave.sync.forward`, `slave.sync.backward` (one increment per SAMPLE, core/Slave.scala:131-150),
    `slave.async.backward` (per sample, :90-95), `slave.async.batch` (:107), `slave.async.grad.update` (:181),
    `master.async.loss` (MasterAsync.scala:126); histograms `master.sync.loss`, `master.sync.acc`
    (Master.scala:150-151 record `losses.head.toLong` and `100 * accs.head.toLong`: the values are TRUNCATED to
    integers before they are recorded -- kept); timer `master.sync.batch.duration` (:183); timers
    `master.sampled.loss.duration`, `master.sampled.accuracy.duration` (the mirrors' own: one entry per sampled check)."""

    def __init__(self):
        import threading

        self._lock = threading.Lock()
        self.counters: dict = {}
        self.histograms: dict = {}

    def counter(self, name: str, times: int = 1):
        with self._lock:
            self.counters[name] = self.counters.get(name, 0) + int(times)

    def histogram(self, name: str, value):
        with self._lock:
            self.histograms.setdefault(name, []).append(int(value))  # .toLong

    def timer(self, name: str):
        metrics = self

        class _T:
            def __enter__(self):
                self.t0 = time.perf_counter_ns()
                return self

            def __exit__(self, *exc):
                with metrics._lock:
                    metrics.histograms.setdefault(name, []).append(time.perf_counter_ns() - self.t0)

        return _T()

    def snapshot(self) -> dict:
        with self._lock:
            return {"counters": dict(self.counters), "histograms": {k: list(v) for k, v in self.histograms.items()}}

    def influx_lines(self, tags: str = "") -> List[str]:
        """InfluxDB line protocol (the reference reports through kamon-influxdb, Main.scala:42)."""
        snap, t = self.snapshot(), time.time_ns()
        tag = ("," + tags) if tags else ""
        out = ["%s%s count=%di %d" % (k, tag, v, t) for k, v in sorted(snap["counters"].items())]
        for k, v in sorted(snap["histograms"].items()):
            if v:
                out.append("%s%s count=%di,sum=%di,min=%di,max=%di %d" % (k, tag, len(v), sum(v), min(v), max(v), t))
        return out


def format_final_weights(w, eps: float = SPARSE_EPSILON) -> str:
    """Main.scala:114: `w1.map.map { case (idx, n) => s"$idx:$n" }.mkString(" ")` -- the stored (non-zero) entries as
    `idx:value`.  The reference iterates an immutable HashMap (unspecified order) and prints fp64; here ascending keys
    and the shortest decimal that round-trips the engine's fp32 value."""
    arr = np.asarray(w)
    return " ".join("%d:%s" % (int(k), repr(float(np.float32(arr[k])))) for k in np.flatnonzero(np.abs(arr) > eps))


# ---- configuration --------------------------------------------------------------------------------------
@dataclass
class Config:
    """utils/Config.scala:3-21; defaults are application.conf:1-52."""

    data_path: str = "data"
    host: str = "127.0.0.1"
    port: int = 4000
    master_host: Optional[str] = None
    master_port: Optional[int] = None
    batch_size: int = 100
    learning_rate: float = 0.5
    lambda_: float = 1e-5
    full: bool = False
    node_count: int = 3
    async_: bool = False
    record: bool = False
    max_epochs: int = 10
    check_every: int = 100
    leaky_loss: float = 0.9
    patience: int = 5
    conv_delta: float = 0.01

    # application.conf key -> (field, env override, parser)
    _KEYS = {
        "data-path": ("data_path", "DSGD_DATA_PATH", str),
        "host": ("host", "DSGD_NODE_HOST", str),
        "port": ("port", "DSGD_NODE_PORT", int),
        "master-host": ("master_host", "DSGD_MASTER_HOST", str),
        "master-port": ("master_port", "DSGD_MASTER_PORT", int),
        "batch-size": ("batch_size", "DSGD_BATCH_SIZE", int),
        "learning-rate": ("learning_rate", "DSGD_LEARNING_RATE", float),
        "lambda": ("lambda_", "DSGD_LAMBDA", float),
        "full": ("full", "DSGD_FULL", lambda s: str(s).lower() == "true"),
        "node-count": ("node_count", "DSGD_NODE_COUNT", int),
        "async": ("async_", "DSGD_ASYNC", lambda s: str(s).lower() == "true"),
        "record": ("record", "DSGD_RECORD", lambda s: str(s).lower() == "true"),
        "max-epochs": ("max_epochs", "DSGD_MAX_EPOCHS", int),
        "check-every": ("check_every", "DSGD_CHECK_EVERY", int),
        "leaky-loss": ("leaky_loss", "DSGD_LEAKY_LOSS", float),
        "patience": ("patience", "DSGD_PATIENCE", int),
        "conv-delta": ("conv_delta", "DSGD_CONV_DELTA", float),
    }

    @classmethod
    def load(cls, conf_text: Optional[str] = None, env=os.environ) -> "Config":
        """`key = value` lines of the dsgd { ... } block, then the DSGD_* environment overrides
        (`key = ${?DSGD_X}` lines of application.conf)."""
        cfg = cls()
        if conf_text:
            depth, in_dsgd = 0, False
            for raw in conf_text.splitlines():
                line = raw.split("#", 1)[0].strip()
                if not line:
                    continue
                if line.startswith("dsgd") and line.endswith("{"):
                    in_dsgd, depth = True, 1
                    continue
                if in_dsgd:
                    depth += line.count("{") - line.count("}")
                    if depth <= 0:
                        in_dsgd = False
                        continue
                    if "=" in line:
                        k, v = (t.strip() for t in line.split("=", 1))
                        if k in cls._KEYS and not v.startswith("${"):
                            name, _, parse = cls._KEYS[k]
                            setattr(cfg, name, parse(v.strip('"')))
        for k, (name, var, parse) in cls._KEYS.items():
            if var in env and env[var] != "":
                setattr(cfg, name, parse(env[var]))
        return cfg

    def role(self) -> str:
        """Main.scala:122-159: master-host/port equal to own -> master; set but different -> slave; unset -> dev."""
        if self.master_host is not None and self.master_port is not None:
            return "master" if (self.master_host == self.host and self.master_port == self.port) else "slave"
        return "dev"


# ---- split / stopping / state -----------------------------------------------------------------------------
def split_vanilla(n: int, n_slaves: int) -> List[range]:
    """SplitStrategy.vanilla: indices.grouped(ceil(n / K)); may yield fewer than K groups."""
    size = int(math.ceil(n / float(n_slaves)))
    return [range(b, min(n, b + size)) for b in range(0, n, size)]


class EarlyStopping:
    @staticmethod
    def target(target: float) -> Callable[[Sequence[float]], bool]:
        return lambda losses: bool(losses) and losses[0] <= target  # EarlyStopping.scala:11

    @staticmethod
    def no_improvement(patience: int = 5, min_delta: float = 1e-3, min_steps: Optional[int] = None):
        """EarlyStopping.scala:13-46 over a NEWEST-FIRST list."""

        def crit(losses: Sequence[float]) -> bool:
            abs_min_delta = abs(min_delta)

            def check() -> bool:
                mn, idx_min = 1.7976931348623157e308, -1
                for index, num in enumerate(losses):
                    if (num - mn) <= abs_min_delta:
                        mn, idx_min = num, index
                return False if idx_min == 0 else idx_min >= patience

            if not losses:
                return False
            if min_steps is None:
                return check()
            return False if min_steps < len(losses) else check()

        return crit


@dataclass
class GradState:
    """GradState.scala:6-24 -- `grad` is the weight vector."""

    grad: np.ndarray
    loss: Optional[float] = None
    start: float = field(default_factory=time.time)
    updates: int = 0
    end: Optional[float] = None

    def replace_grad(self, new_grad) -> "GradState":
        return GradState(new_grad, self.loss, self.start, self.updates + 1, self.end)

    def finish(self, final_loss) -> "GradState":
        return GradState(self.grad, final_loss, self.start, self.updates, time.time())


# ---- the reference's random stream ---------------------------------------------------------------------------
class JavaRandom:
    """java.util.Random: 48-bit LCG; scala.util.Random delegates to it (seed 0 at Main.scala:32)."""

    def __init__(self, seed: int = 0):
        self.seed = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)

    def _next(self, bits: int) -> int:
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        v = self.seed >> (48 - bits)
        return v - (1 << 32) if (bits == 32 and v >= (1 << 31)) else v  # (int) cast of the Java original

    def next_int(self, bound: Optional[int] = None) -> int:
        if bound is None:
            return self._next(32)
        if bound <= 0:
            raise ValueError("bound must be positive")
        r = self._next(31)
        m = bound - 1
        if (bound & m) == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            if u - r + m < (1 << 31):
                return r
            u = self._next(31)


def scala_shuffle(xs: Sequence[int], rnd: JavaRandom) -> List[int]:
    """scala.util.Random.shuffle (2.12): for n <- len to 2 by -1: swap(n - 1, nextInt(n))."""
    buf = list(xs)
    for n in range(len(buf), 1, -1):
        k = rnd.next_int(n)
        buf[n - 1], buf[k] = buf[k], buf[n - 1]
    return buf


# ---- the same stream, natively (csrc/jrand.c -> lib/libdsgd_host.so) -----------------------------------------------
_HOST_LIB = None


def _host_lib():
    """libdsgd_host.so or None (not built: the pure-Python restatement above is the fallback -- HOST logic, not the
    compute path; the product's kernels have no fallback)."""
    global _HOST_LIB
    if _HOST_LIB is None:
        import ctypes as C

        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libdsgd_host.so")
        try:
            lib = C.CDLL(path)
            lib.dsgd_jrand_seed.restype = C.c_uint64
            lib.dsgd_jrand_seed.argtypes = [C.c_int64]
            lib.dsgd_jrand_shuffle.restype = C.c_int64
            lib.dsgd_jrand_epoch_lists.restype = C.c_int
            _HOST_LIB = lib
        except OSError:
            _HOST_LIB = False
    return _HOST_LIB or None


def epoch_lists(rnd: JavaRandom, split: Sequence[range], max_samples: int, batch_size: int, native: Optional[bool] = None):
    """The index lists of ONE epoch of Master.fit (core/Master.scala:179-199), drawn from `rnd` exactly as the reference
    draws them -- for every batch b in (0 until maxSamples by batchSize), for every worker k in order:
    Random.shuffle(split_k).slice(b, b + batchSize) (:184: a fresh shuffle of the WHOLE split per worker and batch).

    Returns (idx int32 [total], offsets int64 [n_steps * K + 1], n_steps): the flat form dsgd_plan_create takes.  Steps are
    emitted up to the first one in which some worker's slice is empty (Vec.sum would throw in that slave, math/Vec.scala:129);
    `rnd` advances over the steps emitted.  Natively (csrc/jrand.c: the epoch's shuffles in parallel, draw for draw the
    same stream) when lib/libdsgd_host.so is there; `native=False` forces the pure-Python restatement."""
    K = len(split)
    lib = _host_lib() if native in (None, True) else None
    if native is True and lib is None:
        raise RuntimeError("libdsgd_host.so is not built")
    # (an empty split takes the Python path, which stops where the reference's Vec.sum throws; a batch size beyond the
    #  longest split selects whole splits either way -- clamped: the native side takes it as an int32)
    if lib is not None and all(r.step == 1 and len(r) > 0 for r in split):
        import ctypes as C

        batch_size = max(1, min(int(batch_size), max(max_samples, max(len(r) for r in split)), 2 ** 31 - 1))
        n_steps_max = len(range(0, max_samples, batch_size))
        sb = np.asarray([r.start for r in split], dtype=np.int64)
        se = np.asarray([r.stop for r in split], dtype=np.int64)
        cap = n_steps_max * sum(min(batch_size, len(r)) for r in split)
        idx = np.empty(max(cap, 1), dtype=np.int32)
        offsets = np.zeros(n_steps_max * K + 1, dtype=np.int64)
        state = C.c_uint64(rnd.seed)
        n_steps, draws = C.c_int64(0), C.c_int64(0)
        rc = lib.dsgd_jrand_epoch_lists(C.byref(state), sb.ctypes.data_as(C.c_void_p), se.ctypes.data_as(C.c_void_p), C.c_int32(K),
                                        C.c_int64(max_samples), C.c_int32(batch_size), idx.ctypes.data_as(C.c_void_p),
                                        offsets.ctypes.data_as(C.c_void_p), C.byref(n_steps), C.byref(draws))
        if rc != 0:
            raise RuntimeError("dsgd_jrand_epoch_lists failed (%d)" % rc)
        rnd.seed = int(state.value)
        ns = int(n_steps.value)
        return idx[:int(offsets[ns * K])], offsets[:ns * K + 1], ns
    flat, offs, n_steps = [], [0], 0
    for batch in range(0, max_samples, batch_size):
        if any(batch >= len(r) for r in split):
            break
        for r in split:
            shuffled = scala_shuffle(list(r), rnd)
            flat.append(np.asarray(shuffled[batch:batch + batch_size], dtype=np.int32))
            offs.append(offs[-1] + len(flat[-1]))
        n_steps += 1
    idx = np.concatenate(flat) if flat else np.zeros(0, dtype=np.int32)
    return idx, np.asarray(offs, dtype=np.int64), n_steps


# ---- distributed aggregate owned by the host (alternative to the in-library RCCL all-reduce) -----------------
class HostAllReduceBackend:
    """Mean over world_size x hosted workers with the collective owned by the host (`torch.distributed`,
    gloo on CPU / nccl on GPU).  core/Master.scala:190-197: every rank computes the regularised sums of its
    own workers, the sums are all-reduced, every rank applies the identical update."""

    def __init__(self, local, dist_module, n_rows_local_train: int):
        self.local, self.dist = local, dist_module
        self.world = dist_module.get_world_size()
        self.n_train = n_rows_local_train

    def sync_step(self, idx_lists, lr):
        import torch

        total = None
        stats = {"n_samples": 0, "n_active": 0}
        for idx in idx_lists:
            g, st = self.local.gradient(idx)
            total = g.astype(np.float64) if total is None else total + g
            stats["n_samples"] += st["n_samples"]
            stats["n_active"] += st["n_active"]
        t = torch.from_numpy(np.ascontiguousarray(total))
        self.dist.all_reduce(t)  # sum over ranks
        k_total = len(idx_lists) * self.world
        self.local.apply((t.numpy() / k_total).astype(np.float32), lr)  # Vec.mean then w - lr * grad
        return stats

    def loss_acc(self, lo, hi):
        import torch

        _, _, counts = self.local.loss_acc(lo, hi)
        t = torch.tensor(list(counts) + [hi - lo], dtype=torch.int64)
        self.dist.all_reduce(t)
        c0, c1, c2, n = (int(x) for x in t)
        w = self.local.get_weights().astype(np.float64)
        lam = getattr(self.local, "lam")
        return lam * float((w * w).sum()) + (c1 + 2.0 * c2) / n, c0 / n, [c0, c1, c2]

    def get_weights(self):
        return self.local.get_weights()

    def set_weights(self, w):
        self.local.set_weights(w)


class HostAsyncExchange:
    """The asynchronous mode across ranks with the collective owned by the host: the host-side twin of
    `dsgd_async_set_exchange` (csrc/dsgd_hip.hip, RCCL inside the library), usable with gloo on CPU.

    core/Slave.scala:99-105 applies every update locally and gossips it to every peer, who subtracts it when it
    arrives (:177-185).  One replica per rank runs `every` local updates per round; between rounds the replicas
    all-reduce what each subtracted since the last exchange (d_local = w_prev - w) and subtract their PEERS' part
    (d_sum - d_local) on top of their own.  With one rank the peers' part is exactly zero."""

    def __init__(self, local, dist_module):
        self.local, self.dist = local, dist_module
        self.world = dist_module.get_world_size()
        self.w_prev = np.asarray(local.get_weights(), dtype=np.float64).copy()
        self.rounds = 0

    def run_round(self, idx_lists, lr):
        """`idx_lists`: the sample lists of this rank's local updates of the round, in order (Slave.asyncTask draws
        them itself; they are an input here so that a run can be replayed)."""
        stats = {"n_samples": 0, "n_active": 0}
        for idx in idx_lists:
            _, st = self.local.async_step(idx, lr)
            stats["n_samples"] += st["n_samples"]
            stats["n_active"] += st["n_active"]
        self.exchange()
        return stats

    def exchange(self):
        import torch

        w = np.asarray(self.local.get_weights(), dtype=np.float64)
        d_local = self.w_prev - w
        t = torch.from_numpy(np.ascontiguousarray(d_local.copy()))
        self.dist.all_reduce(t)  # sum over ranks
        others = t.numpy() - d_local   # exactly 0 with a single rank
        if self.world > 1 or np.any(others != 0.0):
            w = w - others
            self.local.set_weights(w)
            # what the backend really holds now: an fp32 engine rounds on store, and a w_prev that kept the fp64 value
            # would gossip that rounding residue to the peers as if it were an update (the device kernel sets its
            # w_prev to the rounded value too)
            w = np.asarray(self.local.get_weights(), dtype=np.float64)
        self.w_prev = w.copy()
        self.rounds += 1


# MasterSync._run_steps_f64: "1" = an epoch's refused fp64 plan runs as ONE Engine.sync_steps_f64 call, "0" = one sync_step_f64
# call per step (DSGD_F64_STEPS overrides).  The batched call has not been measured yet: the default stays the loop
F64_STEPS_DEFAULT = "0"
# DSGD_F64_RP_PLANS=1: what an fp64 backend's column-slice plans refuse (Double feature values, more than 4 workers or 1,024
# rows per step, a model beyond a slice's LDS) runs as a resident ROW-PARALLEL plan (Engine.plan_from_seed / plan_flat /
# async_plan with rp64=True; include/dsgd.h "THE FP64 MODE", ROW-PARALLEL PLANS) -- the same lists and the same bits, no upload
# per epoch, and MasterAsync.fit works on Double data.  Measured (50 us per 3 x 100 step on Double data against
# 122 us through sync_steps_f64 with host-drawn lists); off by default because the mirrors' behaviour on Double data is pinned
F64_RP_PLANS_DEFAULT = "0"


def _f64_rp_plans() -> bool:
    return os.environ.get("DSGD_F64_RP_PLANS", F64_RP_PLANS_DEFAULT) == "1"

class _Refused(RuntimeError):
    """(MasterSync._make_plan: the column-slice plan of this fit was refused before)"""
    code = -7


# ---- Master.predict / distributedLoss / distributedAccuracy ---------------------------------------------------------
class _DistributedEval:
    """core/Master.scala:61-98 for the workers hosted behind one backend (shared by MasterSync and MasterAsync, which
    both extend AbstractMaster there).  The rows are split as fit splits them (SplitStrategy.vanilla over the train rows,
    one split per worker), every split is one ForwardRequest, the replies are zipped back to their rows.

    A backend with predict_ranges(ranges, w) (Engine: ONE launch for all splits, one byte per prediction and exact
    per-split tallies) serves every call from it, as long as the splits are within its predict_max_ranges.  Any other
    backend needs get_weights(), lam and either forward_splits(idx_lists, w) (wire.WireBackend: the reference's own fan-out,
    split k to slave k, all requests in flight together) or forward(idx, w) (asked once per split: the oracle backend, a
    recording backend); loss and accuracy are then folded here over the labels -- the master's own (`master.labels = y`,
    one label per row: the reference's master holds `data`), else the backend's `labels` / `label` array or its
    labels(rows) method.  weights: None evaluates the backend's resident weights."""

    labels = None   # one label per row, where the fold runs on the host and the backend offers none

    def _splits(self):
        return split_vanilla(self.n_train, self.node_count)   # splitStrategy(data, workers.size)

    def _predict_ranges(self, weights):
        split = self._splits()
        if not all(r.step == 1 for r in split):
            raise ValueError("distributed evaluation needs contiguous splits")
        ranges = [(r.start, r.stop) for r in split]
        if hasattr(self.backend, "predict_ranges") and len(ranges) <= getattr(self.backend, "predict_max_ranges", len(ranges)):
            pred, counts, loss, acc = self.backend.predict_ranges(ranges, weights)
            return split, np.asarray(pred), counts, loss, acc
        return split, None, None, None, None

    def _forward_splits(self, split, weights):
        lists = [np.arange(r.start, r.stop, dtype=np.int32) for r in split]
        if hasattr(self.backend, "forward_splits"):   # workers.zip(split) ... Future.sequence(work): Master.scala:67-73
            preds = self.backend.forward_splits(lists) if weights is None else self.backend.forward_splits(lists, weights)
        else:                                         # worker.forward(ForwardRequest(idx, weights)), split after split
            preds = [self.backend.forward(idx) if weights is None else self.backend.forward(idx, weights) for idx in lists]
        if getattr(self, "metrics", None) is not None:
            self.metrics.counter("slave.sync.forward", sum(len(idx) for idx in lists))   # one increment per sample: Slave.scala:131
        return np.concatenate([np.asarray(p, dtype=np.float64) for p in preds]) if preds else np.zeros(0)

    def _labels(self, rows):
        for src in (self.labels, getattr(self.backend, "labels", None), getattr(self.backend, "label", None)):
            if src is None:
                continue
            return np.asarray(src(rows) if callable(src) else np.asarray(src)[rows], dtype=np.float64)
        raise ValueError("the fold over the predictions needs the rows' labels: set master.labels (one per row), or give the "
                         "backend a `labels` array")

    def _norm_squared(self, weights):
        """math/Vec.scala:55 over the stored entries, added one by one in ascending key order (numpy's pairwise sum rounds
        differently in the last place)."""
        w = np.asarray(self.backend.get_weights() if weights is None else weights, dtype=np.float64)
        w = w[np.abs(w) > SPARSE_EPSILON]
        acc = 0.0
        for v in (w * w).tolist():
            acc += v
        return acc

    def predict(self, weights=None):
        """Master.predict (:61-75): (rows, predictions) in split order -- the reference's Map[Int, Number] as two parallel
        arrays (rows int64; predictions int8 from predict_ranges, else what the backend's forward returns)."""
        split, pred, _, _, _ = self._predict_ranges(weights)
        rows = np.concatenate([np.arange(r.start, r.stop, dtype=np.int64) for r in split]) if split else np.zeros(0, np.int64)
        if pred is None:
            pred = self._forward_splits(split, weights)
        return rows, pred

    def distributed_loss_and_accuracy(self, weights=None):
        """(distributedLoss, distributedAccuracy) from ONE pass over the splits (the reference runs predict once for each)."""
        split, pred, _, loss, acc = self._predict_ranges(weights)
        if pred is not None:
            return loss, acc
        rows = np.concatenate([np.arange(r.start, r.stop, dtype=np.int64) for r in split]) if split else np.zeros(0, np.int64)
        if len(rows) == 0:   # preds.map(...).reduce(_ + _) on an empty map (:96)
            raise ValueError("empty.reduceLeft: no predictions to fold")
        y = self._labels(rows)   # (looked up first: a fold that cannot be made sends no request)
        pred = self._forward_splits(split, weights)
        hinge = np.maximum(0.0, 1.0 - y * pred)   # model.loss(p, y): core/ml/SparseSVM.scala:16
        lam = float(getattr(self.backend, "lam"))
        return lam * self._norm_squared(weights) + float(hinge.sum()) / len(rows), float(np.count_nonzero(pred == y)) / len(rows)

    def distributed_loss(self, weights=None):       # Master.scala:87-98
        return self.distributed_loss_and_accuracy(weights)[0]

    def distributed_accuracy(self, weights=None):   # Master.scala:77-85
        return self.distributed_loss_and_accuracy(weights)[1]


# ---- Master.localSampledLoss / localSampledAccuracy -----------------------------------------------------------------
# DSGD_SAMPLED_DEVICE=1: the sample of a sampled check is drawn by the device (Engine.loss_acc_sampled).  Off by default:
# nobody has measured the device draw of ONE shuffle against the host's (tools/sampled_eval_probe.py is the measurement).
SAMPLED_DEVICE_DEFAULT = "0"
# DSGD_ASYNC_SNAPSHOT=1: MasterAsync.fit on an fp32 backend checks the loss through Engine.async_check -- loss, accuracy,
# update count and best weights of a check describe ONE snapshot of the moving weights (core/MasterAsync.scala:109-138), and
# the best weights stay on the device until the engine has stopped.  Off by default: nobody has measured a check through it
# against loss_acc + get_weights (tools/async_check_probe.py is the measurement).
ASYNC_SNAPSHOT_DEFAULT = "0"


def sampled_list(rnd: JavaRandom, length: int, samples_count: int, native: Optional[bool] = None):
    """`Random.shuffle(0 until length) take samples_count` (core/Master.scala:111, :116) as int32: one WHOLE shuffle from
    `rnd`, which advances over its length - 1 draws (plus rejections), and its first min(samples_count, length) entries.
    Natively (csrc/jrand.c: dsgd_jrand_shuffle) where lib/libdsgd_host.so is there, else scala_shuffle; `native` forces
    one of the two."""
    lib = _host_lib() if native in (None, True) else None
    if native is True and lib is None:
        raise RuntimeError("libdsgd_host.so is not built")
    if lib is None or length < 1 or length > 2 ** 31 - 1:
        return np.asarray(scala_shuffle(range(length), rnd)[:samples_count], dtype=np.int32)
    import ctypes as C

    buf = np.arange(length, dtype=np.int32)
    state = C.c_uint64(rnd.seed)
    lib.dsgd_jrand_shuffle(C.byref(state), buf.ctypes.data_as(C.c_void_p), C.c_int64(length))
    rnd.seed = int(state.value)
    return buf[:samples_count].copy()


class _SampledEval:
    """core/Master.scala:109-118 (shared by MasterSync and MasterAsync, which both extend AbstractMaster there): loss /
    accuracy over `Random.shuffle(workingData.indices) take samplesCount map workingData`.  Every call spends ONE shuffle of
    the whole window from self.rnd, as the reference spends it from the global generator that fit's per-batch shuffles
    use (:184) -- loss and accuracy are two calls and two different samples, and a fit that follows continues from where
    they left the stream.

    A chain of backends, each falling through to the next when it refuses (an error with code EUNSUPPORTED):
      1. backend.loss_acc_sampled (Engine: the DEVICE draws the sample and tallies it, one call), with DSGD_SAMPLED_DEVICE=1;
      2. backend.loss_acc_list (Engine: one launch) over a list drawn here (sampled_list: csrc/jrand.c, else scala_shuffle);
      3. backend.forward over that list and a fold here, as _DistributedEval folds (labels, get_weights and lam likewise).
    The three routes return the same tallies and leave self.rnd in the same state.  For use BETWEEN fits: while a prefetch of
    fit holds lists drawn ahead, the stream is not where the reference's would be, and the calls raise."""

    def _sampled_window(self, samples_count, test):
        lo, hi = (self.n_train, self.n_rows) if test else (0, self.n_train)
        # samples.map(...).reduce on an empty sample throws (core/ml/SparseSVM.scala:21-23).  (The JVM has spent the
        # shuffle's draws by then; here nothing is drawn.)
        if int(samples_count) < 1 or hi <= lo:
            raise ValueError("empty.reduceLeft: no samples to fold (samples_count %d of %d rows)" % (samples_count, max(0, hi - lo)))
        if getattr(self, "_pending", None) is not None or getattr(self, "_lists_future", None) is not None:
            raise RuntimeError("a prefetch of fit holds lists drawn ahead: the random stream is not where a sampled check "
                               "would draw from (sampled checks run between fits)")
        if getattr(self, "rnd", None) is None:
            self.rnd = JavaRandom(0)   # (the global Random, seeded 0 at Main.scala:32)
        return lo, hi

    @staticmethod
    def _refusal(e):
        return getattr(e, "code", None) == -7   # DSGD_EUNSUPPORTED

    def _sampled(self, samples_count, test, want_loss):
        """(loss or None, accuracy, counts {#p==y, #p==0, #p==-y}) over one freshly drawn sample."""
        lo, hi = self._sampled_window(samples_count, test)
        k = int(samples_count)
        if os.environ.get("DSGD_SAMPLED_DEVICE", SAMPLED_DEVICE_DEFAULT) == "1" and hasattr(self.backend, "loss_acc_sampled"):
            try:
                loss, acc, counts, state, _ = self.backend.loss_acc_sampled(self.rnd.seed, lo, hi, k)[:5]
                self.rnd.seed = int(state)
                return loss, acc, [int(c) for c in counts]
            except Exception as e:   # (refused: nothing was drawn)
                if not self._refusal(e):
                    raise
        idx = (sampled_list(self.rnd, hi - lo, k) + np.int32(lo)).astype(np.int32)
        if hasattr(self.backend, "loss_acc_list"):
            try:
                loss, acc, counts = self.backend.loss_acc_list(idx)
                return loss, acc, [int(c) for c in counts]
            except Exception as e:
                if not self._refusal(e):
                    raise
        y = self._labels(idx)   # (looked up first: a fold that cannot be made sends no request)
        pred = np.asarray(self.backend.forward(idx), dtype=np.float64)
        if getattr(self, "metrics", None) is not None:
            self.metrics.counter("slave.sync.forward", len(idx))   # one increment per sample: Slave.scala:131
        yp = y * pred
        counts = [int(np.count_nonzero(yp > 0)), int(np.count_nonzero(yp == 0)), int(np.count_nonzero(yp < 0))]
        n = len(idx)
        loss = None
        if want_loss:   # model.loss(p, y) = max(0, 1 - y p): 0, 1 or 2 per row (core/ml/SparseSVM.scala:16)
            loss = float(getattr(self.backend, "lam")) * self._norm_squared(None) + (counts[1] + 2.0 * counts[2]) / n
        return loss, counts[0] / n, counts

    def _sampled_timed(self, name, samples_count, test, want_loss):
        metrics = getattr(self, "metrics", None)
        if metrics is None:
            return self._sampled(samples_count, test, want_loss)
        with metrics.timer(name):
            return self._sampled(samples_count, test, want_loss)

    def local_sampled_loss(self, samples_count: int, test: bool = False):       # Master.scala:109-112
        return self._sampled_timed("master.sampled.loss.duration", samples_count, test, True)[0]

    def local_sampled_accuracy(self, samples_count: int, test: bool = False):   # Master.scala:114-118
        return self._sampled_timed("master.sampled.accuracy.duration", samples_count, test, False)[1]


# ---- Master.fit (synchronous) ---------------------------------------------------------------------------------
class MasterSync(_DistributedEval, _SampledEval):
    """core/Master.scala:120-218 for the workers hosted behind one backend.

    data layout: rows [0, n_train) are the train set, [n_train, n_rows) the test set (Main.scala:52)."""

    def __init__(self, backend, n_train: int, n_rows: int, node_count: int, rnd: Optional[JavaRandom] = None, log=None,
                 metrics: Optional[Metrics] = None, plans: Optional[bool] = None, prefetch: bool = True):
        """plans: run an epoch's batches as ONE resident plan of the backend (Engine.plan_flat / plan_run: the column-slice
        kernel runs all of the epoch's steps in one launch, 5 us per 3 x 100 step) instead of one backend.sync_step call per
        batch (32 us each); None = whenever the backend offers plans.  The random stream, the lists, the order of the
        steps and the arithmetic are the same either way; what changes is when the host sees a batch: the per-batch log
        lines and the `master.sync.batch.duration` timer are written after the epoch's launch (one entry per batch, the
        epoch's time shared evenly).  prefetch: while an epoch's steps run, the next epoch's plan is laid out and the lists of
        the epoch after it are drawn on a helper thread (if fit stops early the stream is put back to where the reference's
        would be: nothing of an epoch that never ran is kept)."""
        self.backend, self.n_train, self.n_rows, self.node_count = backend, n_train, n_rows, node_count
        self.metrics = metrics or Metrics()
        self.rnd = rnd or JavaRandom(0)
        self._logging = log is not None
        self.log = log or (lambda *a: None)
        self.plans = hasattr(backend, "plan_flat") if plans is None else bool(plans)
        # the epoch's lists drawn BY THE DEVICE, draw for draw the same stream (Engine.plan_from_seed, csrc/dsgd_shuffle.hpp):
        # 14 ms per epoch of RCV1 at full = true against 195 ms on 32 host threads; off by itself where the device form does
        # not apply (batches beyond 1,024 rows, splits beyond 2^20 rows) or DSGD_DEVICE_LISTS=0
        self.device_lists = self.plans and hasattr(backend, "plan_from_seed") and os.environ.get("DSGD_DEVICE_LISTS", "1") != "0"
        # ... and only for epochs of at least this many draws: the device form has ~1.5 ms of fixed cost per epoch (two
        # synchronisations, the host's walk over the candidates), the host draws 7 G values per second -- the full = false
        # configuration (1.15 M draws per epoch) is cheaper on the host (profiles/r06_fit_loop.txt)
        self.device_lists_min_draws = int(os.environ.get("DSGD_DEVICE_LISTS_MIN_DRAWS", 8 << 20))
        self.prefetch = prefetch
        self.losses: List[float] = []
        self.accs: List[float] = []
        self.test_losses: List[float] = []
        self.test_accs: List[float] = []
        self._pending = None
        self._lists_future = None
        self._executor = None
        self._rp_plans = False       # DSGD_F64_RP_PLANS=1 and an fp64 plan was refused: row-parallel plans from here on
        self._rp_seed_ok = True      # ... their lists drawn by the device until it refuses
        # DSGD_DEVICE_LISTS_JOB=1: where the device draw is refused, its job form is tried before the host's generator
        # (_plan_from_seed), per form (rp64 or not): "" = off or refused, "on" = to be tried, "serving" = it drew the last epoch
        self._job_form = dict.fromkeys((False, True), "on" if os.environ.get("DSGD_DEVICE_LISTS_JOB", "0") == "1" else "")
        self.batch_loop_s = 0.0      # wall time of the batch loops (shuffles, plan set-up, steps): Master.scala:179-199
        self.shuffle_s = 0.0         # ... of which drawing the lists (not overlapped by prefetch: see fit)
        self.steps_run = 0

    def local_loss(self, test: bool = False):  # Master.scala:104-106
        lo, hi = (self.n_train, self.n_rows) if test else (0, self.n_train)
        return self.backend.loss_acc(lo, hi)[0]

    def local_accuracy(self, test: bool = False):  # Master.scala:100-102
        lo, hi = (self.n_train, self.n_rows) if test else (0, self.n_train)
        return self.backend.loss_acc(lo, hi)[1]

    def fit(self, initial_weights, max_epochs: int, batch_size: int, learning_rate: float,
            stopping_criterion: Callable[[Sequence[float]], bool]) -> GradState:
        split = split_vanilla(self.n_train, self.node_count)  # Master.scala:136
        max_samples = max(len(r) for r in split)              # :138
        self.backend.set_weights(np.asarray(initial_weights, dtype=np.float32))
        state = GradState(np.asarray(initial_weights, dtype=np.float32))
        self._pending = None   # (plans + prefetch) the next epoch's plan, laid out while the current one runs
        try:
            return self._fit_loop(state, 0, split, max_samples, max_epochs, batch_size, learning_rate, stopping_criterion)
        finally:
            self._drop_pending()

    def _drop_pending(self):
        """fit is over: whatever was drawn or laid out for epochs that never ran is dropped, and the stream goes back to
        where the reference's generator stands (the draws are undone oldest first)."""
        fut, self._lists_future = getattr(self, "_lists_future", None), None
        ahead = fut.result() if fut is not None else None
        p, self._pending = getattr(self, "_pending", None), None
        if p is not None:
            self.rnd.seed = p["seed_before"]
            if p["plan"] is not None:
                p["plan"].destroy()
        elif ahead is not None:
            self.rnd.seed = ahead["seed_before"]
        ex, self._executor = getattr(self, "_executor", None), None
        if ex is not None:
            ex.shutdown(wait=True)

    def _draw_lists(self, split, max_samples, batch_size):
        seed_before = self.rnd.seed
        t0 = time.perf_counter()
        idx, offsets, n_steps = epoch_lists(self.rnd, split, max_samples, batch_size)
        return {"idx": idx, "offsets": offsets, "n_steps": n_steps, "seed_before": seed_before, "shuffle_s": time.perf_counter() - t0}

    def _take_lists(self, split, max_samples, batch_size):
        """The next epoch's lists: drawn ahead by the helper thread if one is at it (the wait, if any, counts as shuffle time
        that was not hidden), otherwise drawn now."""
        fut, self._lists_future = getattr(self, "_lists_future", None), None
        t0 = time.perf_counter()
        lists = fut.result() if fut is not None else self._draw_lists(split, max_samples, batch_size)
        self.shuffle_s += time.perf_counter() - t0
        return lists

    def _draw_ahead(self, split, max_samples, batch_size):
        """Start drawing the lists of the epoch after the next on a helper thread (the native generator releases the GIL):
        the main thread lays the next epoch's plan out meanwhile.  One drawer at a time: the stream is sequential."""
        if getattr(self, "_executor", None) is None:
            from concurrent.futures import ThreadPoolExecutor

            self._executor = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dsgd-lists")
        self._lists_future = self._executor.submit(self._draw_lists, split, max_samples, batch_size)

    def _make_plan(self, lists, n_workers, split=None, max_samples=0, batch_size=0):
        entry = {"plan": None, "n_steps": lists["n_steps"], "n_samples": int(lists["offsets"][lists["n_steps"] * n_workers]),
                 "seed_before": lists["seed_before"]}
        if lists["n_steps"]:
            try:
                if self._rp_plans:   # (refused before: not asked again)
                    raise _Refused()
                entry["plan"] = self.backend.plan_flat(lists["idx"], lists["offsets"], lists["n_steps"], n_workers)
            except Exception as e:
                # an fp64 backend refuses plans beyond its column-slice limits (DSGD_EUNSUPPORTED: more than 4 workers or
                # 1,024 rows per step): the epoch's steps run one by one through sync_step_f64, on the same lists
                if getattr(e, "code", None) != -7 or not self._fp64_steps():
                    raise
                if _f64_rp_plans():
                    # DSGD_F64_RP_PLANS=1: a row-parallel plan instead -- the device draws the lists the host has just drawn (the
                    # same stream from the same state: the generator stays where the host left it), else the host's go up
                    # (with a communicator attached the device draw is refused, -7: "try the next", and plan_flat(rp64=True)
                    # succeeds -- the epoch is ONE plan_run per rank)
                    self._rp_plans = True
                    rp = self._rp64_from_seed(lists["seed_before"], split, max_samples, batch_size) if split is not None else None
                    if rp is not None and rp["n_steps"] == lists["n_steps"]:
                        entry["plan"] = rp["plan"]
                        return entry
                    if rp is not None and rp["plan"] is not None:
                        rp["plan"].destroy()
                    try:
                        entry["plan"] = self.backend.plan_flat(lists["idx"], lists["offsets"], lists["n_steps"], n_workers, rp64=True)
                        return entry
                    except Exception as e2:
                        if getattr(e2, "code", None) != -7:
                            raise
                entry["lists"] = lists
        return entry

    def _rp64_from_seed(self, seed_before, split, max_samples, batch_size):
        """The epoch in front of generator state seed_before as a row-parallel plan whose lists the device draws
        (Engine.plan_from_seed(rp64=True)); None where that does not apply or is refused (DSGD_EUNSUPPORTED)."""
        if not (self._rp_seed_ok and hasattr(self.backend, "plan_from_seed") and os.environ.get("DSGD_DEVICE_LISTS", "1") != "0"
                and all(r.step == 1 for r in split)):
            return None
        t0 = time.perf_counter()
        try:
            plan, n_steps, state, _ = self._plan_from_seed(seed_before, split, max_samples, batch_size, rp64=True)
        except Exception as e:
            if getattr(e, "code", None) != -7:
                raise
            self._rp_seed_ok = False
            return None
        self.shuffle_s += time.perf_counter() - t0
        return {"plan": plan, "n_steps": n_steps, "n_samples": plan.n_samples if plan is not None else 0, "seed_before": seed_before,
                "state": state}

    def _plan_from_seed(self, seed_before, split, max_samples, batch_size, rp64=False):
        """backend.plan_from_seed -- and, with DSGD_DEVICE_LISTS_JOB=1, where that is refused (DSGD_EUNSUPPORTED: a batch
        beyond 1,024 rows, more than 64 rejections inside a shuffle, a communicator attached) the job form before the
        refusal reaches the caller (Engine.plan_from_seed_job: any batch size, 512 rejections, a local call under a
        communicator).  The job is the split hosted here -- or, where the backend reports `job_window` = (the split lengths
        of every worker of the job, the job index of the first worker hosted here), the window of that job, the hosted
        workers' rows starting where `split` says.  The same stream from the same state: the lists, the step count and the
        generator's state are the host's.  Once the job form has served an epoch the refused form is not asked again; a
        refusal of the job form is remembered too, and the first refusal is what the caller sees."""
        e1 = None
        if self._job_form[rp64] != "serving":
            try:
                return self.backend.plan_from_seed(seed_before, split, max_samples, batch_size, rp64=rp64) if rp64 else \
                    self.backend.plan_from_seed(seed_before, split, max_samples, batch_size)
            except Exception as e:
                if getattr(e, "code", None) != -7 or not self._job_form[rp64] or not hasattr(self.backend, "plan_from_seed_job"):
                    raise
                e1 = e
        job_lens, first = getattr(self.backend, "job_window", None) or ([len(r) for r in split], 0)
        try:
            out = self.backend.plan_from_seed_job(seed_before, job_lens, first, [r.start for r in split], max_samples, batch_size, rp64=rp64)
        except Exception as e2:
            if getattr(e2, "code", None) != -7:
                raise
            self._job_form[rp64] = ""
            raise (e1 or e2)
        self._job_form[rp64] = "serving"
        return out

    def _fp64_steps(self):
        return getattr(self.backend, "precision", "fp32") == "fp64" and hasattr(self.backend, "sync_step_f64")

    def _run_steps_f64(self, lists, n_workers, learning_rate):
        """The epoch's steps in order; returns the rows whose gradient was computed.  ONE sync_steps_f64 call where the backend
        has it (Engine.sync_steps_f64: the same bits, the boundary paid once); one sync_step_f64 call per step where it has
        not, where it refuses (DSGD_EUNSUPPORTED: a communicator is attached) or with DSGD_F64_STEPS=0."""
        idx, offs = lists["idx"], lists["offsets"]
        # (an epoch without a step -- a worker's slice empty from the first batch -- makes no call: fit raises the reference's error)
        if lists["n_steps"] >= 1 and hasattr(self.backend, "sync_steps_f64") and os.environ.get("DSGD_F64_STEPS", F64_STEPS_DEFAULT) != "0":
            try:
                st = self.backend.sync_steps_f64(idx, offs, lists["n_steps"], n_workers, learning_rate)
                return int(st.get("n_samples", 0)) if st else 0
            except RuntimeError as e:   # (DsgdError, and what the tests' backends raise)
                if getattr(e, "code", None) != -7:
                    raise
        n_samples = 0
        for s_ in range(lists["n_steps"]):
            o = offs[s_ * n_workers:(s_ + 1) * n_workers + 1]
            st = self.backend.sync_step_f64([idx[o[j]:o[j + 1]] for j in range(n_workers)], learning_rate)
            n_samples += int(st.get("n_samples", 0)) if st else 0
        return n_samples

    def _next_plan(self, split, max_samples, batch_size, n_workers, ahead_ok=False):
        """The next epoch as a plan: its lists drawn by the device where that applies, else by the host (csrc/jrand.c)."""
        draws = len(range(0, max_samples, batch_size)) * sum(len(r) - 1 for r in split)
        if self._rp_plans and getattr(self, "_lists_future", None) is None:   # (no draw of the host's is under way)
            seed_before = self.rnd.seed
            rp = self._rp64_from_seed(seed_before, split, max_samples, batch_size)
            if rp is not None:
                self.rnd.seed = rp.pop("state")
                return rp
        if not self._rp_plans and self.device_lists and draws >= self.device_lists_min_draws and all(r.step == 1 for r in split):
            seed_before = self.rnd.seed
            t0 = time.perf_counter()
            try:
                plan, n_steps, state, _ = self._plan_from_seed(seed_before, split, max_samples, batch_size)
            except Exception as e:   # (DSGD_EUNSUPPORTED: outside the device form -- the host draws from here on)
                if getattr(e, "code", None) != -7:
                    raise
                self.device_lists = False
                if _f64_rp_plans() and self._fp64_steps():   # (DSGD_F64_RP_PLANS=1: the same draws into a row-parallel plan)
                    self._rp_plans = True
                    rp = self._rp64_from_seed(seed_before, split, max_samples, batch_size)
                    if rp is not None:
                        self.rnd.seed = rp.pop("state")
                        return rp
            else:
                self.rnd.seed = state
                self.shuffle_s += time.perf_counter() - t0
                return {"plan": plan, "n_steps": n_steps, "n_samples": plan.n_samples if plan is not None else 0, "seed_before": seed_before}
        lists = self._take_lists(split, max_samples, batch_size)
        if ahead_ok and lists["n_steps"] == len(range(0, max_samples, batch_size)):
            self._draw_ahead(split, max_samples, batch_size)
        return self._make_plan(lists, n_workers, split, max_samples, batch_size)

    def _epoch_through_a_plan(self, split, max_samples, batch_size, learning_rate, epochs_left):
        """One epoch's batch loop (core/Master.scala:179-199) as one resident plan."""
        K = len(split)
        n_expected = len(range(0, max_samples, batch_size))
        # (not for an fp64 backend: its steps run through plans only -- include/dsgd.h "THE FP64 MODE")
        if batch_size >= max_samples and all(r.step == 1 for r in split) and hasattr(self.backend, "sync_step_ranges") \
                and getattr(self.backend, "precision", "fp32") != "fp64":
            # batch-size >= split size: slice(0, batchSize) of a shuffled split is the WHOLE split, and a sum does not
            # depend on the order -- the step is a sum over contiguous row ranges (dsgd_sync_step_ranges: the streaming
            # kernels).  The shuffles are still drawn: the generator must stand where the reference's stands.
            t_sh = time.perf_counter()
            epoch_lists(self.rnd, split, max_samples, batch_size)
            self.shuffle_s += time.perf_counter() - t_sh
            t0 = time.perf_counter_ns()
            self.backend.sync_step_ranges([(r.start, r.stop) for r in split], learning_rate)
            self.log("samples %d - %d / %d" % (1, max_samples, max_samples))
            with self.metrics._lock:
                self.metrics.histograms.setdefault("master.sync.batch.duration", []).append(time.perf_counter_ns() - t0)
            self.metrics.counter("slave.sync.backward", sum(len(r) for r in split))
            self.steps_run += 1
            return
        cur = getattr(self, "_pending", None)
        self._pending = None
        if cur is None:
            cur = self._next_plan(split, max_samples, batch_size, K)
        t0 = time.perf_counter_ns()
        try:
            if cur.get("lists") is not None:   # (an fp64 backend's refused plan: the steps one by one, synchronous)
                self._run_steps_f64(cur["lists"], K, learning_rate)
            elif cur["n_steps"]:
                self.backend.plan_run(cur["plan"], 0, cur["n_steps"], learning_rate)   # enqueued: ALL the epoch's steps, one launch
            if self.prefetch and epochs_left > 1 and cur["n_steps"] == n_expected:
                # ... and while they run: the next epoch's lists (drawn ahead already, from the second epoch on), the draw of the
                # epoch after it started on the helper thread, the next epoch's plan laid out (the device's build stream)
                self._pending = self._next_plan(split, max_samples, batch_size, K, ahead_ok=epochs_left > 2)
        finally:
            if cur["plan"] is not None:        # (also when the run or the next plan's set-up failed: the device blocks go back)
                cur["plan"].destroy()                                                # (behind the run; no synchronisation)
                cur["plan"] = None
        self.backend.synchronize()
        dt = time.perf_counter_ns() - t0
        # what the per-batch closure would have logged and recorded (:181-183, Slave.scala:145-150), written now
        if self._logging:
            for s_ in range(cur["n_steps"]):
                batch = s_ * batch_size
                self.log("samples %d - %d / %d" % (batch + 1, min(batch + batch_size, max_samples), max_samples))
        if cur["n_steps"]:
            with self.metrics._lock:   # one entry per batch, as the per-batch closure records them
                self.metrics.histograms.setdefault("master.sync.batch.duration", []).extend([dt // cur["n_steps"]] * cur["n_steps"])
            self.metrics.counter("slave.sync.backward", cur["n_samples"])
        self.steps_run += cur["n_steps"]
        if cur["n_steps"] < n_expected:
            # the reference's next batch hands some slave an empty slice: Vec.sum throws there (math/Vec.scala:129)
            raise ValueError("Cannot sum an empty list of vectors (batch %d of the epoch: a worker's slice is empty)" % cur["n_steps"])

    def _finished(self, state):
        if self.plans and state.updates:
            state = GradState(self.backend.get_weights(), state.loss, state.start, state.updates, state.end)
        return state.finish(self.losses[0] if self.losses else None)

    def _fit_loop(self, state, epoch, split, max_samples, max_epochs, batch_size, learning_rate, stopping_criterion):
        while True:
            if self.losses:
                self.log("loss after epoch %d: %s" % (epoch, self.losses[0]))
                self.log("acc after epoch %d: %s" % (epoch, self.accs[0]))
                self.metrics.histogram("master.sync.loss", self.losses[0])       # Master.scala:150 (.toLong)
                self.metrics.histogram("master.sync.acc", 100 * int(self.accs[0]))  # :151: 100 * accs.head.toLong
            if epoch >= max_epochs:                             # :154
                self.log("Reached max number of epochs: stopping computation")
                return self._finished(state)
            if stopping_criterion(self.test_losses):            # :166
                self.log("Converged to target: stopping computation")
                return self._finished(state)
            t_loop = time.perf_counter()
            if self.plans:
                self._epoch_through_a_plan(split, max_samples, batch_size, learning_rate, epochs_left=max_epochs - epoch)
            else:
                # :184 -- every worker's split is reshuffled for EVERY batch, then sliced.  Nothing else draws from the
                # generator inside the loop: the epoch's lists are drawn up front (the same draws in the same order;
                # natively when lib/libdsgd_host.so is there), then one request per batch
                t_sh = time.perf_counter()
                idx, offs, n_steps = epoch_lists(self.rnd, split, max_samples, batch_size)
                self.shuffle_s += time.perf_counter() - t_sh
                K = len(split)
                for s_, batch in enumerate(range(0, max_samples, batch_size)):    # :179
                    self.log("samples %d - %d / %d" % (batch + 1, min(batch + batch_size, max_samples), max_samples))   # :181
                    if s_ >= n_steps:
                        # a slice past the end of a short last split is empty: Vec.sum throws in that slave (math/Vec.scala:129)
                        raise ValueError("Cannot sum an empty list of vectors (batch %d of the epoch: a worker's slice is empty)" % s_)
                    lists = [idx[offs[s_ * K + j]:offs[s_ * K + j + 1]] for j in range(K)]
                    with self.metrics.timer("master.sync.batch.duration"):   # :183
                        st = self.backend.sync_step(lists, learning_rate)    # :186-197
                    self.steps_run += 1
                    if st:
                        self.metrics.counter("slave.sync.backward", st.get("n_samples", 0))  # Slave.scala:145-150
            if self.plans:
                # (the weights stay on the device between the epochs: GradState.grad is filled when fit returns -- the
                #  reference's master needs the vector every batch only because it ships it to the slaves)
                self.batch_loop_s += time.perf_counter() - t_loop
                state = state.replace_grad(state.grad)
            else:
                w = self.backend.get_weights()   # (synchronises: the epoch's steps are done)
                self.batch_loop_s += time.perf_counter() - t_loop
                state = state.replace_grad(w)
            # :206-209 -- four full passes per epoch; newest first
            l, a, _ = self.backend.loss_acc(0, self.n_train)
            tl, ta, _ = self.backend.loss_acc(self.n_train, self.n_rows)
            self.losses.insert(0, l)
            self.accs.insert(0, a)
            self.test_losses.insert(0, tl)
            self.test_accs.insert(0, ta)
            epoch += 1


# ---- MasterAsync.fit ------------------------------------------------------------------------------------------------
class MasterAsync(_DistributedEval, _SampledEval):
    """core/MasterAsync.scala:32-177 on top of the lock-free engine: start the workers, check the test loss
    every `check_every` updates with a leaky average, keep the best weights, stop on the criterion or at
    maxSteps = n_train * max_epochs updates (MasterAsync.scala:83)."""

    def __init__(self, backend, n_train: int, n_rows: int, node_count: int, log=None, poll_s: float = 0.0,
                 rnd: Optional[JavaRandom] = None):
        self.backend, self.n_train, self.n_rows, self.node_count = backend, n_train, n_rows, node_count
        self.rnd = rnd or JavaRandom(0)   # (the stream of the sampled checks: local_sampled_loss / local_sampled_accuracy)
        self.log = log or (lambda *a: None)
        self.poll_s = poll_s
        self.test_losses: List[float] = []
        self.test_accs: List[float] = []

    def fit(self, initial_weights, max_epoch: int, batch_size: int, learning_rate: float,
            stopping_criterion: Callable[[Sequence[float]], bool], check_every: int, leak_loss_coef: float,
            seed: int = 0, positional_bug: bool = True, max_steps: Optional[int] = None) -> GradState:
        if not (0 <= leak_loss_coef <= 1):
            raise ValueError("leaking coefficient must be between 0 and 1")  # MasterAsync.scala:97
        split = [(r.start, r.stop) for r in split_vanilla(self.n_train, self.node_count)]
        steps = self.n_train * max_epoch if max_steps is None else max_steps
        if getattr(self.backend, "precision", "fp32") == "fp64":
            value_bits = getattr(self.backend, "value_bits", None)
            if value_bits is not None and value_bits() == 64 and not _f64_rp_plans():
                # the zero-lag schedule runs resident asynchronous plans (column slices), which hold float values
                raise NotImplementedError(
                    "MasterAsync.fit is not available on Double feature values (Engine.load_csr with float64 values): resident "
                    "asynchronous plans are refused there (include/dsgd.h \"THE FP64 MODE\"); async_step_f64 serves single "
                    "iterations, DSGD_F64_RP_PLANS=1 runs the schedule on row-parallel plans, or load float32 values")
            return self._fit_fp64(initial_weights, split, steps, batch_size, learning_rate, stopping_criterion, check_every,
                                  leak_loss_coef, seed, positional_bug)
        self.backend.set_weights(np.asarray(initial_weights, dtype=np.float32))
        self.backend.async_start(split, batch=batch_size, lr=learning_rate, max_updates=steps, seed=seed,
                                 positional_bug=positional_bug)
        best_w, best_loss = np.asarray(initial_weights, dtype=np.float32), float("inf")
        last_step = -check_every
        state = GradState(best_w)
        # DSGD_ASYNC_SNAPSHOT=1: loss, accuracy, best weights and the update count of a check describe ONE snapshot
        snapshot = os.environ.get("DSGD_ASYNC_SNAPSHOT", ASYNC_SNAPSHOT_DEFAULT) == "1" and hasattr(self.backend, "async_check")
        kept = False
        try:
            while True:
                updates, running = self.backend.async_updates()
                if updates - last_step >= check_every or not running:
                    if snapshot:
                        computed_loss, computed_acc, _, window = self.backend.async_check(self.n_train, self.n_rows)
                        updates = int(window[0])   # (every update up to here is in the weights the loss is of)
                    else:
                        computed_loss, computed_acc, _ = self.backend.loss_acc(self.n_train, self.n_rows)
                    prev_l = self.test_losses[0] if self.test_losses else computed_loss
                    prev_a = self.test_accs[0] if self.test_accs else computed_acc
                    loss = leak_loss_coef * computed_loss + (1 - leak_loss_coef) * prev_l   # :122-125
                    acc = leak_loss_coef * computed_acc + (1 - leak_loss_coef) * prev_a
                    if best_loss > loss:                                                     # :132-138
                        if snapshot:
                            best_loss, kept = loss, True
                            self.backend.async_check_keep()   # (two device handles change places; read once, after the stop)
                        else:
                            best_loss, best_w = loss, self.backend.get_weights()
                    self.test_losses.insert(0, loss)
                    self.test_accs.insert(0, acc)
                    last_step = updates
                    if stopping_criterion(self.test_losses):                                # :146
                        self.log("converged to target: stopping computation")
                        break
                if not running:
                    break
                if self.poll_s:
                    time.sleep(self.poll_s)
        finally:
            self.backend.async_stop()                                                        # endComputation :87-94
        if kept:
            best_w = self.backend.async_check_weights(1)
        updates, _ = self.backend.async_updates()
        state = GradState(best_w, updates=int(updates)).finish(best_loss)
        return state

    # updates drawn per device plan of the fp64 schedule (one plan holds chunk x batch row indices and its layout)
    FP64_CHUNK = 4096

    def _check(self, leak_loss_coef):
        """One loss check (MasterAsync.scala:96-146): the leaky average of the test loss / accuracy."""
        computed_loss, computed_acc, _ = self.backend.loss_acc(self.n_train, self.n_rows)
        prev_l = self.test_losses[0] if self.test_losses else computed_loss
        prev_a = self.test_accs[0] if self.test_accs else computed_acc
        loss = leak_loss_coef * computed_loss + (1 - leak_loss_coef) * prev_l   # :122-125
        acc = leak_loss_coef * computed_acc + (1 - leak_loss_coef) * prev_a
        self.test_losses.insert(0, loss)
        self.test_accs.insert(0, acc)
        return loss

    def _fit_fp64(self, initial_weights, split, steps, batch_size, learning_rate, stopping_criterion, check_every,
                  leak_loss_coef, seed, positional_bug) -> GradState:
        """An fp64 backend (include/dsgd.h "THE FP64 MODE"): the ZERO-LAG schedule -- one update at a time, update u by
        worker u mod K at its iteration u div K, every update seen by all workers before the next one -- one
        deterministic schedule among those the reference allows (its own is racy).  The updates run on device plans
        drawn FP64_CHUNK at a time, check_every of them between two loss checks; no lock-free engine is started."""
        w0 = np.asarray(initial_weights, dtype=np.float64)
        self.backend.set_weights(w0)
        best_w, best_loss = w0.copy(), float("inf")
        updates, plan, plan_first = 0, None, 0
        chunk = max(self.FP64_CHUNK, check_every)
        rp64 = False   # DSGD_F64_RP_PLANS=1: from the first refused plan on (Double data, a batch or a model beyond the column slices)
        try:
            while True:
                loss = self._check(leak_loss_coef)
                if best_loss > loss:                                                         # :132-138
                    best_loss, best_w = loss, np.asarray(self.backend.get_weights(), dtype=np.float64).copy()
                if stopping_criterion(self.test_losses):                                    # :146
                    self.log("converged to target: stopping computation")
                    break
                if updates >= steps:
                    break
                target = min(steps, updates + check_every)
                while updates < target:
                    if plan is None or updates >= plan_first + plan.n_steps:
                        if plan is not None:
                            plan.destroy()
                        plan_first = updates
                        kw = dict(seed=seed, positional_bug=positional_bug, first_update=plan_first, n_updates=min(chunk, steps - plan_first))
                        try:
                            plan = self.backend.async_plan(split, batch_size, rp64=True, **kw) if rp64 else self.backend.async_plan(split, batch_size, **kw)
                        except Exception as e:
                            if rp64 or getattr(e, "code", None) != -7 or not _f64_rp_plans():
                                raise
                            rp64 = True
                            plan = self.backend.async_plan(split, batch_size, rp64=True, **kw)
                    end = min(target, plan_first + plan.n_steps)
                    self.backend.plan_run_async(plan, updates - plan_first, end - plan_first, learning_rate)
                    updates = end
        finally:
            if plan is not None:
                plan.destroy()
        return GradState(best_w, updates=int(updates)).finish(best_loss)


# ---- Master.fit for the logistic model ---------------------------------------------------------------------------------
def _logistic_rank_layout(n_train: int, n_rows: int, node_count: int, world: int, rank: int):
    """(the job's K train splits, k = K / world, the `world` test slices as ranges of global rows) of LogisticSync(ranks=...)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of a world of %d" % (rank, world))
    if not 0 < n_train < n_rows:
        raise ValueError("train rows [0, n_train) and test rows [n_train, n_rows)")
    if node_count < world or node_count % world:
        raise ValueError("a job of %d workers is not k x %d ranks: every rank hosts the same number" % (node_count, world))
    split = split_vanilla(n_train, node_count)
    if len(split) != node_count:
        raise ValueError("SplitStrategy.vanilla cuts %d train rows into %d groups, not %d: some rank would host a worker without rows"
                         % (n_train, len(split), node_count))
    tsplit = split_vanilla(n_rows - n_train, world)
    if len(tsplit) != world:
        raise ValueError("SplitStrategy.vanilla cuts %d test rows into %d slices, not %d: some rank would hold no test rows"
                         % (n_rows - n_train, len(tsplit), world))
    return split, node_count // world, [range(n_train + t.start, n_train + t.stop) for t in tsplit]


def logistic_rank_rows(n_train: int, n_rows: int, node_count: int, world: int, rank: int) -> np.ndarray:
    """The global row numbers rank `rank` of LogisticSync(ranks=(world, rank)) has loaded, in its order: the rows of the job's
    workers rank * k .. rank * k + k - 1 (k = node_count / world; SplitStrategy.vanilla over the n_train train rows), then test
    slice `rank` of SplitStrategy.vanilla over the test rows cut into `world`.  ValueError where the job does not cut that way."""
    split, k, tsplit = _logistic_rank_layout(n_train, n_rows, node_count, world, rank)
    parts = [np.arange(r.start, r.stop, dtype=np.int64) for r in split[rank * k:(rank + 1) * k]]
    parts.append(np.arange(tsplit[rank].start, tsplit[rank].stop, dtype=np.int64))
    return np.concatenate(parts)


class LogisticSync:
    """core/Master.scala:120-218 for the LOGISTIC model of one engine (include/dsgd.h "THE LOGISTIC MODEL").

    The flow is Master.fit's: SplitStrategy.vanilla splits; per epoch every worker's split is reshuffled for every batch
    from the reference's random stream; an epoch's steps run as ONE resident logistic plan (Engine.plan_run), whose lists
    the device draws (Engine.lg_plan_from_seed) -- or, where that is refused (DSGD_EUNSUPPORTED: a batch beyond 1,024
    rows, ...) or switched off, the host draws from the same stream (epoch_lists) and uploads (Engine.lg_plan_flat).  With
    `prefetch` the next epoch's plan is created while this one runs.  After the epoch train and test loss and accuracy
    come from ONE Engine.lg_loss_acc_ranges call, and the reference's stopping criterion looks at the test losses,
    newest first.  The lists, the weights and the figures are the same bits whichever side drew the lists.
    `slices` (off by default) asks both plan constructors for the column-slice form (Engine.lg_plan_flat): an epoch is then ONE
    persistent launch where the slices apply; the lists and the random stream are the same, the weights deterministic but
    not the bits of the default form.

    data layout: rows [0, n_train) are the train set, [n_train, n_rows) the test set (Main.scala:52).

    Evaluation as Master evaluates: predict / distributed_loss / distributed_accuracy over the splits fit steps on, as ONE
    Engine.lg_predict_ranges call (classes signum(x . w): the textbook sign, not the SVM's); local_sampled_loss /
    local_sampled_accuracy with _SampledEval's stream discipline -- every call spends one whole shuffle of the window from
    self.rnd, drawn by the device (DSGD_SAMPLED_DEVICE=1, Engine.lg_loss_acc_sampled) or here (sampled_list, then
    Engine.lg_loss_acc_list), the same numbers and the same generator state either way; for use between fits.

    ACROSS RANKS (`ranks=(world, rank)`; the backend is attached with Engine.comm_init_lg; include/dsgd.h "ACROSS RANKS").  n_train,
    n_rows and node_count stay the JOB's: node_count = K = k x world workers, rank r has loaded logistic_rank_rows(...) -- the rows
    of the job's workers r k .. r k + k - 1 in order, then test slice r of the test rows cut into `world`.  Per epoch the rank's
    window of the job's lists comes from Engine.lg_plan_from_seed_job (ONE stream over all K workers) or, where that is refused
    or switched off, from epoch_lists over the whole job, of which the rank keeps its window mapped to its local rows
    (Engine.lg_plan_flat): the random stream ends where one process's ends either way.  plan_run is collective; then two
    Engine.lg_eval_job calls, the k train ranges and the one test range, give train and test loss and accuracy of the JOB --
    identical on every rank (the bits of ONE engine's lg_predict_ranges over the K splits / the `world` test slices), so every
    rank takes the same stopping decision with nothing more exchanged.  The weights after every epoch are the bits of the
    one-process mirror.  distributed_loss / distributed_accuracy / local_loss / local_accuracy go through lg_eval_job (collective);
    predict returns this rank's rows (global numbers) and classes.  local_sampled_* raise: the sampled window is the master's data,
    which no rank holds.  slices=True raises: column slices do not span ranks.

    Limits: without `ranks` one engine hosts every worker (at most 256 of them for the distributed calls) and the evaluation is
    this engine's; with `ranks` at most 256 workers in the job; no asynchronous fit across ranks, no JNI."""

    def __init__(self, backend, n_train: int, n_rows: int, node_count: int, rnd: Optional[JavaRandom] = None, log=None,
                 metrics: Optional[Metrics] = None, device_lists: Optional[bool] = None, prefetch: bool = True, slices: bool = False,
                 ranks: Optional[Sequence[int]] = None):
        if not 0 < n_train < n_rows:
            raise ValueError("LogisticSync needs train rows [0, n_train) and test rows [n_train, n_rows)")
        self.backend, self.n_train, self.n_rows, self.node_count = backend, n_train, n_rows, node_count
        self.ranks = None
        if ranks is not None:
            world, rank = int(ranks[0]), int(ranks[1])
            if slices:
                raise ValueError("LogisticSync(ranks=...): column slices do not span ranks (slices=True is one process's)")
            self._job_split, self._k, tsplit = _logistic_rank_layout(n_train, n_rows, node_count, world, rank)
            self.ranks = (world, rank)
            self._first = rank * self._k
            mine = self._job_split[self._first:self._first + self._k]
            self._local_begin = [int(b) for b in np.cumsum([0] + [len(r) for r in mine])]   # k + 1: the local train rows end at [-1]
            self._train_ranges = [(self._local_begin[j], self._local_begin[j + 1]) for j in range(self._k)]
            self._test_range = (self._local_begin[-1], self._local_begin[-1] + len(tsplit[rank]))
        self.metrics = metrics or Metrics()
        self.rnd = rnd or JavaRandom(0)
        self.log = log or (lambda *a: None)
        self.device_lists = os.environ.get("DSGD_DEVICE_LISTS", "1") != "0" if device_lists is None else bool(device_lists)
        self.prefetch = prefetch
        self.slices = bool(slices)
        self.losses: List[float] = []
        self.accs: List[float] = []
        self.test_losses: List[float] = []
        self.test_accs: List[float] = []
        self.steps_run = 0
        self.device_drawn_epochs = 0
        self._pending = None

    def _job_eval(self, test: bool = False, weights=None):
        """(ranks) (loss, acc) of the JOB's train splits or test slices: ONE collective Engine.lg_eval_job call."""
        out = self.backend.lg_eval_job([self._test_range] if test else self._train_ranges, weights)
        return out[2], out[3]

    def local_loss(self, test: bool = False):       # Master.scala:104-106
        if self.ranks:
            return self._job_eval(test)[0]
        lo, hi = (self.n_train, self.n_rows) if test else (0, self.n_train)
        return self.backend.lg_loss_acc(lo, hi)[0]

    def local_accuracy(self, test: bool = False):   # Master.scala:100-102
        if self.ranks:
            return self._job_eval(test)[1]
        lo, hi = (self.n_train, self.n_rows) if test else (0, self.n_train)
        return self.backend.lg_loss_acc(lo, hi)[1]

    def predict_proba(self, rows):
        """P(y = +1 | x) of the listed rows under the resident weights (Engine.lg_predict_proba)."""
        return self.backend.lg_predict_proba(rows)

    # -- Master.predict / distributedLoss / distributedAccuracy (core/Master.scala:61-98) --
    def _predict_ranges(self, weights, want_proba=False):
        """ONE Engine.lg_predict_ranges call over the splits fit steps on: (split, its return value)."""
        split = split_vanilla(self.n_train, self.node_count)   # splitStrategy(data, workers.size)
        if len(split) > getattr(self.backend, "lg_predict_max_ranges", 256):
            raise ValueError("%d splits: more than the %d ranges of one lg_predict_ranges call"
                             % (len(split), getattr(self.backend, "lg_predict_max_ranges", 256)))
        ranges = [(r.start, r.stop) for r in split]
        out = self.backend.lg_predict_ranges(ranges, weights, True) if want_proba else self.backend.lg_predict_ranges(ranges, weights)
        return split, out

    def predict(self, weights=None):
        """Master.predict (:61-75): (rows, classes) in split order -- rows int64, classes int8 signum(x . w), the textbook
        sign.  weights: None evaluates the resident weights, a vector replaces them."""
        if self.ranks:   # this rank's rows (the job's numbers) and their classes: a local call
            mine = self._job_split[self._first:self._first + self._k]
            out = self.backend.lg_predict_ranges(self._train_ranges, weights)
            return np.concatenate([np.arange(r.start, r.stop, dtype=np.int64) for r in mine]), np.asarray(out[0])
        split, out = self._predict_ranges(weights)
        rows = np.concatenate([np.arange(r.start, r.stop, dtype=np.int64) for r in split]) if split else np.zeros(0, np.int64)
        return rows, np.asarray(out[0])

    def distributed_loss_and_accuracy(self, weights=None):
        """(distributedLoss, distributedAccuracy) from ONE pass over the splits (the reference runs predict once for each)."""
        if self.ranks:
            return self._job_eval(False, weights)
        _, out = self._predict_ranges(weights)
        return out[4], out[5]

    def distributed_loss(self, weights=None):       # Master.scala:87-98
        return self.distributed_loss_and_accuracy(weights)[0]

    def distributed_accuracy(self, weights=None):   # Master.scala:77-85
        return self.distributed_loss_and_accuracy(weights)[1]

    # -- Master.localSampledLoss / localSampledAccuracy (core/Master.scala:109-118): _SampledEval's stream discipline --
    _sampled_window = _SampledEval._sampled_window   # (the window, the refusal of an empty sample, and of a pending prefetch)

    def _sampled(self, samples_count, test):
        """(loss, accuracy, counts) over one freshly drawn sample: ONE whole shuffle of the window is spent from self.rnd.  With
        DSGD_SAMPLED_DEVICE=1 the device draws (Engine.lg_loss_acc_sampled); otherwise, or where it refuses (EUNSUPPORTED:
        nothing was drawn), sampled_list feeds Engine.lg_loss_acc_list -- the same numbers and the same generator state.
        Across ranks (ranks=...) it raises: the sampled window is the master's data, which no rank holds."""
        if self.ranks:
            raise ValueError("LogisticSync(ranks=...): local_sampled_* draw from the master's data, which no rank holds")
        lo, hi = self._sampled_window(samples_count, test)
        k = int(samples_count)
        if os.environ.get("DSGD_SAMPLED_DEVICE", SAMPLED_DEVICE_DEFAULT) == "1" and hasattr(self.backend, "lg_loss_acc_sampled"):
            try:
                loss, acc, counts, state, _ = self.backend.lg_loss_acc_sampled(self.rnd.seed, lo, hi, k)[:5]
                self.rnd.seed = int(state)
                return loss, acc, [int(c) for c in counts]
            except Exception as e:   # (refused: nothing was drawn)
                if not _SampledEval._refusal(e):
                    raise
        idx = (sampled_list(self.rnd, hi - lo, k) + np.int32(lo)).astype(np.int32)
        loss, acc, counts = self.backend.lg_loss_acc_list(idx)
        return loss, acc, [int(c) for c in counts]

    def local_sampled_loss(self, samples_count: int, test: bool = False):       # Master.scala:109-112
        with self.metrics.timer("master.sampled.loss.duration"):
            return self._sampled(samples_count, test)[0]

    def local_sampled_accuracy(self, samples_count: int, test: bool = False):   # Master.scala:114-118
        with self.metrics.timer("master.sampled.accuracy.duration"):
            return self._sampled(samples_count, test)[1]

    def _next_plan(self, split, max_samples, batch_size):
        """The next epoch as a logistic plan: its lists drawn by the device where that applies, else by the host."""
        if self.ranks:
            return self._next_plan_ranks(split, max_samples, batch_size)
        seed_before = self.rnd.seed
        if self.device_lists and all(r.step == 1 for r in split):
            try:
                kw = {"slices": True} if self.slices else {}   # (a backend without the keyword serves the default)
                plan, n_steps, state, _ = self.backend.lg_plan_from_seed(seed_before, split, max_samples, batch_size, **kw)
            except Exception as e:   # (DSGD_EUNSUPPORTED: outside the device form -- the host draws from here on)
                if getattr(e, "code", None) != -7:
                    raise
                self.device_lists = False
            else:
                self.rnd.seed = state
                return {"plan": plan, "n_steps": n_steps, "n_samples": plan.n_samples if plan is not None else 0, "seed_before": seed_before,
                        "device_drawn": True}
        idx, offsets, n_steps = epoch_lists(self.rnd, split, max_samples, batch_size)
        kw = {"slices": True} if self.slices else {}
        plan = self.backend.lg_plan_flat(idx, offsets, n_steps, len(split), **kw) if n_steps else None
        return {"plan": plan, "n_steps": n_steps, "n_samples": int(offsets[n_steps * len(split)]), "seed_before": seed_before, "device_drawn": False}

    def _next_plan_ranks(self, split, max_samples, batch_size):
        """(ranks) This rank's window of the JOB's next epoch: the k hosted workers' lists over the local rows.  The stream advances
        over the whole job either way."""
        seed_before = self.rnd.seed
        k, first = self._k, self._first
        if self.device_lists:
            try:
                plan, n_steps, state, _ = self.backend.lg_plan_from_seed_job(seed_before, [len(r) for r in split], first, self._local_begin[:k],
                                                                             max_samples, batch_size)
            except Exception as e:   # (DSGD_EUNSUPPORTED: outside the device form -- the host draws from here on)
                if getattr(e, "code", None) != -7:
                    raise
                self.device_lists = False
            else:
                self.rnd.seed = state
                return {"plan": plan, "n_steps": n_steps, "n_samples": plan.n_samples if plan is not None else 0, "seed_before": seed_before,
                        "device_drawn": True}
        idx, offsets, n_steps = epoch_lists(self.rnd, split, max_samples, batch_size)   # the whole job, from the same stream
        K = len(split)
        flat, offs = [], [0]
        for s_ in range(n_steps):
            for j in range(k):
                g = s_ * K + first + j
                rows = np.asarray(idx[int(offsets[g]):int(offsets[g + 1])], dtype=np.int64) - split[first + j].start + self._local_begin[j]
                flat.append(rows.astype(np.int32))
                offs.append(offs[-1] + len(rows))
        plan = self.backend.lg_plan_flat(np.concatenate(flat), np.asarray(offs, dtype=np.int64), n_steps, k) if n_steps else None
        return {"plan": plan, "n_steps": n_steps, "n_samples": offs[-1], "seed_before": seed_before, "device_drawn": False}

    def _drop_pending(self):
        """fit is over: the plan of an epoch that never ran is dropped and the stream goes back to where the reference's stands."""
        p, self._pending = self._pending, None
        if p is not None:
            self.rnd.seed = p["seed_before"]
            if p["plan"] is not None:
                p["plan"].destroy()

    def _epoch(self, split, max_samples, batch_size, learning_rate, epochs_left):
        """One epoch's batch loop (core/Master.scala:179-199) as one plan run."""
        n_expected = len(range(0, max_samples, batch_size))
        cur, self._pending = self._pending, None
        if cur is None:
            cur = self._next_plan(split, max_samples, batch_size)
        t0 = time.perf_counter_ns()
        try:
            if cur["n_steps"]:
                self.backend.plan_run(cur["plan"], 0, cur["n_steps"], learning_rate)   # enqueued: two launches per step, no read
            if self.prefetch and epochs_left > 1 and cur["n_steps"] == n_expected:
                self._pending = self._next_plan(split, max_samples, batch_size)        # ... and while they run: the next epoch's plan
        finally:
            if cur["plan"] is not None:
                cur["plan"].destroy()                                                  # (behind the run; no synchronisation)
                cur["plan"] = None
        if cur["n_steps"] < n_expected:
            self.backend.synchronize()
            # the reference's next batch hands some slave an empty slice: Vec.sum throws there (math/Vec.scala:129)
            raise ValueError("Cannot sum an empty list of vectors (batch %d of the epoch: a worker's slice is empty)" % cur["n_steps"])
        # :206-209 -- the epoch's evaluation passes: one launch, one synchronisation (behind the epoch's steps)
        if self.ranks:   # the JOB's figures on every rank: two collective calls, the k train ranges, then the one test range
            (l, a), (tl, ta) = self._job_eval(False), self._job_eval(True)
        else:
            (l, a), (tl, ta) = self.backend.lg_loss_acc_ranges([(0, self.n_train), (self.n_train, self.n_rows)])
        dt = time.perf_counter_ns() - t0
        self.backend.synchronize()   # (the stream is idle: the rows the plan ran are collected)
        for s_ in range(cur["n_steps"]):
            batch = s_ * batch_size
            self.log("samples %d - %d / %d" % (batch + 1, min(batch + batch_size, max_samples), max_samples))
        with self.metrics._lock:
            self.metrics.histograms.setdefault("master.sync.batch.duration", []).extend([dt // cur["n_steps"]] * cur["n_steps"])
        self.metrics.counter("slave.sync.backward", cur["n_samples"])
        self.steps_run += cur["n_steps"]
        self.device_drawn_epochs += 1 if cur["device_drawn"] else 0
        self.losses.insert(0, l)
        self.accs.insert(0, a)
        self.test_losses.insert(0, tl)
        self.test_accs.insert(0, ta)

    def fit(self, initial_weights, max_epochs: int, batch_size: int, learning_rate: float,
            stopping_criterion: Callable[[Sequence[float]], bool]) -> GradState:
        split = split_vanilla(self.n_train, self.node_count)  # Master.scala:136
        max_samples = max(len(r) for r in split)              # :138
        self.backend.set_weights(np.asarray(initial_weights, dtype=np.float32))
        state = GradState(np.asarray(initial_weights, dtype=np.float32))
        self._pending = None
        epoch = 0
        try:
            while True:
                if self.losses:
                    self.log("loss after epoch %d: %s" % (epoch, self.losses[0]))
                    self.log("acc after epoch %d: %s" % (epoch, self.accs[0]))
                    self.metrics.histogram("master.sync.loss", self.losses[0])          # Master.scala:150
                    self.metrics.histogram("master.sync.acc", 100 * int(self.accs[0]))  # :151
                if epoch >= max_epochs:                             # :154
                    self.log("Reached max number of epochs: stopping computation")
                    break
                if stopping_criterion(self.test_losses):            # :166
                    self.log("Converged to target: stopping computation")
                    break
                self._epoch(split, max_samples, batch_size, learning_rate, epochs_left=max_epochs - epoch)
                state = state.replace_grad(state.grad)   # (the weights stay on the device between the epochs)
                epoch += 1
        finally:
            self._drop_pending()
        if state.updates:
            state = GradState(self.backend.get_weights(), state.loss, state.start, state.updates, state.end)
        return state.finish(self.losses[0] if self.losses else None)


# ---- Master.fit over several topics -------------------------------------------------------------------------------
class LogisticTopics:
    """Master.fit's flow (core/Master.scala:120-218) for T one-vs-rest logistic models on ONE engine whose topics are set
    (Engine.lg_topics_set; include/dsgd.h "SEVERAL TOPICS"), the lists shared: SplitStrategy.vanilla's splits, per epoch
    epoch_lists from ONE JavaRandom, ONE Engine.lg_topics_sync_steps (two launches per step whatever T), ONE
    Engine.lg_topics_loss_acc each over the train and the test rows.

    The stopping rule is applied PER TOPIC, to that topic's test losses, newest first.  A topic's GradState is taken at the
    epoch where its own rule first fires (or max_epochs is reached): its weights are read then, the other topics go on --
    the finished topic keeps being stepped with them, which nobody looks at.  So topic t's GradState (weights, loss,
    updates) is what host.LogisticSync alone returns for an engine whose labels are plane t, from the same seed.

    data layout: rows [0, n_train) are the train set, [n_train, n_rows) the test set.  Limits: one engine, no plans, no
    ranks, no column slices, one learning rate and one lambda for all topics."""

    def __init__(self, backend, n_train: int, n_rows: int, node_count: int, rnd: Optional[JavaRandom] = None, log=None):
        if not 0 < n_train < n_rows:
            raise ValueError("LogisticTopics needs train rows [0, n_train) and test rows [n_train, n_rows)")
        self.backend, self.n_train, self.n_rows, self.node_count = backend, n_train, n_rows, node_count
        self.rnd = rnd or JavaRandom(0)
        self.log = log or (lambda *a: None)
        self.losses: List[List[float]] = []        # per topic, newest first
        self.accs: List[List[float]] = []
        self.test_losses: List[List[float]] = []
        self.test_accs: List[List[float]] = []
        self.steps_run = 0

    def fit(self, initial_weights, max_epochs: int, batch_size: int, learning_rate: float,
            stopping_criterion: Callable[[Sequence[float]], bool]) -> List[GradState]:
        split = split_vanilla(self.n_train, self.node_count)
        max_samples = max(len(r) for r in split)
        n_expected = len(range(0, max_samples, batch_size))
        W0 = np.ascontiguousarray(initial_weights, dtype=np.float32)
        if W0.ndim != 2:
            raise ValueError("initial_weights must be [T, D + 1]")
        T = W0.shape[0]
        self.backend.lg_topics_set_weights(W0)
        self.losses, self.accs = [[] for _ in range(T)], [[] for _ in range(T)]
        self.test_losses, self.test_accs = [[] for _ in range(T)], [[] for _ in range(T)]
        start = time.time()
        done: List[Optional[GradState]] = [None] * T
        epoch = 0
        while True:
            fired = []
            for t in range(T):
                if done[t] is not None:
                    continue
                if epoch >= max_epochs:
                    self.log("topic %d: reached max number of epochs" % t)
                    fired.append(t)
                elif stopping_criterion(self.test_losses[t]):
                    self.log("topic %d: converged to target after epoch %d" % (t, epoch))
                    fired.append(t)
            if fired:
                W = self.backend.lg_topics_get_weights() if epoch else W0
                for t in fired:
                    done[t] = GradState(np.array(W[t], dtype=np.float32), None, start, epoch, None).finish(self.losses[t][0] if self.losses[t] else None)
            if all(s is not None for s in done):
                break
            idx, offsets, n_steps = epoch_lists(self.rnd, split, max_samples, batch_size)
            if n_steps:
                self.backend.lg_topics_sync_steps(idx, offsets, n_steps, len(split), learning_rate)
            if n_steps < n_expected:
                # the reference's next batch hands some slave an empty slice: Vec.sum throws there (math/Vec.scala:129)
                raise ValueError("Cannot sum an empty list of vectors (batch %d of the epoch: a worker's slice is empty)" % n_steps)
            l, a = self.backend.lg_topics_loss_acc(0, self.n_train)
            tl, ta = self.backend.lg_topics_loss_acc(self.n_train, self.n_rows)
            self.steps_run += n_steps
            for t in range(T):
                self.losses[t].insert(0, float(l[t]))
                self.accs[t].insert(0, float(a[t]))
                self.test_losses[t].insert(0, float(tl[t]))
                self.test_accs[t].insert(0, float(ta[t]))
            epoch += 1
        return done


# ---- MasterAsync.fit for the logistic model ---------------------------------------------------------------------------
class LogisticAsync:
    """core/MasterAsync.scala:32-178 for the LOGISTIC model of one engine, on the ZERO-LAG schedule (include/dsgd.h "THE LOGISTIC
    MODEL": ASYNCHRONOUS) -- the way MasterAsync runs an fp64 backend: one update at a time, update u by worker u mod K at its
    iteration u div K over SplitStrategy.vanilla's splits, every update seen by all workers before the next one.  One
    deterministic schedule among those the reference allows (its own is racy); no lock-free engine is started.

    The updates run on one-worker logistic plans whose lists the device draws (Engine.lg_async_plan), CHUNK updates per plan,
    `check_every` of them between two loss checks (Engine.plan_run_async_lg).  A check takes the test loss and accuracy from
    ONE Engine.lg_loss_acc_ranges call, folds them into the leaky average (MasterAsync.scala:122-125), keeps the best weights
    (:132-138) and asks the stopping criterion, newest first (:146); the run ends at maxSteps = n_train * max_epoch updates
    (:83).  `slices` (off by default) asks for the column-slice form: a window of updates is then ONE persistent launch; the
    lists are the same, the weights deterministic but not the bits of the default form.

    data layout: rows [0, n_train) are the train set, [n_train, n_rows) the test set (Main.scala:52)."""

    CHUNK = 4096   # updates drawn per device plan

    def __init__(self, backend, n_train: int, n_rows: int, node_count: int, log=None, slices: bool = False):
        if not 0 < n_train < n_rows:
            raise ValueError("LogisticAsync needs train rows [0, n_train) and test rows [n_train, n_rows)")
        self.backend, self.n_train, self.n_rows, self.node_count = backend, n_train, n_rows, node_count
        self.log = log or (lambda *a: None)
        self.slices = bool(slices)
        self.test_losses: List[float] = []
        self.test_accs: List[float] = []
        self.checks = 0

    def _check(self, leak_loss_coef):
        """One loss check (MasterAsync.scala:96-146): the leaky average of the test loss / accuracy."""
        (computed_loss, computed_acc), = self.backend.lg_loss_acc_ranges([(self.n_train, self.n_rows)])
        prev_l = self.test_losses[0] if self.test_losses else computed_loss
        prev_a = self.test_accs[0] if self.test_accs else computed_acc
        loss = leak_loss_coef * computed_loss + (1 - leak_loss_coef) * prev_l   # :122-125
        acc = leak_loss_coef * computed_acc + (1 - leak_loss_coef) * prev_a
        self.test_losses.insert(0, loss)
        self.test_accs.insert(0, acc)
        self.checks += 1
        return loss

    def fit(self, initial_weights, max_epoch: int, batch_size: int, learning_rate: float,
            stopping_criterion: Callable[[Sequence[float]], bool], check_every: int, leak_loss_coef: float,
            seed: int = 0, positional_bug: bool = True, max_steps: Optional[int] = None) -> GradState:
        if not (0 <= leak_loss_coef <= 1):
            raise ValueError("leaking coefficient must be between 0 and 1")  # MasterAsync.scala:97
        if check_every < 1:
            raise ValueError("check_every must be at least 1")
        split = [(r.start, r.stop) for r in split_vanilla(self.n_train, self.node_count)]
        steps = self.n_train * max_epoch if max_steps is None else max_steps   # :83
        w0 = np.asarray(initial_weights, dtype=np.float32)
        self.backend.set_weights(w0)
        best_w, best_loss = w0.copy(), float("inf")
        updates, plan, plan_first = 0, None, 0
        kw = {"slices": True} if self.slices else {}
        try:
            while True:
                loss = self._check(leak_loss_coef)
                if best_loss > loss:                                                         # :132-138
                    best_loss, best_w = loss, np.asarray(self.backend.get_weights(), dtype=np.float32).copy()
                if stopping_criterion(self.test_losses):                                    # :146
                    self.log("converged to target: stopping computation")
                    break
                if updates >= steps:
                    break
                target = min(steps, updates + check_every)
                while updates < target:
                    if plan is None or updates >= plan_first + plan.n_steps:
                        if plan is not None:
                            plan.destroy()
                        plan, plan_first = None, updates
                        plan = self.backend.lg_async_plan(split, batch_size, seed=seed, positional_bug=positional_bug, first_update=plan_first,
                                                          n_updates=min(self.CHUNK, steps - plan_first), **kw)
                    end = min(target, plan_first + plan.n_steps)
                    self.backend.plan_run_async_lg(plan, updates - plan_first, end - plan_first, learning_rate)
                    updates = end
                self.backend.synchronize()   # (the rows the window ran are collected; the check below reads behind them)
        finally:
            if plan is not None:
                plan.destroy()
        return GradState(best_w, updates=int(updates)).finish(best_loss)
