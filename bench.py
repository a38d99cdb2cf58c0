#!/usr/bin/env python3
"""bench.py -- RCV1 examples/s of the synchronous SGD hot path on N MI355X (one process per GPU).

    python bench.py --gpus 1 --steps 20 --warmup 3          (the headline alone: exactly K timed steps)
    python bench.py --gpus 1 --steps 20 --warmup 3 --full   (with every leg, check and baseline described below)
    python bench.py --gpus N ...            (no launcher: spawns its own N ranks, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N --scaling strong --rows-total 804414      (ONE data set split over the ranks)

A "step" is one synchronous SGD step of the reference's Master.fit batch closure
(core/Master.scala:184-197) over one batch of synthetic RCV1-like rows: per-worker gated
sub-gradient sum + support-only regulariser (core/Slave.scala:142-157), mean over workers
(an RCCL all-reduce when N > 1), w <- w - lr * mean.  The batch is the worker's whole train
shard (batch-size >= split size), i.e. every step streams the resident CSR shard once --
the configuration in which the path is HBM-bound.  A plain run sets up, ramps the clocks, warms up, times
the K steps once and prints the line (--dump-outputs DIR also writes the weights the last timed step left).  With --full
the K steps are timed --repeats times (default 5, the median is quoted) and beside the headline the line carries the
roofline of the dominant kernel, the CPU baseline, the reference's own shapes (N = 804,414 and 23,149 rows:
`reference_shapes`), a batch sweep incl. the reference's default batch-size 100 (`sweep`), wall-clock time to the
oracle's target loss per batch size (`time_to_target`), the lock-free mode with its traced parity check (`hogwild`) and
the dense variant.

Scaling: "weak" (default) gives every rank its own --rows rows; "strong" splits ONE data set of --rows-total rows over
the ranks with the reference's SplitStrategy.vanilla (core/ml/SplitStrategy.scala:13-14), as its Master does over its
slaves (core/Master.scala:136).

With --full every number is gated by the oracle first (checker only, outside every timed region): the benchmarked
whole-shard step at N = 1; with N > 1 a step over the first --gate-rows train rows of EVERY rank against the oracle hosting all of them
as world x workers workers (Master.scala:194: the mean runs over the workers).

Inputs are generated on the host, uploaded once and resident in HBM before the timed region.
Rank 0 writes the FULL result object to --detail (default gpurun_out/bench_detail.json) and prints ONE compact JSON line
(< 8 KB: contract keys, roofline, cpu_baseline, one summary row per leg) as the LAST line of stdout.
"""

from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12      # B/s, spec (MI355X_MICROARCH.md "Chip-level parameters")
HBM_MEASURED = 6.29e12  # B/s, float4-copy ceiling from the same table
LR0, LAMBDA = 0.5, 1e-5  # application.conf:18,21 (learning-rate is per batch of 100, application.conf:15)
LINE_TARGET, LINE_LIMIT = 4096, 8192   # bytes of the final stdout line: aimed at / never exceeded (the driver keeps an 8 KB tail)
STATED_TOL = 1e-5        # BASELINE.md's parity gate: max|w - w_oracle| <= 1e-5 * max(1, |w_oracle|_inf), asserted beside the derived bound


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K timed steps are measured this many times (each between barriers); value = the median "
                         "(default: 1, so that exactly K steps are timed; 5 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline as well: the parity gate, the replica digest, roofline (HIP events "
                         "inside the clock), the sweep and the other legs, the CPU baseline (each still subject to its "
                         "--no-* switch); a plain run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (the weights a caller of the step "
                         "receives) as DIR/weights.npy (float32); the inputs depend on the arguments alone")
    ap.add_argument("--rows", type=int, default=int(os.environ.get("DSGD_BENCH_ROWS", 8388608)),
                    help="weak scaling: rows per GPU.  8388608 (5.1 GB of CSR, BASELINE.md section 3) keeps the stream in HBM; "
                         "804414 = RCV1 full=true (DatasetTests.scala:18) fits mostly in the 256 MiB Infinity Cache")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--rows-total", type=int, default=804414,
                    help="strong scaling: rows of the ONE data set that SplitStrategy.vanilla splits over the ranks")
    ap.add_argument("--workers", type=int, default=1, help="virtual workers (node-count share) per GPU")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gate-rows", type=int, default=200000, help="N > 1: train rows per rank of the parity gate's step")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-sweep", action="store_true", help="--full: skip every leg beside the headline (sweep, reference shapes, ...)")
    ap.add_argument("--no-parity-gate", action="store_true", help="--full: skip every oracle comparison (profiling runs)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget for each CPU baseline leg")
    ap.add_argument("--clock-ramp", type=float, default=0.5, help="seconds of untimed lr=0 steps before the warmup steps")
    ap.add_argument("--detail", default=os.path.join(ROOT, "gpurun_out", "bench_detail.json"),
                    help="where the FULL result object goes (every leg with its parity records, curves and tables); the LAST "
                         "stdout line is the compact summary of it (< %d bytes)" % LINE_LIMIT)
    return ap.parse_args(argv)


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N copies of this command, one rank per GPU, with the
    environment torch.distributed.run would have set; rank 0 prints the JSON line."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    # poll all ranks: a rank that dies before the rendezvous would leave the others waiting for it forever
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs):
            # a rank failed: give the survivors a moment to report, then end exactly the processes started here --
            # terminate ONCE, wait, and kill whatever ignored it (no loop: a survivor stuck in a collective never exits)
            deadline = time.time() + 5.0
            while time.time() < deadline and any(p.poll() is None for p in procs):
                time.sleep(0.1)
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10.0)
                except subprocess.TimeoutExpired:
                    p.kill()
            break
        time.sleep(0.2)
    return max(abs(p.wait()) for p in procs)


def clock_ramp(run_group, nominal_s, world=1, dist=None):
    """Run groups of untimed steps until two groups in a row (not counting the first, which has nothing to be compared
    with) took within 1.5 % of the fastest group seen and at least `nominal_s` have passed, or 6 x `nominal_s` at the
    latest.  Returns the number of groups.  With more than one rank every step carries an all-reduce, so the ranks must
    leave after the SAME number of groups: they decide on the same numbers (the slowest rank's group time, the longest
    elapsed time), agreed through `dist`."""
    t_ramp = time.perf_counter()
    best, settled, groups = float("inf"), 0, 0
    while True:
        t_g = time.perf_counter()
        run_group()
        now = time.perf_counter()
        g, elapsed = now - t_g, now - t_ramp
        if world > 1:
            import torch

            t = torch.tensor([g, elapsed], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            g, elapsed = float(t[0].item()), float(t[1].item())
        groups += 1
        if best < float("inf"):
            settled = settled + 1 if g <= 1.015 * best else 0
        best = min(best, g)
        if (elapsed >= nominal_s and settled >= 2) or elapsed >= 6.0 * nominal_s:
            return groups


def split_vanilla(n, k):
    """SplitStrategy.vanilla (core/ml/SplitStrategy.scala:13-14): indices.grouped(ceil(n / k)) -- contiguous ranges, the
    last may be shorter, fewer than k groups are possible."""
    size = -(-n // k)
    return [(b, min(n, b + size)) for b in range(0, n, size)]


def concat_csr(parts):
    from dsgd_amd.synth import Csr

    row_ptr = [np.zeros(1, dtype=np.int64)]
    off = 0
    for p in parts:
        row_ptr.append(p.row_ptr[1:] + off)
        off += p.nnz
    return Csr(parts[0].dim, np.concatenate(row_ptr), np.concatenate([p.col for p in parts]),
               np.concatenate([p.val for p in parts]), np.concatenate([p.label for p in parts]))


def load_shard(dsgd_amd, args, rank, world):
    """This rank's rows: (CSR = its train rows followed by its test rows, train rows, global index of its first train row,
    train rows of the whole job).  Weak: rows [rank * R, (rank + 1) * R) of the synthetic stream, 80/20 (Main.scala:52).
    Strong: ONE data set of --rows-total rows, 80/20, its train part split over the ranks by SplitStrategy.vanilla
    (core/Master.scala:136), its test part likewise (evaluation shards the same way)."""
    if args.scaling == "weak":
        data = dsgd_amd.synth.generate(args.rows, seed=args.seed, row0=rank * args.rows)
        n_train = int(args.rows * 0.8)
        return data, n_train, rank * args.rows, n_train * world
    n_tot = args.rows_total
    n_train_tot = int(n_tot * 0.8)
    tr, te = split_vanilla(n_train_tot, world), split_vanilla(n_tot - n_train_tot, world)
    if len(tr) != world or len(te) != world:
        raise SystemExit("--rows-total %d splits into %d train / %d test groups for %d ranks (SplitStrategy.vanilla yields fewer "
                         "groups than workers: the reference's zip would silently drop ranks)" % (n_tot, len(tr), len(te), world))
    lo, hi = tr[rank]
    tlo, thi = te[rank]
    parts = [dsgd_amd.synth.generate(hi - lo, seed=args.seed, row0=lo),
             dsgd_amd.synth.generate(thi - tlo, seed=args.seed, row0=n_train_tot + tlo)]
    return concat_csr(parts), hi - lo, lo, n_train_tot


def check_step(o, orb, w_engine, w_before, w_ref, tol, n_near, act_engine, act_oracle, what):
    """The two statements every gated step is held to: the DERIVED per-coordinate bound (oracle/bounds.py) and the STATED
    tolerance of BASELINE.md, 1e-5 * max(1, |w_oracle|_inf).  Returns the record; raises SystemExit on a violation."""
    ratio, j = orb.worst_ratio(w_engine, w_ref, tol)
    err = float(np.abs(np.asarray(w_engine, dtype=np.float64) - w_ref).max())
    rel = err / max(1.0, float(np.abs(w_ref).max()))
    rec = {"n_active_engine": int(act_engine), "n_active_oracle": int(act_oracle), "rows_near_gate": int(n_near),
           "max_abs_err": err, "max_rel_err": rel, "stated_tolerance": STATED_TOL, "worst_err_over_bound": ratio,
           "worst_coordinate": j}
    if not ratio <= 1.0:
        raise SystemExit("parity failed (%s): coordinate %d is %.3g x its derived bound (max rel err %.3e)" % (what, j, ratio, rel))
    if not rel <= STATED_TOL:
        raise SystemExit("parity failed (%s): max|w - w_oracle| = %.3e exceeds the stated tolerance %.0e * max(1, |w|_inf)"
                         % (what, err, STATED_TOL))
    if abs(act_engine - act_oracle) > n_near:
        raise SystemExit("parity failed (%s): active rows %d vs oracle %d with only %d rows near the gate"
                         % (what, act_engine, act_oracle, n_near))
    return rec


def parity_gate_single(eng, data, n_train, ranges, lr):
    """N = 1: two steps of the TIMED configuration (the same whole-shard step, the same ranges, every row) against the
    fp64 oracle (OpenMP restatement on the host cores), each from identical weights."""
    from oracle import bounds as orb  # checker only
    from oracle import oracle as orc

    t_gate = time.time()
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAMBDA)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    parity = {"rows": n_train, "ranges": len(ranges), "world": 1, "steps": []}
    for _ in range(2):
        w0 = eng.get_weights()
        w_ref = w0.astype(np.float64)
        st = eng.sync_step_ranges(ranges, lr)
        shift = eng.tuning_info()["fix_shift"]
        w_before = w_ref.copy()
        if len(ranges) == 1:
            act_ref = o.sync_step_range_omp(w_ref, 0, n_train, lr)
        else:
            o.sync_step(w_ref, [np.arange(a, b, dtype=np.int32) for a, b in ranges], lr)
            act_ref = o.last_stats["n_active"]
        tol, n_near = orb.step_bound(o, w_before, w_ref, ranges, lr, shift)
        rec = check_step(o, orb, eng.get_weights(), w_before, w_ref, tol, n_near, st["n_active"], act_ref,
                         "whole-shard step of the benchmarked configuration")
        rec["fix_shift"] = shift
        parity["steps"].append(rec)
    parity["seconds"] = round(time.time() - t_gate, 1)
    return parity


def parity_gate_multi(dsgd_amd, eng, data, n_train, train_row0, k, args, rank, world, dist):
    """N > 1: replica bit-identity alone would pass a wrong-but-identical update.  Every rank runs two synchronous steps
    over the first n_gate rows of its train shard (k hosted workers each, the all-reduce inside), rank 0 regenerates
    those rows of EVERY rank (the synthetic stream is indexed by global row), hosts them in one oracle as world x k
    workers -- Master.scala:194's mean runs over the workers -- with dimSparsity from the feature counts summed over
    the ranks' WHOLE train shards (Main.scala:57-60 counts the whole train set), and checks the update under the derived
    bound (the coarsest shift any rank used) and the stated tolerance."""
    import torch

    t_gate = time.time()
    t = torch.tensor([n_train], dtype=torch.int64)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    n_gate = int(min(args.gate_rows, t.item()))
    ranges = split_vanilla(n_gate, k)
    lr = LR0 * 100.0 / (n_gate / float(k))
    # feature counts of this rank's train rows (entries the Sparse constructor keeps: math/Sparse.scala:108-118), summed
    b, e = 0, int(data.row_ptr[n_train])
    keep = np.abs(data.val[b:e]) > 1e-20
    cnt = torch.from_numpy(np.bincount(data.col[b:e][keep], minlength=data.dim + 1).astype(np.int64))
    dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
    row0s = [None] * world
    dist.all_gather_object(row0s, int(train_row0))
    o = None
    if rank == 0:
        from oracle import bounds as orb  # checker only
        from oracle import oracle as orc

        gate = concat_csr([dsgd_amd.synth.generate(n_gate, seed=args.seed, row0=r0) for r0 in row0s])
        o = orc.Oracle(gate.dim, gate.row_ptr, gate.col, gate.val, gate.label, LAMBDA)
        c = cnt.numpy().astype(np.float64)
        ds = np.zeros(gate.dim + 1)
        ds[:gate.dim] = np.where(c[1:] != 0, 1.0 / (c[1:] + 1.0), 0.0)     # Main.scala:60-62: key i carries feature i + 1
        o.set_dim_sparsity(ds)
        g_ranges = [(r * n_gate + a, r * n_gate + bb) for r in range(world) for a, bb in ranges]   # rank order = all-reduce order
    parity = {"rows_per_rank": n_gate, "ranges": len(ranges) * world, "world": world, "workers_total": k * world, "steps": []}
    for _ in range(2):
        w0 = eng.get_weights()
        st = eng.sync_step_ranges(ranges, lr)
        s_min = torch.tensor([eng.tuning_info()["fix_shift"]], dtype=torch.int64)   # the coarsest grid any rank used
        dist.all_reduce(s_min, op=dist.ReduceOp.MIN)
        act = torch.tensor([st["n_active"]], dtype=torch.int64)
        dist.all_reduce(act, op=dist.ReduceOp.SUM)
        if rank == 0:
            w_before = w0.astype(np.float64)
            w_ref = w_before.copy()
            o.sync_step(w_ref, [np.arange(a, bb, dtype=np.int32) for a, bb in g_ranges], lr)
            shift = int(s_min[0].item())
            tol, n_near = orb.step_bound(o, w_before, w_ref, g_ranges, lr, shift)
            rec = check_step(o, orb, eng.get_weights(), w_before, w_ref, tol, n_near, int(act.item()), o.last_stats["n_active"],
                             "N = %d step over %d rows per rank, %d workers" % (world, n_gate, k * world))
            rec["fix_shift_min_over_ranks"] = shift
            parity["steps"].append(rec)
    parity["replicas_bit_identical_after_gate"] = replicas_identical(eng, dist)
    if not parity["replicas_bit_identical_after_gate"]:
        raise SystemExit("rank %d: weight replicas diverged in the parity gate" % rank)
    parity["seconds"] = round(time.time() - t_gate, 1)
    return parity


def replicas_identical(eng, dist):
    """every rank applied the same all-reduced gradient to the same weights: the replicas must agree BIT FOR BIT
    (SURVEY.md 8(e)); compared through a 56-bit digest of the fp32 words"""
    import hashlib

    import torch

    digest = int.from_bytes(hashlib.sha256(eng.get_weights().tobytes()).digest()[:7], "little")
    dmin = torch.tensor([digest], dtype=torch.int64)
    dmax = torch.tensor([digest], dtype=torch.int64)
    dist.all_reduce(dmin, op=dist.ReduceOp.MIN)
    dist.all_reduce(dmax, op=dist.ReduceOp.MAX)
    return bool(dmin.item() == dmax.item())


def timed_steps(eng, ranges, lr, steps, repeats, sync_all, barrier, world, dist):
    """`repeats` measurements of EXACTLY `steps` steps, each bracketed by barrier + synchronize on both sides, MAX over
    ranks.  (A 20-step window is 14 ms: less than the box-to-box and run-to-run spread it is meant to resolve -- the
    line reports the median with min / max.)"""
    out = []
    for _ in range(repeats):
        barrier()
        sync_all(eng)
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.sync_step_ranges(ranges, lr, asynchronous=True)
        sync_all(eng)
        barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            import torch

            t = torch.tensor([dt], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        out.append(dt)
    return out


def dump_outputs(path, eng):
    """--dump-outputs: what the last timed step computed -- the weight vector (D + 1 floats, 189 KB) a caller of the
    step reads back -- so that two builds run with the same arguments can be compared output for output."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "weights.npy"), np.asarray(eng.get_weights(), dtype=np.float32))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # (tests only: several ranks on ONE device through the tests' seam build of the library, tests/test_gpu_world2.py)
    device = 0 if os.environ.get("DSGD_BENCH_ONE_DEVICE") == "1" else local_rank

    # torch is plumbing only: rendezvous, barrier, the max-over-ranks reduction, cuda.synchronize
    import torch  # imported BEFORE libdsgd_hip so the process holds exactly one HIP runtime
    import torch.distributed as dist

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ["MASTER_ADDR"] in ("127.0.0.1", "localhost"):
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")   # one node: no need to resolve the container's hostname
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    if torch.cuda.is_available():
        torch.cuda.set_device(device)

    import dsgd_amd

    if dsgd_amd.device_count() <= device:
        raise SystemExit("rank %d: no gfx950 device %d visible (%d found): libdsgd_hip has no CPU fallback"
                         % (rank, device, dsgd_amd.device_count()))

    def barrier():
        if world > 1:
            dist.barrier()

    def sync_all(eng):
        eng.synchronize()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    t_gen = time.time()
    data, n_train, train_row0, n_train_job = load_shard(dsgd_amd, args, rank, world)
    t_gen = time.time() - t_gen
    nnz_train = int(data.row_ptr[n_train])
    bytes_per_row = (8.0 * nnz_train + 12.0 * n_train) / n_train

    eng = dsgd_amd.Engine(data.dim, LAMBDA, device=device)
    t_up = time.time()
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    t_up = time.time() - t_up
    t_setup_coll = time.time()
    if world > 1:
        uid = [dsgd_amd.Engine.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        eng.comm_init(uid[0], world, rank)
    eng.build_dim_sparsity(n_train)   # (layout + with N > 1 the all-reduce of the column and feature counts: setup, reported)
    t_setup_coll = time.time() - t_setup_coll

    k = args.workers
    # the reference SUMS the gated sub-gradients of a batch (core/Slave.scala:153), so its step length
    # scales with batch-size; keep the per-sample step of the defaults (0.5 per 100 samples).  A worker's batch: its
    # share of this rank's train rows (weak) / of the whole train set (strong: ceil(N_train / (k * world)))
    batch_per_worker = (n_train / float(k)) if args.scaling == "weak" else -(-n_train_job // (k * world))
    LR = LR0 * 100.0 / batch_per_worker
    ranges = split_vanilla(n_train, k)

    # ---- parity gate (before any timing is reported) ------------------------------------------------------------
    parity = None
    if args.full and not args.no_parity_gate:
        if world == 1:
            parity = parity_gate_single(eng, data, n_train, ranges, LR)
        else:
            parity = parity_gate_multi(dsgd_amd, eng, data, n_train, train_row0, k, args, rank, world, dist)
    eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))

    # ---- clock ramp (setup, not warmup): the parity gate and the layout leave the GPU idle for seconds while the host
    # works; the first milliseconds afterwards run at idle clocks (measured: 2.9 ms per step straight after the gate vs
    # 0.84 ms once the clocks are up -- 3 warmup steps are 3 ms, far less than the ramp).  Steps with lr = 0 (weights
    # unchanged) for a fixed wall time bring the clocks up; the W warmup steps and the K timed steps follow unchanged.
    def ramp_group():
        for _ in range(8):
            eng.sync_step_ranges(ranges, 0.0, asynchronous=True)
        sync_all(eng)

    t_ramp = time.perf_counter()
    clock_ramp(ramp_group, args.clock_ramp, world, dist if world > 1 else None)
    ramp_s = time.perf_counter() - t_ramp
    eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))

    # ---- timed region ------------------------------------------------------------------------------
    for _ in range(args.warmup):
        eng.sync_step_ranges(ranges, LR, asynchronous=True)
    sync_all(eng)
    repeats = max(1, args.repeats if args.repeats is not None else (5 if args.full else 1))
    if args.full:
        eng.prof_enable(2)   # HIP events around the DOMINANT kernel only: two event records per step inside the clock
        eng.prof_read(reset=True)
    times = timed_steps(eng, ranges, LR, args.steps, repeats, sync_all, barrier, world, dist)
    dt = float(np.median(times))
    if args.full:
        kernel_ms, n_launch = eng.prof_read(reset=True)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng)   # the state the LAST timed step left, before anything else runs

    identical = None
    if args.full:
        # (outside the clock) the two cold-stream kernels, bracketed the same way over a few more steps
        eng.prof_enable(1)
        for _ in range(5):
            eng.sync_step_ranges(ranges, LR, asynchronous=True)
        sync_all(eng)
        kinds = eng.prof_read_kinds()
        eng.prof_read(reset=True)
        eng.prof_enable(0)
        last = eng.sync_step_ranges(ranges, 0.0)   # (outside the clock) gate statistics of the state the timed steps ended in

        loss, acc, _ = eng.loss_acc(n_train, data.n_rows)
        if world > 1:
            identical = replicas_identical(eng, dist)
            if not identical:
                raise SystemExit("rank %d: weight replicas diverged after the timed steps" % rank)
    value = n_train_job * args.steps / dt if args.scaling == "strong" else world * n_train * args.steps / dt

    if args.scaling == "weak":
        workload = ("rcv1-synth sync SGD: %d rows/GPU (D=47236, nnz/row=%.1f), 80/20 split, whole-shard batch B=%d rows/GPU/step, "
                    "%d worker(s)/GPU, lr=0.5*100/B=%.3g, lambda=%g" % (args.rows, data.nnz / data.n_rows, n_train, k, LR, LAMBDA))
    else:
        workload = ("rcv1-synth sync SGD: ONE data set of %d rows (D=47236, nnz/row=%.1f), 80/20 split, its %d train rows "
                    "split over %d GPU(s) x %d worker(s) by SplitStrategy.vanilla, whole-split batch B=%d rows/worker/step, "
                    "lr=0.5*100/B=%.3g, lambda=%g" % (args.rows_total, data.nnz / data.n_rows, n_train_job, world, k,
                                                      int(batch_per_worker), LR, LAMBDA))
    out = {
        "metric": "RCV1 examples/sec (sync SGD, sparse hinge-SVM gradient step)",
        "value": value,
        "unit": "examples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": workload,
            "rows_per_gpu": data.n_rows,
            "train_rows_per_gpu": n_train,
            "train_rows_job": n_train_job,
            "workers_per_gpu": k,
            "parallelism": "dp%d (row-partitioned, RCCL all-reduce of the %d-float gradient)" % (world, data.dim + 1),
            "seed": args.seed,
        },
        "repeats": {"n": len(times), "statistic": "median", "ms_per_step": [1e3 * t / args.steps for t in times],
                    "ms_per_step_min": 1e3 * min(times) / args.steps, "ms_per_step_max": 1e3 * max(times) / args.steps},
        "setup_s": {"generate": round(t_gen, 2), "upload": round(t_up, 2), "clock_ramp": round(ramp_s, 2),
                    "communicator_layout_dim_sparsity": round(t_setup_coll, 2)},
    }
    if args.full:
        out.update({"active_fraction_after": last["n_active"] / max(1, last["n_samples"]), "test_loss_after": loss,
                    "test_acc_after": acc})
    if identical is not None:
        out["replicas_bit_identical"] = identical
    if parity is not None:
        out["parity_gate_rows"] = parity.get("rows", parity.get("rows_per_rank"))
        if rank == 0:
            out["parity_gate_max_rel_err"] = max(p["max_rel_err"] for p in parity["steps"])
        out["parity_gate"] = parity
    out["config"].update({"tuning": eng.tuning_info(),
                          "env_overrides": {kk: v for kk, v in os.environ.items() if kk.startswith("DSGD_")}})

    # ---- roofline of the dominant kernel (the gradient kernel) ---------------------------------------
    # Algorithmic bytes: 8 B per non-zero + 12 B per row.  In the split layout the cold entries are
    # read by the two cold-stream kernels, so the main kernel is credited with the hot entries and the per-row bytes only.
    if args.full:
        out["roofline"] = roofline(eng, args.rows if args.scaling == "weak" else None, n_train, nnz_train, bytes_per_row,
                                   kernel_ms, n_launch, args.steps * len(times), dt / args.steps, kinds)

    # ---- the other shapes and configurations, reported beside the headline (N = 1 only) ----------------------------
    extras = args.full and rank == 0 and world == 1 and not args.no_sweep
    gated = not args.no_parity_gate
    if extras:
        out["sweep"] = sweep(eng, data, n_train, with_parity=gated)
        out["eval_pass"] = eval_pass(eng, n_train, bytes_per_row)
        out["hogwild"] = hogwild(eng, n_train, bytes_per_row)
    eng.close()
    if extras:
        if gated:
            out["hogwild"].update(hogwild_parity(dsgd_amd, device))
        out["reference_shapes"] = [reference_shape(dsgd_amd, device, n, with_parity=gated, repeats=repeats)
                                   for n in (804414, 23149, 100552)]   # DatasetTests.scala:18 (full = true), application.conf:24 (full
        # = false), and what ONE GPU of eight holds of the former (SplitStrategy.scala:13-14: ceil(804414 / 8) rows; 80,441 of
        # them train) -- the per-GPU step of an 8-GPU strong-scaled run, to which a 189 KB all-reduce is added there
        if gated:
            out["time_to_target"] = time_to_target(dsgd_amd, device)
        out["dense_logistic"] = dense_logistic(dsgd_amd, device)

    # ---- CPU baseline on this box's host cores (rank 0, N=1 only) --------------------------------------
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"], out["cpu_literal"] = cpu_baseline(data, n_train, args.cpu_seconds)
        # second half of BASELINE.json's metric ("epochs to target hinge loss"); the target is defined by the oracle, so
        # it is computed in this leg and shown at the top level as well
        out["cpu_baseline"]["epochs_to_target"] = epochs_to_target(dsgd_amd, device)
        e = out["cpu_baseline"]["epochs_to_target"]
        out["epochs_to_target"] = {kk: e[kk] for kk in ("config", "target_test_loss", "engine_epochs", "oracle_epochs", "max_epochs")}
        out["fit"] = e.pop("fit")

    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(out, args.detail)


def _sig(x, digits=6):
    """numbers of the compact line: `digits` significant digits (the detail file keeps every bit)"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return float("%.*g" % (digits, x)) if np.isfinite(x) else None
    if isinstance(x, dict):
        return {k: _sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, digits) for v in x]
    return x


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(out, detail_path=None):
    """The line of record: the driver's contract keys, `roofline` and `cpu_baseline` (numbers only, no prose), the parity
    gate's worst error, epochs to target, and ONE summary row per extra leg.  Everything else -- per-step parity records,
    sweep tables per shape, Hogwild checkpoints, loss curves, band tables -- lives in the detail file.  Returns the dict;
    `emit` serialises it and refuses a line of LINE_LIMIT bytes or more (optional legs are dropped first, the contract
    keys never)."""
    c = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data") if k in out}
    c["config"] = _pick(out.get("config", {}), "workload", "rows_per_gpu", "train_rows_per_gpu", "train_rows_job", "workers_per_gpu",
                        "parallelism", "seed")
    if "repeats" in out:
        c["repeats"] = _pick(out["repeats"], "n", "statistic", "ms_per_step_min", "ms_per_step_max")
    r = out.get("roofline")
    if r:
        c["roofline"] = _pick(r, "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "physical_frac",
                              "algorithmic_bytes_per_launch", "kernel_ms_avg", "kernel_launches", "kernel_share_of_nonzeros")
        if "step" in r:
            c["roofline"]["step"] = _pick(r["step"], "ms", "frac")
        if "other_kernels" in r:
            c["roofline"]["other_kernels_ms"] = {k: v["ms_avg"] for k, v in r["other_kernels"].items()}
    for key in ("cpu_baseline", "cpu_literal"):
        if key in out:
            c[key] = _pick(out[key], "value", "unit", "cores", "kind")
            c[key]["sample"] = str(out[key].get("sample", ""))[:160]
    for key in ("parity_gate_rows", "parity_gate_max_rel_err", "replicas_bit_identical", "test_loss_after", "test_acc_after"):
        if key in out:
            c[key] = out[key]
    if "parity_gate" in out and out["parity_gate"].get("steps"):
        c["parity_gate_worst_err_over_bound"] = max(p["worst_err_over_bound"] for p in out["parity_gate"]["steps"])
    if "epochs_to_target" in out:
        c["epochs_to_target"] = _pick(out["epochs_to_target"], "engine_epochs", "oracle_epochs", "target_test_loss", "max_epochs")
    legs = {}
    for s in out.get("sweep", []):
        row = _pick(s, "us_per_step", "frac_hbm_peak", "kernel")
        if "parity" in s:
            row["parity_max_rel_err"] = s["parity"]["max_rel_err"]
        legs.setdefault("sweep", {})["%dx%d" % (s["workers"], s["batch"])] = row
    for rs in out.get("reference_shapes", []):
        row = {"us_per_step": rs["whole_shard"]["us_per_step"], "kernel_frac": rs["roofline"]["frac"],
               "step_frac": rs["roofline"]["step"]["frac"], "kernel": rs["whole_shard"]["kernel"]}
        if "parity_gate" in rs:
            row["parity_max_rel_err"] = rs["parity_gate"]["max_rel_err"]
        by = {(s["workers"], s["batch"]): s for s in rs.get("sweep", [])}
        if (3, 100) in by:
            row["3x100_us_per_step"] = by[(3, 100)]["us_per_step"]
        legs.setdefault("reference_shapes", {})["N=%d" % rs["rows"]] = row
    for key in ("fit", "per_request"):
        if key in out:
            legs[key] = out[key].get("summary", out[key])
    hw = out.get("hogwild")
    if hw:
        legs["hogwild"] = _pick(hw, "workers", "batch", "examples_per_s", "frac_hbm_peak", "atomics_per_s")
        tr = hw.get("traced_replay")
        if tr:
            legs["hogwild"]["traced_replay"] = _pick(tr, "accounting_agrees", "gates_are", "controls_rejected", "gate_check", "gate_check_4_workers")
    tt = out.get("time_to_target")
    if tt:
        legs["time_to_target"] = _pick(tt, "rows", "target_test_loss", "fastest", "through")
        c0 = tt["configs"][0] if tt.get("configs") else None
        if c0:
            legs["time_to_target"]["reference_config"] = _pick(c0, "workers", "batch", "time_to_target_s", "engine_epochs", "oracle_epochs",
                                                               "first_divergent_step", "divergent_rows_all_near_gate",
                                                               "forced_replay_account_err_over_tol", "epoch1_max_abs_diff")
    if "eval_pass" in out:
        legs["eval_pass"] = _pick(out["eval_pass"], "examples_per_s", "frac_hbm_peak")
    dl = out.get("dense_logistic")
    if dl and dl.get("batches"):
        legs["dense_logistic"] = {str(b["batch"]): _pick(b, "examples_per_s", "kernel_frac_hbm_peak") for b in dl["batches"]}
        if "mfma_variant" in dl:
            legs["dense_logistic"]["mfma_65536"] = _pick(dl["mfma_variant"], "examples_per_s", "kernel_frac_hbm_peak")
    if legs:
        c["legs"] = legs
    if detail_path:
        c["detail"] = os.path.relpath(detail_path, ROOT) if os.path.isabs(detail_path) else detail_path
    return _sig(c)


def emit(out, detail_path, stream=None):
    """Write the full object to `detail_path`, then print the compact line as the LAST stdout line.  A consumer that keeps
    only a tail of the output (the driver: 8 KB) must still get the headline: the line is held below LINE_LIMIT by
    dropping optional legs (largest first) -- never a contract key -- and the run fails rather than print a longer one."""
    stream = stream or sys.stdout
    if detail_path:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(detail_path)), exist_ok=True)
            with open(detail_path, "w") as f:
                json.dump(out, f)
        except OSError as e:
            print("bench.py: could not write %s: %s" % (detail_path, e), file=sys.stderr)
            detail_path = None
    c = compact_line(out, detail_path)
    line = json.dumps(c, separators=(",", ":"))
    while len(line) >= LINE_LIMIT - 1024 and c.get("legs"):
        biggest = max(c["legs"], key=lambda k: len(json.dumps(c["legs"][k])))
        del c["legs"][biggest]
        c.setdefault("legs_dropped_from_line", []).append(biggest)
        line = json.dumps(c, separators=(",", ":"))
    if len(line) >= LINE_LIMIT:
        raise SystemExit("bench.py: the final line is %d bytes (limit %d)" % (len(line), LINE_LIMIT))
    stream.flush()
    print(line, file=stream, flush=True)
    return line


def roofline(eng, rows_key, n_train, nnz_train, bytes_per_row, kernel_ms, n_launch, n_steps, step_s, kinds):
    """The `roofline` object of a whole-shard configuration: the dominant kernel's algorithmic bytes per launch / its
    average duration from HIP events on the library's stream, the whole step against the same peak, the cold kernels."""
    launches_per_step = n_launch / max(1, n_steps)
    nnz_int, cold_int = eng.range_nnz(0, n_train)
    # the chunked launch (csrc/dsgd_fstep.hpp) walks BOTH streams: every non-zero of the step is its own; the three
    # streaming launches split them -- the dominant one (dsgd_wseg_kernel) reads the hot part
    # (the column lists, csrc/dsgd_tcol.hpp, likewise: their dot + gradient launches are bracketed together)
    one_launch = eng.grad_kernel_name() in ("dsgd_fstep_kernel", "dsgd_tc_grad_kernel")
    own_nnz = nnz_train if one_launch else nnz_train - cold_int
    alg_bytes = (8.0 * own_nnz + 12.0 * n_train) / max(1.0, launches_per_step)  # per launch
    achieved = alg_bytes / (kernel_ms * 1e-3) if kernel_ms > 0 else 0.0
    # HBM traffic of the dominant kernel comes from a SEPARATE rocprofv3 --pmc pass (tools/pmc_pass.sh: FETCH_SIZE,
    # x2 gfx950 correction) recorded in profiles/traffic.json -- it cannot be collected inside this run
    traffic, traffic_source = None, None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if rows_key is not None and os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            traffic = tj.get(str(rows_key))
            if isinstance(traffic, dict):   # by dominant kernel: the chunked launch and the three streaming launches differ
                traffic = traffic.get(eng.grad_kernel_name())
            traffic_source = tj.get("source", "profiles/traffic.json (committed rocprofv3 --pmc FETCH_SIZE pass)")
        except Exception:
            traffic = None
    r = {
        "bound": "hbm",
        "kernel": eng.grad_kernel_name(),
        "achieved": achieved / 1e9,
        "peak": HBM_PEAK / 1e9,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK,
        "frac_of_measured_copy_peak": achieved / HBM_MEASURED,
        "traffic": traffic,
        "traffic_source": traffic_source,
        # the PHYSICAL fraction: HBM bytes the kernel really moved (rocprofv3 FETCH_SIZE pass) / its duration / peak --
        # below the algorithmic one because 16-bit column ranks make the stream smaller than 8 B per non-zero
        "physical_frac": (traffic / (kernel_ms * 1e-3) / HBM_PEAK) if (traffic and kernel_ms > 0) else None,
        "physical_frac_of_measured_copy_peak": (traffic / (kernel_ms * 1e-3) / HBM_MEASURED) if (traffic and kernel_ms > 0) else None,
        "algorithmic_bytes_per_launch": alg_bytes,
        "algorithmic_bytes_per_example": bytes_per_row,
        "kernel_ms_avg": kernel_ms,
        "kernel_launches": n_launch,
        "kernel_share_of_nonzeros": own_nnz / max(1, nnz_train),
        # the whole step (all kernels, launch gaps included) against the same roofline
        "step": {"algorithmic_bytes": bytes_per_row * n_train, "ms": 1e3 * step_s,
                 "achieved": bytes_per_row * n_train / step_s / 1e9, "frac": bytes_per_row * n_train / step_s / HBM_PEAK},
    }
    if kinds is not None:
        r["other_kernels"] = {
            name: {"ms_avg": kinds[name][0], "launches": kinds[name][1],
                   "algorithmic_bytes_per_launch": 8.0 * cold_int / max(1.0, kinds[name][1] / 5.0),
                   "achieved": (8.0 * cold_int / max(1.0, kinds[name][1] / 5.0)) / (kinds[name][0] * 1e-3) / 1e9,
                   "measured": "5 untimed steps after the timed region"}
            for name in ("cdot", "cgrad") if kinds[name][1] > 0
        }
    return r


SWEEP = ((1, 100, 300), (3, 100, 300), (4, 200, 200), (1, 200, 200), (1, 4096, 100), (1, 65536, 20))


def sweep(eng, data, n_train, with_parity=True, configs=SWEEP, o=None):
    """examples/s for index-list batches from resident plans: the reference's real defaults (3 workers x batch 100,
    application.conf:15,27; 4 x 200, kube/config-sync.yaml) and SURVEY.md 8(d)'s sweep B in {100, 200, 4096, 65536}.
    Every row carries `parity`: step 0 OF THE TIMED PLAN -- the same kernel, the same packed layout, the same fixed-point
    shift as the timed steps -- from non-zero weights against the fp64 oracle under the derived per-coordinate bound of
    oracle/bounds.py AND the stated 1e-5 tolerance (outside the timed loop; the oracle is the checker, never the thing
    timed); the run fails if the kernel that was checked is not the kernel that was timed."""
    res = []
    rng = np.random.default_rng(123)
    w_nz = None
    if with_parity:
        from oracle import bounds as orb  # checker only
        from oracle import oracle as orc

        if o is None:
            o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAMBDA)
            o.set_dim_sparsity(o.dim_sparsity(n_train))
        w_nz = np.zeros(eng.dp, dtype=np.float32)
        hot = rng.choice(np.arange(1, data.dim + 1), size=6000, replace=False)
        w_nz[hot] = rng.normal(scale=0.05, size=6000).astype(np.float32)
    for k, b, steps in configs:
        if k * b > n_train:
            continue
        split = split_vanilla(n_train, k)
        lists = [[(lo + rng.permutation(hi - lo)[:b]).astype(np.int32) for lo, hi in split] for _ in range(steps)]
        lr = LR0 * 100.0 / b   # the reference sums the batch (core/Slave.scala:153): keep the per-sample step of the defaults
        entry = {"workers": k, "batch": b, "steps": steps}
        plan = eng.plan(lists)
        if with_parity:
            eng.set_weights(w_nz)
            eng.synchronize()                      # (counters of whatever ran before are collected and cleared)
            w0 = w_nz.astype(np.float64)
            w_ref = w0.copy()
            eng.plan_run(plan, 0, 1, lr)           # step 0 of the plan that is timed below
            st = eng.synchronize()
            kern = eng.grad_kernel_name()
            # (one hosted worker with lists of up to 192 rows runs the persistent one-workgroup kernel, which derives
            # its fixed-point shift per batch: 30 - ceil(log2 B); everything else reports the shift of its launch)
            shift = 30 - int(np.ceil(np.log2(b))) if "plan_kernel" in kern else eng.tuning_info()["fix_shift"]
            o.sync_step(w_ref, lists[0], lr)
            tol, n_near = orb.list_bound(o, w0, w_ref, lists[0], lr, shift)
            rec = check_step(o, orb, eng.get_weights(), w0, w_ref, tol, n_near, st["n_active"], o.last_stats["n_active"],
                             "sweep %d x %d" % (k, b))
            rec.update(fix_shift=shift, kernel=kern, checked="step 0 of the timed plan")
            entry["parity"] = rec
        eng.set_weights(np.zeros(eng.dp, dtype=np.float32))
        eng.plan_run(plan, 0, min(10, steps), lr)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.plan_run(plan, 0, steps, lr)
        eng.synchronize()
        dt = time.perf_counter() - t0
        plan.destroy()
        nnz = float(np.mean([sum(int((data.row_ptr[l + 1] - data.row_ptr[l]).sum()) for l in st_) for st_ in lists[:8]]))
        alg = 8.0 * nnz + 12.0 * k * b
        entry.update({"examples_per_s": k * b * steps / dt, "us_per_step": 1e6 * dt / steps, "kernel": eng.grad_kernel_name(),
                      "algorithmic_bytes_per_step": alg, "frac_hbm_peak": alg * steps / dt / HBM_PEAK})
        if with_parity and entry["parity"]["kernel"] != entry["kernel"]:
            raise SystemExit("sweep %d x %d: parity was checked on %s but %s was timed" % (k, b, entry["parity"]["kernel"], entry["kernel"]))
        res.append(entry)
    return res


def eval_pass(eng, n_train, bytes_per_row):
    """Master.localLoss/localAccuracy over the train rows (core/Master.scala:100-107): examples/s of one pass."""
    eng.loss_acc(0, n_train)
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        eng.loss_acc(0, n_train)
    dt = (time.perf_counter() - t0) / reps
    return {"rows": n_train, "examples_per_s": n_train / dt, "ms": 1e3 * dt,
            "frac_hbm_peak": n_train / dt * bytes_per_row / HBM_PEAK, "note": "wall time incl. launch + readback"}


def hogwild(eng, n_train, bytes_per_row, workers=256, batch=100, updates=60000):
    """BASELINE.json configs[3]: asynchronous mode, one workgroup per worker, lock-free atomicAdd into ONE
    device-resident w (core/Slave.scala:79-111); reference defaults batch-size 100, learning-rate 0.5."""
    eng.set_weights(np.zeros(eng.dp, dtype=np.float32))
    split = split_vanilla(n_train, workers)
    # a short untimed run first (clocks, first touch of the engine's buffers), then the timed one from w = 0;
    # wall time from async_start to the end of async_wait, i.e. launch and join included
    eng.async_start(split, batch=batch, lr=LR0, max_updates=updates // 4, seed=7, positional_bug=False)
    eng.async_wait()
    eng.set_weights(np.zeros(eng.dp, dtype=np.float32))
    t0 = time.perf_counter()
    eng.async_start(split, batch=batch, lr=LR0, max_updates=updates, seed=1, positional_bug=False)
    eng.async_wait()
    dt = time.perf_counter() - t0
    st = eng.async_stats()
    u = st["updates"]
    loss, acc, _ = eng.loss_acc(n_train, eng.n_rows)
    return {"workers": len(split), "batch": batch, "updates": int(u), "examples_per_s": u * batch / dt,
            "updates_per_s": u / dt, "ms": 1e3 * dt, "test_loss_after": loss, "test_acc_after": acc,
            # the same algorithmic bytes per example as the synchronous step ("Hogwild (K7): same stream
            # bytes; additionally report atomics/s") against the HBM peak: this mode is bound by device-scope atomics
            "frac_hbm_peak": u * batch / dt * bytes_per_row / HBM_PEAK,
            # lane-level atomicAdd(w[j], -delta_j) counted on the device (the coordinates the updates
            # really moved); the memory system sees them coalesced per 128-byte line: profiles/ (TCP_TCC_ATOMIC_*)
            "atomics_per_s": st["atomics"] / dt, "atomics_per_update": st["atomics"] / max(1, u),
            "active_fraction": st["active"] / max(1, st["samples"]),
            "note": "one lock-free workgroup per worker on ONE device-resident w; wall time incl. launch and join; a single "
                    "end-of-run evaluation of a constant-step lock-free run fluctuates by several points (see traced_replay)"}


def hogwild_parity(dsgd_amd, device, workers=256, batch=100, rows=100000, updates=2048):
    """Parity evidence for the BENCHMARKED Hogwild shape (256 workers x batch 100) on a shard small enough for the oracle:
    the engine records every update's {worker, iteration, update count its weights were read at, regulariser scalar, gate
    decision of every sampled row} in commit order; with the ENGINE'S OWN decisions the oracle recomputes every update of
    core/Slave.scala:92-101 exactly (oracle/hogwild_replay.py -- a constant-step lock-free run is chaotic, nothing that
    re-decides the gates can follow it).  What this pins is the ACCOUNTING: every update applied once, averaged, scaled,
    regularised as the reference does (`accounting_agrees`), and that the check can fail (one lost update, every update
    applied twice: both rejected).  The gates themselves are engine-recorded, not re-derived (`gates_are`); the gate
    checks with teeth -- a single worker replayed exactly, four workers held to the near-gate rows -- and the oracle's band
    of orderings run under `pytest -m gpu` (tests/test_gpu_hogwild_trace.py, tests/test_gpu_parity.py), not in every bench.
    Round 6: the engine also records the x . w EVERY sampled row was gated on and an update count known to be in the
    weights it read; `gate_check` holds every decision of THIS 256-worker run to the reference's rule on its recorded d and
    every d to the range the replayed weights allow (hogwild_replay.gate_check_recorded_dots: rigorous, 100 % of the rows),
    with two negative controls (a decision flipped against its d; a d moved out of its range)."""
    from oracle import hogwild_replay as hr  # checker only
    from oracle import oracle as orc

    data = dsgd_amd.synth.generate(rows, seed=13)
    n_train = int(rows * 0.8)
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAMBDA)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    split = split_vanilla(n_train, workers)
    t0 = time.perf_counter()
    with dsgd_amd.Engine(data.dim, LAMBDA, device=device) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        eng.async_set_trace(updates + workers)
        eng.async_start(split, batch=batch, lr=LR0, max_updates=updates, seed=5, positional_bug=False)
        eng.async_wait()
        trace = eng.async_read_trace()
        w_end = eng.get_weights().astype(np.float64)
    w_rep = np.zeros(data.dim + 1)
    stats = hr.replay_forced(o, w_rep, split, batch, LR0, 5, trace, fractions=(0.0, 0.5, 1.0))
    v = hr.verdict(o, w_end, w_rep, hr.merge([stats]))
    controls = {}
    for fault in ("double_apply", "drop_one"):
        w_bad = np.zeros(data.dim + 1)
        with np.errstate(all="ignore"):
            hr.replay_forced(o, w_bad, split, batch, LR0, 5, trace, fault=fault, check=False)
            err = float(np.abs(w_end - w_bad).max())
        controls[fault] = {"account_max_abs_err": err, "rejected": not err <= hr.ACCOUNT_TOL * max(1.0, float(np.abs(w_bad).max()))}
    # every decision of the benchmarked shape: rule on the recorded x . w, and the x . w inside what the replay allows
    g = hr.gate_check_recorded_dots(o, np.zeros(data.dim + 1), split, batch, LR0, 5, trace, prefix_every=16, collect=True)
    gate = {kk: g[kk] for kk in ("updates", "rows", "gate_rows_checked", "empty_rows", "rule_violations", "range_violations", "max_window",
                                 "mean_window", "share_pinned_by_the_replay", "width_over_abs_d_median", "states_share_inside", "ok")}
    gate["checks"] = "decision == !(y d < 0) on the recorded d (SparseSVM.scala:27-28); d inside sum_j x_j [min, max] of the replayed weights from seen_from to the updates in flight at the commit, + fp32 resolution"
    if not g["ok"]:
        raise SystemExit("Hogwild gate check (%d workers) failed: %r %r" % (workers, g["outside_rule"], g["outside_range"]))
    ctl = {}
    u_c, t_c = len(trace["worker"]) // 2, 5
    bad = dict(trace, mask=np.array(trace["mask"], copy=True))
    bad["mask"][u_c, t_c] ^= True
    bad["n_active"] = bad["mask"][:, :batch].sum(axis=1).astype(np.int32)
    gb = hr.gate_check_recorded_dots(o, np.zeros(data.dim + 1), split, batch, LR0, 5, bad, prefix_every=0)
    ctl["decision_flipped_against_its_d"] = {"rule_violations": gb["rule_violations"], "rejected": not gb["ok"]}
    bad = dict(trace, dot=np.array(trace["dot"], copy=True), mask=np.array(trace["mask"], copy=True))
    bad["dot"][u_c, t_c] = np.float32(g["hi"][u_c, t_c] + 0.05 * (g["hi"][u_c, t_c] - g["lo"][u_c, t_c]) + 1e-3)
    k_c = int(trace["worker"][u_c])
    y_c = float(o.label[hr.hog_rows(5, k_c, int(trace["it"][u_c]), split[k_c][0], split[k_c][1] - split[k_c][0], batch)[t_c]])
    bad["mask"][u_c, t_c] = not (y_c * float(bad["dot"][u_c, t_c]) < 0.0)
    bad["n_active"] = bad["mask"][:, :batch].sum(axis=1).astype(np.int32)
    gb = hr.gate_check_recorded_dots(o, np.zeros(data.dim + 1), split, batch, LR0, 5, bad, prefix_every=0)
    ctl["d_moved_out_of_its_range"] = {"range_violations": gb["range_violations"], "rule_violations": gb["rule_violations"], "rejected": not gb["ok"]}
    gate["negative_controls"] = ctl
    if not all(c["rejected"] for c in ctl.values()):
        raise SystemExit("Hogwild gate check: a negative control was not rejected: %r" % ctl)
    # the few-worker statement of round 5: 4 workers (kube/dsgd.yaml:95), every decision of every update with at most one
    # update in flight held to the reference's gate at both ends of [read_at, commit)
    split4 = split_vanilla(n_train, 4)
    with dsgd_amd.Engine(data.dim, LAMBDA, device=device) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        eng.async_set_trace(1200)
        eng.async_start(split4, batch=batch, lr=LR0, max_updates=1000, seed=9, positional_bug=False)
        eng.async_wait()
        trace4 = eng.async_read_trace()
    g4 = hr.gate_check_small_lag(o, np.zeros(data.dim + 1), split4, batch, LR0, 9, trace4, max_lag=1)
    if not g4["ok"]:
        raise SystemExit("Hogwild gate check (4 workers) failed: %r" % g4)
    gate4 = {kk: g4[kk] for kk in ("updates", "updates_checked", "rows_checked", "differ_at_both_ends", "explained_by_in_flight_or_resolution", "ok")}
    traced = {"rows": rows, "workers": workers, "batch": batch, "updates": int(v.get("updates", updates)), "checkpoint": v,
              "gate_check": gate, "gate_check_4_workers": gate4,
              "accounting_agrees": bool(all(v["ok"].values())),
              "gates_are": "engine-recorded; every one of them checked against the rule on its recorded x . w, every x . w against the replayed weights (gate_check)",
              "negative_controls": controls, "controls_rejected": all(c["rejected"] for c in controls.values()),
              "seconds": round(time.perf_counter() - t0, 1)}
    if not traced["accounting_agrees"] or not traced["controls_rejected"]:
        raise SystemExit("Hogwild traced parity failed: %r" % traced)
    return {"traced_replay": traced}


def reference_shape(dsgd_amd, device, n_rows, with_parity=True, repeats=5, steps=20):
    """The reference's OWN data-set sizes (N = 804,414 = full=true, DatasetTests.scala:18; N = 23,149 =
    full=false, application.conf:24) next to the 8,388,608-row headline: the whole-shard step with its roofline fields
    (median of `repeats` x `steps` steps, parity-gated like the headline) and the batch sweep from resident plans."""
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    n_train = int(n_rows * 0.8)
    nnz_train = int(data.row_ptr[n_train])
    bytes_per_row = (8.0 * nnz_train + 12.0 * n_train) / n_train
    lr = LR0 * 100.0 / n_train
    ranges = [(0, n_train)]
    res = {"rows": n_rows, "train_rows": n_train}
    o = None
    with dsgd_amd.Engine(data.dim, LAMBDA, device=device) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        if with_parity:
            p = parity_gate_single(eng, data, n_train, ranges, lr)
            res["parity_gate"] = {"max_rel_err": max(s["max_rel_err"] for s in p["steps"]),
                                  "worst_err_over_bound": max(s["worst_err_over_bound"] for s in p["steps"]),
                                  "fix_shift": p["steps"][-1]["fix_shift"], "rows": n_train}
            eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        for _ in range(30):
            eng.sync_step_ranges(ranges, lr, asynchronous=True)
        eng.synchronize()
        # the steps as a caller sees them (no event records: two records per step are 6 us -- a fifth of a 23,149-row step),
        # then the same steps with the gradient launches bracketed for the kernel's own duration
        times = timed_steps(eng, ranges, lr, steps, repeats, lambda e: e.synchronize(), lambda: None, 1, None)
        eng.prof_enable(2)
        eng.prof_read(reset=True)
        times_ev = timed_steps(eng, ranges, lr, steps, repeats, lambda e: e.synchronize(), lambda: None, 1, None)
        kernel_ms, n_launch = eng.prof_read(reset=True)
        eng.prof_enable(0)
        dt = float(np.median(times))
        res["whole_shard"] = {"examples_per_s": n_train * steps / dt, "us_per_step": 1e6 * dt / steps,
                              "us_per_step_min": 1e6 * min(times) / steps, "us_per_step_max": 1e6 * max(times) / steps,
                              "us_per_step_with_event_records": 1e6 * float(np.median(times_ev)) / steps,
                              "repeats": len(times), "steps": steps, "kernel": eng.grad_kernel_name()}
        res["roofline"] = roofline(eng, None, n_train, nnz_train, bytes_per_row, kernel_ms, n_launch, steps * len(times_ev), dt / steps, None)
        cfgs = tuple(c for c in SWEEP if c[0] * c[1] <= n_train)
        res["sweep"] = sweep(eng, data, n_train, with_parity=with_parity, configs=cfgs)
    return res


class RecordingBackend:
    """The engine behind host.MasterSync.fit, keeping the record of the FIRST `epochs` plans it runs (dsgd_plan_record: every
    row's gate decision, every step's regulariser scalar) and the weights each of those epochs ended on -- what
    oracle/sync_replay.py replays.  Everything else passes through."""

    def __init__(self, eng, epochs=1):
        self.eng, self.want, self.recs, self.kernels = eng, epochs, [], set()

    def _track(self, plan, k, idx, offsets, n_steps):
        plan.record(True)
        rec = {"plan": plan, "k": k, "idx": np.array(idx, copy=True), "offsets": np.array(offsets, copy=True), "n_steps": n_steps}
        self.recs.append(rec)
        real = plan.destroy

        def destroy():   # (fit destroys a plan right behind its run: the record is read first)
            if "masks" not in rec and rec.get("ran"):
                rec["masks"], rec["s"] = plan.read_record()
                rec["w_end"] = self.eng.get_weights()
            rec["plan"] = None
            real()

        plan.destroy = destroy

    def plan_flat(self, idx, offsets, n_steps, k):
        plan = self.eng.plan_flat(idx, offsets, n_steps, k)
        if len(self.recs) < self.want and n_steps:
            self._track(plan, k, idx, offsets, n_steps)
        return plan

    def plan_from_seed(self, jstate, split, max_samples, batch_size):
        """An epoch whose lists the DEVICE draws (csrc/dsgd_shuffle.hpp): what it drew is read back for the replay."""
        plan, n_steps, state, draws = self.eng.plan_from_seed(jstate, split, max_samples, batch_size)
        if plan is not None and len(self.recs) < self.want and n_steps:
            idx, offsets = self.eng.plan_lists(plan)
            self._track(plan, len(split), idx, offsets, n_steps)
        return plan, n_steps, state, draws

    def plan_run(self, plan, a, b, lr):
        self.eng.plan_run(plan, a, b, lr)
        self.kernels.add(self.eng.grad_kernel_name())
        for rec in self.recs:
            if rec.get("plan") is plan:
                rec["ran"] = True

    def steps_of(self, rec):
        o, k = rec["offsets"], rec["k"]
        return [[rec["idx"][o[s * k + j]:o[s * k + j + 1]] for j in range(k)] for s in range(rec["n_steps"])]

    def __getattr__(self, name):
        return getattr(self.eng, name)


def forced_replay(o, backend, w0, lr):
    """oracle/sync_replay.py over what a RecordingBackend kept: (a) the engine's weights are the replayed ones to rounding,
    (b) every decision that differs from the oracle's own gate on the replayed weights is a row inside fp32 resolution,
    (c) the first step at which the two sides decide differently.  Raises SystemExit when (a) or (b) fails."""
    from oracle import sync_replay as sr  # checker only

    recs = [r for r in backend.recs if "masks" in r]
    if not recs:
        return None
    t0 = time.perf_counter()
    w = np.asarray(w0, dtype=np.float64).copy()
    steps = [st for r in recs for st in backend.steps_of(r)]
    stats = sr.replay(o, w, steps, lr, np.concatenate([r["masks"] for r in recs]), np.concatenate([r["s"] for r in recs]))
    v = sr.verdict(stats, recs[-1]["w_end"], w)
    out = {kk: v[kk] for kk in ("accounting_agrees", "account_err_over_tol", "account_max_abs_err", "decisions", "differing_decisions",
                                "first_divergent_step", "divergent_rows_all_near_gate", "worst_margin_over_resolution", "s_agrees")}
    out.update(steps=len(steps), replay_s=round(time.perf_counter() - t0, 1))
    if not (v["accounting_agrees"] and v["divergent_rows_all_near_gate"] and v["s_agrees"]):
        raise SystemExit("forced replay of the synchronous trajectory failed: %r (outside: %r)" % (out, v["outside"]))
    return out


def fit_through_the_mirror(dsgd_amd, host, eng_backend, o, n_train, n_rows, k, b, lr, max_epochs, criterion, seed=0):
    """host.MasterSync.fit -- the mirror of core/Master.scala:120-218 that the dev role and a patched reference's resident
    master run: every epoch's batches as ONE resident plan, the reference's random stream (java.util.Random seeded 0,
    Main.scala:32; every split reshuffled for every batch, Master.scala:184) drawn natively, the next epoch's lists and plan
    prepared while this epoch runs, the two evaluation passes per epoch (:206-209).  Returns (mirror, wall seconds)."""
    m = host.MasterSync(eng_backend, n_train, n_rows, k, rnd=host.JavaRandom(seed))
    t0 = time.perf_counter()
    m.fit(np.zeros(o.dim + 1), max_epochs, b, lr, criterion)
    return m, time.perf_counter() - t0


def time_to_target(dsgd_amd, device, n_rows=804414, oracle_budget_s=5.0, max_epochs_engine=30):
    """Wall-clock time to the oracle's target test loss per batch size, on the reference's full=true shape, THROUGH
    host.MasterSync.fit (fit_through_the_mirror).  Target = the MEDIAN over 10 epochs (max-epochs, application.conf:37) of
    the ORACLE's test loss at the reference's configuration (3 workers x batch 100, lr 0.5) -- the curve of a constant-step
    run is noisy, so neither its minimum nor its last value is a level another trajectory can be asked to reach.  A
    configuration's clock is the whole fit: drawing the lists (the reference's per-batch reshuffle is O(rows) master work
    per BATCH: 1.4 G draws per epoch here -- `shuffle_s` says what of it was not hidden behind the device), laying the
    plans out, the steps, the evaluation passes.  The oracle runs the same mirror with the same stream (at most
    `oracle_budget_s` past its first epoch).  The reference's own configuration (configs[0]) also carries the FORCED REPLAY of
    its first epoch: the engine's recorded gate decisions replayed by the oracle -- `first_divergent_step`,
    `divergent_rows_all_near_gate`, the accounting error -- next to the free-running difference after that epoch."""
    from dsgd_amd import host
    from oracle import oracle as orc  # checker / target only
    from oracle.backend import OracleBackend

    data = dsgd_amd.synth.generate(n_rows, seed=0)
    n_train = int(n_rows * 0.8)
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAMBDA)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    t0 = time.perf_counter()
    mo, _ = fit_through_the_mirror(dsgd_amd, host, OracleBackend(o), o, n_train, n_rows, 3, 100, LR0, 10, lambda losses: False)
    ref_curve = list(reversed(mo.test_losses))
    target = float(np.median(ref_curve))
    out = {"rows": n_rows, "train_rows": n_train, "target_test_loss": target, "through": "host.MasterSync.fit (an epoch = one plan; its lists drawn by the device from 8 M draws per epoch on, else by csrc/jrand.c; prefetch)",
           "target": "median over 10 oracle epochs at 3 x 100, lr 0.5", "oracle_target_curve": ref_curve,
           "oracle_target_s": round(time.perf_counter() - t0, 1), "configs": []}
    with dsgd_amd.Engine(data.dim, LAMBDA, device=device) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        eng.sync_step_ranges([(0, n_train)], 0.0)   # layout and first launches outside every clock
        for ci, (k, b) in enumerate(((3, 100), (4, 200), (1, 4096), (1, 65536), (1, None))):
            bb = n_train if b is None else b
            lr = LR0 * 100.0 / bb
            # the oracle through the same mirror (its first epoch always; more while the budget lasts)
            t2 = time.perf_counter()
            ob = OracleBackend(o)
            w_o1 = []

            def crit_o(losses):
                if len(losses) == 1 and not w_o1:
                    w_o1.append(ob.w.copy())
                return bool(losses) and (losses[0] <= target or time.perf_counter() - t2 > oracle_budget_s)

            mo, _ = fit_through_the_mirror(dsgd_amd, host, ob, o, n_train, n_rows, k, bb, lr, 10, crit_o)
            if not w_o1:
                w_o1.append(ob.w.copy())
            o_curve = list(reversed(mo.test_losses))
            o_reached = next((i + 1 for i, l in enumerate(o_curve) if l <= target), None)
            t_oracle = time.perf_counter() - t2
            exposed1 = int(sum(mm < 1e-5 for mm in ob.min_margins[:mo.steps_run // max(1, len(o_curve))]))
            # the engine
            rec = RecordingBackend(eng, epochs=1 if ci == 0 else 0)
            w_e1 = []

            def crit_e(losses):
                if len(losses) == 1 and not w_e1:
                    w_e1.append(eng.get_weights().astype(np.float64))
                return bool(losses) and losses[0] <= target

            m, fit_s = fit_through_the_mirror(dsgd_amd, host, rec, o, n_train, n_rows, k, bb, lr, max_epochs_engine, crit_e)
            if not w_e1:
                w_e1.append(eng.get_weights().astype(np.float64))
            curve = list(reversed(m.test_losses))
            reached = next((i + 1 for i, l in enumerate(curve) if l <= target), None)
            cfg = {"workers": k, "batch": bb, "lr": lr, "engine_epochs": reached, "time_to_target_s": fit_s if reached else None,
                   "engine_epochs_run": len(curve), "fit_s": fit_s, "batch_loop_s": m.batch_loop_s, "shuffle_s_not_hidden": m.shuffle_s,
                   "steps": m.steps_run, "batch_loop_us_per_step": 1e6 * m.batch_loop_s / max(1, m.steps_run),
                   "engine_test_loss": curve[:12], "kernel": sorted(rec.kernels) or [eng.grad_kernel_name()], "oracle_epochs": o_reached,
                   "oracle_epochs_run": len(o_curve), "oracle_s": round(t_oracle, 2),
                   "epoch1_max_abs_diff": float(np.abs(w_e1[0] - w_o1[0]).max()), "epoch1_steps_with_a_row_near_the_gate": exposed1,
                   "evaluation": "2 passes per epoch inside the clock (train, test): loss and accuracy of each"}
            if ci == 0:
                fr = forced_replay(o, rec, np.zeros(data.dim + 1), lr)
                if fr:
                    cfg["forced_replay_epoch1"] = fr
                    cfg.update(first_divergent_step=fr["first_divergent_step"], divergent_rows_all_near_gate=fr["divergent_rows_all_near_gate"],
                               forced_replay_account_err_over_tol=fr["account_err_over_tol"])
            out["configs"].append(cfg)
    done = [c for c in out["configs"] if c["time_to_target_s"] is not None]
    out["fastest"] = min(done, key=lambda c: c["time_to_target_s"]) if done else None
    if out["fastest"]:
        out["fastest"] = {kk: out["fastest"][kk] for kk in ("workers", "batch", "engine_epochs", "time_to_target_s")}
    return out


def dense_logistic(dsgd_amd, device, rows=1250000, dim=4096):
    """BASELINE.json configs[4] on ONE GPU's share: 10 M x 4096 over 8 GPUs = 1.25 M rows (20.5 GB) per GPU, generated
    on the device; mini-batch steps of contiguous 4,096 / 65,536-row slices.  No reference counterpart (the optional
    dense variant of north_star); roofline 16,388 B per example."""
    res = {"rows": rows, "dim": dim, "bytes_per_example": 4 * dim + 4, "batches": [],
           "note": "dsgd_dense_step_kernel: row block read once, forward and gradient products from registers (v_fma: an fp32 "
                   "GEMV fills 1/16 of an MFMA at the vector rate -- csrc/dsgd_dense.hpp); no reference counterpart"}
    with dsgd_amd.DenseLogistic(dim, device=device) as eng:
        t0 = time.perf_counter()
        eng.generate(rows, seed=device)
        res["generate_s"] = round(time.perf_counter() - t0, 2)
        for b, steps in ((65536, 40), (4096, 200)):
            starts = [(i * b) % (rows - b) for i in range(steps + 5)]
            for st in starts[:5]:
                eng.step(st, st + b, 1.0)
            eng.synchronize()
            eng.prof(True)
            t0 = time.perf_counter()
            for st in starts[5:]:
                eng.step(st, st + b, 1.0)
            eng.synchronize()
            dt = time.perf_counter() - t0
            kms, kn = eng.prof(False)
            ex = b * steps / dt
            res["batches"].append({"batch": b, "steps": steps, "examples_per_s": ex, "us_per_step": 1e6 * dt / steps,
                                   "frac_hbm_peak": ex * (4 * dim + 4) / HBM_PEAK, "kernel_ms_avg": kms,
                                   "kernel_frac_hbm_peak": (b * (4 * dim + 4) / (kms * 1e-3) / HBM_PEAK) if kms > 0 else None})
        loss, acc = eng.loss(rows - 65536, rows)
        res["loss_after"], res["acc_after"] = loss, acc
    # the variant with the forward product on the matrix cores (configs[4]: "mini-batch GEMV via MFMA"), same data
    os.environ["DSGD_DENSE_MFMA"] = "1"
    try:
        with dsgd_amd.DenseLogistic(dim, device=device) as eng:
            eng.generate(rows, seed=device)
            b, steps = 65536, 40
            starts = [(i * b) % (rows - b) for i in range(steps + 5)]
            for st in starts[:5]:
                eng.step(st, st + b, 1.0)
            eng.synchronize()
            eng.prof(True)
            t0 = time.perf_counter()
            for st in starts[5:]:
                eng.step(st, st + b, 1.0)
            eng.synchronize()
            dt = time.perf_counter() - t0
            kms, _ = eng.prof(False)
            res["mfma_variant"] = {"batch": b, "steps": steps, "examples_per_s": b * steps / dt, "us_per_step": 1e6 * dt / steps,
                                   "kernel_ms_avg": kms,
                                   "kernel_frac_hbm_peak": (b * (4 * dim + 4) / (kms * 1e-3) / HBM_PEAK) if kms > 0 else None,
                                   "note": "dsgd_dense_step_mfma_kernel: v_mfma_f32_16x16x4_f32 forward product (1/16 of each "
                                           "instruction useful for a matrix-vector product: with fp32 inputs the matrix pipe runs "
                                           "at the vector rate, so the variant stays optional and is the slower one), gradient "
                                           "product on the VALU"}
    finally:
        del os.environ["DSGD_DENSE_MFMA"]
    return res


def l3_bytes():
    """Total L3 of the host (all sockets), from sysfs; None if unknown."""
    try:
        seen, total = set(), 0
        base = "/sys/devices/system/cpu"
        for cpu in os.listdir(base):
            p = os.path.join(base, cpu, "cache", "index3")
            if not os.path.isdir(p):
                continue
            key = open(os.path.join(p, "shared_cpu_list")).read().strip()
            if key in seen:
                continue
            seen.add(key)
            sz = open(os.path.join(p, "size")).read().strip()
            total += int(sz[:-1]) * (1024 if sz.endswith("K") else 1024 * 1024) if sz[-1] in "KM" else int(sz)
        return total or None
    except (OSError, ValueError):
        return None


def cpu_baseline(data, n_train, budget_s):
    """The oracle timed on the host cores: (B) OpenMP CSR restatement on all cores, same whole-shard
    step on a bounded sample; (A) literal per-sample sparse-map restatement, one thread, B=100."""
    from oracle import oracle as orc

    LR = LR0
    n_s = min(n_train, 2000000)   # 1.2 GB of CSR: beyond the host's L3 (the 200,000-row sample of round 2 was cache-resident)
    sub = data.rows(0, n_s)
    o = orc.Oracle(sub.dim, sub.row_ptr, sub.col, sub.val, sub.label, LAMBDA)
    o.set_dim_sparsity(o.dim_sparsity(n_s))
    w = np.zeros(sub.dim + 1)
    o.sync_step_range_omp(w, 0, n_s, LR)  # warm
    t0, steps = time.perf_counter(), 0
    while time.perf_counter() - t0 < budget_s and steps < 200:
        o.sync_step_range_omp(w, 0, n_s, LR)
        steps += 1
    dt = time.perf_counter() - t0
    fast = {
        "value": n_s * steps / dt,
        "unit": "examples/s",
        "cores": orc.num_threads(),
        "kind": "port",
        "sample": "OpenMP CSR fp64 restatement (oracle.c orc_sync_step_range_omp): %d whole-shard steps over the "
                  "first %d train rows of the same workload, %.1f s" % (steps, n_s, dt),
        "host_cpus": os.cpu_count(),
        "sample_bytes": int(8 * sub.nnz + 12 * n_s),
        "sample_exceeds_l3": bool(8 * sub.nnz + 12 * n_s > l3_bytes()) if l3_bytes() else None,
        "host_l3_bytes": l3_bytes(),
    }
    # literal: Slave.gradient as one single-threaded request of 100 samples (core/Slave.scala:142)
    rng = np.random.default_rng(5)
    w = np.zeros(sub.dim + 1)
    t0, steps = time.perf_counter(), 0
    while time.perf_counter() - t0 < min(budget_s, 6.0):
        o.sync_step(w, [rng.permutation(n_s)[:100].astype(np.int32)], LR, literal=True)
        steps += 1
    dt = time.perf_counter() - t0
    lit = {
        "value": 100 * steps / dt,
        "unit": "examples/s",
        "cores": 1,
        "kind": "port",
        "sample": "literal per-sample sparse-vector restatement (oracle.c orc_lit_sync_step), 1 worker, "
                  "batch-size 100, %d steps, %.1f s" % (steps, dt),
    }
    return fast, lit


def epochs_to_target(dsgd_amd, device):
    """Second half of BASELINE.json's metric on configs[1]'s shape (full=false: 23,149 rows, 80/20 split, 3 workers,
    batch-size 100, lr 0.5, lambda 1e-5, max-epochs 10 -- application.conf), THROUGH host.MasterSync.fit on both sides with
    the reference's random stream (java.util.Random seeded 0, Main.scala:32): the target is the ORACLE's best test loss
    within the 10 epochs; reported: epochs until the engine's test loss is at or below it, both curves, and what the
    boundary costs -- `fit`: microseconds per batch of the engine's batch loops (drawing the lists, laying the epoch's plan
    out, the steps; Master.scala:179-199), with an epoch as ONE resident plan and, for comparison, one dsgd_sync_step per
    batch (what the Scala patch called before round 5)."""
    from dsgd_amd import host
    from oracle import oracle as orc  # checker / CPU baseline only
    from oracle.backend import OracleBackend

    n_rows, k, batch, lr, epochs = 23149, 3, 100, LR0, 10
    n_train = int(n_rows * 0.8)
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAMBDA)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    never = lambda losses: False
    t0 = time.perf_counter()
    mo, _ = fit_through_the_mirror(dsgd_amd, host, OracleBackend(o), o, n_train, n_rows, k, batch, lr, epochs, never)
    t_ref = time.perf_counter() - t0
    ref_curve = list(reversed(mo.test_losses))
    with dsgd_amd.Engine(data.dim, LAMBDA, device=device) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        fit_through_the_mirror(dsgd_amd, host, eng, o, n_train, n_rows, k, batch, 0.0, 2, never)   # layout, first launches, block cache: outside the clock
        rec = RecordingBackend(eng, epochs=epochs)
        m, t_eng = fit_through_the_mirror(dsgd_amd, host, rec, o, n_train, n_rows, k, batch, lr, epochs, never)
        curve = list(reversed(m.test_losses))
        fr = forced_replay(o, rec, np.zeros(data.dim + 1), lr)
        m2, t2 = fit_through_the_mirror(dsgd_amd, host, eng, o, n_train, n_rows, k, batch, lr, epochs, never)      # (unrecorded: the timing)
        mp = host.MasterSync(eng, n_train, n_rows, k, rnd=host.JavaRandom(0), plans=False)
        tp = time.perf_counter()
        mp.fit(np.zeros(data.dim + 1), 2, batch, lr, never)
        tp = time.perf_counter() - tp
    # Target: the BEST test loss the oracle reaches within max-epochs (the curve of a constant-step run is noisy: its
    # last-epoch loss is worse than its epoch-2 loss, which made "epochs to the last-epoch loss" trivially 2 for both
    # sides in round 2).  The hinge part moves in steps of 1/n_test (predictions are -1/0/+1): one test row of slack.
    target = min(ref_curve)
    slack = 1.0 / (n_rows - n_train)
    reached = next((i + 1 for i, l in enumerate(curve) if l <= target + slack), None)
    reached_ref = next((i + 1 for i, l in enumerate(ref_curve) if l <= target + slack), None)
    half = 0.5 * 1.0   # loss at w = 0 is exactly 1 (every prediction is 0): first epoch at or below half of it
    fit = {"through": "host.MasterSync.fit: an epoch = ONE resident plan, native random stream, next epoch prepared while this one runs",
           "steps": m2.steps_run, "batch_loop_us_per_step": 1e6 * m2.batch_loop_s / max(1, m2.steps_run),
           "shuffle_us_per_step_not_hidden": 1e6 * m2.shuffle_s / max(1, m2.steps_run), "fit_s_10_epochs_with_evaluation": t2,
           "per_request_us_per_step": 1e6 * mp.batch_loop_s / max(1, mp.steps_run),
           "per_request_note": "one dsgd_sync_step per batch (what the Scala patch called before round 5), the epoch's lists from the "
                               "same native generator (%.1f us per step of it)" % (1e6 * mp.shuffle_s / max(1, mp.steps_run)),
           "kernel": sorted(rec.kernels), "forced_replay_10_epochs": fr}
    fit["summary"] = {"us_per_step": fit["batch_loop_us_per_step"], "per_request_us_per_step": fit["per_request_us_per_step"],
                      "kernel": fit["kernel"][0] if fit["kernel"] else None,
                      "forced_replay_agrees": bool(fr and fr["accounting_agrees"] and fr["divergent_rows_all_near_gate"]),
                      "first_divergent_step": fr["first_divergent_step"] if fr else None}
    return {"config": "23149 rows, 3 workers x batch 100, lr 0.5, lambda 1e-5, 10 epochs", "target_test_loss": target,
            "target": "min over the oracle's epochs", "slack": slack, "through": "host.MasterSync.fit on both sides, java.util.Random(0)",
            "epochs_to_half_initial_loss": {"engine": next((i + 1 for i, l in enumerate(curve) if l <= half), None),
                                            "oracle": next((i + 1 for i, l in enumerate(ref_curve) if l <= half), None)},
            "max_curve_difference": float(np.abs(np.asarray(curve) - np.asarray(ref_curve)).max()),
            "max_epochs": epochs, "engine_epochs": reached, "oracle_epochs": reached_ref,
            "engine_test_loss": curve, "oracle_test_loss": ref_curve,
            "engine_s": t_eng, "oracle_s": t_ref, "steps_per_epoch": m.steps_run // epochs, "fit": fit}


if __name__ == "__main__":
    main()
