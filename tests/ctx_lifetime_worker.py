"""Worker of tests/test_gpu_ctx_lifetime.py: runs on the tests' seam build of the library (DSGD_LIB_PATH =
tests/rccl_stub/libdsgd_hip_seam.so), the only build that counts the bytes it holds (dsgd_test_live_bytes, counted inside the
two allocation pairs of csrc/dsgd_buf.hpp).  Every cycle creates one owner, exercises it, destroys it, and reports the
counters before, in the middle and after as one JSON line "CYCLE {...}"; nothing here provokes a fault or an abort."""

import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dsgd_amd  # noqa: E402
from dsgd_amd import _lib  # noqa: E402

N_ROWS, N_TRAIN, DIM, LAM = 3000, 2400, 2000, 1e-5
lib = _lib.load()


def live():
    d, p = C.c_int64(-1), C.c_int64(-1)
    lib.dsgd_test_live_bytes(C.byref(d), C.byref(p))
    return [d.value, p.value]


def report(name, before, during, after, **more):
    print("CYCLE " + json.dumps(dict(name=name, before=before, during=during, after=after, **more)), flush=True)


def lists(rng, n_steps, k, batch):
    return [[rng.permutation(N_TRAIN)[:batch].astype(np.int32) for _ in range(k)] for _ in range(n_steps)]


def sparse_w(rng, dtype):
    keys = np.sort(rng.choice(np.arange(1, DIM + 1), size=300, replace=False)).astype(np.int32)
    return keys, rng.normal(scale=0.05, size=300).astype(dtype)


def context_cycle(name, precision, double_values):
    rng = np.random.default_rng(7)
    data = dsgd_amd.synth.generate(N_ROWS, seed=11, dim=DIM)
    val = data.val.astype(np.float64) if double_values else data.val
    fp64 = precision == "fp64"
    kernels = {}
    before = live()
    eng = dsgd_amd.Engine(DIM, LAM, precision=precision)
    eng.load_csr(data.row_ptr, data.col, val, data.label)
    eng.build_dim_sparsity(N_TRAIN)
    eng.load_csr(data.row_ptr, data.col, val, data.label)   # the reload: everything of the first load goes
    ds = eng.build_dim_sparsity(N_TRAIN)
    eng.set_dim_sparsity(ds)
    wdt = np.float64 if fp64 else np.float32
    eng.set_weights(rng.normal(scale=0.05, size=DIM + 1).astype(wdt))
    eng.get_weights()
    eng.set_weights_sparse(*sparse_w(rng, wdt))
    eng.get_weights_sparse()
    idx = rng.permutation(N_TRAIN)[:100].astype(np.int32)
    if fp64:
        eng.gradient_f64(idx)
        eng.gradient_sparse(idx)
        eng.sync_step_f64(lists(rng, 1, 2, 100)[0], 0.5)
        steps = lists(rng, 4, 2, 50)
        flat = np.concatenate([a for s in steps for a in s])
        offs = np.concatenate([[0], np.cumsum([len(a) for s in steps for a in s])]).astype(np.int64)
        eng.sync_steps_f64(flat, offs, 4, 2, 0.5, per_step=True)   # (DSGD_RP64_FUSED unset: the two-launch queue)
        eng.forward_f64(idx)
    else:
        eng.gradient(idx)
        eng.gradient_sparse(idx)
        eng.sync_step(lists(rng, 1, 2, 100)[0], 0.5)   # index lists, 2 workers
        # range steps through the three families (DSGD_TCOL_MIN / _MAX, DSGD_FSTEP_MIN set by the test)
        for key, ranges in (("row_wise", [(0, 300)]), ("column_lists", [(0, 700), (700, 1500)]), ("row_chunks", [(0, 1200), (1200, N_TRAIN)])):
            eng.sync_step_ranges(ranges, 0.01)
            kernels[key] = eng.grad_kernel_name()
        eng.forward(idx)
    eng.loss_acc(N_TRAIN, N_ROWS)
    delta, _ = eng.async_step(idx, 0.1, want_delta=True)
    eng.async_step_sparse(idx, 0.1)
    keys = np.flatnonzero(delta).astype(np.int32)[:200]
    eng.update_grad(keys, delta[keys])
    during = live()
    alive = None
    if not double_values:   # (plans are refused while Double values are loaded)
        plan = eng.plan(lists(rng, 3, 2, 100))
        eng.plan_run(plan, 0, 3, 0.5)
        eng.synchronize()
        kernels["plan"] = plan.info()["kind"]
        plan.destroy()
        if not fp64:
            big = eng.plan(lists(rng, 2, 1, 2300))   # beyond the one-workgroup and column-slice steps: virtual tiles
            eng.plan_run(big, 0, 2, 0.05)
            eng.synchronize()
            kernels["big_plan"] = big.info()["kind"]
            big.destroy()
            third = N_TRAIN // 3   # (one epoch of Master.fit over three splits, the lists drawn on the device)
            seeded, n_steps, _, _ = eng.plan_from_seed(0x5DEECE66D, [range(0, third), range(third, 2 * third), range(2 * third, N_TRAIN)], third, 100)
            eng.plan_run(seeded, 0, n_steps, 0.5)
            eng.synchronize()
            seeded.destroy()
        alive = eng.plan(lists(rng, 3, 2, 100))
        if not fp64:   # the record's two blocks: taken, handed back, taken again -- and held at dsgd_destroy
            alive.record(True)
            eng.plan_run(alive, 0, 1, 0.5)
            alive.record(False)
            alive.record(True)
            kernels["alive_plan"] = alive.info()["kind"]
            kernels["alive_record_words"] = alive.info()["record_words"]
        eng.plan_run(alive, 0, 3, 0.5)   # (left alive at dsgd_destroy, its steps not synchronised)
    if not fp64:
        eng.async_set_trace(64)
        split = [(0, N_TRAIN // 2), (N_TRAIN // 2, N_TRAIN)]
        eng.async_start(split, batch=32, lr=0.05, max_updates=40, seed=3, positional_bug=False)
        eng.async_wait()
        eng.async_read_trace()
        eng.async_start(split, batch=32, lr=0.05, max_updates=10**9, seed=4, positional_bug=False)
        eng.async_stop()
    eng.close()   # `alive` is never destroyed: dsgd_destroy gives its blocks back through the cache and deletes it
    if alive is not None:
        alive.handle = None
    report(name, before, during, live(), kernels=kernels)


def host_layout_cycle():
    """The column slices laid out by the host (DSGD_CS_HOST_LAYOUT=1, read at dsgd_create): blocks of the plan's own, outside
    the cache.  Built, run, rebuilt over the freed ones after a second load, and alive at dsgd_destroy."""
    rng = np.random.default_rng(9)
    data = dsgd_amd.synth.generate(N_ROWS, seed=11, dim=DIM)
    before = live()
    os.environ["DSGD_CS_HOST_LAYOUT"] = "1"
    try:
        eng = dsgd_amd.Engine(DIM, LAM)
    finally:
        del os.environ["DSGD_CS_HOST_LAYOUT"]
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.set_dim_sparsity(eng.build_dim_sparsity(N_TRAIN))
    eng.set_weights(rng.normal(scale=0.05, size=DIM + 1).astype(np.float32))
    plan = eng.plan(lists(rng, 3, 2, 100))
    eng.plan_run(plan, 0, 3, 0.5)
    eng.synchronize()
    first = plan.info()
    during = live()
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)   # the slices are stale: the next run frees and rebuilds them
    eng.set_dim_sparsity(eng.build_dim_sparsity(N_TRAIN))
    eng.plan_run(plan, 0, 3, 0.5)
    eng.synchronize()
    second = plan.info()
    eng.close()   # (the plan alive, holding host-built slices)
    plan.handle = None
    report("host_layout", before, during, live(), kinds=[first["kind"], second["kind"]], device_built=[first["device_built"], second["device_built"]])


def failure_cycle():
    data = dsgd_amd.synth.generate(N_ROWS, seed=11, dim=DIM)
    before = live()
    eng = dsgd_amd.Engine(DIM, LAM)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    during = live()
    refused = False
    try:
        eng.sync_step([np.asarray([5, N_ROWS + 3], dtype=np.int32)], 0.5)   # an index outside the rows: refused by validation
    except dsgd_amd.DsgdError:
        refused = True
    eng.close()
    report("failure_path", before, during, live(), refused=refused)


def dense_cycle():
    before = live()
    d = dsgd_amd.dense.DenseLogistic(512)   # (the narrowest the engine accepts: a lane owns 8 columns)
    d.generate(4096, seed=1)
    d.step(0, 4096, 0.1)
    d.synchronize()
    d.loss(0, 4096)
    during = live()
    d.close()
    report("dense", before, during, live())


which = sys.argv[1:] or ["fp32", "host_layout", "fp64_float", "fp64_double", "failure_path", "dense"]
for w in which:
    if w == "fp32":
        context_cycle("fp32", "fp32", False)
    elif w == "fp64_float":
        context_cycle("fp64_float", "fp64", False)
    elif w == "fp64_double":
        context_cycle("fp64_double", "fp64", True)
    elif w == "host_layout":
        host_layout_cycle()
    elif w == "failure_path":
        failure_cycle()
    elif w == "dense":
        dense_cycle()
print("CTX_LIFETIME_DONE", flush=True)
