"""One rank of tests/test_gpu_fp64_world2.py (and of tests/test_gpu_fp64_rccl_multi.py): an fp64 engine over its shard
of the rows, attached with comm_init_f64, stepping the sequence below.  Over the tests' seam build and the stand-in
collective both ranks share device 0; with `--real` the product library over real RCCL, one device per rank.
usage: python fp64_world2_worker.py <rank> <world> <workdir> [steps|mismatch] [--real]"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dsgd_amd  # noqa: E402
from dsgd_amd import _lib  # noqa: E402
from world2_common import CFG, local_lists, shard_of  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402

# the steps behind CFG["list_steps"] ((k, rows): 1 x 100, 3 x 100, 1 x 5,000, 2 x 700 per rank)
EXTRA = ["whole", "unequal", "dups", "sliced"]
N_STEPS = len(CFG["list_steps"]) + len(EXTRA)
SLICED_AT = N_STEPS - 1   # entered with the weights slice-major: K = 4, also the negative control's step


def step_lists(rank, i, ntl):
    """(lists of rank `rank`, lr) of step i; every rank hosts the same number of workers"""
    if i < len(CFG["list_steps"]):
        k, b = CFG["list_steps"][i]
        return local_lists(rank, i, k, b, ntl), 0.5 * 100 / b
    kind = EXTRA[i - len(CFG["list_steps"])]
    rng = np.random.default_rng(5000 + 10 * i + rank)
    if kind == "whole":      # one worker per rank, its whole local split
        return [np.arange(ntl, dtype=np.int32)], 0.5 * 100 / ntl
    if kind == "unequal":    # different list lengths among the workers of one step: different shifts
        sizes = [(100, 700), (300, 5000)][rank % 2]
        return [rng.permutation(ntl)[:n].astype(np.int32) for n in sizes], 0.05
    if kind == "dups":       # duplicates count twice, as in the oracle
        a, b = (rng.permutation(ntl)[:400].astype(np.int32) for _ in range(2))
        return [np.concatenate([a, a[:50]]), np.concatenate([b, b[:1], b[:1]])], 0.1
    return [rng.permutation(ntl)[:n].astype(np.int32) for n in (100, 130)], 0.5   # "sliced"


def small_plan_lists(ntl):
    rng = np.random.default_rng(99)
    return [[rng.permutation(ntl)[:100].astype(np.int32) for _ in range(2)] for _ in range(3)]


def bits(v):
    return np.ascontiguousarray(v).view(np.uint64)


def code_of(fn):
    try:
        fn()
    except _lib.DsgdError as e:
        return e.code
    return 0


def run_steps(eng, rank, world, wd, sh, out):
    ntl = sh.n_train
    eng.comm_init_f64(exchange_uid(wd, "uid_a.bin", rank, dsgd_amd.Engine.comm_unique_id), world, rank)
    out["ds"] = eng.build_dim_sparsity(ntl)        # feature counts all-reduced
    out["ranks"] = eng.column_ranks()              # column counts all-reduced
    w_hist, stats = [], []
    for i in range(N_STEPS):
        lists, lr = step_lists(rank, i, ntl)
        if i == SLICED_AT:
            # a plan leaves the weights slice-major; plans are refused under a communicator, so: detach, run a small plan
            # with lr = 0 (every replica keeps its bits), attach again -- comm_init_f64 keeps the layout it finds
            eng.comm_destroy()
            p = eng.plan(small_plan_lists(ntl))
            eng.plan_run(p, 0, 3, 0.0)
            eng.comm_init_f64(exchange_uid(wd, "uid_b.bin", rank, dsgd_amd.Engine.comm_unique_id), world, rank)
            p.destroy()
        st = eng.sync_step_f64(lists, lr) if i % 2 else eng.sync_step(lists, lr)   # (both entry points; the slice-major step: _f64, which keeps the layout)
        w_hist.append(eng.get_weights())
        stats.append([st["n_samples"], st["n_active"]])
    out["w_hist"] = np.stack(w_hist)
    out["stats"] = np.asarray(stats)
    l_tr, a_tr, c_tr = eng.loss_acc(0, ntl)
    l_te, a_te, c_te = eng.loss_acc(ntl, sh.csr.n_rows)
    out["eval"] = np.asarray([l_tr, a_tr] + list(c_tr) + [l_te, a_te] + list(c_te), dtype=np.float64)
    # refusals with the communicator attached: EUNSUPPORTED, the weights keep their bits
    w_before = eng.get_weights()
    out["refused"] = np.asarray([code_of(lambda: eng.plan(small_plan_lists(ntl))),
                                 code_of(lambda: eng.plan_from_seed(12345, [(0, ntl // 2), (ntl // 2, ntl)], ntl, 100)),
                                 code_of(lambda: eng.async_plan([(0, ntl)], 100, seed=3, n_updates=4))])
    out["refused_w_same"] = np.asarray(np.array_equal(bits(w_before), bits(eng.get_weights())))
    # detached again: a local step
    eng.comm_destroy()
    lists, lr = step_lists(rank, 3, ntl)
    st = eng.sync_step_f64(lists, lr)
    out["w_local_from"] = w_before
    out["w_local"] = eng.get_weights()
    out["stats_local"] = np.asarray([st["n_samples"], st["n_active"]])


def run_mismatch(eng, rank, world, wd, sh, out):
    """rank r calls with 1 + r hosted workers: DSGD_EINVAL on every rank, nothing changed; the next agreed step runs"""
    ntl = sh.n_train
    eng.comm_init_f64(exchange_uid(wd, "uid_m.bin", rank, dsgd_amd.Engine.comm_unique_id), world, rank)
    eng.build_dim_sparsity(ntl)
    rng = np.random.default_rng(300 + rank)
    common = np.zeros(eng.dp)
    common[np.random.default_rng(7).permutation(eng.dp - 1)[:2000] + 1] = 0.01   # the same on every rank
    eng.set_weights(common)
    lists = [rng.permutation(ntl)[:200].astype(np.int32) for _ in range(1 + rank)]
    out["code"] = np.asarray(code_of(lambda: eng.sync_step_f64(lists, 0.5)))
    out["w_same"] = np.asarray(np.array_equal(bits(common), bits(eng.get_weights())))
    st = eng.sync_step_f64(lists[:1], 0.5)
    out["w_after"] = eng.get_weights()
    out["stats_after"] = np.asarray([st["n_samples"], st["n_active"]])
    eng.comm_destroy()


def main():
    rank, world, wd = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    mode = sys.argv[4] if len(sys.argv) > 4 and not sys.argv[4].startswith("--") else "steps"
    real = "--real" in sys.argv
    if real:
        assert not os.environ.get("DSGD_LIB_PATH"), "the product library over real RCCL"
    else:
        assert os.environ.get("DSGD_RCCL_LIB"), "the worker must run with the shim selected explicitly"
        assert os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so"), "... through the tests' seam build of the library"
    data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    sh = shard_of(data, CFG["n_train"], rank, world)
    out = {}
    with dsgd_amd.Engine(data.dim, CFG["lam"], device=rank if real else 0, precision="fp64") as eng:
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val, sh.csr.label)
        (run_steps if mode == "steps" else run_mismatch)(eng, rank, world, wd, sh, out)
    np.savez(os.path.join(wd, "out_%d.npz" % rank), **out)
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
