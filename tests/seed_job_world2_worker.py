"""One rank of tests/test_gpu_seed_job_world2.py: an fp64 engine over the rank's shard of the rows (float feature values),
attached with comm_init_f64 through the tests' seam build and the stand-in collective (tests/rccl_stub; both ranks share
device 0).  The rank creates its plan with Engine.plan_from_seed_job(rp64=True) -- the stream of the JOB of 4 workers from
the seed every rank is given, the lists of the K_LOCAL workers hosted here -- and runs it as ONE collective plan_run.
usage: python seed_job_world2_worker.py <rank> <world> <workdir>

Also the test's shared construction: the job, the seed, the starting weights, the learning rate."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dsgd_amd  # noqa: E402
from dsgd_amd import host  # noqa: E402
from fp64_rank_plans_worker import float_w0  # noqa: E402
from world2_common import CFG, shard_of, split_range  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402

WORLD, K_LOCAL = 2, 2
N_STEPS, BATCH = 6, 16
LR = 0.25
STATE0 = host.JavaRandom(4711).seed


def job_splits():
    """the job's 4 workers in the master's order (rank-major): every rank's train rows cut in K_LOCAL, as GLOBAL row ranges"""
    out = []
    for r in range(WORLD):
        lo, hi = split_range(0, CFG["n_train"], r, WORLD)
        out += [split_range(lo, hi, j, K_LOCAL) for j in range(K_LOCAL)]
    return out


def main():
    rank, world, wd = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    assert world == WORLD
    assert os.environ.get("DSGD_RCCL_LIB"), "the worker must run with the shim selected explicitly"
    assert os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so"), "... through the tests' seam build of the library"
    data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    sh = shard_of(data, CFG["n_train"], rank, world)
    splits = job_splits()
    job_lens = [b - a for a, b in splits]
    begins = [a - sh.train_lo for a, _ in splits[rank * K_LOCAL:(rank + 1) * K_LOCAL]]   # where the hosted splits start HERE
    out = {}
    with dsgd_amd.Engine(data.dim, CFG["lam"], device=0, precision="fp64") as eng:
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val.astype(np.float32), sh.csr.label)
        eng.comm_init_f64(exchange_uid(wd, "uid_1.bin", rank, dsgd_amd.Engine.comm_unique_id), world, rank)
        eng.build_dim_sparsity(sh.n_train)
        eng.set_weights(float_w0(data.dim))
        plan, n_steps, state, draws = eng.plan_from_seed_job(STATE0, job_lens, rank * K_LOCAL, begins, N_STEPS * BATCH, BATCH, rp64=True)
        out["n_steps"], out["state"], out["draws"] = np.asarray(n_steps), np.asarray(state, dtype=np.uint64), np.asarray(draws)
        idx, offs = eng.plan_lists(plan)
        out["idx_global"], out["offs"] = idx.astype(np.int64) + sh.train_lo, offs
        eng.plan_run(plan, 0, n_steps, LR)
        st = eng.synchronize()
        out["w"] = eng.get_weights()
        out["stats"] = np.asarray([st["n_samples"], st["n_active"]])
        out["kernel"] = np.asarray(eng.grad_kernel_name())
        plan.destroy()
        eng.comm_destroy()
    np.savez(os.path.join(wd, "out_%d.npz" % rank), **out)
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
