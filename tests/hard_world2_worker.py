"""One rank of tests/test_gpu_hard_values.py::test_fp64_two_ranks_with_different_vexp: an fp64 engine over its half of
the rows -- rank 0's values scaled by 2^10, rank 1's as they are -- attached with comm_init_f64 over the tests' seam build
and the stand-in collective (both ranks share device 0).
usage: python hard_world2_worker.py <rank> <world> <workdir>"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dsgd_amd  # noqa: E402
import hard_data as hd  # noqa: E402
from world2_common import shard_of  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402

LAM = 1e-5
STEPS = [((100,), 0.5), ((100, 100), 0.5), ((700, 300), 0.1), ((2000,), 0.02)]   # per rank: list lengths, lr


def union_data():
    """signed values; the train and test rows of rank 0 (shard_of's partition) times 2^10"""
    d = hd.build("signed").data
    val = d.val.copy()
    for lo, hi in ((0, hd.N_TRAIN // 2), (hd.N_TRAIN, hd.N_TRAIN + (hd.N_ROWS - hd.N_TRAIN) // 2)):
        val[d.row_ptr[lo]:d.row_ptr[hi]] = np.ldexp(val[d.row_ptr[lo]:d.row_ptr[hi]], 10)
    return dsgd_amd.synth.Csr(d.dim, d.row_ptr, d.col, val, d.label)


def step_lists(rank, i, ntl):
    rng = np.random.default_rng([41, rank, i])
    sizes, lr = STEPS[i]
    return [rng.permutation(ntl)[:n].astype(np.int32) for n in sizes], lr


def main():
    rank, world, wd = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    assert os.environ.get("DSGD_RCCL_LIB") and os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so")
    sh = shard_of(union_data(), hd.N_TRAIN, rank, world)
    w_hist, stats = [], []
    with dsgd_amd.Engine(sh.csr.dim, LAM, device=0, precision="fp64") as eng:
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val, sh.csr.label)
        eng.comm_init_f64(exchange_uid(wd, "uid_h.bin", rank, dsgd_amd.Engine.comm_unique_id), world, rank)
        eng.build_dim_sparsity(sh.n_train)
        eng.set_weights(np.ldexp(hd.build("signed").w, -5))
        for i in range(len(STEPS)):
            lists, lr = step_lists(rank, i, sh.n_train)
            st = eng.sync_step_f64(lists, lr)
            w_hist.append(eng.get_weights())
            stats.append([st["n_samples"], st["n_active"]])
        eng.comm_destroy()
    np.savez(os.path.join(wd, "out_%d.npz" % rank), w_hist=np.stack(w_hist), stats=np.asarray(stats), vexp=np.asarray(hd.vexp_of(sh.csr.val)))
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
