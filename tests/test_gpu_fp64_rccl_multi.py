"""-m gpu, needs >= 2 visible gfx950 devices (skipped otherwise, as tests/test_gpu_rccl_multi.py): the fp64 mode across
ranks over REAL RCCL, one process and one device per rank, the product library.  The step sequence of
tests/test_gpu_fp64_world2.py: after every step the replicas hold the same bits, and those are the bits of ONE fp64
context over all the rows stepping the same K = k x world lists."""

import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
from fp64_world2_worker import N_STEPS, bits, step_lists
from world2_common import CFG, shard_of


def n_devices():
    try:
        return dsgd_amd.device_count()
    except Exception:
        return 0


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(n_devices() < 2, reason="needs two gfx950 devices (real RCCL refuses two ranks on one)")]

HERE = os.path.dirname(os.path.abspath(__file__))
WORLD = 2


@pytest.fixture(scope="module")
def two_processes(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("fp64_rccl2"))
    env = {k: v for k, v in os.environ.items() if k not in ("DSGD_LIB_PATH", "DSGD_RCCL_LIB")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fp64_world2_worker.py"), str(r), str(WORLD), wd, "steps", "--real"],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(WORLD)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=900)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-4000:])
    return [dict(np.load(os.path.join(wd, "out_%d.npz" % r))) for r in range(WORLD)]


def test_replicas_bit_equal_and_equal_to_one_context_over_real_rccl(two_processes):
    r0, r1 = two_processes
    assert np.array_equal(bits(r0["w_hist"]), bits(r1["w_hist"]))
    data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    shards = [shard_of(data, CFG["n_train"], r, WORLD) for r in range(WORLD)]
    with dsgd_amd.Engine(data.dim, CFG["lam"], precision="fp64") as single:
        single.load_csr(data.row_ptr, data.col, data.val, data.label)
        single.build_dim_sparsity(CFG["n_train"])
        for i in range(N_STEPS):
            lists, lr = [], None
            for r, sh in enumerate(shards):
                mine, lr = step_lists(r, i, sh.n_train)
                lists += [(l.astype(np.int64) + sh.train_lo).astype(np.int32) for l in mine]
            st = single.sync_step_f64(lists, lr if i % 2 else float(np.float32(lr)))
            assert np.array_equal(bits(single.get_weights()), bits(r0["w_hist"][i])), i
            assert r0["stats"][i].tolist() == r1["stats"][i].tolist() == [st["n_samples"], st["n_active"]]
    assert np.abs(r0["w_hist"][-1]).max() > 0
