"""-m gpu, needs >= 2 visible gfx950 devices (skipped otherwise, as tests/test_gpu_fp64_rccl_multi.py): row-parallel fp64
plans under a communicator over REAL RCCL, one process and one device per rank, the product library.  The float legs of
tests/test_gpu_fp64_rank_plans.py: the plan as ONE call and cut in three gives, on both replicas, the bits of the loop of
sync_step_f64 calls under the same communicator, and the job's statistics."""

import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
from fp64_rank_plans_worker import CUTS, N_STEPS, WORLD
from fp64_world2_worker import bits


def n_devices():
    try:
        return dsgd_amd.device_count()
    except Exception:
        return 0


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(n_devices() < 2, reason="needs two gfx950 devices (real RCCL refuses two ranks on one)")]

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def two_processes(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("fp64_rank_plans_rccl2"))
    env = {k: v for k, v in os.environ.items() if k not in ("DSGD_LIB_PATH", "DSGD_RCCL_LIB")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fp64_rank_plans_worker.py"), str(r), str(WORLD), wd, "float", "--real"],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(WORLD)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-4000:])
    return [dict(np.load(os.path.join(wd, "out_%d.npz" % r))) for r in range(WORLD)]


@pytest.mark.parametrize("tag", ["k2", "k1"])
def test_plan_runs_bit_equal_to_the_per_step_loop_over_real_rccl(two_processes, tag):
    r0, r1 = two_processes
    loop = r0[tag + "_loop_w"]
    assert loop.shape[0] == N_STEPS and np.array_equal(bits(loop), bits(r1[tag + "_loop_w"]))
    for r in (r0, r1):
        assert np.array_equal(bits(r[tag + "_one_w"][0]), bits(loop[-1]))
        for (a, b), w in zip(CUTS, r[tag + "_cut_w"]):
            assert np.array_equal(bits(w), bits(loop[b - 1])), (a, b)
        assert r[tag + "_one_stats"].tolist() == r[tag + "_cut_stats"].tolist() == r[tag + "_loop_stats"].tolist()
    assert np.abs(loop[-1] - loop[0]).max() > 0
