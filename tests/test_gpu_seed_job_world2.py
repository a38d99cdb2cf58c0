"""-m gpu: a distributed epoch from a seed equals the single process's, with no host draw.  Two rank processes on ONE device
through the tests' seam build and the stand-in collective (tests/rccl_stub), as tests/test_gpu_fp64_rank_plans.py runs its
plans: a job of 4 workers, k = 2 per rank, 6 steps of batch 16 over the world2_common shards, float feature values.  Each
rank creates its row-parallel plan with Engine.plan_from_seed_job(rp64=True) from the same seed and runs it as one
collective plan_run.  The replicas are bit-equal to each other and to ONE detached fp64 context that holds all the rows
and runs plan_from_seed(rp64=True) over the four splits from that seed; every rank's generator state is that context's.
Nothing here has a tolerance and nothing is a timing (the stand-in stages through host memory).  Real RCCL with more than
one rank is not executed here."""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from fp64_rank_plans_worker import float_w0
from fp64_world2_worker import bits
from seed_job_world2_worker import BATCH, K_LOCAL, LR, N_STEPS, STATE0, WORLD, job_splits
from test_rccl_stub import seam_env
from world2_common import CFG

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
RANK_FAILED = []   # a rank failed or ran into its time limit: nothing more is started on the device by this module


def stop_after_a_failed_rank():
    if RANK_FAILED:
        pytest.fail("a rank failed earlier in this module: nothing more is started on the device")


def run_ranks(wd, timeout=240):
    """the rank processes, each under the time limit; a rank that failed ends its peer at once, ends the test and bars every
    later use of the device by this module"""
    stop_after_a_failed_rank()
    env = seam_env()
    logs = [open(os.path.join(wd, "log_%d.txt" % r), "w+") for r in range(WORLD)]
    procs = []
    why = None
    try:
        for r in range(WORLD):
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "seed_job_world2_worker.py"), str(r), str(WORLD), wd],
                                          env=env, stdout=logs[r], stderr=subprocess.STDOUT))
        deadline = time.monotonic() + timeout
        live = list(range(WORLD))
        while live and why is None:
            for r in list(live):
                try:
                    procs[r].wait(timeout=0.1)
                except subprocess.TimeoutExpired:
                    continue
                live.remove(r)
                if procs[r].returncode != 0:
                    why = "rank %d failed with exit status %d" % (r, procs[r].returncode)
                    break
            if why is None and live and time.monotonic() > deadline:
                why = "rank(s) %s ran into the time limit of %d s" % (live, timeout)
    except BaseException:
        RANK_FAILED.append(True)
        raise
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        outs = []
        for f in logs:
            f.seek(0)
            outs.append(f.read())
            f.close()
    if why is not None or len(procs) != WORLD:
        RANK_FAILED.append(True)
        pytest.fail("%s\n%s" % (why, "\n".join("--- rank %d ---\n%s" % (r, o[-4000:]) for r, o in enumerate(outs))))
    return [dict(np.load(os.path.join(wd, "out_%d.npz" % r))) for r in range(WORLD)]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("seed_job_world2")))


@pytest.fixture(scope="module")
def single(ranks):
    """ONE detached fp64 context over all the rows: plan_from_seed(rp64=True) over the job's four splits from the same seed"""
    stop_after_a_failed_rank()
    d = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    with dsgd_amd.Engine(d.dim, CFG["lam"], precision="fp64") as eng:
        eng.load_csr(d.row_ptr, d.col, d.val.astype(np.float32), d.label)
        eng.build_dim_sparsity(CFG["n_train"])
        eng.set_weights(float_w0(d.dim))
        plan, n_steps, state, draws = eng.plan_from_seed(STATE0, job_splits(), N_STEPS * BATCH, BATCH, rp64=True)
        idx, offs = eng.plan_lists(plan)
        eng.plan_run(plan, 0, n_steps, LR)
        st = eng.synchronize()
        out = {"w": eng.get_weights(), "stats": [st["n_samples"], st["n_active"]], "n_steps": n_steps, "state": state, "draws": draws,
               "idx": idx, "offs": offs, "w0": float_w0(d.dim)}
        plan.destroy()
    return out


def test_every_rank_leaves_with_the_single_process_generator(ranks, single):
    assert single["n_steps"] == N_STEPS and single["state"] != STATE0
    for r in ranks:
        assert int(r["n_steps"]) == N_STEPS and int(r["state"]) == single["state"] and int(r["draws"]) == single["draws"]


def test_the_ranks_hold_the_single_process_lists_of_their_workers(ranks, single):
    K = WORLD * K_LOCAL
    offs = single["offs"]
    for rank, r in enumerate(ranks):
        want = [single["idx"][offs[s * K + rank * K_LOCAL + i]:offs[s * K + rank * K_LOCAL + i + 1]] for s in range(N_STEPS) for i in range(K_LOCAL)]
        assert np.array_equal(r["idx_global"], np.concatenate(want)) and len(r["idx_global"]) == N_STEPS * K_LOCAL * BATCH


def test_the_distributed_epoch_is_the_single_process_epoch_bit_for_bit(ranks, single):
    r0, r1 = ranks
    assert r0["w"].dtype == np.float64 and np.array_equal(bits(r0["w"]), bits(r1["w"]))
    assert not np.array_equal(bits(r0["w"]), bits(single["w0"]))
    for r in ranks:
        assert np.array_equal(bits(r["w"]), bits(single["w"])), "differs from ONE context over all rows"
        assert r["stats"].tolist() == single["stats"] and single["stats"][0] == N_STEPS * WORLD * K_LOCAL * BATCH
        assert "gather_plan" in str(r["kernel"])
