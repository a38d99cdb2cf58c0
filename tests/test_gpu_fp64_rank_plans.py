"""-m gpu: row-parallel fp64 plans under a communicator (dsgd_plan_create_rp64_n accepted attached, dsgd_plan_run_f64 a
collective call; include/dsgd.h "ACROSS RANKS") -- two rank processes on ONE device through the tests' seam
build and the stand-in collective (tests/rccl_stub), as tests/test_gpu_fp64_world2.py runs its steps.  The ranks agree once
per call and then every step's integer column sums are gathered and folded by the single context's finish, so nothing here
has a tolerance except the comparison with oracle/ref_dict.py, which is tests/test_gpu_fp64_values.py's criterion
(1e-12 * max(1, |w|_inf), equal supports, equal active counts) taken as it stands.  The yardstick of every bit comparison
is the loop of sync_step_f64 calls under the same communicator.  Nothing here is a timing: the stand-in stages through
host memory.

The plans and the legs are tests/fp64_rank_plans_worker.py's: 12 steps per rank, k = 2 and k = 1, lists of 1, 16, 17 and
100 rows and one with a repeated row, lengths that differ between the ranks and between the workers of a step."""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib
from fp64_rank_plans_worker import CUTS, LR, N_STEPS, WORLD, float_w0, plan_steps
from fp64_world2_worker import bits
from fp64v_world2_worker import planted_global, start_weights, union_data
from oracle import ref_dict as rd
from test_gpu_fp64v_world2 import lo_words, vexp64
from test_rccl_stub import seam_env
from world2_common import CFG, shard_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
RP64_HOT = 1024   # csrc/dsgd_rp64.hpp: the column ranks summed in LDS
N_TRAIN = CFG["n_train"]


RANK_FAILED = []   # the first leg one of whose ranks failed or ran into its time limit: nothing more is started after it


def stop_after_a_failed_rank():
    """every leg and every test that would use the device asks here first"""
    if RANK_FAILED:
        pytest.fail("a rank of the '%s' leg failed earlier in this module: nothing more is started on the device" % RANK_FAILED[0])


def run_ranks(wd, mode, timeout=300):
    """the rank processes, each under the time limit; a rank that failed ends its peer at once, ends the test and bars every
    later leg of the module (nothing more is started)"""
    stop_after_a_failed_rank()
    env = seam_env()
    logs = [open(os.path.join(wd, "log_%d.txt" % r), "w+") for r in range(WORLD)]
    procs = []
    why = None
    try:
        for r in range(WORLD):
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "fp64_rank_plans_worker.py"), str(r), str(WORLD), wd, mode],
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
        RANK_FAILED.append(mode)
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
        RANK_FAILED.append(mode)
        pytest.fail("%s\n%s" % (why, "\n".join("--- rank %d ---\n%s" % (r, o[-4000:]) for r, o in enumerate(outs))))
    return [dict(np.load(os.path.join(wd, "out_%d.npz" % r))) for r in range(WORLD)]


@pytest.fixture(scope="module")
def float_ranks(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("fp64_rank_plans_float")), "float")


@pytest.fixture(scope="module")
def double_ranks(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("fp64_rank_plans_double")), "double")


class Problem:
    """all the rows, the starting weights and the K = k x world lists per step in the global worker order (rank-major), row
    indices shifted to global"""

    def __init__(self, kind):
        if kind == "synth":
            self.data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
            self.w0 = float_w0(self.data.dim)
        else:
            self.data, ab = union_data(kind)
            self.w0 = start_weights(self.data.dim, ab)
        self.planted = kind != "synth"
        self.shards = [shard_of(self.data, N_TRAIN, r, WORLD) for r in range(WORLD)]

    def global_steps(self, k):
        per_rank = [plan_steps(r, sh.n_train, k, planted=self.planted) for r, sh in enumerate(self.shards)]
        return [[(l.astype(np.int64) + sh.train_lo).astype(np.int32) for r, sh in enumerate(self.shards) for l in per_rank[r][t]]
                for t in range(N_STEPS)]

    def single(self, k, as_float32):
        """ONE detached fp64 context over all the rows: sync_steps_f64 on the K global lists -> (weights, [n_samples, n_active])"""
        stop_after_a_failed_rank()
        steps = self.global_steps(k)
        flat = np.concatenate([l for s in steps for l in s]).astype(np.int32)
        offs = np.concatenate([[0], np.cumsum([len(l) for s in steps for l in s])]).astype(np.int64)
        d = self.data
        with dsgd_amd.Engine(d.dim, CFG["lam"], precision="fp64") as eng:
            eng.load_csr(d.row_ptr, d.col, d.val.astype(np.float32 if as_float32 else np.float64), d.label)
            eng.build_dim_sparsity(N_TRAIN)
            eng.set_weights(self.w0)
            st = eng.sync_steps_f64(flat, offs, N_STEPS, k * WORLD, LR)
            return eng.get_weights(), [st["n_samples"], st["n_active"]]


@pytest.fixture(scope="module")
def synth():
    return Problem("synth")


def check_three_ways(ranks, tag, single_w, single_stats):
    """between the replicas, to the per-step loop under the same communicator, to one detached context over all rows"""
    r0, r1 = ranks
    loop = r0[tag + "_loop_w"]
    assert loop.shape[0] == N_STEPS and loop.dtype == np.float64
    assert np.array_equal(bits(loop), bits(r1[tag + "_loop_w"]))
    for r in ranks:
        assert np.array_equal(bits(r[tag + "_one_w"][0]), bits(loop[-1])), "ONE call differs from the per-step loop"
        for (a, b), w in zip(CUTS, r[tag + "_cut_w"]):
            assert np.array_equal(bits(w), bits(loop[b - 1])), "the call [%d, %d) differs from the per-step loop" % (a, b)
        assert np.array_equal(bits(r[tag + "_one_w"][0]), bits(single_w)), "differs from ONE context over all rows"
        assert r[tag + "_one_stats"].tolist() == r[tag + "_cut_stats"].tolist() == r[tag + "_loop_stats"].tolist() == single_stats
    assert not np.array_equal(bits(loop[-1]), bits(loop[0]))


def test_the_plans_cover_what_the_kernels_branch_on(float_ranks, synth):
    """asserted on the CPU: list lengths on both sides of the 16-row seam, a repeated row, lengths that differ between the ranks
    and between the workers of a step, columns below and above the ranks kept in LDS"""
    steps = synth.global_steps(2)
    lens = {len(l) for s in steps for l in s}
    assert {1, 16, 17, 100} <= lens
    assert any(len(np.unique(l)) < len(l) for s in steps for l in s)
    assert any(len({len(l) for l in s}) == 4 for s in steps)   # four lists of four lengths in one step: four shifts' worth
    assert any(len(s[0]) != len(s[1]) for s in steps) and any(len(s[0]) != len(s[2]) for s in steps)
    d = synth.data
    touched = np.unique(np.concatenate([d.col[d.row_ptr[r]:d.row_ptr[r + 1]] for s in steps for l in s for r in l]))
    col_rank = float_ranks[0]["ranks"][touched]
    assert col_rank.min() < RP64_HOT <= col_rank.max()


def test_float_data_k2_bits_three_ways(float_ranks, synth):
    """1: fails on the code before row-parallel plans ran under a communicator with DSGD_EUNSUPPORTED at plan creation"""
    w, st = synth.single(2, True)
    assert st[0] == sum(len(l) for s in synth.global_steps(2) for l in s)
    check_three_ways(float_ranks, "k2", w, st)
    assert str(float_ranks[0]["k2_kernel"]) == "dsgd_rp64_grad_gather_plan_kernel"
    assert int(float_ranks[0]["k2_value_bits"]) == 32


def test_float_data_k1_bits_three_ways(float_ranks, synth):
    """2: the reference's one worker per node"""
    w, st = synth.single(1, True)
    check_three_ways(float_ranks, "k1", w, st)
    assert not np.array_equal(bits(float_ranks[0]["k1_one_w"]), bits(float_ranks[0]["k2_one_w"]))


def _ref_problem(problem, steps):
    """oracle/ref_dict.py over the rows the steps touch; dimSparsity of ALL the train rows by Main.scala:54-65's rule"""
    d = problem.data
    dp = d.dim + 1
    data = [None] * d.n_rows
    for r in sorted({int(r) for s in steps for l in s for r in l}):
        s, e = int(d.row_ptr[r]), int(d.row_ptr[r + 1])
        data[r] = (rd.Sparse({int(c): float(v) for c, v in zip(d.col[s:e], d.val[s:e])}, dp), int(d.label[r]))
    e_train = int(d.row_ptr[N_TRAIN])
    keep = np.abs(d.val[:e_train]) > rd.EPS
    cnt = np.bincount((d.col[:e_train][keep].astype(np.int64) - 1) % dp, minlength=dp)
    return data, rd.SparseSVM(CFG["lam"], rd.Sparse({int(i): 1.0 / (int(c) + 1) for i, c in enumerate(cnt) if c != 0}, dp))


def test_double_data_bits_three_ways_and_the_planted_row(double_ranks):
    """3: comm_init_f64v on values with non-zero LO words; rank 1's planted row, whose gate flips when the values are rounded
    to float, follows oracle/ref_dict.py on the doubles; doubles a float holds give the float run's bits"""
    prob = Problem("double")
    steps = prob.global_steps(2)
    assert np.count_nonzero(lo_words(prob.data, steps[0], vexp64(prob.data.val))) > 0
    assert planted_global() in steps[0][2]   # rank 1's first list of step 0
    assert int(double_ranks[0]["dbl_value_bits"]) == 64
    assert str(double_ranks[0]["dbl_kernel"]) == "dsgd_rp64v_grad_gather_plan_kernel"
    w1, st1 = prob.single(2, False)
    check_three_ways(double_ranks, "dbl", w1, st1)
    # the planted row: inactive on the doubles, active once x is rounded to float
    data, model = _ref_problem(prob, steps)
    as_float = Problem("float")
    data32, _ = _ref_problem(as_float, steps)
    row = planted_global()
    w = rd.Sparse({int(j): float(prob.w0[j]) for j in np.flatnonzero(prob.w0)}, len(prob.w0))
    assert data[row][0].dot(w) == 2.0 ** -30 and data[row][1] == -1 and data32[row][0].dot(w) == 0.0
    active = lambda dd, ww, l: sum(1 for i in l if not (dd[i][1] * dd[i][0].dot(ww) < 0))   # noqa: E731
    assert sum(active(data, w, l.tolist()) for l in steps[0]) != sum(active(data32, w, l.tolist()) for l in steps[0])
    n_active = 0
    for s in steps:
        lists = [l.tolist() for l in s]
        n_active += sum(active(data, w, l) for l in lists)
        w = rd.master_sync_step(model, data, w, lists, LR)
    want = np.zeros(w.size)
    for j, v in w.map.items():
        want[j] = v
    got = double_ranks[0]["dbl_one_w"][0]
    assert int(double_ranks[0]["dbl_one_stats"][1]) == n_active
    assert np.array_equal(np.flatnonzero(got), np.flatnonzero(want))
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))
    # ... and it is not the float result; float-representable doubles under comm_init_f64v give the float run's bits
    for r in double_ranks:
        assert int(r["frep_value_bits"]) == 64 and int(r["f32_value_bits"]) == 32
        assert np.array_equal(bits(r["frep_w"]), bits(r["f32_w"])) and r["frep_stats"].tolist() == r["f32_stats"].tolist()
        assert not np.array_equal(bits(r["f32_w"]), bits(r["dbl_one_w"]))
    w32, st32 = as_float.single(2, True)
    assert np.array_equal(bits(double_ranks[0]["f32_w"][0]), bits(w32)) and double_ranks[0]["f32_stats"].tolist() == st32


def test_slice_major_weights_and_a_plan_made_detached(float_ranks):
    """4: the weights left slice-major by a column-slice plan; the row-parallel plan, created BEFORE attaching, reads and writes
    them there with test 1's bits -- and the plan made attached runs detached as a local plan does"""
    for r in float_ranks:
        assert np.array_equal(bits(r["sliced_w"]), bits(r["k2_one_w"]))
        assert r["sliced_stats"].tolist() == r["k2_one_stats"].tolist()
    # detached, the plan steps the rank's OWN k lists: other bits on the two ranks, its own rows in the statistics
    assert not np.array_equal(bits(float_ranks[0]["detached_w"]), bits(float_ranks[1]["detached_w"]))
    for rank, r in enumerate(float_ranks):
        assert int(r["detached_stats"][0]) == sum(len(l) for s in plan_steps(rank, 50000, 2) for l in s)


def test_what_stays_refused_under_the_communicator(float_ranks):
    """6: every call of the list keeps its code with the weights unchanged; a recorded plan is refused at its run"""
    for r in float_ranks:
        assert len(r["refused"]) == 11
        assert r["refused"].tolist() == [_lib.EUNSUPPORTED] * 11, dict(zip(r["refused_names"].tolist(), r["refused"].tolist()))
        assert int(r["recorded_code"]) == _lib.EUNSUPPORTED
        assert bool(r["refused_w_same"])


def test_ranks_that_disagree_get_einval_and_the_matched_run_follows(tmp_path, float_ranks):
    """5: (a) 1 + r hosted workers, (b) 3 + r steps, (c) float data on one rank and Double on the other under comm_init_f64v"""
    out = run_ranks(str(tmp_path), "mismatch")
    for rank, r in enumerate(out):
        for case, word in (("k", "hosted workers"), ("steps", "steps"), ("type", "feature values")):
            assert int(r[case + "_code"]) == _lib.EINVAL, (case, rank)
            assert bool(r[case + "_w_same"]), (case, rank)
            assert word in str(r[case + "_msg"]) and "rank %d" % (1 - rank) in str(r[case + "_msg"]), str(r[case + "_msg"])
            assert np.array_equal(bits(r[case + "_w_after"]), bits(float_ranks[rank]["k2_one_w"])), (case, rank)
            assert r[case + "_stats_after"].tolist() == float_ranks[rank]["k2_one_stats"].tolist(), (case, rank)


def test_real_rccl_world_1_equals_no_communicator():
    """7: the product library, no seam: real RCCL on the hardware, one rank; float data under comm_init_f64 and Double data
    under comm_init_f64v give the bits of the same plan with no communicator"""
    stop_after_a_failed_rank()
    n_rows, n_train = 23149, 18519
    base = dsgd_amd.synth.generate(n_rows, seed=3)
    rng = np.random.default_rng(78)
    dbl = base.val.astype(np.float64) * (1.0 + rng.random(len(base.val)) * 2.0 ** -20)
    steps = plan_steps(0, n_train, 2)
    w0 = float_w0(base.dim)
    for val, attach_name, vbits in ((base.val.astype(np.float32), "comm_init_f64", 32), (dbl, "comm_init_f64v", 64)):
        res = []
        for attach in (False, True):
            with dsgd_amd.Engine(base.dim, CFG["lam"], precision="fp64") as eng:
                eng.load_csr(base.row_ptr, base.col, val, base.label)
                assert eng.value_bits() == vbits
                if attach:
                    getattr(eng, attach_name)(dsgd_amd.Engine.comm_unique_id(), 1, 0)
                eng.build_dim_sparsity(n_train)
                eng.set_weights(w0)
                p = eng.plan(steps, rp64=True)
                eng.plan_run(p, 0, 5, LR)
                eng.plan_run(p, 5, 5, LR)   # (an empty run: the agreement and nothing else)
                eng.plan_run(p, 5, N_STEPS, LR)
                st = eng.synchronize()
                res.append((bits(eng.get_weights()).copy(), st, eng.grad_kernel_name()))
                p.destroy()
                if attach:
                    eng.comm_destroy()
        assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
        assert res[0][1]["n_samples"] == sum(len(l) for s in steps for l in s)
        assert "gather_plan" in res[1][2] and "gather" not in res[0][2]
        assert not np.array_equal(res[0][0], bits(w0))


def test_a_per_step_call_closes_the_statistics_window():
    """real RCCL, one rank: plan runs, then a sync_step_f64, then a synchronize on ONE engine.  The step reports its own rows
    and closes the window of the plan runs before it (include/dsgd.h "ACROSS RANKS", THE STATISTICS WINDOW): the synchronize
    behind it reports no rows a second time, the next plan run counts from zero, and the weights are those of the plan run
    uninterrupted (the step's lists are the plan's step 5)"""
    stop_after_a_failed_rank()
    n_rows, n_train = 23149, 18519
    base = dsgd_amd.synth.generate(n_rows, seed=3)
    steps = plan_steps(0, n_train, 2)
    rows = lambda a, b: sum(len(l) for s in steps[a:b] for l in s)   # noqa: E731
    w0 = float_w0(base.dim)
    res = []
    for interleave in (False, True):
        with dsgd_amd.Engine(base.dim, CFG["lam"], precision="fp64") as eng:
            eng.load_csr(base.row_ptr, base.col, base.val.astype(np.float32), base.label)
            eng.comm_init_f64(dsgd_amd.Engine.comm_unique_id(), 1, 0)
            eng.build_dim_sparsity(n_train)
            eng.set_weights(w0)
            p = eng.plan(steps, rp64=True)
            if interleave:
                eng.plan_run(p, 0, 5, LR)
                st_step = eng.sync_step_f64(steps[5], LR)
                assert st_step["n_samples"] == rows(5, 6)
                assert eng.synchronize()["n_samples"] == 0   # (the step's rows are not reported twice; the runs' window is closed)
                eng.plan_run(p, 6, N_STEPS, LR)
                st = eng.synchronize()
                assert st["n_samples"] == rows(6, N_STEPS)
                res.append((bits(eng.get_weights()).copy(), st["n_active"]))
            else:
                eng.plan_run(p, 0, 6, LR)
                eng.synchronize()
                eng.plan_run(p, 6, N_STEPS, LR)
                st = eng.synchronize()
                assert st["n_samples"] == rows(6, N_STEPS)
                res.append((bits(eng.get_weights()).copy(), st["n_active"]))
            p.destroy()
            eng.comm_destroy()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
