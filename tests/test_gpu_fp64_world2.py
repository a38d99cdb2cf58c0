"""-m gpu: the fp64 mode across ranks (dsgd_comm_init_f64; include/dsgd.h "ACROSS RANKS") -- two rank
processes on ONE device through the tests' seam build and the stand-in collective (tests/rccl_stub), as
tests/test_gpu_world2.py does for fp32.  Every worker's exact integer column sums are gathered on every rank and folded
by the single-context finish, so nothing here needs a tolerance: after every step the replicas hold the same bits, and
those are the bits of ONE fp64 context over all the rows stepping the same K = k x world lists.  The oracle comparison is
the single context's own criterion (tests/test_gpu_fp64_requests.py), taken as it stands.  Nothing here is a timing:
the stand-in stages through host memory."""

import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib
from fp64_world2_worker import N_STEPS, SLICED_AT, bits, code_of, step_lists
from oracle import oracle as orc
from test_rccl_stub import seam_env
from world2_common import CFG, shard_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
WORLD = 2


def run_ranks(wd, mode, timeout=900):
    """the rank processes, each under its time limit; a rank that failed ends the test (nothing more is started)"""
    env = seam_env()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fp64_world2_worker.py"), str(r), str(WORLD), wd, mode], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(WORLD)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-4000:])
    return [dict(np.load(os.path.join(wd, "out_%d.npz" % r))) for r in range(WORLD)]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("fp64_world2")), "steps")


@pytest.fixture(scope="module")
def problem():
    data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, CFG["lam"])
    o.set_dim_sparsity(o.dim_sparsity(CFG["n_train"]))
    shards = [shard_of(data, CFG["n_train"], r, WORLD) for r in range(WORLD)]
    return data, o, shards


def single_engine(data):
    eng = dsgd_amd.Engine(data.dim, CFG["lam"], precision="fp64")
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(CFG["n_train"])
    return eng


def global_step(shards, i):
    """step i's K = k x world lists in the global worker order (rank-major), row indices shifted to global, and its lr"""
    glob, lr = [], None
    for r, sh in enumerate(shards):
        lists, lr = step_lists(r, i, sh.n_train)
        glob += [(l.astype(np.int64) + sh.train_lo).astype(np.int32) for l in lists]
    return glob, (lr if i % 2 else float(np.float32(lr)))   # (even steps go through the float entry point)


def _scale(v):
    return max(1.0, float(np.abs(v).max()))


def test_one_ranking_one_dim_sparsity(ranks, problem):
    data, o, shards = problem
    np.testing.assert_array_equal(ranks[0]["ranks"], ranks[1]["ranks"])
    assert ranks[0]["ds"].dtype == np.float64
    assert np.array_equal(bits(ranks[0]["ds"]), bits(ranks[1]["ds"]))
    assert np.array_equal(bits(ranks[0]["ds"]), bits(np.asarray(o.dim_sparsity(CFG["n_train"]), dtype=np.float64)))
    with single_engine(data) as eng:
        assert np.array_equal(bits(eng.get_dim_sparsity()), bits(ranks[0]["ds"]))
        np.testing.assert_array_equal(eng.column_ranks(), ranks[0]["ranks"])


def test_steps_bit_equal_on_the_replicas_and_to_one_context(ranks, problem):
    data, o, shards = problem
    assert ranks[0]["w_hist"].shape == (N_STEPS, data.dim + 1) and ranks[0]["w_hist"].dtype == np.float64
    ks = set()
    with single_engine(data) as single:
        for i in range(N_STEPS):
            lists, lr = global_step(shards, i)
            ks.add(len(lists) // WORLD)
            st = single.sync_step_f64(lists, lr)
            w1 = single.get_weights()
            for r in range(WORLD):
                assert np.array_equal(bits(ranks[r]["w_hist"][i]), bits(w1)), "step %d: rank %d differs from the single context" % (i, r)
                assert ranks[r]["stats"][i].tolist() == [st["n_samples"], st["n_active"]], (i, r)
            assert st["n_samples"] == sum(len(l) for l in lists)
    assert {1, 2} <= ks
    assert np.abs(ranks[0]["w_hist"][-1]).max() > 0


def test_steps_against_the_oracle(ranks, problem):
    data, o, shards = problem
    w_o = np.zeros(data.dim + 1)
    for i in range(N_STEPS):
        lists, lr = global_step(shards, i)
        o.sync_step(w_o, lists, lr)
        assert int(ranks[0]["stats"][i][1]) == o.last_stats["n_active"], i
    w = ranks[0]["w_hist"][-1]
    assert np.abs(w - w_o).max() <= 1e-12 * _scale(w_o)


def test_evaluation_is_the_jobs_on_every_rank(ranks, problem):
    data, o, shards = problem
    assert np.array_equal(bits(ranks[0]["eval"]), bits(ranks[1]["eval"]))
    with single_engine(data) as single:
        single.set_weights(ranks[0]["w_hist"][-1])
        l_tr, a_tr, c_tr = single.loss_acc(0, CFG["n_train"])
        l_te, a_te, c_te = single.loss_acc(CFG["n_train"], data.n_rows)
    want = np.asarray([l_tr, a_tr] + list(c_tr) + [l_te, a_te] + list(c_te), dtype=np.float64)
    assert np.array_equal(bits(want), bits(ranks[0]["eval"])), (want, ranks[0]["eval"])


def test_refusals_and_the_local_step_after_comm_destroy(ranks, problem):
    data, o, shards = problem
    for r in range(WORLD):
        assert ranks[r]["refused"].tolist() == [_lib.EUNSUPPORTED] * 3
        assert bool(ranks[r]["refused_w_same"])
    with single_engine(data) as single:   # (no communicator; the ranking, vexp and dimSparsity the ranks agreed on)
        for r, sh in enumerate(shards):
            lists, lr = step_lists(r, 3, sh.n_train)
            single.set_weights(ranks[r]["w_local_from"])
            st = single.sync_step_f64([(l.astype(np.int64) + sh.train_lo).astype(np.int32) for l in lists], lr)
            assert np.array_equal(bits(single.get_weights()), bits(ranks[r]["w_local"]))
            assert ranks[r]["stats_local"].tolist() == [st["n_samples"], st["n_active"]]
        uid = b"\0" * _lib.UNIQUE_ID_BYTES
        assert code_of(lambda: single.comm_init(uid, 1, 0)) == _lib.EUNSUPPORTED   # (the fp32 entry point: as before)
    with dsgd_amd.Engine(data.dim, CFG["lam"]) as e32:
        assert code_of(lambda: e32.comm_init_f64(uid, 1, 0)) == _lib.ESTATE


def test_ranks_that_disagree_on_the_workers_get_einval(tmp_path):
    out = run_ranks(str(tmp_path), "mismatch", timeout=600)
    for r in range(WORLD):
        assert int(out[r]["code"]) == _lib.EINVAL
        assert bool(out[r]["w_same"])
    # ... and the next step, agreed, runs from a clean buffer: the replicas' bits, the job's statistics
    assert np.array_equal(bits(out[0]["w_after"]), bits(out[1]["w_after"]))
    assert out[0]["stats_after"].tolist() == out[1]["stats_after"].tolist() and int(out[0]["stats_after"][0]) == 400


def test_negative_control_the_fold_order_shows(ranks, problem):
    """the bit comparison can fail: workers 0 and 3 of the K = 4 step swapped in the single context (their sums are the
    same integers, the fold adds them in another order) gives other bits"""
    data, o, shards = problem
    lists, lr = global_step(shards, SLICED_AT)
    assert len(lists) == 4
    swapped = [lists[3], lists[1], lists[2], lists[0]]
    w_from = ranks[0]["w_hist"][SLICED_AT - 1]
    # the oracle on the CPU says the fold does not commute for these inputs
    w_a, w_b = w_from.copy(), w_from.copy()
    o.sync_step(w_a, lists, lr)
    o.sync_step(w_b, swapped, lr)
    assert not np.array_equal(bits(w_a), bits(w_b))
    with single_engine(data) as single:
        single.set_weights(w_from)
        single.sync_step_f64(lists, lr)
        assert np.array_equal(bits(single.get_weights()), bits(ranks[0]["w_hist"][SLICED_AT]))
        single.set_weights(w_from)
        single.sync_step_f64(swapped, lr)
        assert not np.array_equal(bits(single.get_weights()), bits(ranks[0]["w_hist"][SLICED_AT]))


def test_real_rccl_world_1_equals_no_communicator():
    """the product library, no seam: ncclAllReduce(ncclInt64) of real RCCL on the hardware, one rank"""
    n_rows, n_train = 23149, 18519
    data = dsgd_amd.synth.generate(n_rows, seed=3)
    rng = np.random.default_rng(4)
    steps = [([rng.permutation(n_train)[:n].astype(np.int32) for n in sizes], lr)
             for sizes, lr in (((100, 100, 100), 0.5), ((700, 2000), 0.1), ((n_train,), 0.002), ((100, 130, 90, 100), 0.5))]
    res = []
    for attach in (False, True):
        with dsgd_amd.Engine(data.dim, CFG["lam"], precision="fp64") as eng:
            eng.load_csr(data.row_ptr, data.col, data.val, data.label)
            if attach:
                eng.comm_init_f64(dsgd_amd.Engine.comm_unique_id(), 1, 0)
            eng.build_dim_sparsity(n_train)
            hist = []
            for lists, lr in steps:
                st = eng.sync_step_f64(lists, lr)
                hist.append((bits(eng.get_weights()).copy(), st))
            ev = eng.loss_acc(0, n_train) + eng.loss_acc(n_train, n_rows)
            if attach:
                eng.comm_destroy()
            res.append((hist, ev))
    for (w0, st0), (w1, st1) in zip(res[0][0], res[1][0]):
        assert np.array_equal(w0, w1) and st0 == st1
    assert res[0][1] == res[1][1]
    assert res[0][0][-1][0].any()
