"""-m gpu: the logistic model across ranks (dsgd_comm_init_lg; include/dsgd.h "THE LOGISTIC MODEL", ACROSS RANKS) -- two rank
processes on ONE device through the tests' seam build and the stand-in collective (tests/rccl_stub), as
tests/test_gpu_fp64_world2.py does for the fp64 mode.  Every worker's exact integer column sums are gathered on every rank and
folded by the single context's finish arithmetic at the job's vexp, so nothing here needs a tolerance: after every step the
replicas hold the same bits, and those are the bits of ONE context over shard 0 || shard 1 stepping the same K = k x world
lists or ranges.  The comparison with the fp64 model is the single context's own derived bound (tests/logistic_bound.py: dw),
taken as it stands.  Nothing here is a timing: the stand-in stages through host memory."""

import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_hard_cases as hc
import logistic_ref as ref
from conftest import has_gpu
from dsgd_amd import _lib
from logistic_ranks_cases import S_ROWS, WIDTHS, concat, global_lists, job_op, op_steps, run_op, scenario
from logistic_ranks_worker import LOCAL_RANGES, bits, code_of, local_probe
from test_rccl_stub import seam_env

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
WORLD = 2


def run_ranks(wd, mode, timeout=300):
    """the rank processes, each under its time limit; a rank that failed ends the test (nothing more is started)"""
    env = seam_env()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "logistic_ranks_worker.py"), str(r), str(WORLD), wd, mode], env=env,
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
    return run_ranks(str(tmp_path_factory.mktemp("lg_ranks")), "steps")


@pytest.fixture(scope="module")
def synth():
    return scenario("steps")[0]


def single_engine(s):
    eng = dsgd_amd.Engine(s["dim"], s["lam"])
    eng.load_csr(*concat(s["shards"]))
    eng.set_weights(s["w0"])
    return eng


def check_set(out, tag, s):
    """after every op: both replicas and ONE context over the job's rows hold the same bits and report the job's rows"""
    kernels = []
    with single_engine(s) as single:
        np.testing.assert_array_equal(out[0][tag + "__ranks"], out[1][tag + "__ranks"])
        np.testing.assert_array_equal(out[0][tag + "__ranks"], single.column_ranks())
        for i, op in enumerate(s["ops"]):
            st, kern = run_op(single, job_op(op, s["rows_per_rank"]))
            w1 = single.get_weights()
            kernels.append(kern)
            for r in range(WORLD):
                assert np.array_equal(bits(out[r][tag + "__w_hist"][i]), bits(w1)), "%s op %d (%s): rank %d differs from the single context" % (
                    s["name"], i, op["kind"], r)
                assert out[r][tag + "__stats"][i].tolist() == st, (s["name"], i, r)
            assert st[0] == st[1] > 0
        assert np.count_nonzero(w1 != s["w0"]) > 0
    return kernels


def test_steps_bit_equal_on_the_replicas_and_to_one_context(ranks, synth):
    kernels = check_set(ranks, "synth", synth)
    kinds = [op["kind"] for op in synth["ops"]]
    assert kinds == ["lists", "lists", "lists", "ranges", "steps_ranges", "steps", "plan"]
    i = kinds.index("steps_ranges")
    for r in range(WORLD):   # the column lists ran, on the ranks as in the single context
        assert str(ranks[r]["synth__kernels"][i]) == "dsgd_lg_cgrad_kernel" == kernels[i]
        assert str(ranks[r]["synth__kernels"][kinds.index("ranges")]) == "dsgd_lg_grad_range_kernel"
    # the job's rows: both ranks' together (a multi-step call reports what the single context's call reports)
    assert ranks[0]["synth__stats"][0].tolist() == [200, 200] and ranks[0]["synth__stats"][3].tolist() == [2 * S_ROWS, 2 * S_ROWS]
    assert ranks[0]["synth__stats"][4].tolist() == [2 * S_ROWS, 2 * S_ROWS] and ranks[0]["synth__stats"][6].tolist() == [2000, 2000]


def test_final_weights_within_the_derived_bound_of_the_fp64_model(ranks, synth):
    job = concat(synth["shards"])
    w_ref = synth["w0"].astype(np.float64)
    E = np.zeros_like(w_ref)
    n = 0
    for op in synth["ops"]:
        for lists, lr in op_steps(op):
            lr = float(np.float32(lr))
            E = lb.dw(job, w_ref, lists, lr, synth["lam"], E)
            w_ref = ref.sync_step(job, w_ref, lists, lr, synth["lam"])
            n += 1
    assert n == 17
    err = np.abs(ranks[0]["synth__w_hist"][-1].astype(np.float64) - w_ref)
    print("17 steps: max err %.3e, max err/bound %.3f" % (float(err.max()), float(np.max(err / E))))
    assert np.all(err <= E)


def test_local_calls_under_the_communicator_are_the_shards_own(ranks, synth):
    """gradient, probabilities and the evaluation: the bits of a context without a communicator on the same shard and weights.
    (The loss is asked on weights of the grid 2^-10: its lambda |w|^2 term is summed in rank order, the ranking under the
    communicator is the job's and not the shard's, and on the grid that sum is exact in any order.)"""
    for r in range(WORLD):
        with dsgd_amd.Engine(synth["dim"], synth["lam"]) as eng:
            eng.load_csr(*synth["shards"][r])
            g, ev, p, st = local_probe(eng, ranks[r]["synth__w_hist"][-1])
        assert np.array_equal(bits(g), bits(ranks[r]["local_g"])) and np.array_equal(bits(p), bits(ranks[r]["local_p"]))
        assert np.array_equal(ev.view(np.uint64), ranks[r]["local_eval"].view(np.uint64)), (ev, ranks[r]["local_eval"])
        assert st.tolist() == ranks[r]["local_stats"].tolist() == [300, 300]
        assert ev.shape == (len(LOCAL_RANGES), 2) and np.all(ev[:, 0] > 0)
    assert not np.array_equal(bits(ranks[0]["local_g"]), bits(ranks[1]["local_g"]))   # (the shards' own figures, not the job's)


def test_refusals_the_local_step_after_comm_destroy_and_plain_comm_init(ranks, synth):
    for r in range(WORLD):
        assert ranks[r]["refused"].tolist() == [_lib.EUNSUPPORTED] * 4
        assert bool(ranks[r]["refused_w_same"])
        with dsgd_amd.Engine(synth["dim"], synth["lam"]) as eng:   # a context that never had a communicator
            eng.load_csr(*synth["shards"][r])
            eng.set_weights(ranks[r]["w_local_from"])
            st = eng.lg_sync_step([ranks[r]["local_lists_0"], ranks[r]["local_lists_1"]], 0.5)
            assert np.array_equal(bits(eng.get_weights()), bits(ranks[r]["w_local"]))
            assert ranks[r]["stats_local"].tolist() == [st["n_samples"], st["n_active"]] == [137, 137]
        assert int(ranks[r]["plain_code"]) == _lib.EUNSUPPORTED and bool(ranks[r]["plain_w_same"])
    with dsgd_amd.Engine(synth["dim"], synth["lam"], precision="fp64") as e64:
        assert code_of(lambda: e64.comm_init_lg(b"\0" * _lib.UNIQUE_ID_BYTES, 1, 0)) == _lib.EUNSUPPORTED
    with dsgd_amd.Engine(synth["dim"], synth["lam"]) as e32:
        assert code_of(lambda: e32.comm_init_lg(b"\0" * _lib.UNIQUE_ID_BYTES, 65, 0)) == _lib.EUNSUPPORTED
        assert code_of(lambda: e32.comm_init_lg(b"\0" * _lib.UNIQUE_ID_BYTES, 2, 2)) == _lib.EINVAL


def test_ranks_with_their_own_vexp_and_the_negative_control(tmp_path):
    """the job's largest value lies on rank 1 only: the ranks' own vexp differ, the weights are the single context's all the
    same.  On these inputs the order of the fold shows in the float weights (tests/logistic_ranks_cases.py): workers 0 and 3
    swapped in the single context give other bits -- the comparison above can fail."""
    s = scenario("cancel")[0]
    assert lb.vexp_of(s["shards"][0][2]) < lb.vexp_of(s["shards"][1][2]) == 40
    out = run_ranks(str(tmp_path), "cancel")
    check_set(out, "set0", s)
    job, lists, lr = concat(s["shards"]), global_lists(s["ops"][0]["per_rank"], s["rows_per_rank"]), s["ops"][0]["lr"]
    swapped = [lists[3], lists[1], lists[2], lists[0]]
    # the emulation on the CPU says the fold does not commute for these inputs, and agrees with the ranks
    w_a, w_b = lb.emu_step(job, s["w0"], lists, lr, s["lam"]), lb.emu_step(job, s["w0"], swapped, lr, s["lam"])
    assert not np.array_equal(bits(w_a), bits(w_b))
    assert np.array_equal(bits(w_a), bits(out[0]["set0__w_hist"][0]))
    with single_engine(s) as single:
        single.lg_sync_step(swapped, lr)
        assert not np.array_equal(bits(single.get_weights()), bits(out[0]["set0__w_hist"][0]))
        assert np.array_equal(bits(single.get_weights()), bits(w_b))


def test_widths(tmp_path):
    """dp = 2, 256, 2,048 and 2,049 (the LDS head's edge, the last column) and dp = 319 = 63 (mod 64) (the stride's padding)"""
    sets = scenario("widths")
    assert [s["dim"] for s in sets] == list(WIDTHS) and (WIDTHS[-1] + 1) % 64 == 63
    out = run_ranks(str(tmp_path), "widths")
    for i, s in enumerate(sets):
        kernels = check_set(out, "set%d" % i, s)
        assert kernels[-1] in ("dsgd_lg_cgrad_kernel", "dsgd_lg_grad_range_kernel")
        if s["dim"] in hc.W_EDGE_RANKS:   # the columns on the edges moved
            rank_of = out[0]["set%d__ranks" % i]
            moved = out[0]["set%d__w_hist" % i][0] != s["w0"]
            for edge in hc.W_EDGE_RANKS[s["dim"]]:
                assert moved[int(np.where(rank_of == edge)[0][0])], (s["dim"], edge)


def test_a_column_sum_of_2_to_the_62_crosses_the_gather(tmp_path):
    s = scenario("exact")[0]
    out = run_ranks(str(tmp_path), "exact")
    check_set(out, "set0", s)
    job = concat(s["shards"])
    op = s["ops"][0]
    lists = global_lists(op["per_rank"], s["rows_per_rank"])
    want = hc.exact_step(job, s["w0"], lists, op["lr"])
    assert np.array_equal(bits(want), bits(out[0]["set0__w_hist"][0]))
    acc, S = lb.emu_acc(s["shards"][1], s["w0"], op["per_rank"][1][0])
    assert S == 50 and int(acc[hc.E_F]) == -(1 << 62)   # what rank 1's slot holds on the shared column


def test_ranks_that_disagree_get_einval(tmp_path):
    out = run_ranks(str(tmp_path), "mismatch")
    for r in range(WORLD):
        assert int(out[r]["code"]) == _lib.EINVAL and bool(out[r]["w_same"])              # 1 + r workers
        assert int(out[r]["code_steps"]) == _lib.EINVAL and bool(out[r]["w_same_steps"])  # 2 - r steps
    # ... and the next step, agreed, runs from a clean buffer: the replicas' bits, the job's rows
    assert np.array_equal(bits(out[0]["w_after"]), bits(out[1]["w_after"]))
    assert out[0]["stats_after"].tolist() == out[1]["stats_after"].tolist() == [400, 400]
    s = scenario("steps")[0]
    rngs = [np.random.default_rng(300 + r) for r in range(WORLD)]
    lists = [[rngs[r].permutation(S_ROWS)[:200].astype(np.int32)] for r in range(WORLD)]
    with single_engine(s) as single:
        single.lg_sync_step(global_lists(lists, S_ROWS), 0.5)
        assert np.array_equal(bits(single.get_weights()), bits(out[0]["w_after"]))


def test_real_rccl_world_1_equals_no_communicator(synth):
    """the product library, no seam: ncclAllReduce(ncclInt64) of real RCCL on the hardware, one rank"""
    res = []
    for attach in (False, True):
        with dsgd_amd.Engine(synth["dim"], synth["lam"]) as eng:
            eng.load_csr(*synth["shards"][0])
            eng.set_weights(synth["w0"])
            if attach:
                eng.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)
            hist = []
            for op in synth["ops"]:
                one = dict(op, per_rank=op["per_rank"][:1])
                st, kern = run_op(eng, dict(one, args=one["per_rank"][0]))
                hist.append((bits(eng.get_weights()).copy(), st, kern))
            ev = eng.lg_loss_acc_ranges(LOCAL_RANGES)
            if attach:
                eng.comm_destroy()
            res.append((hist, ev))
    for (w0, st0, k0), (w1, st1, k1) in zip(res[0][0], res[1][0]):
        assert np.array_equal(w0, w1) and st0 == st1 and k0 == k1
    assert res[0][1] == res[1][1]
    assert res[0][0][-1][0].any()
