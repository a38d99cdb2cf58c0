"""-m gpu: Master.fit of the logistic model across ranks (include/dsgd.h "THE LOGISTIC MODEL", ACROSS RANKS:
dsgd_plan_create_from_seed_job_lg, dsgd_lg_eval_job; host.LogisticSync(ranks=...)) -- two rank processes on ONE device through the
tests' seam build and the stand-in collective (tests/rccl_stub), as tests/test_gpu_logistic_ranks.py, plus one single-context
reference in this process.  Integers and whole fp64 words cross the ranks, so every equality here is on BITS: a rank's lists are
the windows of csrc/jrand.c's lists over the job; the weights behind a collective run are those of ONE context over the ranks'
rows; lg_eval_job's counts, per-range losses, loss and accuracy are those of lg_predict_ranges on that context.  Nothing here is
a timing.  Real RCCL runs at world = 1 only (the last test); with more than one rank it has never run here."""

import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
import logistic_job_worker as jw
from conftest import has_gpu
from dsgd_amd import _lib, host
from logistic_ranks_cases import _width_set, concat
from logistic_ranks_worker import bits, code_of, grid_weights
from test_rccl_stub import seam_env

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
WORLD = jw.WORLD
SHARD = jw.SHARD


def run_ranks(wd, mode, timeout=240):
    """the rank processes, each under its time limit; a rank that failed ends the test (nothing more is started)"""
    env = seam_env()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "logistic_job_worker.py"), str(r), str(WORLD), wd, mode], env=env,
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


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def job():
    csr, dim = jw.job_data()
    return csr, dim, jw.start_weights(dim)


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("lg_job")), "main")


@pytest.fixture(scope="module")
def single(job):
    """ONE context that holds the ranks' rows concatenated in rank order"""
    csr, dim, _ = job
    with dsgd_amd.Engine(dim, jw.LAM) as eng:
        eng.load_csr(*concat([jw.shard(csr, r) for r in range(WORLD)]))
        yield eng


def concat_split(K):
    """the job's K workers as row ranges of the single context (rank r's rows start at r * SHARD)"""
    out = []
    for r in range(WORLD):
        lens, _, begins, _ = jw.local_layout(K, r)
        k = K // WORLD
        out += [(r * SHARD + begins[j], r * SHARD + begins[j] + lens[r * k + j]) for j in range(k)]
    return out


def global_ranges(per_rank):
    return [(a + r * SHARD, b + r * SHARD) for r, rs in enumerate(per_rank) for a, b in rs]


def assert_eval_equal(out, key, want, what):
    """a rank's lg_eval_job against lg_predict_ranges' (classes, proba, counts, range_loss, loss, acc) of the single context"""
    assert np.array_equal(out[key + "__counts"], want[2]), what
    assert np.array_equal(u64(out[key + "__rl"]), u64(want[3])), (what, out[key + "__rl"], want[3])
    assert np.array_equal(u64(out[key + "__la"]), u64([want[4], want[5]])), (what, out[key + "__la"], want[4:])


# ---- 1. the lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,batch", jw.LIST_CASES)
def test_a_ranks_plan_is_its_window_of_the_jobs_lists(ranks, K, batch):
    split = host.split_vanilla(jw.N_TRAIN, K)
    rnd = host.JavaRandom(0)
    rnd.seed = jw.JSTATE
    idx, offs, n_steps = host.epoch_lists(rnd, split, max(len(g) for g in split), batch, native=True)   # csrc/jrand.c
    assert n_steps == len(range(0, len(split[0]), batch)) >= 3
    k = K // WORLD
    tag = "lists_%d_%d" % (K, batch)
    for r in range(WORLD):
        got_idx, got_offs, meta = ranks[r][tag + "__idx"], ranks[r][tag + "__offs"], ranks[r][tag + "__meta"]
        assert meta[0] == n_steps and meta[2] == rnd.seed and meta[3] == 1       # the job's steps and state; plan code 7
        assert meta.tolist() == ranks[0][tag + "__meta"].tolist()               # ... and draws: the same on both ranks
        assert len(got_offs) == n_steps * k + 1
        for s in range(n_steps):
            for j in range(k):
                g = s * K + r * k + j
                want = idx[offs[g]:offs[g + 1]] - r * (jw.N_TRAIN // WORLD)      # the job's rows as this rank's
                got = got_idx[got_offs[s * k + j]:got_offs[s * k + j + 1]]
                assert np.array_equal(got, want), (K, batch, r, s, j)


@pytest.mark.parametrize("K,batch", jw.LIST_CASES[:2])
def test_the_whole_job_hosted_here_is_the_plan_of_lg_plan_from_seed(single, K, batch):
    split = concat_split(K)
    lens = [b - a for a, b in split]
    p1, n1, s1, d1 = single.lg_plan_from_seed(jw.JSTATE, split, max(lens), batch)
    p2, n2, s2, d2 = single.lg_plan_from_seed_job(jw.JSTATE, lens, 0, [a for a, _ in split], max(lens), batch)
    try:
        assert (n1, s1, d1) == (n2, s2, d2) and n1 >= 3 and p2.info()["kind"] == "logistic"
        (i1, o1), (i2, o2) = single.plan_lists(p1), single.plan_lists(p2)
        assert np.array_equal(i1, i2) and np.array_equal(o1, o2) and p1.n_samples == p2.n_samples
    finally:
        p1.destroy()
        p2.destroy()


# ---- 2. a collective run of such a plan ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single_run(single, job):
    K, batch = jw.LIST_CASES[0]
    split = concat_split(K)
    single.set_weights(job[2])
    plan, n_steps, _, _ = single.lg_plan_from_seed(jw.JSTATE, split, max(b - a for a, b in split), batch)
    single.plan_run(plan, 0, jw.RUN_STEPS, jw.LR)
    st = single.synchronize()
    plan.destroy()
    return single.get_weights(), [st["n_samples"], st["n_active"]]


def test_five_collective_steps_leave_the_single_contexts_bits(ranks, single_run, job):
    w, st = single_run
    assert st == [jw.RUN_STEPS * 200] * 2 and np.count_nonzero(w != job[2]) > 0
    for r in range(WORLD):
        assert np.array_equal(bits(ranks[r]["w_run"]), bits(w)), r
        assert ranks[r]["run_stats"].tolist() == st


# ---- 3. the evaluation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["run", "grid", "zero"])
def test_eval_job_on_both_ranks_is_predict_ranges_on_one_context(ranks, single, single_run, weights):
    w_run = single_run[0]
    w = {"run": w_run, "grid": grid_weights(w_run), "zero": np.zeros_like(w_run)}[weights]
    shapes = [jw.range_sets(r) for r in range(WORLD)]
    for shape in ("n1", "n3", "n6"):
        want = single.lg_predict_ranges(global_ranges([shapes[r][shape] for r in range(WORLD)]), w=w)
        assert len(want[3]) == WORLD * int(shape[1:]) and want[2].sum() == sum(b - a for s in shapes for a, b in s[shape])
        for r in range(WORLD):
            assert_eval_equal(ranks[r], "eval_%s_%s" % (weights, shape), want, (weights, shape, r))


@pytest.fixture(scope="module")
def widths_out(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("lg_job_widths")), "widths")      # ONE pair of rank processes serves both widths


@pytest.mark.parametrize("dim", [1, 2048], ids=lambda d: "dp%d" % (d + 1))
def test_eval_job_at_the_models_edge_widths(widths_out, dim):
    out = widths_out
    s = _width_set(dim)
    half = s["rows_per_rank"]
    with dsgd_amd.Engine(s["dim"], s["lam"]) as eng:
        eng.load_csr(*concat(s["shards"]))
        want = eng.lg_predict_ranges([(a + r * half, b + r * half) for r in range(WORLD) for a, b in jw.width_ranges(half, r)], w=s["w0"])
    for r in range(WORLD):
        assert_eval_equal(out[r], "w%d" % dim, want, (dim, r))


def test_negative_control_the_order_of_the_fold_shows(tmp_path):
    """One range of ~2^5 (a saturated logit) beside ranges of ~2^-19: lg_eval_job has the single context's bits, which are the
    host's fold of the gathered per-range sums in POSITION order -- and on at least one of the weight settings (expected: nearly
    all) a rank-minor fold of the same sums has other bits.  Without that the equalities above would say nothing about order."""
    out = run_ranks(str(tmp_path), "order")
    shards = [jw.order_shard(r) for r in range(WORLD)]
    n0 = len(shards[0][0][3])
    ranges = shards[0][1] + [(a + n0, b + n0) for a, b in shards[1][1]]
    rows = np.asarray([b - a for a, b in ranges], dtype=np.float64)
    K, k = len(ranges), jw.ORDER_K
    sensitive = 0
    with dsgd_amd.Engine(3, 0.0) as eng:
        eng.load_csr(*concat([s[0] for s in shards]))
        for i, a in enumerate(jw.ORDER_A):
            want = eng.lg_predict_ranges(ranges, w=jw.order_weights(a))
            for r in range(WORLD):
                assert_eval_equal(out[r], "order%d" % i, want, (a, r))
            sums = want[3] * rows      # lambda = 0, rows a power of two: the ranges' sums, exactly
            assert 2.0 ** -22 < sums[0] < 2.0 ** -17 and 2.0 ** 4.9 < sums[k] < 2.0 ** 5.1, sums[[0, k]]
            in_position_order = rank_minor = 0.0
            for p in range(K):
                in_position_order += sums[p]
            for j in range(k):
                for r in range(WORLD):
                    rank_minor += sums[r * k + j]
            assert u64(in_position_order / rows.sum())[0] == u64(want[4])[0]
            sensitive += int(u64(rank_minor)[0] != u64(in_position_order)[0])
    print("rank-minor fold differs on %d of %d weight settings" % (sensitive, len(jw.ORDER_A)))
    assert sensitive >= 1


# ---- 4. the state -------------------------------------------------------------------------------------------------------------
def test_a_step_a_gradient_and_a_loss_behind_eval_job_keep_their_bits(ranks):
    for r in range(WORLD):
        assert ranks[r]["state_same"].tolist() == [True, True, True] and bool(ranks[r]["state_moved"])


def test_eval_job_without_a_communicator_is_predict_ranges(single, single_run):
    ranges = global_ranges([jw.range_sets(r)["n6"] for r in range(WORLD)])
    for w in (None, grid_weights(single_run[0])):
        want = single.lg_predict_ranges(ranges, w=w)
        counts, rl, loss, acc = single.lg_eval_job(ranges, w=w)
        assert np.array_equal(counts, want[2]) and np.array_equal(u64(rl), u64(want[3])) and u64([loss, acc]).tolist() == u64(want[4:]).tolist()


# ---- 5. refusals and mismatch -----------------------------------------------------------------------------------------------------
def test_ranks_that_disagree_get_einval_and_the_refusals(tmp_path, single, job):
    out = run_ranks(str(tmp_path), "mismatch")
    w0 = job[2]
    want = single.lg_predict_ranges([(0, 100), (100, 300), (SHARD, SHARD + 100), (SHARD + 100, SHARD + 300)], w=w0)
    many = single.lg_predict_ranges([(i + r * SHARD, i + 1 + r * SHARD) for r in range(WORLD) for i in range(128)], w=w0)
    for r in range(WORLD):
        assert int(out[r]["code"]) == _lib.EINVAL and bool(out[r]["w_same"])       # n_local 1 against 2
        assert_eval_equal(out[r], "after", want, ("the next call, agreed", r))
        assert int(out[r]["code_many"]) == _lib.EINVAL                              # K = 258
        assert_eval_equal(out[r], "k256", many, ("K = 256", r))
        assert out[r]["limit"].tolist() == [_lib.EUNSUPPORTED, 1, 1]                # a job_len of 2^20 + 1: *jstate untouched, no plan
        assert out[r]["plain"].tolist() == [_lib.EUNSUPPORTED, _lib.EUNSUPPORTED, 1, 1, 1]   # dsgd_comm_init: refused, nothing changed


def test_refused_contexts(job):
    csr, dim, w0 = job
    small = jw.take_rows(csr, np.arange(600))
    lens, begins = [300, 300], [0, 300]
    with dsgd_amd.Engine(dim, jw.LAM, precision="fp64") as eng:    # an fp64 context
        eng.load_csr(*small)
        assert code_of(lambda: eng.lg_eval_job([(0, 10)])) == _lib.EUNSUPPORTED
        assert jw.raw_job_plan(eng, lens, 0, begins, 300, 100)[0::2] == (_lib.EUNSUPPORTED, None)
    with dsgd_amd.Engine(dim, jw.LAM) as eng:                      # the lock-free engine running
        eng.load_csr(*small)
        eng.set_weights(w0)
        eng.build_dim_sparsity(600)
        eng.async_start([(0, 600)], batch=100, lr=0.5, max_updates=1 << 40, seed=1, positional_bug=True)
        try:
            assert code_of(lambda: eng.lg_eval_job([(0, 10)], w=np.ones_like(w0))) == _lib.ESTATE
        finally:
            eng.async_stop()
        assert eng.lg_eval_job([(0, 10)])[0].sum() == 10            # usable afterwards
    with dsgd_amd.Engine(dim, jw.LAM) as eng:                      # no data
        assert code_of(lambda: eng.lg_eval_job([(0, 10)])) == _lib.ESTATE


# ---- 6. the mirror --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_process(job):
    """host.LogisticSync.fit on ONE engine over the job's rows in their own order, and the single context's figures behind every
    epoch: lg_predict_ranges over the 4 train splits and over the 2 test slices"""
    csr, dim, w0 = job
    with dsgd_amd.Engine(dim, jw.LAM) as eng:
        eng.load_csr(*csr)
        m = host.LogisticSync(eng, jw.N_TRAIN, jw.N_ROWS, jw.MIRROR_K, rnd=host.JavaRandom(jw.MIRROR_SEED))
        w_hist = jw.record_epochs(m, eng, w0, jw.MIRROR_EPOCHS, jw.MIRROR_BATCH)
        train = [(g.start, g.stop) for g in host.split_vanilla(jw.N_TRAIN, jw.MIRROR_K)]
        test = [(jw.N_TRAIN + g.start, jw.N_TRAIN + g.stop) for g in host.split_vanilla(jw.N_ROWS - jw.N_TRAIN, WORLD)]
        figures = []
        for w in w_hist:
            a, b = eng.lg_predict_ranges(train, w=w), eng.lg_predict_ranges(test, w=w)
            figures.append([a[4], a[5], b[4], b[5]])
        return w_hist, np.asarray(figures[::-1]).T, m.rnd.seed, m.steps_run      # (the mirror keeps its figures newest first)


@pytest.mark.parametrize("mode", ["mirror", "mirror_host"])
def test_logistic_sync_across_ranks_is_the_one_process_fit(tmp_path, one_process, mode):
    w_hist, figures, seed, steps = one_process
    out = run_ranks(str(tmp_path), mode)
    assert len(w_hist) == jw.MIRROR_EPOCHS and not np.array_equal(bits(w_hist[0]), bits(w_hist[-1]))
    for r in range(WORLD):
        assert np.array_equal(bits(out[r]["w_hist"]), bits(w_hist)), (mode, r)          # after every epoch
        assert np.array_equal(u64(out[r]["figures"]), u64(figures)), (mode, r, out[r]["figures"], figures)
        assert out[r]["meta"].tolist() == [seed, steps, jw.MIRROR_EPOCHS if mode == "mirror" else 0]
    assert np.array_equal(u64(out[0]["figures"]), u64(out[1]["figures"]))               # every rank decides alike


# ---- 7. real RCCL at world = 1, the product library ---------------------------------------------------------------------------------
def test_real_rccl_world_1(job):
    """ncclAllReduce(ncclInt64) of real RCCL on the hardware, one rank: lg_eval_job is lg_predict_ranges, the job plan is
    lg_plan_from_seed's.  (Real RCCL with more than one rank has never run here.)"""
    csr, dim, w0 = job
    ranges = jw.range_sets(0)["n6"]
    split = [(0, 2000), (2000, 4000)]
    with dsgd_amd.Engine(dim, jw.LAM) as eng:
        eng.load_csr(*jw.shard(csr, 0))
        eng.set_weights(w0)
        want = eng.lg_predict_ranges(ranges)
        p1, n1, s1, d1 = eng.lg_plan_from_seed(jw.JSTATE, split, 2000, 100)
        lists1 = eng.plan_lists(p1)
        p1.destroy()
        eng.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        try:
            counts, rl, loss, acc = eng.lg_eval_job(ranges)
            p2, n2, s2, d2 = eng.lg_plan_from_seed_job(jw.JSTATE, [2000, 2000], 0, [0, 2000], 2000, 100)
            lists2 = eng.plan_lists(p2)
            eng.plan_run(p2, 0, 2, jw.LR)
            st = eng.synchronize()
            p2.destroy()
        finally:
            eng.comm_destroy()
    assert np.array_equal(counts, want[2]) and np.array_equal(u64(rl), u64(want[3])) and u64([loss, acc]).tolist() == u64(want[4:]).tolist()
    assert (n1, s1, d1) == (n2, s2, d2) and np.array_equal(lists1[0], lists2[0]) and np.array_equal(lists1[1], lists2[1])
    assert st["n_samples"] == 400
