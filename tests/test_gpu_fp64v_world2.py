"""-m gpu: the fp64 mode across ranks on DOUBLE feature values (dsgd_comm_init_f64v; include/dsgd.h "ACROSS RANKS",
DESIGN.md 7.4) -- two rank processes on ONE device through the tests' seam build and the stand-in collective
(tests/rccl_stub), as tests/test_gpu_fp64_world2.py does for float values.  Both words of every worker's exact column sums
are gathered on every rank and folded by the single context's Double finish, so nothing here has a tolerance except the
comparison with oracle/ref_dict.py, which is tests/test_gpu_fp64_values.py's criterion (1e-12 * max(1, |w|_inf), equal
supports, equal active counts) taken as it stands.  Nothing here is a timing: the stand-in stages through host memory.

The data and the lists are tests/fp64v_world2_worker.py's: world2_common.CFG's synthetic rows with full 53-bit mantissas,
lists of 1, 16, 17 and 100 rows and one with a repeated row, k = 1 and k = 2 workers per rank."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib
from fp64_world2_worker import bits
from fp64v_world2_worker import LOCAL_STEP, N_STEPS, STEPS, WORLD, planted_global, start_weights, step_lists, union_data
from oracle import ref_dict as rd
from test_rccl_stub import seam_env
from world2_common import CFG, shard_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
RP64_HOT = 1024   # csrc/dsgd_rp64.hpp: the column ranks summed in LDS
N_TRAIN = CFG["n_train"]


def run_ranks(wd, mode, timeout=600):
    """the rank processes, each under its time limit; a rank that failed ends the test (nothing more is started)"""
    env = seam_env()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fp64v_world2_worker.py"), str(r), str(WORLD), wd, mode], env=env,
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
    return run_ranks(str(tmp_path_factory.mktemp("fp64v_world2")), "steps")


class Problem:
    """the union of the ranks' rows (kind: fp64v_world2_worker.union_data), the starting weights, and the steps' K = k x world
    lists in the global worker order (rank-major), row indices shifted to global"""

    def __init__(self, kind):
        self.data, self.ab = union_data(kind)
        self.w0 = start_weights(self.data.dim, self.ab)
        self.shards = [shard_of(self.data, N_TRAIN, r, WORLD) for r in range(WORLD)]

    def global_lists(self, i, rank=None):
        glob, lr = [], None
        for r, sh in enumerate(self.shards):
            if rank is None or r == rank:
                lists, lr = step_lists(r, i, sh.n_train)
                glob += [(l.astype(np.int64) + sh.train_lo).astype(np.int32) for l in lists]
        return glob, lr

    def engine(self, as_float=False):
        d = self.data
        eng = dsgd_amd.Engine(d.dim, CFG["lam"], precision="fp64")
        eng.load_csr(d.row_ptr, d.col, d.val.astype(np.float32) if as_float else d.val, d.label)
        eng.build_dim_sparsity(N_TRAIN)
        return eng

    def single_history(self):
        """ONE context over all the rows as doubles, the same K lists per step: (weights, [n_samples, n_active]) per step"""
        hist = []
        with self.engine() as eng:
            assert eng.value_bits() == 64
            eng.set_weights(self.w0)
            for i in range(N_STEPS):
                lists, lr = self.global_lists(i)
                st = eng.sync_step_f64(lists, lr)
                hist.append((eng.get_weights(), [st["n_samples"], st["n_active"]]))
        return hist


@pytest.fixture(scope="module")
def problem():
    return Problem("double")


@pytest.fixture(scope="module")
def single(problem):
    return problem.single_history()


def vexp64(val):
    """dsgd_load_csr_f64's vexp: the smallest e with max |x| <= 2^e"""
    m, e = math.frexp(float(np.abs(val).max()))
    return e - 1 if m == 0.5 else e


def lo_words(data, lists, vexp):
    """the LO words the two-word accumulator adds for the lists' entries: rn((v - floor(v)) * 2^32), v = x * 2^(S - vexp),
    S = 62 - ceil(log2 n) (every operation exact in Python floats: powers of two and differences below 2^53)"""
    out = []
    for l in lists:
        shift = 62 - (len(l) - 1).bit_length()
        for r in l:
            for x in data.val[data.row_ptr[r]:data.row_ptr[r + 1]]:
                v = math.ldexp(float(x), shift - vexp)
                out.append(round((v - math.floor(v)) * 2.0 ** 32))
    return np.asarray(out)


def ref_problem(problem, as_float=False):
    """oracle/ref_dict.py over the rows the steps touch (the others stay None: no step reads them); dimSparsity of ALL the
    train rows by Main.scala:54-65's rule (oracle/ref_dict.dim_sparsity, in numpy: buff(idx - 1) += 1, 1 / (count + 1))"""
    d = problem.data
    val = d.val.astype(np.float32).astype(np.float64) if as_float else d.val
    dp = d.dim + 1
    used = sorted({int(r) for i in range(N_STEPS) for l in problem.global_lists(i)[0] for r in l})
    data = [None] * d.n_rows
    for r in used:
        s, e = int(d.row_ptr[r]), int(d.row_ptr[r + 1])
        data[r] = (rd.Sparse({int(c): float(v) for c, v in zip(d.col[s:e], val[s:e])}, dp), int(d.label[r]))
    e_train = int(d.row_ptr[N_TRAIN])
    keep = np.abs(val[:e_train]) > rd.EPS
    cnt = np.bincount((d.col[:e_train][keep].astype(np.int64) - 1) % dp, minlength=dp)
    ds = rd.Sparse({int(i): 1.0 / (int(c) + 1) for i, c in enumerate(cnt) if c != 0}, dp)
    return data, rd.SparseSVM(CFG["lam"], ds)


def _sparse(w):
    return rd.Sparse({int(k): float(w[k]) for k in np.flatnonzero(w)}, len(w))


def _dense(sp):
    out = np.zeros(sp.size)
    for k, v in sp.map.items():
        out[k] = v
    return out


def _active(data, w, idx):
    return sum(1 for i in idx if not (data[i][1] * data[i][0].dot(w) < 0))


def test_the_steps_use_both_words_and_both_sides_of_the_hot_ranks(ranks, problem):
    """what the module exercises, asserted on the CPU: entries with a non-zero LO word at the steps' shifts, list lengths on
    both sides of the 16-row seam, k = 1 and k = 2, a repeated row, columns below and above the ranks kept in LDS"""
    d = problem.data
    vexp = vexp64(d.val)
    lens, ks, nonzero = set(), set(), 0
    touched = []
    for i in range(N_STEPS):
        lists, _ = problem.global_lists(i)
        ks.add(len(lists) // WORLD)
        lens |= {len(l) for l in lists}
        nonzero += int(np.count_nonzero(lo_words(d, lists, vexp)))
        touched += [d.col[d.row_ptr[r]:d.row_ptr[r + 1]] for l in lists for r in l]
    assert nonzero > 0
    assert {1, 16, 17, 100} <= lens and ks == {1, 2}
    assert any(len(np.unique(l)) < len(l) for i in range(N_STEPS) for l in problem.global_lists(i)[0])
    col_rank = ranks[0]["ranks"][np.unique(np.concatenate(touched))]
    assert col_rank.min() < RP64_HOT <= col_rank.max()
    assert planted_global() in problem.global_lists(0)[0][1]   # rank 1's list of step 0 holds the planted row
    assert int(ranks[0]["dbl_value_bits"]) == 64 and int(ranks[1]["dbl_value_bits"]) == 64


def test_steps_bit_equal_on_the_replicas_and_to_one_double_context(ranks, problem, single):
    """1: after every step both replicas hold the bits of ONE fp64 context with all the rows loaded as doubles; the
    statistics are the job's.  (The ranks loaded their doubles with the communicator attached: lifecycle 7.)"""
    np.testing.assert_array_equal(ranks[0]["ranks"], ranks[1]["ranks"])
    assert np.array_equal(bits(ranks[0]["dbl_ds"]), bits(ranks[1]["dbl_ds"]))
    assert ranks[0]["dbl_w_hist"].shape == (N_STEPS, problem.data.dim + 1) and ranks[0]["dbl_w_hist"].dtype == np.float64
    for i, (w1, st1) in enumerate(single):
        lists, _ = problem.global_lists(i)
        assert st1[0] == sum(len(l) for l in lists)
        for r in range(WORLD):
            assert np.array_equal(bits(ranks[r]["dbl_w_hist"][i]), bits(w1)), "step %d: rank %d differs from the single context" % (i, r)
            assert ranks[r]["dbl_stats"][i].tolist() == st1, (i, r)
    assert not np.array_equal(bits(single[-1][0]), bits(problem.w0))


def test_it_is_the_double_result_not_the_float_one(ranks, problem):
    """2: the same steps on the data rounded to float under dsgd_comm_init_f64 end in other bits; the planted row's gate
    follows the doubles; against oracle/ref_dict.py on the doubles: active counts, support, 1e-12 * max(1, |w|_inf)"""
    assert int(ranks[0]["f32_value_bits"]) == 32
    assert np.array_equal(bits(ranks[0]["f32_w_hist"]), bits(ranks[1]["f32_w_hist"]))
    assert not np.array_equal(bits(ranks[0]["f32_w_hist"][-1]), bits(ranks[0]["dbl_w_hist"][-1]))
    data, model = ref_problem(problem)
    row = planted_global()
    w = _sparse(problem.w0)
    assert data[row][0].dot(w) == 2.0 ** -30 and data[row][1] == -1          # inactive on the doubles ...
    data32, _ = ref_problem(problem, as_float=True)
    assert data32[row][0].dot(w) == 0.0                                      # ... active once x is rounded to float
    lists0 = [l.tolist() for l in problem.global_lists(0)[0]]
    act64, act32 = (sum(_active(dd, w, l) for l in lists0) for dd in (data, data32))
    assert act32 != act64
    assert int(ranks[0]["f32_stats"][0][1]) == act32
    for i in range(N_STEPS):
        lists, lr = problem.global_lists(i)
        lists = [l.tolist() for l in lists]
        assert int(ranks[0]["dbl_stats"][i][1]) == sum(_active(data, w, l) for l in lists), i
        w = rd.master_sync_step(model, data, w, lists, lr)
    got, want = ranks[0]["dbl_w_hist"][-1], _dense(w)
    assert np.array_equal(np.flatnonzero(got), np.flatnonzero(want))
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))


def test_float_representable_doubles_give_the_float_runs_bits(ranks, problem):
    """3: doubles a float holds, under dsgd_comm_init_f64v: every LO word is zero (CPU) and the weights are bit for bit
    those of the float data under dsgd_comm_init_f64"""
    as_float = Problem("float")
    vexp = vexp64(as_float.data.val)
    for i in range(N_STEPS):
        assert not lo_words(as_float.data, as_float.global_lists(i)[0], vexp).any(), i
    for r in range(WORLD):
        assert int(ranks[r]["frep_value_bits"]) == 64 and int(ranks[r]["f32_value_bits"]) == 32
        assert np.array_equal(bits(ranks[r]["frep_w_hist"]), bits(ranks[r]["f32_w_hist"]))
        assert ranks[r]["frep_stats"].tolist() == ranks[r]["f32_stats"].tolist()
        assert np.array_equal(bits(ranks[r]["frep_ds"]), bits(ranks[r]["f32_ds"]))


def test_one_vexp_over_the_ranks(ranks):
    """4: rank 0's values times 2^10: the ranks agree on the larger vexp and equality 1 holds"""
    scaled = Problem("vexp")
    assert vexp64(scaled.shards[0].csr.val) == vexp64(scaled.shards[1].csr.val) + 10
    for i, (w1, st1) in enumerate(scaled.single_history()):
        for r in range(WORLD):
            assert np.array_equal(bits(ranks[r]["vexp_w_hist"][i]), bits(w1)), (i, r)
            assert ranks[r]["vexp_stats"][i].tolist() == st1, (i, r)


def test_ranks_that_disagree_get_einval_and_the_next_matched_step_runs(tmp_path, problem):
    """5: Double data against float data, then k = 1 against k = 2: DSGD_EINVAL on every rank, the weights keep their bits, and
    the next matched step is the single Double context's"""
    out = run_ranks(str(tmp_path), "mismatch")
    lists, lr = problem.global_lists(1)
    per_rank = len(lists) // WORLD
    with problem.engine() as eng:
        eng.set_weights(problem.w0)
        st = eng.sync_step_f64(lists, lr)
        w_type, st_type = eng.get_weights(), [st["n_samples"], st["n_active"]]
        eng.set_weights(problem.w0)
        st = eng.sync_step_f64([lists[r * per_rank] for r in range(WORLD)], lr)
        w_k, st_k = eng.get_weights(), [st["n_samples"], st["n_active"]]
    for r in range(WORLD):
        for what, w1, st1 in (("type", w_type, st_type), ("k", w_k, st_k)):
            assert int(out[r][what + "_code"]) == _lib.EINVAL, (what, r)
            assert bool(out[r][what + "_w_same"]), (what, r)
            assert np.array_equal(bits(out[r][what + "_w_after"]), bits(w1)), (what, r)
            assert out[r][what + "_stats_after"].tolist() == st1, (what, r)


def test_evaluation_is_the_jobs_on_every_rank(ranks, problem):
    """6: loss_acc over the train and the test ranges: the same on both ranks, the single Double context's bits"""
    assert np.array_equal(bits(ranks[0]["eval"]), bits(ranks[1]["eval"]))
    with problem.engine() as eng:
        eng.set_weights(ranks[0]["dbl_w_hist"][-1])
        l_tr, a_tr, c_tr = eng.loss_acc(0, N_TRAIN)
        l_te, a_te, c_te = eng.loss_acc(N_TRAIN, problem.data.n_rows)
    want = np.asarray([l_tr, a_tr] + list(c_tr) + [l_te, a_te] + list(c_te), dtype=np.float64)
    assert np.array_equal(bits(want), bits(ranks[0]["eval"])), (want, ranks[0]["eval"])


def test_refusals_under_the_communicator_and_the_local_step_behind_it(ranks, problem):
    """7: plans and dsgd_sync_steps_f64 stay DSGD_EUNSUPPORTED under the communicator with the weights untouched; after
    comm_destroy a local sync_step_f64 on the Double data matches a context that never had a communicator"""
    for r in range(WORLD):
        assert ranks[r]["refused"].tolist() == [_lib.EUNSUPPORTED] * 2
        assert bool(ranks[r]["refused_w_same"])
    with problem.engine() as eng:   # (no communicator; the ranking, vexp and dimSparsity the ranks agreed on)
        for r in range(WORLD):
            lists, lr = problem.global_lists(LOCAL_STEP, rank=r)
            eng.set_weights(ranks[r]["dbl_w_hist"][-1])
            st = eng.sync_step_f64(lists, lr)
            assert np.array_equal(bits(eng.get_weights()), bits(ranks[r]["w_local"])), r
            assert ranks[r]["stats_local"].tolist() == [st["n_samples"], st["n_active"]]


def test_real_rccl_world_1_on_double_data_equals_no_communicator():
    """8: the product library, no seam: ncclAllReduce(ncclInt64) of real RCCL on the hardware, one rank, two planes per slot"""
    n_rows, n_train = 4096, 3276
    base = dsgd_amd.synth.generate(n_rows, seed=3)
    rng = np.random.default_rng(4)
    val = base.val.astype(np.float64) * (1.0 + rng.random(len(base.val)) * 2.0 ** -20)
    steps = [([rng.permutation(n_train)[:n].astype(np.int32) for n in sizes], lr)
             for sizes, lr in (((100, 100, 100), 0.5), ((17, 200), 0.1), ((1, 16, 90, 100), 0.5))]
    res = []
    for attach in (False, True):
        with dsgd_amd.Engine(base.dim, CFG["lam"], precision="fp64") as eng:
            eng.load_csr(base.row_ptr, base.col, val, base.label)
            assert eng.value_bits() == 64
            if attach:
                eng.comm_init_f64v(dsgd_amd.Engine.comm_unique_id(), 1, 0)
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
