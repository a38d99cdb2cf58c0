"""One rank of tests/test_gpu_fp64_rank_plans.py (and of tests/test_gpu_fp64_rank_plans_rccl_multi.py): fp64 engines over
the rank's shard of the rows, attached with comm_init_f64 / comm_init_f64v, running ROW-PARALLEL PLANS under the communicator
(dsgd_plan_run_f64 as a collective call: include/dsgd.h "ACROSS RANKS").  Over the tests' seam build and the stand-in
collective both ranks share device 0; with `--real` the product library over real RCCL, one device per rank.  One process
runs its mode's legs one after the other, each on a fresh engine with its own unique id.
usage: python fp64_rank_plans_worker.py <rank> <world> <workdir> float|double|mismatch [--real]

Also the tests' shared construction: the plan's lists per rank, the starting weights, the learning rate."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dsgd_amd  # noqa: E402
import hard_data as hd  # noqa: E402
from dsgd_amd import _lib  # noqa: E402
from fp64_world2_worker import bits, code_of, small_plan_lists  # noqa: E402
from fp64v_world2_worker import PLANTED_LOCAL, start_weights, union_data  # noqa: E402
from world2_common import CFG, shard_of  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402

WORLD = 2
LR = 0.25
# per rank and step the list lengths of its two hosted workers (k = 1: the first of each): 1, 16 | 17 (the 16-rows-per-workgroup
# seam) and 100, "dup" a list of 17 rows with one of them three times; the lengths differ between the ranks and between the
# workers of a step, so the shifts do
LENS = (
    ((100, 17), (1, 16), (16, 100), (17, 1), (100, "dup"), (50, 100), (100, 100), (33, 64), (16, 16), (100, 1), (17, 100), (65, 30)),
    ((16, 100), (17, 1), (100, 1), (100, 16), ("dup", 100), (100, 50), (1, 100), (64, 17), (17, 17), (1, 100), (100, 17), (30, 129)),
)
N_STEPS = len(LENS[0])
CUTS = ((0, 5), (5, 6), (6, N_STEPS))


def plan_steps(rank, ntl, k, planted=False):
    """the plan of rank `rank`: per step the k lists of local row indices.  planted: rank 1's first list of step 0 holds
    fp64v_world2_worker's planted row"""
    steps = []
    for t, sizes in enumerate(LENS[rank]):
        rng = np.random.default_rng([71, rank, t])
        lists = []
        for n in sizes[:k]:
            if n == "dup":
                a = rng.permutation(ntl)[:15].astype(np.int32)
                lists.append(np.concatenate([a, a[:1], a[:1]]))
            else:
                lists.append(rng.permutation(ntl)[:n].astype(np.int32))
        if planted and rank == 1 and t == 0 and PLANTED_LOCAL not in lists[0]:
            lists[0][0] = PLANTED_LOCAL
        steps.append(lists)
    return steps


def float_w0(dim):
    return hd.base_weights(dim, 79, n=2000, scale=0.01)


class Rank:
    def __init__(self, rank, world, wd, real):
        self.rank, self.world, self.wd, self.real = rank, world, wd, real
        self.n_uid = 0

    def uid(self):
        self.n_uid += 1
        return exchange_uid(self.wd, "uid_%d.bin" % self.n_uid, self.rank, dsgd_amd.Engine.comm_unique_id)

    def engine(self, dim):
        return dsgd_amd.Engine(dim, CFG["lam"], device=self.rank if self.real else 0, precision="fp64")

    def ready(self, eng, sh, w0, v=False, as_float32=True):
        """loaded (as floats, or as doubles), attached, dimSparsity built (collective), the starting weights set"""
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val.astype(np.float32 if as_float32 else np.float64), sh.csr.label)
        (eng.comm_init_f64v if v else eng.comm_init_f64)(self.uid(), self.world, self.rank)
        eng.build_dim_sparsity(sh.n_train)
        eng.set_weights(w0)


def err_of(fn):
    """(code, message) of a call that is expected to fail"""
    try:
        fn()
    except _lib.DsgdError as e:
        return np.asarray(e.code), np.asarray(str(e))
    return np.asarray(0), np.asarray("")


def run_plan(eng, steps, cuts, lr=LR, plan=None):
    """the plan's steps as the calls `cuts`: the weights behind every call and the closing statistics"""
    p = plan if plan is not None else eng.plan(steps, rp64=True)
    ws = []
    for a, b in cuts:
        eng.plan_run(p, a, b, lr)
        ws.append(eng.get_weights())
    st = eng.synchronize()
    p.destroy()
    return np.stack(ws), np.asarray([st["n_samples"], st["n_active"]])


def run_loop(eng, steps, lr=LR):
    """the yardstick: one sync_step_f64 per step under the same communicator"""
    ws, ns, na = [], 0, 0
    for lists in steps:
        st = eng.sync_step_f64(lists, lr)
        ws.append(eng.get_weights())
        ns += st["n_samples"]
        na += st["n_active"]
    return np.stack(ws), np.asarray([ns, na])


def three_ways(rk, out, tag, dim, sh, w0, steps, **kw):
    """ONE call, the cut calls and the per-step loop, each on a fresh engine"""
    whole = ((0, len(steps)),)
    for name, fn in (("one", lambda e: run_plan(e, steps, whole)), ("cut", lambda e: run_plan(e, steps, CUTS)), ("loop", lambda e: run_loop(e, steps))):
        with rk.engine(dim) as eng:
            rk.ready(eng, sh, w0, **kw)
            out["%s_%s_w" % (tag, name)], out["%s_%s_stats" % (tag, name)] = fn(eng)
            if name == "one":
                out[tag + "_kernel"] = np.asarray(eng.grad_kernel_name())
                out[tag + "_value_bits"] = np.asarray(eng.value_bits())
            eng.comm_destroy()


def mode_float(rk, out):
    data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    sh = shard_of(data, CFG["n_train"], rk.rank, rk.world)
    ntl, w0 = sh.n_train, float_w0(data.dim)
    for k in (2, 1):
        three_ways(rk, out, "k%d" % k, data.dim, sh, w0, plan_steps(rk.rank, ntl, k))
    if rk.real:
        return
    steps = plan_steps(rk.rank, ntl, 2)
    with rk.engine(data.dim) as eng:
        # slice-major weights: a column-slice plan run with lr = 0 while detached; the row-parallel plan is made detached too
        rk.ready(eng, sh, w0)
        out["ranks"] = eng.column_ranks()
        eng.comm_destroy()
        rp = eng.plan(steps, rp64=True)
        cs = eng.plan(small_plan_lists(ntl))
        eng.plan_run(cs, 0, 3, 0.0)
        eng.synchronize()   # (its rows are reported here: the statistics behind the attached run are that run's; the layout stays)
        eng.comm_init_f64(rk.uid(), rk.world, rk.rank)
        cs.destroy()
        out["sliced_w"], out["sliced_stats"] = run_plan(eng, steps, ((0, N_STEPS),), plan=rp)
        # what stays refused under the communicator, the weights keeping their bits
        w_before = eng.get_weights()
        flat = np.concatenate([l for s in steps[:2] for l in s]).astype(np.int32)
        offs = np.concatenate([[0], np.cumsum([len(l) for s in steps[:2] for l in s])]).astype(np.int64)
        rp2 = eng.plan(steps, rp64=True)   # (accepted attached)
        group = dsgd_amd.engine.EngineGroup([eng])
        calls = [("plan_create", lambda: eng.plan(small_plan_lists(ntl))),
                 ("plan_create_n", lambda: eng.plan_flat(flat, offs, 2, 2)),
                 ("plan_from_seed", lambda: eng.plan_from_seed(12345, [(0, ntl // 2), (ntl // 2, ntl)], ntl, 100)),
                 ("plan_from_seed_rp64", lambda: eng.plan_from_seed(12345, [(0, ntl // 2), (ntl // 2, ntl)], ntl, 100, rp64=True)),
                 ("async_plan", lambda: eng.async_plan([(0, ntl)], 100, seed=3, n_updates=4)),
                 ("async_plan_rp64", lambda: eng.async_plan([(0, ntl)], 100, seed=3, n_updates=4, rp64=True)),
                 ("plan_run_async", lambda: eng.plan_run_async(rp2, 0, 1, LR)),
                 ("sync_steps_f64", lambda: eng.sync_steps_f64(flat, offs, 2, 2, LR)),
                 ("sync_step_devices", lambda: group.sync_step([steps[0]], LR)),
                 ("sync_step_ranges_devices", lambda: group.sync_step_ranges([[(0, 100), (100, 200)]], LR)),
                 ("loss_acc_devices", lambda: group.loss_acc([(0, ntl)]))]
        out["refused_names"] = np.asarray([n for n, _ in calls])
        out["refused"] = np.asarray([code_of(fn) for _, fn in calls])
        rp2.record(True)
        out["recorded_code"] = np.asarray(code_of(lambda: eng.plan_run(rp2, 0, 2, LR)))
        rp2.record(False)
        out["refused_w_same"] = np.asarray(np.array_equal(bits(w_before), bits(eng.get_weights())))
        # ... and an attached plan runs detached: the local steps
        eng.comm_destroy()
        eng.set_weights(w0)
        out["detached_w"], out["detached_stats"] = run_plan(eng, steps, ((0, N_STEPS),), plan=rp2)


def mode_double(rk, out):
    data, ab = union_data("double")
    w0 = start_weights(data.dim, ab)
    sh = shard_of(data, CFG["n_train"], rk.rank, rk.world)
    as_float = shard_of(union_data("float")[0], CFG["n_train"], rk.rank, rk.world)
    steps = plan_steps(rk.rank, sh.n_train, 2, planted=True)
    three_ways(rk, out, "dbl", data.dim, sh, w0, steps, v=True, as_float32=False)
    whole = ((0, N_STEPS),)
    for tag, kw in (("f32", dict(v=False, as_float32=True)), ("frep", dict(v=True, as_float32=False))):
        with rk.engine(data.dim) as eng:
            rk.ready(eng, as_float, w0, **kw)
            out[tag + "_value_bits"] = np.asarray(eng.value_bits())
            out[tag + "_w"], out[tag + "_stats"] = run_plan(eng, steps, whole)
            eng.comm_destroy()


def mode_mismatch(rk, out):
    """rank r calls with (a) a plan of 1 + r hosted workers, (b) 3 + r steps, (c) float data on one rank and Double on the other:
    DSGD_EINVAL everywhere with the weights as they were, and the matched run behind each gives the float leg's bits"""
    data = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    sh = shard_of(data, CFG["n_train"], rk.rank, rk.world)
    ntl, w0 = sh.n_train, float_w0(data.dim)
    steps = plan_steps(rk.rank, ntl, 2)
    whole = ((0, N_STEPS),)
    same = lambda eng: np.asarray(np.array_equal(bits(w0), bits(eng.get_weights())))   # noqa: E731
    with rk.engine(data.dim) as eng:
        rk.ready(eng, sh, w0)
        p = eng.plan(plan_steps(rk.rank, ntl, 1 + rk.rank), rp64=True)
        out["k_code"], out["k_msg"] = err_of(lambda: eng.plan_run(p, 0, N_STEPS, LR))
        out["k_w_same"] = same(eng)
        p.destroy()
        out["k_w_after"], out["k_stats_after"] = run_plan(eng, steps, whole)
        eng.set_weights(w0)
        p = eng.plan(steps, rp64=True)
        out["steps_code"], out["steps_msg"] = err_of(lambda: eng.plan_run(p, 0, 3 + rk.rank, LR))
        out["steps_w_same"] = same(eng)
        out["steps_w_after"], out["steps_stats_after"] = run_plan(eng, steps, whole, plan=p)
        eng.comm_destroy()
    with rk.engine(data.dim) as eng:   # rank 0 holds the values as doubles, rank 1 as floats
        rk.ready(eng, sh, w0, v=True, as_float32=rk.rank == 1)
        p = eng.plan(steps, rp64=True)
        out["type_code"], out["type_msg"] = err_of(lambda: eng.plan_run(p, 0, N_STEPS, LR))
        out["type_w_same"] = same(eng)
        # every rank loads the floats (the load is collective); the plan outlives the load
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val.astype(np.float32), sh.csr.label)
        eng.build_dim_sparsity(ntl)
        eng.set_weights(w0)
        out["type_w_after"], out["type_stats_after"] = run_plan(eng, steps, whole, plan=p)
        eng.comm_destroy()


def main():
    rank, world, wd, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    real = "--real" in sys.argv
    assert world == WORLD
    if real:
        assert not os.environ.get("DSGD_LIB_PATH"), "the product library over real RCCL"
    else:
        assert os.environ.get("DSGD_RCCL_LIB"), "the worker must run with the shim selected explicitly"
        assert os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so"), "... through the tests' seam build of the library"
    out = {}
    {"float": mode_float, "double": mode_double, "mismatch": mode_mismatch}[mode](Rank(rank, world, wd, real), out)
    np.savez(os.path.join(wd, "out_%d.npz" % rank), **out)
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
