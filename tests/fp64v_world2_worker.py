"""One rank of tests/test_gpu_fp64v_world2.py: fp64 engines over the rank's shard of the rows as DOUBLE feature values,
attached with comm_init_f64v over the tests' seam build and the stand-in collective (both ranks share device 0).  One
process runs the module's legs one after the other, each on a fresh engine with its own unique id.
usage: python fp64v_world2_worker.py <rank> <world> <workdir> [steps|mismatch]

Also the test's shared construction: the data (world2_common.CFG's synthetic rows with full 53-bit mantissas, one planted
row on rank 1 whose gate the float rounding flips), the starting weights and the steps' lists."""

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
from world2_common import CFG, shard_of, split_range  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402

WORLD = 2
# per rank and step: the list lengths of its hosted workers (k = 1 and k = 2; 16 | 17 is the 16-rows-per-workgroup seam;
# "dup" is a list of 17 rows with one of them three times) and the learning rate
STEPS = [((100,), 0.5), ((16, 17), 0.5), ((1,), 0.5), ((100, "dup"), 0.25), ((17, 1), 0.5)]
N_STEPS = len(STEPS)
PLANTED_LOCAL = 5          # the planted row: rank 1's local train row 5, held by rank 1's list of step 0
LOCAL_STEP = 1             # the lists of the local step behind comm_destroy


def union_data(kind="double"):
    """CFG's rows as float64 values.  double: every value times (1 + u * 2^-20), u in [0, 1) -- full mantissas that no
    float holds -- and the planted row x = {a: 1 + 2^-30, b: 1}, y = -1 on the two rarest columns (with w[a] = 1,
    w[b] = -1: x . w = 2^-30 > 0, the row is inactive; rounded to float x . w = 0 and it is active).  float: the same
    values rounded to float (as float64: what a float holds).  vexp: double, rank 0's rows times 2^10."""
    base = dsgd_amd.synth.generate(CFG["n_rows"], seed=CFG["seed"])
    rng = np.random.default_rng(77)
    val = base.val.astype(np.float64) * (1.0 + rng.random(len(base.val)) * 2.0 ** -20)
    cnt = np.bincount(base.col, minlength=base.dim + 1)
    a, b = sorted(int(c) for c in 1 + np.argsort(cnt[1:], kind="stable")[:2])   # the two rarest columns (every column occurs at this size)
    row = planted_global()
    s, e = int(base.row_ptr[row]), int(base.row_ptr[row + 1])
    col = np.concatenate([base.col[:s], np.asarray([a, b], np.int32), base.col[e:]]).astype(np.int32)
    val = np.concatenate([val[:s], np.asarray([1.0 + 2.0 ** -30, 1.0]), val[e:]])
    row_ptr = base.row_ptr.astype(np.int64).copy()
    row_ptr[row + 1:] += 2 - (e - s)
    label = base.label.copy()
    label[row] = -1
    if kind == "float":
        val = val.astype(np.float32).astype(np.float64)
    if kind == "vexp":
        for r_lo, r_hi in (split_range(0, CFG["n_train"], 0, WORLD), split_range(CFG["n_train"], CFG["n_rows"], 0, WORLD)):
            val[row_ptr[r_lo]:row_ptr[r_hi]] = np.ldexp(val[row_ptr[r_lo]:row_ptr[r_hi]], 10)
    return dsgd_amd.synth.Csr(base.dim, row_ptr, col, val, label), (a, b)


def planted_global():
    return split_range(0, CFG["n_train"], 1, WORLD)[0] + PLANTED_LOCAL


def start_weights(dim, ab):
    w = hd.base_weights(dim, 79, n=2000, scale=0.01)
    w[ab[0]], w[ab[1]] = 1.0, -1.0
    return w


def step_lists(rank, i, ntl):
    """(lists of rank `rank`, lr) of step i: local row indices; every rank hosts the same number of workers"""
    sizes, lr = STEPS[i]
    rng = np.random.default_rng([43, rank, i])
    if i == 0:
        return hd.lists_with(rng, ntl, 1, sizes[0], must_hold=(PLANTED_LOCAL,) if rank == 1 else ()), lr
    out = []
    for n in sizes:
        if n == "dup":
            a = rng.permutation(ntl)[:15].astype(np.int32)
            out.append(np.concatenate([a, a[:1], a[:1]]))
        else:
            out.append(rng.permutation(ntl)[:n].astype(np.int32))
    return out, lr


def run_steps(eng, rank, wd, sh, w0, tag, out, v=True, load_under_comm=False, full=False):
    """the steps on `sh`'s rows under a fresh communicator; full: evaluation, refusals and the local step behind it too"""
    ntl = sh.n_train
    attach = eng.comm_init_f64v if v else eng.comm_init_f64
    uid = lambda: exchange_uid(wd, "uid_%s.bin" % tag, rank, dsgd_amd.Engine.comm_unique_id)   # noqa: E731
    if load_under_comm:   # float data first; the doubles arrive with the communicator attached (a collective load)
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val.astype(np.float32), sh.csr.label)
        attach(uid(), WORLD, rank)
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val, sh.csr.label)
    else:
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val if v else sh.csr.val.astype(np.float32), sh.csr.label)
        attach(uid(), WORLD, rank)
    out[tag + "_value_bits"] = np.asarray(eng.value_bits())
    out[tag + "_ds"] = eng.build_dim_sparsity(ntl)
    eng.set_weights(w0)
    w_hist, stats = [], []
    for i in range(N_STEPS):
        lists, lr = step_lists(rank, i, ntl)
        st = eng.sync_step_f64(lists, lr)
        w_hist.append(eng.get_weights())
        stats.append([st["n_samples"], st["n_active"]])
    out[tag + "_w_hist"] = np.stack(w_hist)
    out[tag + "_stats"] = np.asarray(stats)
    if full:
        out["ranks"] = eng.column_ranks()
        l_tr, a_tr, c_tr = eng.loss_acc(0, ntl)
        l_te, a_te, c_te = eng.loss_acc(ntl, sh.csr.n_rows)
        out["eval"] = np.asarray([l_tr, a_tr] + list(c_tr) + [l_te, a_te] + list(c_te), dtype=np.float64)
        w_before = eng.get_weights()
        out["refused"] = np.asarray([code_of(lambda: eng.plan(small_plan_lists(ntl))),
                                     code_of(lambda: eng.sync_steps_f64(np.arange(4, dtype=np.int32), np.asarray([0, 4], np.int64), 1, 1, 0.5))])
        out["refused_w_same"] = np.asarray(np.array_equal(bits(w_before), bits(eng.get_weights())))
    eng.comm_destroy()
    if full:   # detached: a local step on the Double data
        lists, lr = step_lists(rank, LOCAL_STEP, ntl)
        st = eng.sync_step_f64(lists, lr)
        out["w_local"] = eng.get_weights()
        out["stats_local"] = np.asarray([st["n_samples"], st["n_active"]])


def mode_steps(rank, wd, out):
    data, ab = union_data("double")
    w0 = start_weights(data.dim, ab)
    sh = shard_of(data, CFG["n_train"], rank, WORLD)
    as_float = shard_of(union_data("float")[0], CFG["n_train"], rank, WORLD)
    scaled = shard_of(union_data("vexp")[0], CFG["n_train"], rank, WORLD)
    legs = (("dbl", sh, dict(load_under_comm=True, full=True)),    # Double data under comm_init_f64v
            ("f32", as_float, dict(v=False)),                      # the same data rounded to float under comm_init_f64
            ("frep", as_float, dict()),                            # ... as doubles a float holds, under comm_init_f64v
            ("vexp", scaled, dict()))                              # rank 0's values times 2^10: ONE vexp
    for tag, shard, kw in legs:
        with dsgd_amd.Engine(data.dim, CFG["lam"], device=0, precision="fp64") as eng:
            run_steps(eng, rank, wd, shard, w0, tag, out, **kw)


def mode_mismatch(rank, wd, out):
    """the value type, then the hosted workers: ranks that disagree all get DSGD_EINVAL with the weights as they were, and the
    next matched step runs from a clean buffer"""
    data, ab = union_data("double")
    w0 = start_weights(data.dim, ab)
    sh = shard_of(data, CFG["n_train"], rank, WORLD)
    ntl = sh.n_train
    with dsgd_amd.Engine(data.dim, CFG["lam"], device=0, precision="fp64") as eng:
        # rank 0 holds doubles, rank 1 the same rows rounded to float
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val if rank == 0 else sh.csr.val.astype(np.float32), sh.csr.label)
        eng.comm_init_f64v(exchange_uid(wd, "uid_mm.bin", rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
        eng.build_dim_sparsity(ntl)
        eng.set_weights(w0)
        lists, lr = step_lists(rank, 1, ntl)
        out["type_code"] = np.asarray(code_of(lambda: eng.sync_step_f64(lists, lr)))
        out["type_w_same"] = np.asarray(np.array_equal(bits(w0), bits(eng.get_weights())))
        # every rank loads the doubles (the load is collective: ranking and vexp are agreed at first use)
        eng.load_csr(sh.csr.row_ptr, sh.csr.col, sh.csr.val, sh.csr.label)
        eng.build_dim_sparsity(ntl)
        eng.set_weights(w0)
        st = eng.sync_step_f64(lists, lr)
        out["type_w_after"] = eng.get_weights()
        out["type_stats_after"] = np.asarray([st["n_samples"], st["n_active"]])
        # rank r calls with 1 + r hosted workers
        eng.set_weights(w0)
        out["k_code"] = np.asarray(code_of(lambda: eng.sync_step_f64(lists[:1 + rank], lr)))
        out["k_w_same"] = np.asarray(np.array_equal(bits(w0), bits(eng.get_weights())))
        st = eng.sync_step_f64(lists[:1], lr)
        out["k_w_after"] = eng.get_weights()
        out["k_stats_after"] = np.asarray([st["n_samples"], st["n_active"]])
        eng.comm_destroy()


def main():
    rank, world, wd = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    mode = sys.argv[4] if len(sys.argv) > 4 else "steps"
    assert world == WORLD
    assert os.environ.get("DSGD_RCCL_LIB"), "the worker must run with the shim selected explicitly"
    assert os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so"), "... through the tests' seam build of the library"
    assert "dsgd_comm_init_f64v" in _lib.SYMBOLS
    out = {}
    (mode_steps if mode == "steps" else mode_mismatch)(rank, wd, out)
    np.savez(os.path.join(wd, "out_%d.npz" % rank), **out)
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
