"""One rank of tests/test_gpu_logistic_job.py, and the inputs it shares with the test: an fp32 engine over the rows
host.logistic_rank_rows gives the rank, attached with comm_init_lg over the tests' seam build and the stand-in collective (both
ranks share device 0).
usage: python logistic_job_worker.py <rank> <world> <workdir> <main|widths|order|mismatch|mirror|mirror_host>"""

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dsgd_amd  # noqa: E402
from dsgd_amd import _lib, host  # noqa: E402
from logistic_ranks_cases import _width_set, concat, cut  # noqa: E402
from logistic_ranks_worker import bits, code_of, grid_weights  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402

WORLD = 2
# 8,192 synthetic rows: 6,144 train rows (a multiple of 12: K = 2, 4 and 6 cut them into whole groups and give a rank the same
# rows, [3,072 r, 3,072 (r + 1))), 2,048 test rows in two slices
N_ROWS, N_TRAIN, LAM, SEED = 8192, 6144, 1e-3, 11
SHARD = 4096
LIST_CASES = [(2, 100), (6, 37), (2, 1500)]   # (K, batch): 1,500 is beyond the one-process form's 1,024
JSTATE = host.JavaRandom(77).seed
RUN_STEPS, LR = 5, 0.5


def job_data():
    d = dsgd_amd.synth.generate(N_ROWS, seed=SEED)
    return (d.row_ptr, d.col, d.val, d.label), d.dim


def take_rows(csr, rows):
    """the listed rows (runs of consecutive numbers) as a CSR of their own"""
    rows = np.asarray(rows, dtype=np.int64)
    cuts = np.nonzero(np.diff(rows) != 1)[0] + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(rows)]])
    return concat([cut(csr, int(rows[a]), int(rows[b - 1]) + 1) for a, b in zip(starts, ends)])


def shard(csr, rank, K=4):
    return take_rows(csr, host.logistic_rank_rows(N_TRAIN, N_ROWS, K, WORLD, rank))


def start_weights(dim):
    return (0.05 * np.random.default_rng(13).standard_normal(dim + 1)).astype(np.float32)


def local_layout(K, rank):
    """(the job's lengths, first, the hosted workers' local begins, max_samples)"""
    split = host.split_vanilla(N_TRAIN, K)
    k = K // WORLD
    lens = [len(g) for g in split]
    begins = np.concatenate([[0], np.cumsum(lens[rank * k:(rank + 1) * k])])[:k]
    return lens, rank * k, [int(b) for b in begins], max(lens)


# the evaluation's local range shapes (rows of a rank's 4,096): one whole shard; lengths 1, 63, 64 (a workgroup with a single row,
# the 16-lane groups' edges around one wave's four rows); 1, 63, 64, 65, 1,023, 1,025 (fewer and more rows than one 1,024-lane
# workgroup's groups times the wave count).  Rank r's ranges start r * 3 rows later: the ranks' ranges are not mirror images.
def range_sets(rank):
    def place(lens, at):
        out = []
        for n in lens:
            out.append((at, at + n))
            at += n + 5
        return out
    return {"n1": [(0, SHARD)], "n3": place([1, 63, 64], 40 + 3 * rank), "n6": place([1, 63, 64, 65, 1023, 1025], 10 + 3 * rank)}


def eval_out(out, key, res):
    counts, range_loss, loss, acc = res
    out[key + "__counts"], out[key + "__rl"], out[key + "__la"] = counts, range_loss, np.asarray([loss, acc], dtype=np.float64)


STATE_IDX = np.random.default_rng(5).permutation(SHARD)[:300].astype(np.int32)


def state_probe(eng, w, lists, with_eval):
    """a step, a gradient and a loss behind (or without) an lg_eval_job"""
    eng.set_weights(w)
    if with_eval:
        eng.lg_eval_job(range_sets(0)["n3"])
    eng.lg_sync_step(lists, LR)
    w1 = eng.get_weights()
    g, _ = eng.lg_gradient(STATE_IDX)
    la = np.asarray(eng.lg_loss_acc(0, 3000), dtype=np.float64)
    return w1, g, la


def run_main(eng, rank, wd, out, csr, dim):
    eng.load_csr(*shard(csr, rank))
    w0 = start_weights(dim)
    eng.set_weights(w0)
    eng.comm_init_lg(exchange_uid(wd, "uid.bin", rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
    # 1. the lists: a rank's window of the job's
    run_plan = None
    for K, batch in LIST_CASES:
        lens, first, begins, max_samples = local_layout(K, rank)
        plan, n_steps, state, draws = eng.lg_plan_from_seed_job(JSTATE, lens, first, begins, max_samples, batch)
        idx, offs = eng.plan_lists(plan)
        tag = "lists_%d_%d" % (K, batch)
        out[tag + "__idx"], out[tag + "__offs"] = idx, offs
        out[tag + "__meta"] = np.asarray([n_steps, draws, state, int(plan.info()["kind"] == "logistic")], dtype=np.int64)   # (plan code 7)
        if (K, batch) == LIST_CASES[0]:
            run_plan = plan
        else:
            plan.destroy()
    # 2. a collective run of such a plan
    eng.plan_run(run_plan, 0, RUN_STEPS, LR)
    st = eng.synchronize()
    run_plan.destroy()
    out["run_stats"] = np.asarray([st["n_samples"], st["n_active"]])
    wb = eng.get_weights()
    out["w_run"] = wb
    # 3. the evaluation: the resident weights behind the steps, grid weights, zero weights
    for name, w in (("run", None), ("grid", grid_weights(wb)), ("zero", np.zeros_like(wb))):
        for shape, ranges in range_sets(rank).items():
            eval_out(out, "eval_%s_%s" % (name, shape), eng.lg_eval_job(ranges, w=w))
    # 4. the state: a step, a gradient and a loss behind an lg_eval_job have the bits they have without it
    lists = [np.random.default_rng(60 + rank).permutation(SHARD)[:n].astype(np.int32) for n in (100, 37)]
    a = state_probe(eng, wb, lists, True)
    b = state_probe(eng, wb, lists, False)
    out["state_same"] = np.asarray([np.array_equal(bits(a[0]), bits(b[0])), np.array_equal(bits(a[1]), bits(b[1])),
                                    np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))])
    out["state_moved"] = np.asarray(not np.array_equal(bits(a[0]), bits(wb)))
    eng.comm_destroy()


def run_widths(rank, wd, out):
    for dim in (1, 2048):
        s = _width_set(dim)
        half = s["rows_per_rank"]
        with dsgd_amd.Engine(s["dim"], s["lam"]) as eng:
            eng.load_csr(*s["shards"][rank])
            eng.set_weights(s["w0"])
            eng.comm_init_lg(exchange_uid(wd, "uid_%d.bin" % dim, rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
            eval_out(out, "w%d" % dim, eng.lg_eval_job(width_ranges(half, rank)))
            eng.comm_destroy()


def width_ranges(half, rank):
    return [(0, 1 + rank), (1 + rank, 66), (66, half)]


# the negative control's job: every row has ONE entry.  Type A: key 0, value 1, label +1 -- under w[0] = a its loss is
# log(1 + e^-a) ~ 2^-25, 64 of them per range ~ 2^-19.  Type B: key 1, value 1, label +1 -- under w[1] = -32 its loss is ~ 32 = 2^5
# (a saturated logit).  ORDER_K ranges per rank, all of 64 A rows but rank 1's FIRST, which is the one B row: in position order
# rank 0's small sums add up exactly before they meet the 32; in a rank-minor order every one of them is rounded to the 32's
# grid of 2^-47 on its own.  lambda = 0 and row counts that are powers of two: range_loss * rows is the range's sum, exactly.
ORDER_K = 32
ORDER_A = (17.3, 17.9, 18.6, 19.2)


def order_shard(rank):
    n = [64] * ORDER_K
    if rank == 1:
        n[0] = 1
    rows = sum(n)
    col = np.zeros(rows, dtype=np.int32)
    if rank == 1:
        col[0] = 1
    begins = np.concatenate([[0], np.cumsum(n)])
    csr = (np.arange(rows + 1, dtype=np.int64), col, np.ones(rows, dtype=np.float32), np.ones(rows, dtype=np.int8))
    return csr, [(int(begins[i]), int(begins[i + 1])) for i in range(ORDER_K)]


def order_weights(a):
    return np.asarray([a, -32.0, 0.0, 0.0], dtype=np.float32)


def run_order(rank, wd, out):
    csr, ranges = order_shard(rank)
    with dsgd_amd.Engine(3, 0.0) as eng:
        eng.load_csr(*csr)
        eng.comm_init_lg(exchange_uid(wd, "uid.bin", rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
        for i, a in enumerate(ORDER_A):
            eval_out(out, "order%d" % i, eng.lg_eval_job(ranges, w=order_weights(a)))
        eng.comm_destroy()


def raw_job_plan(eng, lens, first, begins, max_samples, batch):
    """(code, jstate afterwards, plan handle) of the raw call"""
    jl, sb = np.asarray(lens, dtype=np.int64), np.asarray(begins, dtype=np.int64)
    st, h = C.c_uint64(JSTATE), C.c_void_p(0)
    n_steps, draws = C.c_int64(-1), C.c_int64(-1)
    rc = eng._lib.dsgd_plan_create_from_seed_job_lg(eng._ctx, C.byref(st), jl.ctypes.data_as(C.c_void_p), len(jl), first, len(sb),
                                                    sb.ctypes.data_as(C.c_void_p), max_samples, batch, C.byref(h), C.byref(n_steps), C.byref(draws))
    return rc, int(st.value), h.value


def run_mismatch(eng, rank, wd, out, csr, dim):
    """rank r asks with n_local = 1 + r: DSGD_EINVAL on both, nothing changed; the next call, agreed, succeeds"""
    eng.load_csr(*shard(csr, rank))
    w0 = start_weights(dim)
    eng.set_weights(w0)
    eng.comm_init_lg(exchange_uid(wd, "uid.bin", rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
    ranges = [(0, 100), (100, 300)]
    other = np.ones_like(w0)
    out["code"] = np.asarray(code_of(lambda: eng.lg_eval_job(ranges[:1 + rank], w=other)))
    out["w_same"] = np.asarray(np.array_equal(bits(w0), bits(eng.get_weights())))     # (the call's weights did not replace the resident ones)
    eval_out(out, "after", eng.lg_eval_job(ranges))
    # K > 256: 129 ranges on each of two ranks -- a local check, in front of the agreement
    many = [(i, i + 1) for i in range(129)]
    out["code_many"] = np.asarray(code_of(lambda: eng.lg_eval_job(many)))
    eval_out(out, "k256", eng.lg_eval_job(many[:128]))
    # the job form's own limits: a job_len of 2^20 + 1 is DSGD_EUNSUPPORTED with *jstate untouched (the argument check alone)
    rc, state, h = raw_job_plan(eng, [(1 << 20) + 1, 100], rank, [0], 100, 50)
    out["limit"] = np.asarray([rc, int(state == JSTATE), int(not h)])
    eng.comm_destroy()
    # plain dsgd_comm_init: both calls stay refused, nothing changes
    eng.comm_init(exchange_uid(wd, "uid_plain.bin", rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
    lens, first, begins, max_samples = local_layout(4, rank)
    rc, state, h = raw_job_plan(eng, lens, first, begins, max_samples, 100)
    out["plain"] = np.asarray([code_of(lambda: eng.lg_eval_job(ranges, w=other)), rc, int(state == JSTATE), int(not h),
                               int(np.array_equal(bits(w0), bits(eng.get_weights())))])
    eng.comm_destroy()


def record_epochs(m, eng, initial, epochs, batch):
    """fit for `epochs` epochs; the weights behind every epoch (the stopping criterion is asked in front of each)"""
    hist = []

    def never(losses):
        hist.append(eng.get_weights())
        return False
    state = m.fit(initial, epochs, batch, LR, never)
    return np.stack(hist[1:] + [np.asarray(state.grad, dtype=np.float32)])


MIRROR_K, MIRROR_BATCH, MIRROR_EPOCHS, MIRROR_SEED = 4, 100, 3, 9


def run_mirror(eng, rank, wd, out, csr, dim, device_lists):
    eng.load_csr(*shard(csr, rank, MIRROR_K))
    eng.comm_init_lg(exchange_uid(wd, "uid.bin", rank, dsgd_amd.Engine.comm_unique_id), WORLD, rank)
    m = host.LogisticSync(eng, N_TRAIN, N_ROWS, MIRROR_K, rnd=host.JavaRandom(MIRROR_SEED), ranks=(WORLD, rank), device_lists=device_lists)
    out["w_hist"] = record_epochs(m, eng, start_weights(dim), MIRROR_EPOCHS, MIRROR_BATCH)
    out["figures"] = np.asarray([m.losses, m.accs, m.test_losses, m.test_accs], dtype=np.float64)
    out["meta"] = np.asarray([m.rnd.seed, m.steps_run, m.device_drawn_epochs], dtype=np.int64)
    eng.comm_destroy()


def main():
    rank, world, wd, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    assert world == WORLD
    assert os.environ.get("DSGD_RCCL_LIB"), "the worker must run with the shim selected explicitly"
    assert os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so"), "... through the tests' seam build of the library"
    out = {}
    if mode == "widths":
        run_widths(rank, wd, out)
    elif mode == "order":
        run_order(rank, wd, out)
    else:
        csr, dim = job_data()
        with dsgd_amd.Engine(dim, LAM) as eng:
            if mode == "main":
                run_main(eng, rank, wd, out, csr, dim)
            elif mode == "mismatch":
                run_mismatch(eng, rank, wd, out, csr, dim)
            else:
                run_mirror(eng, rank, wd, out, csr, dim, mode == "mirror")
    np.savez(os.path.join(wd, "out_%d.npz" % rank), **out)
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
