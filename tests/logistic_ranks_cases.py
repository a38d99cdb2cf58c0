"""Inputs shared by the tests of the logistic model across ranks (tests/test_logistic_ranks_emu.py on the CPU,
tests/test_gpu_logistic_ranks.py and its rank processes tests/logistic_ranks_worker.py on the GPU).

The job's data is shard 0 || shard 1: rank r's row i is job row r * rows_per_rank + i.

cancel_problem: a K = 4 step (two workers per rank) on which the ORDER of the fold shows in the float32 weights.  The fold adds
the workers' fp64 sums in worker order and rounds to float once, so on ordinary data another order moves a result by 2^-53 of
it and the float hides that.  Here rank 1 holds two rows of ONE entry B = 2^40 on each of N_CANCEL otherwise unused columns F,
with w[F] = 0: their dot is exactly 0, their coefficient exactly -y / 2, so worker 2 (y = +1) sums to -B / 2 and worker 3
(y = -1) to +B / 2 on F, exactly, whatever their shifts.  Rows of all four workers carry small entries on the F columns.  In
worker order the small sums meet 2^39 and lose their bits below 2^-14; in another order they lose other bits or none -- far
above the float's 2^-24.  The largest value of the job, B, lies on rank 1 ONLY: rank 0's own vexp is much smaller."""

import numpy as np

import dsgd_amd

B = np.float32(2.0 ** 40)
N_CANCEL = 8
LAM, LR = 1e-3, 0.25


def cut(csr, a, b):
    row_ptr, col, val, label = csr
    s, e = int(row_ptr[a]), int(row_ptr[b])
    return (np.asarray(row_ptr[a:b + 1], dtype=np.int64) - s, np.asarray(col[s:e], dtype=np.int32).copy(), np.asarray(val[s:e], dtype=np.float32).copy(),
            np.asarray(label[a:b], dtype=np.int8).copy())


def concat(parts):
    row_ptr, at = [np.zeros(1, np.int64)], 0
    for p in parts:
        row_ptr.append(np.asarray(p[0][1:], dtype=np.int64) + at)
        at += int(p[0][-1])
    nz = [int(p[0][-1]) for p in parts]
    return (np.concatenate(row_ptr), np.concatenate([p[1][:n] for p, n in zip(parts, nz)]).astype(np.int32),
            np.concatenate([p[2][:n] for p, n in zip(parts, nz)]).astype(np.float32), np.concatenate([p[3] for p in parts]).astype(np.int8))


def rows_of(csr):
    """the rows as lists of (key, value) pairs, and the labels"""
    row_ptr, col, val, label = csr
    return [list(zip(col[row_ptr[i]:row_ptr[i + 1]].tolist(), val[row_ptr[i]:row_ptr[i + 1]].tolist())) for i in range(len(row_ptr) - 1)], list(label)


def from_rows(rows, labels):
    row_ptr, col, val = [0], [], []
    for r in rows:
        for k, v in sorted(r):
            col.append(k)
            val.append(v)
        row_ptr.append(len(col))
    return (np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float32), np.asarray(labels, np.int8))


def global_lists(lists_per_rank, rows_per_rank):
    """the K = k x world lists in global worker order (rank-major), row indices shifted to the job's"""
    return [(np.asarray(l, dtype=np.int64) + r * rows_per_rank).astype(np.int32) for r, lists in enumerate(lists_per_rank) for l in lists]


def cancel_problem(rows_per_rank=256, dim=2000, seed=5):
    """(job csr, [shard csr] * 2, w float32, lists per rank (2 x 2), the F keys)"""
    d = dsgd_amd.synth.generate(2 * rows_per_rank, seed=seed, dim=dim)
    job = (d.row_ptr, d.col, d.val, d.label)
    free = np.nonzero(np.bincount(d.col[:int(d.row_ptr[-1])], minlength=dim + 1) == 0)[0]
    assert len(free) >= N_CANCEL
    F = [int(k) for k in free[:N_CANCEL]]
    rng = np.random.default_rng([seed, 8])
    # unequal lengths: the same j has another shift on the other rank (100 -> 55, 300 -> 53; 37 -> 56, 5 -> 59)
    lists = [[rng.permutation(rows_per_rank)[:n].astype(np.int32) for n in (100, 37)]]
    p1 = rng.permutation(rows_per_rank).astype(np.int32)
    n_first = min(rows_per_rank - 44, 300)   # rank 1's workers list disjoint rows; 300 positions: duplicates count, but the
    first = p1[:n_first]                      # list's first row, the cancelling one below, stays single
    lists.append([np.concatenate([first, first[1:1 + 300 - n_first]]), p1[n_first:n_first + 5].copy()])
    assert [len(l) for ls in lists for l in ls] == [100, 37, 300, 5]
    shards = []
    for r in range(2):
        rows, labels = rows_of(cut(job, r * rows_per_rank, (r + 1) * rows_per_rank))
        for j, idx in enumerate(lists[r]):   # small entries on every F column in two rows of every worker
            for t in range(min(2, len(idx))):
                row = int(idx[-1 - t])
                rows[row] = [kv for kv in rows[row] if kv[0] not in F] + [(f, float(np.float32(0.1 + 0.8 * rng.random()))) for f in F]
        if r == 1:   # the two cancelling rows: the first listed row of each of rank 1's workers
            for j, y in ((0, 1), (1, -1)):
                row = int(lists[1][j][0])
                rows[row] = [(f, float(B)) for f in F]
                labels[row] = y
            assert int(lists[1][0][0]) not in lists[1][1] and int(lists[1][1][0]) not in lists[1][0]
        shards.append(from_rows(rows, labels))
    w = (0.3 * rng.standard_normal(dim + 1)).astype(np.float32)
    w[F] = 0.0
    return concat(shards), shards, w, lists, F


# ---- the GPU scenarios: what every rank runs, and what ONE context over the job's rows runs for the same bits -----------------
# A scenario is a list of sets; a set = dict(name, shards [csr, csr], dim, lam, w0, ops).  An op = dict(kind, per_rank, lr[, n_steps]):
#   lists         per_rank[r] = the k lists of one lg_sync_step
#   ranges        per_rank[r] = the k (begin, end) ranges of one lg_sync_step_ranges
#   steps_ranges  the same ranges, n_steps steps through lg_sync_steps_ranges
#   steps, plan   per_rank[r] = [step][worker] lists: one lg_sync_steps call / an lg_plan_flat plan run in one plan_run
WORLD = 2
S_ROWS = 4096     # rows per rank of the synthetic job
S_LAM = 1e-3


def _flat(steps):
    idx = np.concatenate([l for s in steps for l in s]).astype(np.int32)
    offs = np.concatenate([[0], np.cumsum([len(l) for s in steps for l in s])]).astype(np.int64)
    return idx, offs, len(steps), len(steps[0])


def job_op(op, rows_per_rank):
    """the op as ONE context over shard 0 || shard 1 runs it: the K = k x world workers rank-major, rows shifted to the job's"""
    out = dict(op)
    if op["kind"] == "lists":
        out["args"] = global_lists(op["per_rank"], rows_per_rank)
    elif op["kind"] in ("ranges", "steps_ranges"):
        out["args"] = [(a + r * rows_per_rank, b + r * rows_per_rank) for r, rs in enumerate(op["per_rank"]) for a, b in rs]
    else:
        n_steps = len(op["per_rank"][0])
        out["args"] = [global_lists([op["per_rank"][r][t] for r in range(WORLD)], rows_per_rank) for t in range(n_steps)]
    return out


def rank_op(op, rank):
    out = dict(op)
    out["args"] = op["per_rank"][rank]
    return out


def run_op(eng, op):
    """one op on an engine (a rank's, or the single context's): (stats, the gradient kernel's name)"""
    kind, a, lr = op["kind"], op["args"], op["lr"]
    if kind == "lists":
        st = eng.lg_sync_step(a, lr)
    elif kind == "ranges":
        st = eng.lg_sync_step_ranges(a, lr)
    elif kind == "steps_ranges":
        st = eng.lg_sync_steps_ranges(a, op["n_steps"], lr)
    elif kind == "steps":
        st = eng.lg_sync_steps(*_flat(a), lr)
    else:
        plan = eng.lg_plan_flat(*_flat(a))
        eng.plan_run(plan, 0, len(a), lr)
        st = eng.synchronize()
        plan.destroy()
    return [int(st["n_samples"]), int(st["n_active"])], eng.grad_kernel_name()


def op_steps(op):
    """the op as a sequence of (K lists, lr) steps of the job, for a reference that steps list by list"""
    j = job_op(op, op["rows_per_rank"])
    if op["kind"] == "lists":
        return [(j["args"], op["lr"])]
    if op["kind"] in ("ranges", "steps_ranges"):
        lists = [np.arange(a, b, dtype=np.int32) for a, b in j["args"]]
        return [(lists, op["lr"])] * (op.get("n_steps", 1))
    return [(ls, op["lr"]) for ls in j["args"]]


def _synth_set():
    d = dsgd_amd.synth.generate(WORLD * S_ROWS, seed=11)
    job = (d.row_ptr, d.col, d.val, d.label)
    shards = [cut(job, r * S_ROWS, (r + 1) * S_ROWS) for r in range(WORLD)]
    rng = np.random.default_rng(12)

    def pick(n):
        return rng.permutation(S_ROWS)[:n].astype(np.int32)

    dup = [pick(60) for _ in range(4)]
    ops = [
        dict(kind="lists", per_rank=[[pick(100)] for _ in range(WORLD)], lr=0.5),
        dict(kind="lists", per_rank=[[pick(100), pick(37), pick(1)] for _ in range(WORLD)], lr=0.5),   # unequal shifts
        dict(kind="lists", per_rank=[[np.concatenate([dup[2 * r], dup[2 * r][:9]]), np.concatenate([dup[2 * r + 1], dup[2 * r + 1][:1], dup[2 * r + 1][:1]])]
                                     for r in range(WORLD)], lr=0.25),                                      # duplicates count
        dict(kind="ranges", per_rank=[[(0, S_ROWS)] for _ in range(WORLD)], lr=2.0 ** -9),
        dict(kind="steps_ranges", per_rank=[[(0, 1500), (1500, S_ROWS)], [(0, 2500), (2500, S_ROWS)]], n_steps=3, lr=2.0 ** -9),
        dict(kind="steps", per_rank=[[[pick(100), pick(100)] for _ in range(5)] for _ in range(WORLD)], lr=0.5),
        dict(kind="plan", per_rank=[[[pick(100), pick(100)] for _ in range(5)] for _ in range(WORLD)], lr=0.5),
    ]
    w0 = (0.05 * np.random.default_rng(13).standard_normal(d.dim + 1)).astype(np.float32)
    return dict(name="synth", shards=shards, dim=d.dim, lam=S_LAM, w0=w0, ops=ops, rows_per_rank=S_ROWS)


def _cancel_set():
    job, shards, w, lists, F = cancel_problem(256)
    return dict(name="cancel", shards=shards, dim=2000, lam=LAM, w0=w, ops=[dict(kind="lists", per_rank=lists, lr=LR)], rows_per_rank=256)


WIDTHS = (1, 255, 2047, 2048, 318)   # dp = 319 = 4 * 64 + 63: the stride's padding is one word


def _width_set(dim):
    import logistic_hard_cases as hc

    case = hc.width(dim)
    half = hc.W_ROWS // 2
    shards = [cut(case.csr, r * half, (r + 1) * half) for r in range(WORLD)]
    rng = np.random.default_rng([44, dim])
    per_rank = [[rng.permutation(half)[:n].astype(np.int32) for n in (100, 37, 1)] for _ in range(WORLD)]
    per_rank[0][1][0] = hc.W_FULL_ROW   # (at the widths of W_FULL: the row of every key; the whole ranges below hold it anyway)
    ops = [dict(kind="lists", per_rank=per_rank, lr=hc.W_LR), dict(kind="ranges", per_rank=[[(0, half)], [(0, half)]], lr=hc.W_LR_RANGES),
           dict(kind="steps_ranges", per_rank=[[(0, 200), (200, half)], [(0, 1), (1, half)]], n_steps=2, lr=hc.W_LR_RANGES)]
    return dict(name="dim %d" % dim, shards=shards, dim=dim, lam=hc.W_LAM, w0=np.array(case.w), ops=ops, rows_per_rank=half)


def _exact_set():
    """a saturated exact case as rank 1's worker beside a worker of 64 saturated rows on rank 0: a column sum of -2^62 crosses
    the gather (4,096 rows of value 1.0 at S = 50)"""
    import logistic_hard_cases as hc

    small, tall = hc.exact_case("tall", 4095, "one", "alt"), hc.exact_case("tall", 4096, "one")
    ops = [dict(kind="lists", per_rank=[[np.arange(64, dtype=np.int32)], [np.arange(4096, dtype=np.int32)]], lr=hc.E_LR_TALL)]
    return dict(name="exact", shards=[small.csr, tall.csr], dim=hc.E_DIM, lam=0.0, w0=np.array(tall.w), ops=ops, rows_per_rank=4095)


def scenario(mode):
    sets = {"steps": lambda: [_synth_set()], "cancel": lambda: [_cancel_set()], "widths": lambda: [_width_set(d) for d in WIDTHS],
            "exact": lambda: [_exact_set()]}[mode]()
    for s in sets:
        for op in s["ops"]:
            op["rows_per_rank"] = s["rows_per_rank"]
    return sets
