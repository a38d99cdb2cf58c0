"""-m gpu: dsgd_load_csr on a LIVE context (include/dsgd.h "LOADING AGAIN").  A context caches a great deal that depends on the
loaded matrix -- the column ranking, the split streams and their tiles, vexp and the measured shifts, eight layouts of row
chunks and eight of column lists keyed by the row ranges alone, the evaluation kernels' lane group, scratch sized by earlier
rows, every live plan's slices, tiles and "fits" -- and a second load of the SAME matrix gets the right answer from every
stale one of them.  Here the second matrix shares nothing with the first (tests/reload_data.py, pinned on the CPU by
tests/test_reload_data.py), and one principle runs through every test:

    context R  loads A, builds dimSparsity, runs the family under test with the cache keys it will use on B (warm caches),
               then loads B, builds dimSparsity, sets w0 and runs the family on B;
    context F  is fresh: loads B, builds dimSparsity, sets w0, runs the same calls.

R and F must agree BIT FOR BIT after every call (every synchronous family is bit-reproducible: nothing to tolerate), in
n_active, the kernel that ran, the shift it used, column_ranks() and build_dim_sparsity().  So that the code is not only
compared with itself, the same calls are held to the fp64 oracle by the suite's own helpers and their derived bounds
(ranged_step, list_step, plan_step of tests/test_gpu_parity.py, plan_step of tests/test_gpu_cs.py).  Each test also shows
that it was sharp: the warm-up on A ran the family, and the result on B differs from the result on A."""

import numpy as np
import pytest

import dsgd_amd
import reload_data as rl
from conftest import has_gpu
from oracle import oracle as orc
from oracle.hogwild_replay import hog_rows
from test_gpu_cs import plan_step as cs_plan_step
from test_gpu_parity import list_step, ranged_step
from test_gpu_parity import plan_step as rp_plan_step

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
GATE_EPS = 1e-5   # (tests/test_gpu_parity.py)
KNOBS = ("DSGD_CS", "DSGD_TCOL", "DSGD_FSTEP", "DSGD_FSTEP_MIN", "DSGD_STREAM_MIN", "DSGD_HSPLIT", "DSGD_CS_REQ", "DSGD_PLAN_KERNEL",
         "DSGD_VT", "DSGD_RP64_FUSED", "DSGD_CS_HOST_LAYOUT", "DSGD_REQ_PLAN")
_ORACLES = {}


@pytest.fixture(autouse=True)
def _product_defaults(monkeypatch):
    """every test starts from the product's dispatch (other modules pin knobs for their whole run) and sets its own"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def oracle_of(name, data, n_train):
    if name not in _ORACLES:
        o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
        o.set_dim_sparsity(o.dim_sparsity(n_train))
        _ORACLES[name] = o
    return _ORACLES[name]


def sets():
    """name -> (data, n_train)"""
    return {"A": (rl.matrix_a(), rl.N_TRAIN_A), "B": (rl.matrix_b(), rl.N_TRAIN_B), "A_long": (rl.matrix_a_long(), rl.N_TRAIN_A)}


def load(eng, name, table=None, w0=None):
    """load + dimSparsity (+ weights); returns (oracle, dimSparsity as built, column ranks)"""
    data, n_train = (table or sets())[name]
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    ds = eng.build_dim_sparsity(n_train)
    if w0 is not None:
        eng.set_weights(w0)
    return oracle_of((name, data.dim), data, n_train), ds, eng.column_ranks()


def same(x, y, what=""):
    """bit-equal observations (arrays by their bytes: -0.0 and 0.0 differ)"""
    assert type(x) is type(y), (what, type(x), type(y))
    if isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), \
            "%s: %d of %d entries differ" % (what, int((x != y).sum()), x.size)
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), what
        for i, (a, b) in enumerate(zip(x, y)):
            same(a, b, "%s[%d]" % (what, i))
    elif isinstance(x, dict):
        assert x.keys() == y.keys(), what
        for k in x:
            same(x[k], y[k], "%s[%r]" % (what, k))
    else:
        assert x == y, (what, x, y)


def reload_vs_fresh(run, seq=("A", "B"), table=None, precision="fp32", w_seed=5, attach=None, sharp=True):
    """R: every matrix of seq in turn, `run` on each; F: a fresh context on the last one.  run(eng, oracle, name) makes the
    family's calls from the weights it finds and returns its observations (anything `same` compares).  Returns (R's
    observations per load, F's)."""
    table = table or sets()
    dim = table[seq[0]][0].dim
    w0 = rl.nonzero_weights(w_seed, dim=dim, n=min(6000, dim // 2))
    w0 = w0.astype(np.float64) if precision == "fp64" else w0
    obs = []
    with dsgd_amd.Engine(dim, LAM, precision=precision) as r:
        if attach:
            attach(r)
        for name in seq:
            o, ds, ranks = load(r, name, table, w0)
            obs.append({"ds": ds, "ranks": ranks, "run": run(r, o, name), "w": r.get_weights()})
    with dsgd_amd.Engine(dim, LAM, precision=precision) as f:
        if attach:
            attach(f)
        o, ds, ranks = load(f, seq[-1], table, w0)
        fresh = {"ds": ds, "ranks": ranks, "run": run(f, o, seq[-1]), "w": f.get_weights()}
    same(obs[-1], fresh, "reloaded vs fresh on %s" % seq[-1])
    if sharp:   # the loads differ where it matters: another ranking, another dimSparsity, another result
        assert not np.array_equal(obs[-2]["ranks"], obs[-1]["ranks"])
        assert not np.array_equal(obs[-2]["ds"], obs[-1]["ds"])
        assert not np.array_equal(obs[-2]["w"], obs[-1]["w"])
    return obs, fresh


def seen(eng):
    return {"kernel": eng.grad_kernel_name(), "shift": eng.tuning_info()["fix_shift"], "w": eng.get_weights()}


# ---- row ranges ---------------------------------------------------------------------------------------------------------------
RANGES = ([(0, 8000)], [(0, 4000), (4000, 8000)], [(5, 300)])
RANGE_FAMILIES = {
    "row_wise": ({"DSGD_TCOL": "0", "DSGD_FSTEP": "0"}, "dsgd_mb_grad_kernel"),
    "column_lists": ({}, "dsgd_tc_grad_kernel"),
    "row_chunks": ({"DSGD_TCOL": "0", "DSGD_FSTEP_MIN": "1000"}, "dsgd_fstep_kernel"),
    "streaming": ({"DSGD_TCOL": "0", "DSGD_FSTEP": "0", "DSGD_STREAM_MIN": "4096"}, "dsgd_wseg_kernel<true>"),
    "streaming_hsplit_3000": ({"DSGD_TCOL": "0", "DSGD_FSTEP": "0", "DSGD_STREAM_MIN": "4096", "DSGD_HSPLIT": "3000"}, "dsgd_wseg_kernel<true>"),
}


def run_ranges(ranges_list, kernel, small=1000):
    def run(eng, o, name):
        out = []
        for ranges in ranges_list:
            rows = sum(b - a for a, b in ranges)
            ratio, shift, _ = ranged_step(o, eng, ranges, 0.5 * 100 / rows * len(ranges))
            out.append((seen(eng), shift))
            if rows >= small:   # (the small range is the row-wise kernel's in every family)
                assert eng.grad_kernel_name() == kernel, (name, ranges, eng.grad_kernel_name())
            else:
                assert eng.grad_kernel_name() == "dsgd_mb_grad_kernel"
        out.append(eng.loss_acc(0, 4000))
        return out
    return run


@pytest.mark.parametrize("family", list(RANGE_FAMILIES))
def test_row_ranges_after_a_reload(monkeypatch, family):
    """the cached layouts are keyed by the row ranges ALONE: the same ranges on A warm them, then on B; and back on A, whose
    12,000 rows are more than the scratch was last sized for (A -> B -> A against a fresh context on A)"""
    env, kernel = RANGE_FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run = run_ranges(RANGES, kernel)
    reload_vs_fresh(run, ("A", "B"))
    reload_vs_fresh(run, ("A", "B", "A"))


def test_row_ranges_on_the_narrow_pair(monkeypatch):
    """D = 3,000: every rank in the hot stream, no cold stream to rebuild -- 6,000 rows, then 4,000"""
    monkeypatch.setenv("DSGD_TCOL", "0")
    monkeypatch.setenv("DSGD_FSTEP", "0")
    monkeypatch.setenv("DSGD_STREAM_MIN", "2048")
    n1, n2 = rl.narrow_pair()
    table = {"N1": (n1, 4800), "N2": (n2, 3200)}
    reload_vs_fresh(run_ranges(([(0, 3800)], [(0, 1900), (1900, 3800)], [(5, 300)]), "dsgd_wseg_kernel<true>"), ("N1", "N2"), table=table)
    reload_vs_fresh(run_ranges(([(0, 3800)], [(5, 300)]), "dsgd_wseg_kernel<true>"), ("N2", "N1", "N2"), table=table)


# ---- per-request calls --------------------------------------------------------------------------------------------------------
def run_requests(eng, o, name):
    out = []
    for k, b in ((3, 100), (1, 700)):
        list_step(o, eng, rl.lists_inside(k, b, seed=3), 0.5 * 100 / b, "reload_requests")
        out.append(seen(eng))
    idx = rl.lists_inside(1, 300, seed=4)[0]
    w = eng.get_weights().astype(np.float64)
    g, st = eng.gradient(idx)
    g_o = o.gradient(w, idx)
    # (the statements of test_gradient_and_forward_against_oracle_with_given_weights / test_async_steps_against_oracle: the
    #  stated tolerance, exact integers, unless the oracle sees a row within 1e-5 of the gate)
    near = o.last_stats["min_abs_margin"] < GATE_EPS
    assert near or (st["n_active"] == o.last_stats["n_active"] and np.abs(g - g_o).max() <= 1e-5 * max(1.0, np.abs(g_o).max()))
    rows = np.arange(0, 7000, 7, dtype=np.int32)
    pred = eng.forward(rows)
    out += [g, st, pred]
    n = 9000 if name == "B" else 12000
    whole, part = eng.loss_acc(0, n), eng.loss_acc(7200, 8800)   # (the lane group of these kernels follows the mean row length)
    loss_o, acc_o, counts_o, mam = o.loss_acc(w, 7200, 8800)
    assert mam < GATE_EPS or (list(part[2]) == list(counts_o) and part[1] == acc_o)
    assert mam < GATE_EPS or abs(part[0] - loss_o) <= 1e-5 * max(1.0, abs(loss_o))
    _, _, _, mam_all = o.loss_acc(w, 0, 7000)
    assert mam_all < GATE_EPS or bool((pred == o.forward(w, rows)).all())
    out += [whole, part]
    idx1 = rl.lists_inside(1, 100, seed=6)[0]
    delta, st = eng.async_step(idx1, 0.5, want_delta=True)
    w_o = w.copy()
    d_o = o.async_step(w_o, idx1, 0.5, want_delta=True)
    if not (o.last_stats["min_abs_margin"] < GATE_EPS and st["n_active"] != o.last_stats["n_active"]):
        assert st["n_active"] == o.last_stats["n_active"]
        np.testing.assert_allclose(eng.get_weights(), w_o, rtol=0, atol=1e-5 * max(1.0, float(np.abs(w_o).max())))
        np.testing.assert_allclose(delta, d_o, rtol=0, atol=1e-5 * max(1.0, float(np.abs(d_o).max())))
    out += [delta, st, seen(eng)]
    return out


@pytest.mark.parametrize("cs_req", [None, "1"])
def test_per_request_calls_after_a_reload(monkeypatch, cs_req):
    if cs_req:
        monkeypatch.setenv("DSGD_CS_REQ", cs_req)
    obs, _ = reload_vs_fresh(run_requests)
    assert obs[0]["run"][0]["kernel"] == ("dsgd_cs_request_kernel" if cs_req else "dsgd_mb_grad_kernel")


# ---- plans created after the reload ---------------------------------------------------------------------------------------------
def run_plans(shapes, helper, kernel):
    def run(eng, o, name):
        out = []
        for k, b in shapes:
            lists = rl.lists_inside(k, b, seed=7)
            helper(o, eng, lists, min(0.5 * 100 / b, 1.0), "reload_plans")
            # (the warm-up on A runs the family; on B the 4 x 200 step of 150-entry rows may exceed a slice's slots and take
            #  the row-parallel kernels -- in R exactly as in F, which `same` holds)
            assert eng.grad_kernel_name() == kernel or (name == "B" and (k, b) == (4, 200)), (name, k, b, eng.grad_kernel_name())
            out.append(seen(eng))
        return out
    return run


@pytest.mark.parametrize("form", ["column_slices", "one_workgroup", "virtual_tiles"])
def test_plans_created_after_a_reload(monkeypatch, form):
    if form == "column_slices":
        run = run_plans(((3, 100), (4, 200)), rp_plan_step, "dsgd_cs_step_kernel")
    elif form == "one_workgroup":
        monkeypatch.setenv("DSGD_CS", "0")
        run = run_plans(((1, 100),), rp_plan_step, "dsgd_plan_kernel")
    else:
        monkeypatch.setenv("DSGD_CS", "0")
        run = run_plans(((1, 4096),), rp_plan_step, "dsgd_vt_grad_kernel")
    reload_vs_fresh(run)


def test_a_device_drawn_plan_after_a_reload():
    """plan_from_seed over three splits of the loaded train rows: the lists equal the fresh context's, and so does the epoch"""
    def run(eng, o, name):
        n_train = rl.N_TRAIN_B if name == "B" else rl.N_TRAIN_A
        third = n_train // 3
        plan, n_steps, _, _ = eng.plan_from_seed(12345, [(0, third), (third, 2 * third), (2 * third, n_train)], 600, 100)
        assert n_steps == 6 and plan.info()["kind"] == "column_slices"
        idx, offsets = eng.plan_lists(plan)
        assert idx.min() >= 0 and idx.max() < n_train
        # the first step against the oracle through the suite's helper, the epoch's other steps through the drawn plan itself
        cs_plan_step(o, eng, [idx[offsets[i]:offsets[i + 1]] for i in range(3)], 0.5, "reload_drawn_plan")
        eng.plan_run(plan, 1, n_steps, 0.5)
        st = eng.synchronize()
        plan.destroy()
        return [idx, offsets, st, seen(eng)]
    reload_vs_fresh(run)


# ---- plans created BEFORE the reload ------------------------------------------------------------------------------------------
def _plans_that_survive(monkeypatch, env, shape, kind, kernel):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    steps = [rl.lists_inside(shape[0], shape[1], seed=s) for s in (8, 9)]
    lr = min(0.5 * 100 / shape[1], 1.0)
    w0 = rl.nonzero_weights(5)
    with dsgd_amd.Engine(rl.DIM, LAM) as r, dsgd_amd.Engine(rl.DIM, LAM) as f:
        load(r, "A", w0=w0)
        plan = r.plan(steps)
        r.plan_run(plan, 0, 2, lr)
        r.synchronize()
        assert plan.info()["kind"] == kind and r.grad_kernel_name() == kernel   # (warm: the plan's layout belongs to A's ranking)
        w_a = r.get_weights()
        o, ds_r, ranks_r = load(r, "B", w0=w0)
        _, ds_f, ranks_f = load(f, "B", w0=w0)
        same([ds_r, ranks_r], [ds_f, ranks_f])
        fresh = f.plan(steps)
        for eng, p in ((r, plan), (f, fresh)):
            assert p.info()["kind"] in (kind, "not_laid_out")   # (laid out again at the run at the latest)
            eng.plan_run(p, 0, 2, lr)
            eng.synchronize()
        same([plan.info(), seen(r)], [fresh.info(), seen(f)], "a plan from before the load vs one created after it")
        assert plan.info()["kind"] == kind and r.grad_kernel_name() == kernel
        assert not np.array_equal(r.get_weights(), w_a)
        # ... and the same steps hold to the oracle from the same start (F only: R is bit-equal to it)
        f.set_weights(w0)
        helper = cs_plan_step if kind == "column_slices" else rp_plan_step
        w1 = None
        for lists in steps:
            helper(o, f, lists, lr, "reload_old_plan")
            w1 = f.get_weights()
        same(w1, r.get_weights(), "one plan per step vs the plan of both")
        plan.destroy()
        fresh.destroy()


@pytest.mark.parametrize("form", ["column_slices", "virtual_tiles", "one_workgroup"])
def test_a_plan_from_before_the_reload_whose_lists_fit(monkeypatch, form):
    env, shape, kind, kernel = {"column_slices": ({}, (3, 100), "column_slices", "dsgd_cs_step_kernel"),
                                "virtual_tiles": ({"DSGD_CS": "0"}, (1, 4096), "virtual_tiles", "dsgd_vt_grad_kernel"),
                                "one_workgroup": ({"DSGD_CS": "0"}, (1, 100), "one_workgroup", "dsgd_plan_kernel")}[form]
    _plans_that_survive(monkeypatch, env, shape, kind, kernel)


@pytest.mark.parametrize("drawn", [False, True])
def test_a_plan_that_reaches_beyond_the_new_rows_is_refused_and_runs_again_later(drawn):
    """host-given lists, or lists the device drew over A's splits (trusted unseen when they were made): after B is loaded the run
    returns DSGD_ERANGE before anything is enqueued, the weights keep their bits, the context and the plan stay usable, and
    under A again the plan equals a fresh one"""
    w0 = rl.nonzero_weights(5)
    with dsgd_amd.Engine(rl.DIM, LAM) as r, dsgd_amd.Engine(rl.DIM, LAM) as f:
        load(r, "A", w0=w0)
        if drawn:
            third = rl.N_TRAIN_A // 3
            plan, n_steps, _, _ = r.plan_from_seed(777, [(0, third), (third, 2 * third), (2 * third, rl.N_TRAIN_A)], 300, 100)
            idx, offsets = r.plan_lists(plan)
            assert idx.max() >= rl.ROWS_B   # (the third split lies beyond B's rows)
        else:
            steps = [rl.lists_inside(3, 100, seed=8), rl.lists_beyond_b(3, 100, seed=2)]
            plan, n_steps = r.plan(steps), 2
            idx, offsets = r.plan_lists(plan)
        r.plan_run(plan, 0, n_steps, 0.5)
        r.synchronize()
        assert r.grad_kernel_name() == "dsgd_cs_step_kernel"
        o, _, _ = load(r, "B", w0=w0)
        before = r.get_weights()
        for call in (lambda: r.plan_run(plan, 0, n_steps, 0.5), lambda: r.plan_run(plan, 0, 1, 0.5), plan.info):
            with pytest.raises(dsgd_amd.DsgdError) as e:
                call()
            assert e.value.code == dsgd_amd._lib.ERANGE, e.value
        st = r.synchronize()
        assert st["n_samples"] == 0
        same(r.get_weights(), before, "the weights behind a refused run")
        list_step(o, r, rl.lists_inside(3, 100, seed=3), 0.5, "reload_after_refusal")   # the next valid call works
        load(r, "A", w0=w0)
        load(f, "A", w0=w0)
        fresh = f.plan_flat(idx, offsets, n_steps, 3)
        for eng, p in ((r, plan), (f, fresh)):
            eng.plan_run(p, 0, n_steps, 0.5)
            eng.synchronize()
        same([plan.info(), seen(r)], [fresh.info(), seen(f)], "the refused plan under A again vs a fresh one")
        assert plan.info()["kind"] == "column_slices"
        plan.destroy()
        fresh.destroy()


def test_longer_rows_at_the_same_row_count_leave_the_one_workgroup_kernel(monkeypatch):
    """A -> A_long: the plan's 100 rows grow to 3,000 entries each, 2,400 work items where the staged sub-batch holds 192"""
    monkeypatch.setenv("DSGD_CS", "0")
    w0 = rl.nonzero_weights(5)
    lists = [rl.LONG_LIST]
    with dsgd_amd.Engine(rl.DIM, LAM) as r, dsgd_amd.Engine(rl.DIM, LAM) as f:
        load(r, "A", w0=w0)
        plan = r.plan([lists])
        assert plan.info()["kind"] == "one_workgroup"
        r.plan_run(plan, 0, 1, 0.5)
        r.synchronize()
        assert r.grad_kernel_name() == "dsgd_plan_kernel"
        w_a = r.get_weights()
        o, ds_r, ranks_r = load(r, "A_long", w0=w0)
        _, ds_f, ranks_f = load(f, "A_long", w0=w0)
        same([ds_r, ranks_r], [ds_f, ranks_f])
        assert plan.info()["kind"] != "one_workgroup"
        fresh = f.plan([lists])
        assert fresh.info()["kind"] != "one_workgroup"
        for eng, p in ((r, plan), (f, fresh)):
            eng.plan_run(p, 0, 1, 0.5)
            eng.synchronize()
        same([plan.info(), seen(r)], [fresh.info(), seen(f)])
        assert r.grad_kernel_name() != "dsgd_plan_kernel" and not np.array_equal(r.get_weights(), w_a)
        f.set_weights(w0)
        rp_plan_step(o, f, lists, 0.5, "reload_long_rows")
        same(f.get_weights(), r.get_weights())
        plan.destroy()
        fresh.destroy()


# ---- resident vectors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_resident_vectors_keep_their_bits_across_a_load(precision):
    a, n_a = sets()["A"]
    b, _ = sets()["B"]
    w0 = rl.nonzero_weights(5)
    with dsgd_amd.Engine(rl.DIM, LAM, precision=precision) as eng:
        eng.load_csr(a.row_ptr, a.col, a.val, a.label)
        ds = eng.build_dim_sparsity(n_a)
        eng.set_weights(w0.astype(np.float64) if precision == "fp64" else w0)
        plan = eng.plan([rl.lists_inside(3, 100, seed=8)])
        eng.plan_run(plan, 0, 1, 0.5)   # (leaves the weights slice-major)
        eng.synchronize()
        assert eng.grad_kernel_name() == ("dsgd_cs64_step_kernel" if precision == "fp64" else "dsgd_cs_step_kernel")
        eng.load_csr(b.row_ptr, b.col, b.val, b.label)
        w_after = eng.get_weights()
        k_after, v_after = eng.get_weights_sparse()
        ds_after = eng.get_dim_sparsity() if precision == "fp64" else None
        # the same state without the load in between
        eng.load_csr(a.row_ptr, a.col, a.val, a.label)
        same(eng.get_weights(), w_after, "weights across two loads")
        plan.destroy()
    with dsgd_amd.Engine(rl.DIM, LAM, precision=precision) as ref:
        ref.load_csr(a.row_ptr, a.col, a.val, a.label)
        same(ref.build_dim_sparsity(n_a), ds)
        ref.set_weights(w0.astype(np.float64) if precision == "fp64" else w0)
        plan = ref.plan([rl.lists_inside(3, 100, seed=8)])
        ref.plan_run(plan, 0, 1, 0.5)
        ref.synchronize()
        same(ref.get_weights(), w_after, "weights before the load vs after it")
        k, v = ref.get_weights_sparse()
        same([k, v], [k_after, v_after], "sparse weights")
        if precision == "fp64":
            same(ref.get_dim_sparsity(), ds_after, "dimSparsity across the load")
        plan.destroy()
    assert not np.array_equal(w_after, w0.astype(w_after.dtype))
    assert np.array_equal(k_after, np.flatnonzero(np.abs(w_after) > 1e-20))


def test_resident_dim_sparsity_fp32_is_what_the_next_step_uses():
    """fp32 has no getter for dimSparsity: a step on B WITHOUT building it again uses A's values -- equal to a fresh context on B
    that was GIVEN A's dimSparsity"""
    a, n_a = sets()["A"]
    b, _ = sets()["B"]
    w0 = rl.nonzero_weights(5)
    lists = rl.lists_inside(3, 100, seed=3)
    with dsgd_amd.Engine(rl.DIM, LAM) as r, dsgd_amd.Engine(rl.DIM, LAM) as f:
        r.load_csr(a.row_ptr, a.col, a.val, a.label)
        ds_a = r.build_dim_sparsity(n_a)
        r.sync_step(lists, 0.5)
        r.load_csr(b.row_ptr, b.col, b.val, b.label)
        r.set_weights(w0)
        st_r = r.sync_step(lists, 0.5)
        f.load_csr(b.row_ptr, b.col, b.val, b.label)
        f.set_dim_sparsity(ds_a)
        f.set_weights(w0)
        st_f = f.sync_step(lists, 0.5)
        same([st_r, r.get_weights()], [st_f, f.get_weights()])


# ---- the lock-free engine with one worker (deterministic) -------------------------------------------------------------------------
def test_one_worker_lock_free_engine_after_a_reload():
    def run(eng, o, name):
        begin, end, batch, n_upd = 1000, 4000, 100, 30
        w_ref = eng.get_weights().astype(np.float64)
        eng.async_start([(begin, end)], batch=batch, lr=0.5, max_updates=n_upd, seed=77, positional_bug=False)
        eng.async_wait()
        updates, running = eng.async_updates()
        assert updates == n_upd and not running
        exposed = False
        for it in range(n_upd):
            o.async_step(w_ref, hog_rows(77, 0, it, begin, end - begin, batch, False), 0.5)
            exposed = exposed or o.last_stats["min_abs_margin"] < 1e-5
        w = eng.get_weights()
        # (the statement of test_hogwild_single_worker_replays_the_oracle)
        assert exposed or np.abs(w.astype(np.float64) - w_ref).max() <= 4e-5 * max(1.0, np.abs(w_ref).max())
        return [w, updates]
    reload_vs_fresh(run)


# ---- the fp64 mode -------------------------------------------------------------------------------------------------------------
def run_fp64(eng, o, name):
    out = []
    double = eng.value_bits() == 64
    w = eng.get_weights()
    lists = rl.lists_inside(3, 100, seed=3)
    st = eng.sync_step_f64(lists, 0.5)
    out += [st, seen(eng)]
    if not double:   # (the oracle holds float values)
        w_o = w.copy()
        o.sync_step(w_o, lists, 0.5)
        assert st["n_active"] == o.last_stats["n_active"] or o.last_stats["min_abs_margin"] < 1e-9
        if st["n_active"] == o.last_stats["n_active"]:
            assert np.abs(eng.get_weights() - w_o).max() <= 1e-12 * max(1.0, np.abs(w_o).max())   # (tests/test_gpu_fp64_requests.py)
    g, st = eng.gradient_f64(rl.lists_inside(1, 700, seed=4)[0])
    out += [g, st]
    steps = [rl.lists_inside(3, 100, seed=s) for s in (11, 12, 13)]
    idx = np.concatenate([l for s in steps for l in s])
    offsets = np.arange(0, 901, 100, dtype=np.int64)
    out += [eng.sync_steps_f64(idx, offsets, 3, 3, 0.5, per_step=True), seen(eng)]
    if not double:   # (plans are refused on Double data)
        plan = eng.plan(steps)
        eng.plan_run(plan, 0, 3, 0.5)
        eng.synchronize()
        assert eng.grad_kernel_name() == "dsgd_cs64_step_kernel"
        plan.destroy()
        out.append(seen(eng))
    delta, st = eng.async_step(rl.lists_inside(1, 100, seed=6)[0], 0.5, want_delta=True)
    out += [delta, st, seen(eng)]
    return out


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("seq", [("A", "B"), ("A", "B64"), ("B64", "A")])
def test_fp64_context_after_a_reload(monkeypatch, seq, fused):
    """float A -> float B, float A -> Double B (values that are no floats), Double B -> float A: every fp64 call bit-equal to a
    fresh fp64 context on the last one"""
    monkeypatch.setenv("DSGD_RP64_FUSED", fused)
    b64 = rl.perturbed_doubles(rl.matrix_b())
    table = dict(sets())
    table["B64"] = (dsgd_amd.synth.Csr(b64.dim, b64.row_ptr, b64.col, b64.val64, b64.label), rl.N_TRAIN_B)
    obs, fresh = reload_vs_fresh(run_fp64, seq, table=table, precision="fp64")
    assert obs[-1]["w"].dtype == np.float64


# ---- a communicator of one rank ----------------------------------------------------------------------------------------------
def test_one_rank_fp32_after_a_reload():
    def run(eng, o, name):
        list_step(o, eng, rl.lists_inside(3, 100, seed=3), 0.5, "reload_one_rank")
        a = seen(eng)
        ranged_step(o, eng, [(0, 8000)], 0.5 * 100 / 8000)
        return [a, seen(eng), eng.loss_acc(0, 4000)]
    reload_vs_fresh(run, attach=lambda e: e.comm_init(dsgd_amd.Engine.comm_unique_id(), 1, 0))


def test_one_rank_fp64_after_a_reload():
    """dsgd_comm_init_f64v: the agreed vexp is the communicator's only until the next load (B's values are 8 times A's)"""
    def run(eng, o, name):
        w = eng.get_weights()
        lists = rl.lists_inside(3, 100, seed=3)
        st = eng.sync_step_f64(lists, 0.5)
        w_o = w.copy()
        o.sync_step(w_o, lists, 0.5)
        if st["n_active"] == o.last_stats["n_active"]:
            assert np.abs(eng.get_weights() - w_o).max() <= 1e-12 * max(1.0, np.abs(w_o).max())
        return [st, seen(eng), eng.loss_acc(0, 4000)]
    reload_vs_fresh(run, precision="fp64", attach=lambda e: e.comm_init_f64v(dsgd_amd.Engine.comm_unique_id(), 1, 0))
