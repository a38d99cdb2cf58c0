"""-m gpu: the device code and host paths that only a knob selects (csrc/dsgd_route.hpp, KNOBS[]), each run on the GPU.
tests/cpp/route_test.cpp holds the DECISIONS on the CPU; here the kernels and paths those decisions select run.

Every variant gets two statements.
 (A) AGAINST THE fp64 ORACLE under the family's own criterion: the derived per-coordinate bound of oracle/bounds.py with the
     shift the launch reports and active-row counts within the near-gate rows (list_step / ranged_step of
     tests/test_gpu_parity.py; for plans the statements of tests/test_gpu_cs.py: every step as a launch of its own under
     that bound, and a launch of several steps equal to them BIT FOR BIT).  No new tolerance.
 (B) BIT-EQUAL TO THE DEFAULT VARIANT: two contexts on the same data from the same weights, one with the knob, one without;
     bits() of the weights and n_active equal.  Asserted wherever the knob changes only staging, waiting, grid size or the
     lane count over integer (fixed-point) column sums.  Two cases where reading the kernels shows otherwise:
       * DSGD_CS_NT=256 changes a FLOAT sum's order: a slice's share of w . ds (cs_wds_share<NT>: lane t adds the quads
         t, t + NT, ...; cs_block_sum<NT>: NT / 64 wave sums), so s = 2 lambda (w . ds) may differ in its last bits and with
         it every regularised column.  (B) is asserted at lambda = 0, where s is an exact 0 and everything else -- the slots'
         partial dots, the rows' sums in slot order, the exchange in slice order, the integer column sums -- is the same
         arithmetic; at lambda = 1e-5 the narrow kernel is held to (A).
       * DSGD_VT_TPW sizes the grid, and the fixed-point shift of a step follows the rows ONE workgroup can meet
         (csrc/dsgd_layout_host.hpp, vt_tables: shift = min(21, 30 - bits(worst))): a coarser grid may run on a coarser
         shift, which is another fixed-point grid.  (B) is asserted for every step on which both contexts report the same
         shift (k3b100 always: 300 rows cannot exceed 512 in one workgroup); a step whose shifts differ keeps (A).
"""

import numpy as np
import pytest

import dsgd_amd
import waivers
from conftest import has_gpu
from hard_data import ragged_data
from oracle import bounds as orb
from oracle.hogwild_replay import hog_rows
from test_gpu_hard_values import KNOBS as HARD_KNOBS, bits
from test_gpu_parity import GATE_EPS, batches, list_step, make_pair, ranged_step, tol

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
KNOBS = HARD_KNOBS + ("DSGD_CS_NT", "DSGD_PLAN_PROF", "DSGD_REQ_MAPPED", "DSGD_REQ_SPIN", "DSGD_VT_TPW", "DSGD_CS_MAX_MB", "DSGD_CACHE_MB",
                      "DSGD_FSTEP_REBALANCE", "DSGD_FIX_BOUND", "DSGD_FSTEP_DUMP")
CS, VT, MB, ONE_WG, FSTEP, TCOL = ("dsgd_cs_step_kernel", "dsgd_vt_grad_kernel", "dsgd_mb_grad_kernel", "dsgd_plan_kernel", "dsgd_fstep_kernel",
                                   "dsgd_tc_grad_kernel")
N_ROWS, N_TRAIN = 6000, 4800
ROW_CHUNKS = {"DSGD_TCOL": "0", "DSGD_FSTEP_MIN": "4096"}   # (the row_chunks family of tests/test_gpu_hard_values.py)
# TcolGate (csrc/dsgd_route.hpp; tests/cpp/route_test.cpp states them): layouts built in a row, steps sat out, the streak it resumes with
GATE_MISSES, GATE_COOLDOWN, GATE_RESUME = 12, 256, 8


def pin(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_DATA = {}


def data_of(seed, ragged=False):
    key = (seed, ragged)
    if key not in _DATA:
        _DATA[key] = ragged_data(seed, N_ROWS) if ragged else dsgd_amd.synth.generate(N_ROWS, seed=seed)
    return _DATA[key]


def context(monkeypatch, env, data, lam=LAM, warm=True):
    """(oracle, engine) created under `env` (knobs are read at dsgd_create), one default step in: non-zero weights"""
    pin(monkeypatch, env)
    o, eng = make_pair(data, lam, N_TRAIN)
    logged(eng)
    if warm:
        eng.sync_step(batches(np.random.default_rng(1), N_TRAIN, 3, 100, 1)[0], 0.5)
    return o, eng


def logged(eng):
    """keep the statistics of the engine's last step in eng.last_st (list_step / ranged_step return ratios, not statistics)"""
    for name in ("sync_step", "sync_step_ranges"):
        def run(*a, _fn=getattr(eng, name), **kw):
            eng.last_st = _fn(*a, **kw)
            return eng.last_st
        setattr(eng, name, run)


def same_bits(e_knob, e_default, where):
    a, b = e_knob.get_weights(), e_default.get_weights()
    assert e_knob.last_st == e_default.last_st, (where, e_knob.last_st, e_default.last_st)
    assert np.array_equal(bits(a), bits(b)), "%s: %d coordinates differ from the default variant" % (where, int((bits(a) != bits(b)).sum()))


def lr_of(lists):
    return min(0.5 * 100 / max(len(a) for a in lists), 0.5)


def stated_step(o, eng, lists, lr):
    """A per-request step of the ONE-WORKGROUP kernel from the engine's weights.  It adds its cold ranks in FLOAT
    (csrc/dsgd_batch.hpp, gcold), so not every column sum is on the fixed-point grid the derived bound prices: this family's
    standing criterion is run_sync's (tests/test_gpu_parity.py) -- equal active-row counts and the stated
    1e-5 * max(1, |w|_inf), waived only for a row within 1e-5 of the gate."""
    w_ref = eng.get_weights().astype(np.float64)
    st = eng.sync_step(lists, lr)
    o.sync_step(w_ref, lists, lr)
    assert st["n_samples"] == sum(len(a) for a in lists)
    err = float(np.abs(eng.get_weights() - w_ref).max())
    ok = st["n_active"] == o.last_stats["n_active"] and err <= tol(w_ref)
    waivers.tight("variants:one_workgroup:step", ok, o.last_stats["min_abs_margin"] < GATE_EPS, "err %.3g" % err)


def plan_steps(o, eng, plan, steps, lr, kernel, kind):
    """(A) for a resident plan, the statements of tests/test_gpu_cs.py: every step as ONE launch from the engine's weights
    under the derived bound with the shift that launch reports, then the whole plan in one launch and in two, bit-equal to
    the steps.  Returns (the final weights, active rows of the whole-plan launch, the shift of every step)."""
    w_start = eng.get_weights()
    eng.synchronize()
    shifts, near_any = [], False
    for s, lists in enumerate(steps):
        w0 = eng.get_weights().astype(np.float64)
        w_ref = w0.copy()
        eng.plan_run(plan, s, s + 1, lr)
        st = eng.synchronize()
        assert kernel in eng.grad_kernel_name(), (eng.grad_kernel_name(), kernel)
        shift = eng.tuning_info()["fix_shift"]
        shifts.append(shift)
        o.sync_step(w_ref, lists, lr)
        tol_v, n_near, near_part = orb.list_bound(o, w0, w_ref, lists, lr, shift, parts=True)
        assert st["n_samples"] == sum(len(a) for a in lists)
        assert abs(st["n_active"] - o.last_stats["n_active"]) <= n_near, (st, o.last_stats, n_near)
        w = eng.get_weights()
        if kernel == ONE_WG:
            # the one-workgroup kernel adds its cold ranks in FLOAT (csrc/dsgd_batch.hpp, gcold): not every column sum is on the
            # fixed-point grid the derived bound prices, and this family's standing criterion is run_sync's stated tolerance
            # (tests/test_gpu_parity.py, test_plan_kernel_and_multi_launch_path_agree_with_the_oracle)
            err = float(np.abs(w - w_ref).max())
            ok = st["n_active"] == o.last_stats["n_active"] and err <= tol(w_ref)
            waivers.tight("variants:one_workgroup:step", ok, o.last_stats["min_abs_margin"] < GATE_EPS, "err %.3g" % err)
            near_any = near_any or o.last_stats["min_abs_margin"] < GATE_EPS
            continue
        ratio, j = orb.worst_ratio(w, w_ref, tol_v)
        assert ratio <= 1.0, "step %d, coordinate %d: error %.3g x its derived bound (shift %d, %d rows near the gate)" % (s, j, ratio, shift, n_near)
        if kernel == CS:
            assert np.abs(w - w_ref).max() <= tol(w_ref) or n_near > 0
        tight = st["n_active"] == o.last_stats["n_active"] and orb.worst_ratio(w, w_ref, tol_v - near_part)[0] <= 1.0
        waivers.tight("variants:plan_step:gates_as_the_oracle", tight, n_near > 0, "%d rows near the gate" % n_near)
        near_any = near_any or n_near > 0
    assert plan.info()["kind"] == kind, plan.info()
    w_steps = eng.get_weights()
    n = len(steps)
    eng.set_weights(w_start)
    eng.plan_run(plan, 0, n, lr)
    st_all = eng.synchronize()
    assert st_all["n_samples"] == sum(len(a) for ls in steps for a in ls)
    w_all = eng.get_weights()
    if kernel == CS:   # (tests/test_gpu_cs.py: the same slices, sums and order either way; s is carried as a launch derives it)
        assert np.array_equal(bits(w_all), bits(w_steps)), "one launch of %d steps differs from its steps" % n
    else:              # (tests/test_gpu_parity.py, test_plan_run_equals_step_by_step: s is carried across the steps of a run)
        err = float(np.abs(w_all.astype(np.float64) - w_steps).max())
        waivers.tight("variants:plan_run:replay", err <= tol(w_steps), near_any, "err %.3g" % err)
    if n > 2:
        eng.set_weights(w_start)
        eng.plan_run(plan, 0, n // 2 + 1, lr)
        eng.plan_run(plan, n // 2 + 1, n, lr)
        eng.synchronize()
        assert kernel != CS or np.array_equal(bits(eng.get_weights()), bits(w_all))
    assert not np.array_equal(w_all, w_start)
    return w_all, st_all["n_active"], shifts


def run_plan(eng, steps, lr, w_start):
    """the whole plan in one launch from w_start: (weights, stats, plan.info())"""
    eng.set_weights(w_start)
    plan = eng.plan(steps)
    eng.synchronize()
    eng.plan_run(plan, 0, len(steps), lr)
    st = eng.synchronize()
    info = plan.info()
    plan.destroy()
    return eng.get_weights(), st, info


# ---- 1. narrow column slices: dsgd_cs_step_kernel<CS_THREADS_NARROW, 2, 8> ------------------------------------------------------
@pytest.mark.parametrize("cs_g", [None, "16"])
def test_narrow_column_slices(monkeypatch, cs_g):
    """DSGD_CS_NT=256.  plan.info()["threads"] (dsgd_plan_info word [8]) says which width a plan's launches take: 256 where
    narrow_fits holds (k1b100, k3b100), 512 for 4 x 200 (800 rows in a step: more than 2 x 256 lane positions).  Eight steps
    and more per plan: the next step's slots ride in registers across the exchange."""
    data = data_of(41)
    env = {"DSGD_CS_NT": "256"}
    if cs_g:
        env["DSGD_CS_G"] = cs_g
    base = {k: v for k, v in env.items() if k != "DSGD_CS_NT"}
    rng = np.random.default_rng(41)
    cases = [(1, 100, 9, 256), (3, 100, 8, 256), (4, 200, 8, 512)]
    plans = [(k, b, batches(rng, N_TRAIN, k, b, n), threads) for k, b, n, threads in cases]
    # (A) at lambda = 1e-5
    o, eng = context(monkeypatch, env, data)
    with eng:
        for k, b, steps, threads in plans:
            plan = eng.plan(steps)
            info = plan.info()
            assert info["kind"] == "column_slices" and info["threads"] == threads and info["slices"] == (16 if cs_g else 8), info
            assert info["slots_per_lane"] == 2   # (both the narrow kernel and the wide one of 4 x 200: what word [5] cannot tell apart)
            plan_steps(o, eng, plan, steps, lr_of(steps[0]), CS, "column_slices")
            plan.destroy()
    # ... and the default variant says 512 for the same plans (one slot per lane where that fits)
    o, e_def = context(monkeypatch, base, data)
    with e_def:
        for k, b, steps, threads in plans:
            plan = e_def.plan(steps)
            info = plan.info()
            assert info["kind"] == "column_slices" and info["threads"] == 512 and info["slots_per_lane"] == (1 if threads == 256 else 2), info
            plan.destroy()
    # (B) at lambda = 0 (the module's docstring: the one float sum whose order the lane count changes is multiplied by lambda)
    _, e_knob = context(monkeypatch, env, data, lam=0.0)
    _, e_def = context(monkeypatch, base, data, lam=0.0)
    with e_knob, e_def:
        w_start = e_def.get_weights()
        assert w_start.any()
        for k, b, steps, threads in plans:
            w1, st1, info1 = run_plan(e_knob, steps, lr_of(steps[0]), w_start)
            w0, st0, info0 = run_plan(e_def, steps, lr_of(steps[0]), w_start)
            assert info1["threads"] == threads and info0["threads"] == 512
            assert st1 == st0 and 0 < st0["n_active"] < st0["n_samples"]
            assert np.array_equal(bits(w1), bits(w0)), "%d x %d: %d coordinates differ" % (k, b, int((w1 != w0).sum()))
            assert not np.array_equal(w0, w_start)


def test_narrow_knob_leaves_fp64_contexts_on_512_lanes(monkeypatch):
    """cs_build sends an fp64 context to the device builder whatever DSGD_CS_HOST_LAYOUT says, and that builder excludes fp64
    from the narrow width; the host builder, which does not, is unreachable for fp64.  dsgd_cs64_step_kernel has one width."""
    data = data_of(41)
    steps = batches(np.random.default_rng(5), N_TRAIN, 3, 100, 4)
    out = []
    for env in ({"DSGD_CS_NT": "256"}, {"DSGD_CS_NT": "256", "DSGD_CS_HOST_LAYOUT": "1"}, {}):
        pin(monkeypatch, env)
        eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64")
        with eng:
            eng.load_csr(data.row_ptr, data.col, data.val, data.label)
            eng.build_dim_sparsity(N_TRAIN)
            plan = eng.plan(steps)
            info = plan.info()
            assert info["kind"] == "column_slices_fp64" and info["threads"] == 512 and info["device_built"], info
            eng.plan_run(plan, 0, len(steps), 0.5)
            st = eng.synchronize()
            assert eng.grad_kernel_name() == "dsgd_cs64_step_kernel"
            plan.destroy()
            out.append((eng.get_weights(), st))
    for w, st in out[:2]:
        assert st == out[2][1] and np.array_equal(bits(w), bits(out[2][0]))
    assert out[2][0].any()


# ---- 2. phase counters: DSGD_PLAN_PROF=1 ---------------------------------------------------------------------------------------
def counters(eng, launches_word, where):
    """debug_cycles of a profiled context: 16 words, [15] the exact count, some phase word non-zero; reset zeroes them"""
    cyc = eng.debug_cycles(reset=False)
    assert len(cyc) == 16 and cyc[15] == launches_word, (where, cyc)
    assert any(c > 0 for c in cyc[:15]), (where, cyc)
    assert eng.debug_cycles(reset=True) == cyc
    assert eng.debug_cycles(reset=False) == [0] * 16, where
    return cyc


def test_phase_counters_one_workgroup_plan(monkeypatch):
    """dsgd_plan_kernel's counter branches ([15] += the steps of a launch): one worker, DSGD_CS=0"""
    data = data_of(42)
    steps = batches(np.random.default_rng(42), N_TRAIN, 1, 100, 8)
    o, e_prof = context(monkeypatch, {"DSGD_CS": "0", "DSGD_PLAN_PROF": "1"}, data)
    _, e_def = context(monkeypatch, {"DSGD_CS": "0"}, data)
    with e_prof, e_def:
        w_start = e_def.get_weights()
        same_bits(e_prof, e_def, "the warm-up step")
        e_prof.debug_cycles(reset=True)
        plan = e_prof.plan(steps)
        w1, act1, _ = plan_steps(o, e_prof, plan, steps, 0.5, ONE_WG, "one_workgroup")
        plan.destroy()
        counters(e_prof, 3 * len(steps), "one-workgroup plan")   # (plan_steps: every step once, the plan in one launch, and in two)
        w0, st0, info0 = run_plan(e_def, steps, 0.5, w_start)
        assert info0["kind"] == "one_workgroup" and st0["n_active"] == act1
        assert np.array_equal(bits(w1), bits(w0))
        assert e_def.debug_cycles(reset=False) == [0] * 16


def test_phase_counters_column_slice_plan(monkeypatch):
    """dsgd_cs_step_kernel with tprof ([15] += the steps of a launch, thread 0 of slice 0)"""
    data = data_of(42)
    steps = batches(np.random.default_rng(43), N_TRAIN, 3, 100, 8)
    o, e_prof = context(monkeypatch, {"DSGD_PLAN_PROF": "1"}, data)
    _, e_def = context(monkeypatch, {}, data)
    with e_prof, e_def:
        w_start = e_def.get_weights()
        e_prof.debug_cycles(reset=True)
        plan = e_prof.plan(steps)
        w1, act1, _ = plan_steps(o, e_prof, plan, steps, 0.5, CS, "column_slices")
        plan.destroy()
        cyc = counters(e_prof, 3 * len(steps), "column-slice plan")
        assert all(c > 0 for c in cyc[:8]), cyc   # dot, publish, exchange, scatter, sweep, reduce, the set-up, the write-back: all ran
        w0, st0, info0 = run_plan(e_def, steps, 0.5, w_start)
        assert info0["kind"] == "column_slices" and st0["n_active"] == act1
        assert np.array_equal(bits(w1), bits(w0))
        assert e_def.debug_cycles(reset=False) == [0] * 16


def test_phase_counters_row_wise_requests(monkeypatch):
    """dsgd_mb_grad_kernel with tprof ([15] += 1 per launch: wave 0 of workgroup (0, 0))"""
    data = data_of(42)
    rng = np.random.default_rng(44)
    reqs = batches(rng, N_TRAIN, 3, 100, 2) + batches(rng, N_TRAIN, 2, 700, 1)
    o, e_prof = context(monkeypatch, {"DSGD_PLAN_PROF": "1"}, data)
    _, e_def = context(monkeypatch, {}, data)
    with e_prof, e_def:
        assert e_prof.debug_cycles(reset=True)[15] == 1   # (the warm-up step was one launch of this kernel)
        for lists in reqs:
            list_step(o, e_prof, lists, lr_of(lists), "variants:list_step")
            assert e_prof.grad_kernel_name() == MB
            e_def.sync_step(lists, lr_of(lists))
            same_bits(e_prof, e_def, "row-wise request")
        counters(e_prof, len(reqs), "row-wise requests")
        g1, s1 = e_prof.gradient(reqs[0][0])
        g0, s0 = e_def.gradient(reqs[0][0])
        assert s1 == s0 and g0.any() and np.array_equal(bits(g1), bits(g0))
        counters(e_prof, 1, "gradient")
        assert e_def.debug_cycles(reset=False) == [0] * 16


def test_phase_counters_row_chunks_and_the_dump(monkeypatch, tmp_path):
    """dsgd_fstep_kernel with tprof: thread 0 of EVERY workgroup adds 1 to [15] (workgroups x launches); DSGD_FSTEP_DUMP
    (read when dsgd_debug_cycles is called) appends one line per workgroup of the last chunked launch, whose last word packs
    what the chunk held: hot tiles << 8, cold tiles << 24, rows << 40.  The rows must sum to the range's; the tile counts have
    no second source on the host side of the C ABI, so they are required to be there (non-zero in total), no more."""
    data = data_of(42)
    whole, halves = [(0, N_TRAIN)], [(0, N_TRAIN // 2), (N_TRAIN // 2, N_TRAIN)]
    lr = 0.5 * 100 / N_TRAIN
    # the grid fstep_grid (csrc/dsgd_route.hpp) gives: min(CUs per worker, smallest range / DSGD_FSTEP_ROWS) workgroups per worker
    wg_whole, wg_halves = N_TRAIN // 512, 2 * (N_TRAIN // 2 // 512)
    o, e_prof = context(monkeypatch, dict(ROW_CHUNKS, DSGD_PLAN_PROF="1"), data)
    _, e_def = context(monkeypatch, ROW_CHUNKS, data)
    with e_prof, e_def:
        e_prof.debug_cycles(reset=True)
        for ranges, n, wgs in ((halves, 1, wg_halves), (whole, 2, wg_whole)):
            for _ in range(n):
                ranged_step(o, e_prof, ranges, lr * len(ranges))
                assert e_prof.grad_kernel_name() == FSTEP
                e_def.sync_step_ranges(ranges, lr * len(ranges))
                assert e_def.grad_kernel_name() == FSTEP
                same_bits(e_prof, e_def, "row chunks")
            if ranges is whole:
                dump = tmp_path / "fstep_dump.txt"
                monkeypatch.setenv("DSGD_FSTEP_DUMP", str(dump))
            cyc = counters(e_prof, n * wgs, "row chunks")
            assert all(c > 0 for c in cyc[:10]), cyc   # the phases of A, B and C, the workgroups' totals and the slowest one
        monkeypatch.delenv("DSGD_FSTEP_DUMP")
        lines = [ln.split() for ln in dump.read_text().splitlines() if not ln.startswith("#")]
        lines = lines[:len(lines) // 3]   # (counters() read the words three times: the same lines each time)
        assert [int(f[0]) for f in lines] == list(range(wg_whole)), lines
        held = [int(f[4]) for f in lines]
        assert sum((h >> 40) & 0xffff for h in held) == N_TRAIN
        assert all((h >> 40) & 0xffff for h in held) and sum((h >> 8) & 0xffff for h in held) > 0 and sum((h >> 24) & 0xffff for h in held) > 0
        assert all(int(f[2]) >= int(f[1]) > 0 for f in lines)
        assert e_def.debug_cycles(reset=False) == [0] * 16


@pytest.mark.parametrize("trace", [True, False])
def test_phase_counters_lock_free_engine(monkeypatch, trace):
    """dsgd_hogwild_kernel<true, true> (a trace attached) and <true, false>: one worker is deterministic -- the replay of
    test_hogwild_single_worker_replays_the_oracle, and bit for bit an unprofiled engine with the same seed.  [15]: thread 0
    of worker 0 counts its iterations, which with one worker are the updates."""
    data = data_of(12)
    batch, n_upd, begin, end = 100, 40, 1000, 4000
    o, e_prof = context(monkeypatch, {"DSGD_PLAN_PROF": "1"}, data, warm=False)
    _, e_def = context(monkeypatch, {}, data, warm=False)
    with e_prof, e_def:
        for eng in (e_prof, e_def):
            if trace:
                eng.async_set_trace(n_upd)
            eng.async_start([(begin, end)], batch=batch, lr=0.5, max_updates=n_upd, seed=77, positional_bug=False)
            eng.async_wait()
            assert eng.async_updates() == (n_upd, False)
        w_ref = np.zeros(data.dim + 1)
        exposed = False
        for it in range(n_upd):
            o.async_step(w_ref, hog_rows(77, 0, it, begin, end - begin, batch, False), 0.5)
            exposed = exposed or o.last_stats["min_abs_margin"] < GATE_EPS
        w1, w0 = e_prof.get_weights(), e_def.get_weights()
        err = float(np.abs(w1.astype(np.float64) - w_ref).max())
        waivers.tight("variants:hogwild_single_worker", err <= 4 * tol(w_ref), exposed, "err %.3g" % err)
        assert w0.any() and np.array_equal(bits(w1), bits(w0))
        s1, s0 = e_prof.async_stats(), e_def.async_stats()
        assert (s1["updates"], s1["samples"], s1["active"]) == (s0["updates"], s0["samples"], s0["active"]) == (n_upd, n_upd * batch, s0["active"])
        if trace:
            t1, t0 = e_prof.async_read_trace(), e_def.async_read_trace()
            assert len(t1["it"]) == n_upd and all(np.array_equal(t1[k], t0[k]) for k in ("worker", "it", "n_active", "mask", "s"))
        counters(e_prof, n_upd, "lock-free engine")
        assert e_def.debug_cycles(reset=False) == [0] * 16


# ---- 3. request staging: the REQ_MAPPED_ITEMS seam, DSGD_REQ_MAPPED=0, DSGD_REQ_SPIN=0 ---------------------------------------------
def request_of(rng, total, k):
    """k lists of `total` entries in all over the train rows, repeated rows allowed"""
    cuts = [total * i // k for i in range(k + 1)]
    return [rng.integers(0, N_TRAIN, size=cuts[i + 1] - cuts[i]).astype(np.int32) for i in range(k)]


def test_request_staging_across_the_mapped_seam(monkeypatch):
    """stage_lists: up to 16,384 index entries are read in place from a host-mapped buffer, more are copied on the stream into
    d_idx -- mapped, mapped (the last size that is), copied, copied, mapped again inside ONE context; DSGD_REQ_MAPPED=0
    copies every time.  The kernels read the same entries either way: (A) on both, (B) between them, gradient() too."""
    data = data_of(43)
    rng = np.random.default_rng(43)
    reqs = [request_of(rng, n, 3) for n in (16383, 16384, 16385, 40000)] + batches(rng, N_TRAIN, 3, 100, 1)
    o, e_copy = context(monkeypatch, {"DSGD_REQ_MAPPED": "0"}, data)
    _, e_def = context(monkeypatch, {}, data)
    with e_copy, e_def:
        same_bits(e_copy, e_def, "the warm-up step")
        for lists in reqs:
            for eng in (e_def, e_copy):
                list_step(o, eng, lists, lr_of(lists), "variants:list_step")
                assert eng.grad_kernel_name() == MB and eng.last_st["n_samples"] == sum(len(a) for a in lists)
            same_bits(e_copy, e_def, "%d entries" % sum(len(a) for a in lists))
        for lists in reqs[1:3] + reqs[4:]:
            idx = np.concatenate(lists)
            g1, s1 = e_copy.gradient(idx)
            g0, s0 = e_def.gradient(idx)
            assert s1 == s0 and g0.any() and np.array_equal(bits(g1), bits(g0)), len(idx)
            g_ref = o.gradient(e_def.get_weights().astype(np.float64), idx)
            assert np.abs(g0 - g_ref).max() <= 1e-5 * max(1.0, np.abs(g_ref).max()) or o.last_stats["min_abs_margin"] < GATE_EPS


@pytest.mark.parametrize("arm", ["row_wise", "column_slice_request", "one_workgroup_request"])
def test_requests_that_wait_for_the_stream(monkeypatch, arm):
    """DSGD_REQ_SPIN=0: finish_mail(spin = false) waits for the stream instead of polling the mailbox.  Only the one-launch
    arms poll at all (route_request: REQ_CS under DSGD_CS_REQ=1, REQ_ONE_WG_MAIL under DSGD_REQ_PLAN=1); the row-wise arm
    always waits for the stream, so there the knob must change nothing.  The 3 x 100 request takes the arm under test, the
    16,385-entry request is row-wise (and copied) in every arm."""
    base, kernel, k = {"row_wise": ({}, MB, 3), "column_slice_request": ({"DSGD_CS_REQ": "1"}, "dsgd_cs_request_kernel", 3),
                       "one_workgroup_request": ({"DSGD_CS": "0", "DSGD_REQ_PLAN": "1"}, ONE_WG, 1)}[arm]
    data = data_of(43)
    rng = np.random.default_rng(45)
    reqs = batches(rng, N_TRAIN, k, 100, 3) + [request_of(rng, 16385, k)] + batches(rng, N_TRAIN, k, 100, 1)
    o, e_wait = context(monkeypatch, dict(base, DSGD_REQ_SPIN="0"), data)
    _, e_def = context(monkeypatch, base, data)
    with e_wait, e_def:
        for lists in reqs:
            small = sum(len(a) for a in lists) <= 300
            for eng in (e_def, e_wait):
                if small and kernel == ONE_WG:
                    stated_step(o, eng, lists, lr_of(lists))
                else:
                    list_step(o, eng, lists, lr_of(lists), "variants:list_step")
                assert eng.grad_kernel_name() == (kernel if small else MB)
            same_bits(e_wait, e_def, arm)


# ---- 4. the virtual-tile grid: DSGD_VT_TPW ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack_mb", [None, "0"])
def test_virtual_tile_grids(monkeypatch, pack_mb):
    """dsgd_vt_grad_kernel on grids sized for 2 and 4 tiles per wave (vt_tables(..., tpw, ...): gx = tiles / (16 tpw)) against
    the default 1, on ragged rows, with the plan's packed copy and with descriptors only (DSGD_VT_PACK_MB=0)."""
    data = data_of(23, ragged=True)
    rng = np.random.default_rng(23)
    plans = [(k, b, batches(rng, N_TRAIN, k, b, 2)) for k, b in ((3, 100), (2, 700), (1, 4096))]
    base = {"DSGD_CS": "0"}
    if pack_mb is not None:
        base["DSGD_VT_PACK_MB"] = pack_mb
    ref = {}
    for tpw in ("1", "2", "4"):
        o, eng = context(monkeypatch, dict(base, DSGD_VT_TPW=tpw), data)
        with eng:
            w_start = eng.get_weights()
            for k, b, steps in plans:
                eng.set_weights(w_start)
                plan = eng.plan(steps)
                w, act, shifts = plan_steps(o, eng, plan, steps, lr_of(steps[0]), VT, "virtual_tiles")
                plan.destroy()
                if tpw == "1":
                    ref[(k, b)] = (w, act, shifts)
                    continue
                w0, act0, shifts0 = ref[(k, b)]
                print("DSGD_VT_TPW=%s %d x %d: shifts %s against %s" % (tpw, k, b, shifts, shifts0))
                if b == 100:
                    assert shifts == shifts0   # (300 rows in a step: no workgroup of any grid meets more than 512)
                if shifts == shifts0:          # (B): the same fixed-point grid -- integer sums, whatever the workgroups
                    assert act == act0 and np.array_equal(bits(w), bits(w0)), "%d x %d: %d coordinates differ" % (k, b, int((w != w0).sum()))
                else:                          # a coarser shift is another grid (the module's docstring): (A) held above
                    assert all(s <= s0 for s, s0 in zip(shifts, shifts0))


# ---- 5. the column-slice budget: DSGD_CS_MAX_MB ------------------------------------------------------------------------------------
def layout_bytes(info, n_steps):
    """bytes of a plan's column-slice layout from the strides dsgd_plan_info reports (cs_build: 16 entries per slot, a
    4-byte word, 16-bit columns and float values per slot; 16-bit row and column-list words; an 8-byte header per cell)"""
    cells = info["slices"] * n_steps
    return cells * (info["slot_stride"] * (4 + 16 * 2 + 16 * 4) + info["row_stride"] * 2 + info["col_list_stride"] * 2 + 8)


@pytest.mark.parametrize("host_layout", [False, True])
def test_column_slice_budget(monkeypatch, host_layout):
    """`bytes > cs_max_mb << 20` in both layout builders: a refused plan runs through the next family route_plan names
    (virtual tiles for three workers, the one-workgroup kernel for one), bit-equal to a DSGD_CS=0 context, and strands no block."""
    data = data_of(44)
    rng = np.random.default_rng(44)
    plans = [(3, batches(rng, N_TRAIN, 3, 100, 8), VT, "virtual_tiles"), (1, batches(rng, N_TRAIN, 1, 100, 8), ONE_WG, "one_workgroup")]
    layout = {"DSGD_CS_HOST_LAYOUT": "1"} if host_layout else {}
    _, twin = context(monkeypatch, layout, data)
    with twin:
        p = twin.plan(plans[0][1])
        info = p.info()
        p.destroy()
        assert info["kind"] == "column_slices" and info["device_built"] == (not host_layout)
        nbytes = layout_bytes(info, 8)
    assert nbytes > 1 << 20   # (so that a whole number of MiB lies just under it)
    under, over = (nbytes - 1) >> 20, (nbytes + (1 << 20) - 1) >> 20
    _, e_off = context(monkeypatch, {"DSGD_CS": "0"}, data)
    with e_off:
        w_start = e_off.get_weights()
        off = [run_plan(e_off, steps, 0.5, w_start) for _, steps, _, _ in plans]
    for mb in ("0", str(under)):
        o, eng = context(monkeypatch, dict(layout, DSGD_CS_MAX_MB=mb), data)
        with eng:
            for (k, steps, kernel, kind), (w0, st0, info0) in zip(plans, off):
                if k == 1 and mb != "0":
                    continue   # (the one-worker layout is smaller than the three-worker one the budget was cut for)
                eng.set_weights(w_start)
                plan = eng.plan(steps)
                assert plan.info()["kind"] != "column_slices"
                w, act, _ = plan_steps(o, eng, plan, steps, 0.5, kernel, kind)
                assert plan.info()["threads"] == 0 and info0["kind"] == kind
                plan.destroy()
                assert act == st0["n_active"] and np.array_equal(bits(w), bits(w0)), (mb, k)
            for _ in range(3):   # plans made and destroyed under the budget leave nothing behind
                for _, steps, _, _ in plans:
                    eng.plan(steps).destroy()
            eng.synchronize()
            assert eng.cache_trim(0) == 0
    _, eng = context(monkeypatch, dict(layout, DSGD_CS_MAX_MB=str(over)), data)   # the seam's other side: the layout just fits
    with eng:
        p = eng.plan(plans[0][1])
        assert p.info()["kind"] == "column_slices"
        p.destroy()


def test_column_slice_budget_refuses_an_fp64_plan(monkeypatch):
    """include/dsgd.h, THE FP64 MODE: a plan beyond the limits is refused with DSGD_EUNSUPPORTED when it is created -- an fp64
    context has no other family -- and the message names the budget; nothing is stranded, and the context goes on."""
    from dsgd_amd import _lib

    data = data_of(44)
    steps = batches(np.random.default_rng(44), N_TRAIN, 3, 100, 4)
    pin(monkeypatch, {"DSGD_CS_MAX_MB": "0"})
    eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64")
    with eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(N_TRAIN)
        for _ in range(2):
            with pytest.raises(dsgd_amd.DsgdError) as e:
                eng.plan(steps)
            assert e.value.code == _lib.EUNSUPPORTED and "DSGD_CS_MAX_MB" in str(e.value), str(e.value)
        eng.synchronize()   # (a block whose last reader the stream has not finished stays: nothing is pending now)
        assert eng.cache_trim(0) == 0
        assert not eng.get_weights().any()
        assert sum(eng.loss_acc(N_TRAIN, N_ROWS)[2]) == N_ROWS - N_TRAIN   # (the context still evaluates)


# ---- 6. the column lists' back-off on a live context -----------------------------------------------------------------------------
def test_column_lists_back_off_and_come_back(monkeypatch):
    """TcolGate through tcol_layout: 12 configurations in a row build a layout each, the 13th sits out (the row-wise kernel
    takes the range), a configuration still in the cache is used again even during the cool-down (hit), a new one is not;
    load_csr resets the gate.  The way out after COOLDOWN = 256 declined steps is stepped on the CPU (tests/cpp/route_test.cpp);
    here 256 steps of real work are not run: the way out through load_csr is."""
    assert (GATE_MISSES, GATE_COOLDOWN, GATE_RESUME) == (12, 256, 8)
    data = data_of(45)
    o, eng = context(monkeypatch, {}, data)
    rows, lr = 1000, 0.5 * 100 / 1000

    def step(begin, kernel):
        ranged_step(o, eng, [(begin, begin + rows)], lr)
        assert eng.grad_kernel_name() == kernel, (begin, eng.grad_kernel_name())

    with eng:
        for i in range(GATE_MISSES):
            step(i, TCOL)
        step(GATE_MISSES, MB)            # the 13th new configuration in a row
        step(GATE_MISSES - 1, TCOL)      # one of the eight the cache holds: used again, cool-down or not
        step(GATE_MISSES + 1, MB)        # ... and a new one still sits out
        step(GATE_MISSES - 2, TCOL)
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(N_TRAIN)
        step(GATE_MISSES + 2, TCOL)      # the gate is reset: a new configuration builds a layout again
        step(GATE_MISSES + 2, TCOL)
