"""-m gpu: every gradient kernel family on the hostile feature values of tests/hard_data.py (values scaled by 2^10 and
2^-30, negative values and columns that cancel to an exact 0, entries 45 binades apart and columns that vanish on the
grid, rows exactly ON the gate at non-zero weights, empty / one-element / 3,000- and 8,000-entry rows).

Statements (tests/test_hard_data.py pins the data and the oracle side of each on the CPU):

 (a) SCALE COVARIANCE, no tolerance, the kernel against itself: X' = 2^k X, w' = 2^-k w, lr' = 2^-2k lr, lambda = 0.  Every
     product x'w' is bit-equal to x w, the grid sits at the same place relative to vexp, so g' == 2^k g and
     w_after' == 2^-k w_after BIT FOR BIT, active counts, predictions and tallies equal -- in fp32 too (powers of two, nothing
     subnormal).  A wrong vexp anywhere cannot pass.
 (b) AGAINST THE ORACLE, every trait (the scaled ones too, at lambda = 1e-5 and the base's lr: vexp != 0 through the
     regulariser and support path) under the derived per-coordinate bound of oracle/bounds.py with the shift the launch
     reports (fp32; the near-gate allowance relative, rel_gate_eps; the 1e-9 on s in the scaled frame) / the fp64 suite's
     standing 1e-12 * max(1, |ref|_inf), equal supports and active counts, no waiver (fp64, inside the exact range).
     zero_margin: the planted rows alone (nothing near the gate, every row ON it) must give exactly the oracle's count.
 (c) OUTSIDE THE EXACT RANGE (wide): bounds.out_of_range_bound per coordinate (fp64), list_bound (fp32), and the
     vanishing-column allowance QUANTISED (quantised_allowance below): whole regularisers of candidate workers only.

After every leg grad_kernel_name() / plan.info()["kind"] say that the family under test is the one that ran."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
import hard_data as hd
import waivers
from conftest import has_gpu
from oracle import bounds as orb
from oracle import oracle as orc
from oracle.hogwild_replay import hog_rows
from test_gpu_fp64_requests import _check_grad
from test_gpu_parity import list_step, make_pair, ranged_step, tol as tol32

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
LAM = 1e-5
KNOBS = ("DSGD_CS", "DSGD_CS_REQ", "DSGD_CS_HOST_LAYOUT", "DSGD_CS_G", "DSGD_REQ_PLAN", "DSGD_PLAN_KERNEL", "DSGD_VT", "DSGD_VT_PACK_MB",
         "DSGD_STREAM_MIN", "DSGD_FSTEP", "DSGD_FSTEP_MIN", "DSGD_FSTEP_MAX", "DSGD_FSTEP_ROWS", "DSGD_TCOL", "DSGD_TCOL_MIN", "DSGD_TCOL_MAX",
         "DSGD_TCOL_MAX_NNZ", "DSGD_TCOL_SHARE", "DSGD_FIX_SHIFT", "DSGD_HSPLIT", "DSGD_COLD_UNPACKED")
ORACLE_TRAITS = ("plain", "scaled_p10", "scaled_m30", "signed", "wide", "zero_margin", "ragged64")


def s_abs_of(h):
    """the standing 1e-9 allowance on s in the frame of a scaled trait: s' = 2^-k s exactly (oracle/bounds.py, s_abs)"""
    return math.ldexp(1e-9, -h.planted.get("k", 0))

# family -> (environment read when the context is created, how a step runs, the lists / ranges, the kernel that must run)
LIST_FAMILIES = {
    "one_workgroup": ({"DSGD_CS": "0", "DSGD_REQ_PLAN": "1", "DSGD_PLAN_KERNEL": "1"}, "step", ("k1b100",), "dsgd_plan_kernel"),
    "row_wise": ({"DSGD_CS": "0"}, "step", ("k3b100", "k2b700", "k1b4096"), "dsgd_mb_grad_kernel"),
    "virtual_tiles": ({"DSGD_CS": "0"}, "plan", ("k3b100", "k2b700", "k1b4096"), "dsgd_vt_grad_kernel"),
    "column_slices_host": ({"DSGD_CS_HOST_LAYOUT": "1"}, "plan", ("k1b100", "k3b100"), "dsgd_cs_step_kernel"),
    "column_slices_device": ({"DSGD_CS_HOST_LAYOUT": "0"}, "plan", ("k1b100", "k3b100"), "dsgd_cs_step_kernel"),
}
RANGE_FAMILIES = {
    "streaming": ({"DSGD_STREAM_MIN": "8192", "DSGD_FSTEP": "0", "DSGD_TCOL": "0"}, ("whole",), "dsgd_wseg_kernel"),
    "row_chunks": ({"DSGD_TCOL": "0", "DSGD_FSTEP_MIN": "4096"}, ("whole", "halves"), "dsgd_fstep_kernel"),
    "column_lists": ({}, ("whole", "halves"), "dsgd_tc_grad_kernel"),
}


def pin(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def lr_of(lists):
    return min(0.5 * 100 / max(len(a) for a in lists), 0.5)


def ran(eng, kernel):
    name = eng.grad_kernel_name()
    assert kernel in name, "the family under test did not run: %s, wanted %s" % (name, kernel)


def run_lists(eng, how, lists, lr, kernel):
    """one synchronous step over index lists as a per-request call or as a resident plan of one step"""
    if how == "step":
        st = eng.sync_step(lists, lr)
    else:
        plan = eng.plan([lists])
        eng.synchronize()
        eng.plan_run(plan, 0, 1, lr)
        st = eng.synchronize()
        kind = plan.info()["kind"]   # (virtual tiles are laid out at the first run)
        plan.destroy()
        assert kind == {"dsgd_vt_grad_kernel": "virtual_tiles", "dsgd_cs_step_kernel": "column_slices"}[kernel], kind
    ran(eng, kernel)
    return st


def planted_columns(trait, h):
    """the columns planted to vanish on an fp32 grid"""
    if trait == "wide":
        return h.planted["vanishing_columns"]
    if trait == "zero_margin":
        return h.planted["columns_b"]   # (x = 2^-34: below every fp32 grid of data with vexp = 0)
    return np.zeros(0, np.int32)


# families whose EVERY column sum is a fixed-point integer; the one-workgroup kernel adds its cold ranks in float
# (csrc/dsgd_batch.hpp, gcold), so a column below the grid keeps its sum, and its regulariser, there
ALL_ON_THE_GRID = {"one_workgroup": False}


def quantised_allowance(trait, h, diff, base_tol, unit, cand, must, on_grid, where, expect_planted=True):
    """Statement (c)'s assertion (oracle/bounds.py `vanishing` / `vanished`).  The issue expected the |s| allowance to be
    needed on the planted columns alone; on `wide` hundreds of unplanted columns vanish too (a rare column whose few entries
    all drew a large u is below the grid like a planted one, in fp32 and, at 2^-45 against half a unit of 2^-51, in
    fp64).  So instead of a list of columns the allowance is QUANTISED per column: the error minus m_j whole regularisers
    of a worker (m_j an integer, at most the cand_j workers whose oracle sum lies within the grid error of 0) must be
    within the bound that has no support term; where every entry of the column is below half a grid unit the engine's sum
    MUST have vanished (m_j >= must_j) -- the planted columns of wide / zero_margin are among those, counted; and a trait
    that plants none (signed, ragged64, plain, scaled) has no candidate at all."""
    m, residual = orb.vanished(diff, base_tol, unit, cand)
    j = int(np.argmax(residual))
    assert residual[j] <= 1.0, "%s: coordinate %d is %.3g x its bound after %d of %d regularisers" % (where, j, residual[j], m[j], cand[j])
    planted = planted_columns(trait, h)
    held = planted[cand[planted] > 0] if len(planted) else planted
    if on_grid:
        short = np.flatnonzero(m < must)
        assert len(short) == 0, "%s: columns below the grid kept their regulariser: %s" % (where, short[:10])
        assert (must[held] == cand[held]).all() and (m[held] == cand[held]).all(), (where, held, m[held], cand[held])
    if trait in ("wide", "zero_margin"):
        assert len(held) > 0 or not expect_planted, where
    else:
        assert not cand.any(), (where, np.flatnonzero(cand)[:10])
    return int((m > 0).sum()), len(held)


def hard_step(o, eng, trait, h, run, idx_lists, lr, family, ranges, s_abs=1e-9):
    """one step on both sides from the engine's weights under the derived bound, the relative near-gate allowance and the
    quantised vanishing-column term.  Returns (engine stats, rows near the gate)."""
    w0 = eng.get_weights().astype(np.float64)
    w_ref = w0.copy()
    st = run()
    shift = eng.tuning_info()["fix_shift"]
    o.sync_step(w_ref, idx_lists, lr)
    k = len(idx_lists)
    tol, n_near, near_part = orb.list_bound(o, w0, w_ref, idx_lists, lr, shift, parts=True, rel_eps=orb.rel_gate_eps(o), s_abs=s_abs,
                                            rounding=not ranges)
    half = orb.vmax2_of(h.data.val) * 2.0 ** -(shift + 1)
    cand, must = orb.vanishing(o, w0, idx_lists, [half] * k)
    unit = lr / k * orb.reg_scalar(o, w0)
    w = eng.get_weights().astype(np.float64)
    print("%s %s: %d rows, active %d vs %d, %d near, shift %d" % (family, trait, st["n_samples"], st["n_active"], o.last_stats["n_active"], n_near, shift))
    assert st["n_samples"] == sum(len(a) for a in idx_lists)
    assert abs(st["n_active"] - o.last_stats["n_active"]) <= n_near, (st, o.last_stats, n_near)
    used, held = quantised_allowance(trait, h, w - w_ref, tol, unit, cand, must, ALL_ON_THE_GRID.get(family, True) and n_near == 0, (family, trait))
    print("    %d columns lost a regulariser (%d could), %d planted columns among them" % (used, int((cand > 0).sum()), held))
    tight = st["n_active"] == o.last_stats["n_active"] and orb.vanished(w - w_ref, tol - near_part, unit, cand)[1].max() <= 1.0
    waivers.tight("hard_values:%s:gates_as_the_oracle" % family, tight, n_near > 0, "%s: %d rows near the gate" % (trait, n_near))
    return st, n_near


def on_the_gate(o, eng, h, run_with, family):
    """zero_margin's planted rows ALONE, as two workers and as three (one worker's 36 rows would be the one-workgroup
    kernel's in every plan family): nothing is near the gate, every row is ON it"""
    p = h.planted
    rows = np.asarray(p["rows_a"] + p["rows_b"] + p["rows_c"], dtype=np.int32)
    for lists in ([rows[0::2].copy(), rows[1::2].copy()], [rows[0::3].copy(), rows[1::3].copy(), rows[2::3].copy()]):
        eng.set_weights(h.w.astype(np.float32))
        st, n_near = run_with(lists)
        assert n_near == 0 and st["n_active"] == len(rows) == o.last_stats["n_active"], (st, o.last_stats, n_near)
        waivers.strict("hard_values:%s:on_the_gate" % family)


# ---- fp32, index lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(LIST_FAMILIES))
def test_fp32_list_families_against_the_oracle(monkeypatch, family):
    env, how, names, kernel = LIST_FAMILIES[family]
    pin(monkeypatch, env)
    for trait in ORACLE_TRAITS:
        h = hd.build(trait)
        o, eng = make_pair(h.data, LAM, hd.N_TRAIN)
        with eng:
            for name in names:
                lists = hd.lists_of(trait, name)
                lr = lr_of(lists)
                eng.set_weights(h.w.astype(np.float32))
                hard_step(o, eng, trait, h, lambda: run_lists(eng, how, lists, lr, kernel), lists, lr, family, False, s_abs_of(h))
            if trait == "zero_margin" and family != "one_workgroup":
                on_the_gate(o, eng, h, lambda ls: hard_step(o, eng, trait, h, lambda: run_lists(eng, how, ls, 0.5, kernel), ls, 0.5, family, False), family)
            if trait == "zero_margin" and family == "one_workgroup":
                rows = np.asarray(h.planted["rows_a"] + h.planted["rows_b"] + h.planted["rows_c"], dtype=np.int32)
                eng.set_weights(h.w.astype(np.float32))
                st, n_near = hard_step(o, eng, trait, h, lambda: run_lists(eng, how, [rows], 0.5, kernel), [rows], 0.5, family, False)
                assert n_near == 0 and st["n_active"] == len(rows)
            if trait == "signed":   # the pairs' private columns: an exact integer 0, no regulariser -- the weight keeps its bits
                priv = h.planted["private_columns"]
                eng.set_weights(h.w.astype(np.float32))
                run_lists(eng, how, hd.lists_of(trait, names[0]), 0.5, kernel)
                assert not eng.get_weights()[priv].any()
                # ... and under the suite's existing bound as it stands (absolute allowance, no support term)
                if how == "step":
                    eng.set_weights(h.w.astype(np.float32))
                    list_step(o, eng, hd.lists_of(trait, names[0]), 0.5, "hard_values:%s:signed_existing_bound" % family)
                    ran(eng, kernel)


@pytest.mark.parametrize("family", list(LIST_FAMILIES))
@pytest.mark.parametrize("k", [10, -30])
def test_fp32_list_families_are_scale_covariant_bit_for_bit(monkeypatch, family, k):
    env, how, names, kernel = LIST_FAMILIES[family]
    pin(monkeypatch, env)
    plain, h = hd.build("plain"), hd.build("scaled_p10" if k == 10 else "scaled_m30")
    _, e0 = make_pair(plain.data, 0.0, hd.N_TRAIN)
    _, e1 = make_pair(h.data, 0.0, hd.N_TRAIN)
    with e0, e1:
        for name in names:
            lists = hd.lists_of("scaled_p10" if k == 10 else "scaled_m30", name)
            lr = lr_of(lists)
            e0.set_weights(plain.w.astype(np.float32))
            e1.set_weights(h.w.astype(np.float32))
            st0 = run_lists(e0, how, lists, lr, kernel)
            st1 = run_lists(e1, how, lists, math.ldexp(lr, -2 * k), kernel)
            assert e0.tuning_info()["fix_shift"] == e1.tuning_info()["fix_shift"]
            w0, w1 = e0.get_weights(), e1.get_weights()
            assert st0 == st1 and 0 < st0["n_active"] < st0["n_samples"]
            assert not np.array_equal(w0, plain.w.astype(np.float32))
            assert np.array_equal(bits(np.ldexp(w1, k)), bits(w0)), "%s %s: %d coordinates differ" % (family, name, (np.ldexp(w1, k) != w0).sum())


# ---- fp32, row ranges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(RANGE_FAMILIES))
def test_fp32_range_families_against_the_oracle(monkeypatch, family):
    env, names, kernel = RANGE_FAMILIES[family]
    pin(monkeypatch, env)
    for trait in ORACLE_TRAITS:
        h = hd.build(trait)
        o, eng = make_pair(h.data, LAM, hd.N_TRAIN)
        with eng:
            for name in names:
                ranges = hd.RANGES[name]
                lr = 0.5 * 100 / hd.N_TRAIN * len(ranges)
                eng.set_weights(h.w.astype(np.float32))

                def run():
                    st = eng.sync_step_ranges(ranges, lr)
                    ran(eng, kernel)
                    return st

                hard_step(o, eng, trait, h, run, [np.arange(a, b, dtype=np.int32) for a, b in ranges], lr, family, True, s_abs_of(h))
            if trait == "signed":   # the suite's existing bound as it stands
                eng.set_weights(h.w.astype(np.float32))
                ranged_step(o, eng, hd.RANGES[names[0]], 0.5 * 100 / hd.N_TRAIN)
                ran(eng, kernel)
                assert not eng.get_weights()[h.planted["private_columns"]].any()


@pytest.mark.parametrize("family", list(RANGE_FAMILIES))
@pytest.mark.parametrize("k", [10, -30])
def test_fp32_range_families_are_scale_covariant_bit_for_bit(monkeypatch, family, k):
    env, names, kernel = RANGE_FAMILIES[family]
    pin(monkeypatch, env)
    plain, h = hd.build("plain"), hd.build("scaled_p10" if k == 10 else "scaled_m30")
    _, e0 = make_pair(plain.data, 0.0, hd.N_TRAIN)
    _, e1 = make_pair(h.data, 0.0, hd.N_TRAIN)
    with e0, e1:
        for name in names:
            ranges = hd.RANGES[name]
            lr = 0.5 * 100 / hd.N_TRAIN * len(ranges)
            e0.set_weights(plain.w.astype(np.float32))
            e1.set_weights(h.w.astype(np.float32))
            st0 = e0.sync_step_ranges(ranges, lr)
            st1 = e1.sync_step_ranges(ranges, math.ldexp(lr, -2 * k))
            ran(e0, kernel), ran(e1, kernel)
            assert e0.tuning_info()["fix_shift"] == e1.tuning_info()["fix_shift"]
            assert st0 == st1 and 0 < st0["n_active"] < st0["n_samples"]
            w0, w1 = e0.get_weights(), e1.get_weights()
            assert np.array_equal(bits(np.ldexp(w1, k)), bits(w0)), "%s %s: %d coordinates differ" % (family, name, (np.ldexp(w1, k) != w0).sum())


# ---- fp32: gradient / forward / evaluation with given weights, the lock-free engine with one worker ------------------------
def test_fp32_gradient_forward_and_tallies_with_given_weights(monkeypatch):
    pin(monkeypatch, {"DSGD_CS": "0"})
    plain = hd.build("plain")
    idx = hd.lists_of("plain", "k2b700")[0]
    test_rows = np.arange(hd.N_TRAIN, hd.N_ROWS, dtype=np.int32)
    _, e0 = make_pair(plain.data, 0.0, hd.N_TRAIN)
    with e0:
        g0, st0 = e0.gradient(idx, w=plain.w.astype(np.float32))
        p0 = e0.forward(test_rows)
        t0 = e0.loss_acc(hd.N_TRAIN, hd.N_ROWS, w=plain.w.astype(np.float32))[2]
    for trait in ("scaled_p10", "scaled_m30"):   # (a): g' == 2^k g bit for bit, counts, predictions and tallies equal
        h = hd.build(trait)
        k = h.planted["k"]
        _, e1 = make_pair(h.data, 0.0, hd.N_TRAIN)
        with e1:
            g1, st1 = e1.gradient(idx, w=h.w.astype(np.float32))
            assert st1 == st0 and g0.any()
            assert np.array_equal(bits(g1), bits(np.ldexp(g0, k))), (trait, (g1 != np.ldexp(g0, k)).sum())
            assert np.array_equal(e1.forward(test_rows), p0)
            assert e1.loss_acc(hd.N_TRAIN, hd.N_ROWS, w=h.w.astype(np.float32))[2] == t0
    for trait in ("signed", "wide", "zero_margin", "ragged64"):   # (b), (c)
        h = hd.build(trait)
        o, eng = make_pair(h.data, LAM, hd.N_TRAIN)
        w32 = h.w.astype(np.float32)
        with eng:
            for name in ("k1b100", "k2b700", "k1b4096"):
                rows = hd.lists_of(trait, name)[0]
                g, st = eng.gradient(rows, w=w32)
                shift = eng.tuning_info()["fix_shift"]
                g_ref = o.gradient(h.w, rows)
                tol, n_near = orb.gradient_bound(o, h.w, g_ref, rows, shift, rel_eps=orb.rel_gate_eps(o))
                cnt = orb._list_profile(o, h.w, rows, orb.GATE_EPS)[0]
                quantum = orb.vmax2_of(h.data.val) * 2.0 ** -(shift + 1)
                cand, must = orb.vanishing(o, h.w, [rows], [quantum])
                diff = g.astype(np.float64) - g_ref
                assert abs(st["n_active"] - o.last_stats["n_active"]) <= n_near
                quantised_allowance(trait, h, diff, tol, -orb.reg_scalar(o, h.w), cand, must, n_near == 0, (trait, name))
                m, _ = orb.vanished(diff, tol, -orb.reg_scalar(o, h.w), cand)
                assert not g[m > 0].any()   # one worker: a column that lost its regulariser has no gradient at all
                only_ref = set(np.flatnonzero((g_ref != 0) & (g == 0)).tolist())   # supports: only what may vanish on the grid
                assert only_ref <= set(np.flatnonzero(np.abs(orb._g0(o, h.w, rows)) <= cnt * quantum).tolist())
                assert n_near > 0 or not ((g_ref == 0) & (g != 0)).any()
                waivers.tight("hard_values:gradient_given_weights", st["n_active"] == o.last_stats["n_active"], n_near > 0, "%s %d near" % (trait, n_near))
            if trait == "zero_margin":
                p = h.planted
                rows = np.asarray(p["rows_a"] + p["rows_b"] + p["rows_c"], dtype=np.int32)
                g, st = eng.gradient(rows, w=w32)
                assert st["n_active"] == len(rows)
                assert not eng.forward(rows, w=w32).any()   # -signum(0) = 0: the prediction of a row on the gate
                assert np.array_equal(eng.forward(rows), o.forward(h.w, rows))
                for r in rows[:6]:
                    assert eng.loss_acc(int(r), int(r) + 1)[2] == [0, 1, 0]
            if trait == "signed":
                g, _ = eng.gradient(hd.lists_of(trait, "k2b700")[0], w=w32)
                assert not g[h.planted["private_columns"]].any()
            pred = eng.forward(test_rows, w=w32)
            pred_ref = o.forward(h.w, test_rows)
            _, _, n_near = orb._list_profile(o, h.w, test_rows, orb.GATE_EPS, orb.rel_gate_eps(o))
            assert (pred != pred_ref).sum() <= n_near
            waivers.tight("hard_values:forward_given_weights", bool((pred == pred_ref).all()), n_near > 0, "%s %d near" % (trait, n_near))
            _, _, counts = eng.loss_acc(hd.N_TRAIN, hd.N_ROWS)
            _, _, counts_ref, _ = o.loss_acc(h.w, hd.N_TRAIN, hd.N_ROWS)
            assert sum(abs(a - b) for a, b in zip(counts, counts_ref)) <= 2 * n_near


def test_fp32_lock_free_engine_with_one_worker(monkeypatch):
    """a replay of the oracle, as test_hogwild_single_worker_replays_the_oracle, from NON-ZERO weights on signed values, rows
    on the gate and ragged rows; and (a): the scaled run ends on the same bits.  `wide` is left out: the statement here is
    the existing blanket 4e-5 after twelve updates, and every update may drop lr * |s| = 1.7e-5 on each vanishing column, which
    that tolerance cannot price; the per-step legs above hold the engine's kernels on `wide` under the derived bound."""
    pin(monkeypatch, {"DSGD_CS": "0"})
    begin, end, batch, n_upd = 0, 3000, 64, 12
    for trait in ("signed", "zero_margin", "ragged64"):
        h = hd.build(trait)
        o, eng = make_pair(h.data, LAM, hd.N_TRAIN)
        with eng:
            eng.set_weights(h.w.astype(np.float32))
            w_ref = h.w.copy()
            eng.async_start([(begin, end)], batch=batch, lr=0.5, max_updates=n_upd, seed=77, positional_bug=False)
            eng.async_wait()
            assert eng.async_updates() == (n_upd, False)
            exposed = 0
            for it in range(n_upd):
                rows = hog_rows(77, 0, it, begin, end - begin, batch, False)
                exposed += orb._list_profile(o, w_ref, rows, orb.GATE_EPS, orb.rel_gate_eps(o))[2]
                o.async_step(w_ref, rows, 0.5)
            err = np.abs(eng.get_weights().astype(np.float64) - w_ref).max()
            print("lock_free %s: err %.3g, tol %.3g, %d replayed rows near the gate" % (trait, err, 4 * tol32(w_ref), exposed))
            waivers.tight("hard_values:lock_free_one_worker", err <= 4 * tol32(w_ref), exposed > 0, "%s: err %.3g" % (trait, err))
    out = {}
    for trait in ("plain", "scaled_p10", "scaled_m30"):
        h = hd.build(trait)
        k = h.planted.get("k", 0)
        _, eng = make_pair(h.data, 0.0, hd.N_TRAIN)
        with eng:
            eng.set_weights(h.w.astype(np.float32))
            eng.async_start([(begin, end)], batch=batch, lr=math.ldexp(0.5, -2 * k), max_updates=n_upd, seed=77, positional_bug=False)
            eng.async_wait()
            out[trait] = np.ldexp(eng.get_weights(), k)
    assert not np.array_equal(out["plain"], hd.build("plain").w.astype(np.float32))
    for trait in ("scaled_p10", "scaled_m30"):
        assert np.array_equal(bits(out[trait]), bits(out["plain"])), (trait, (out[trait] != out["plain"]).sum())


# ---- fp64 ------------------------------------------------------------------------------------------------------------------
def pair64(data, lam=LAM):
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, lam)
    o.set_dim_sparsity(o.dim_sparsity(hd.N_TRAIN))
    eng = dsgd_amd.Engine(data.dim, lam, precision="fp64")
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(hd.N_TRAIN)
    return o, eng


def shift64(n):
    return 62 - (math.ceil(math.log2(n)) if n > 1 else 0)


def scale64(v):
    return max(1.0, float(np.abs(v).max()))


def test_fp64_requests_scale_covariant_bit_for_bit(monkeypatch):
    """(a) for dsgd_gradient_f64, dsgd_forward_f64, dsgd_sync_step_f64 (rank-order weights) and the cs64 plans"""
    pin(monkeypatch, {})
    plain = hd.build("plain")
    res = {}
    for trait in ("plain", "scaled_p10", "scaled_m30"):
        h = hd.build(trait)
        k = h.planted.get("k", 0)
        _, eng = pair64(h.data, 0.0)
        r = []
        with eng:
            for name in hd.LISTS:
                lists = hd.lists_of("scaled_p10", name)
                g, st = eng.gradient_f64(lists[0], w=h.w)
                r.append((np.ldexp(g, -k), st, eng.forward_f64(lists[0])))
                eng.set_weights(h.w)
                st = eng.sync_step_f64(lists, math.ldexp(lr_of(lists), -2 * k))
                r.append((np.ldexp(eng.get_weights(), k), st, None))
                if sum(len(a) for a in lists) <= 1024:
                    eng.set_weights(h.w)
                    p = eng.plan([lists, lists[::-1]])
                    assert p.info()["kind"] == "column_slices_fp64"
                    eng.plan_run(p, 0, 2, math.ldexp(0.5, -2 * k))
                    eng.synchronize()
                    ran(eng, "dsgd_cs64_step_kernel")
                    r.append((np.ldexp(eng.get_weights(), k), None, None))
                    p.destroy()
                    eng.set_weights(h.w)
                    d, st = eng.async_step(lists[0], math.ldexp(0.5, -2 * k), want_delta=True)
                    ran(eng, "dsgd_cs64_async_kernel")
                    r.append((np.ldexp(d, k), st, np.ldexp(eng.get_weights(), k)))
        res[trait] = r
    assert res["plain"][0][0].any() and not np.array_equal(res["plain"][1][0], plain.w)
    for trait in ("scaled_p10", "scaled_m30"):
        for i, ((a, sa, pa), (b, sb, pb)) in enumerate(zip(res["plain"], res[trait])):
            assert sa == sb, (trait, i)
            assert np.array_equal(bits(a), bits(b)), (trait, i, (a != b).sum())
            assert pa is None or np.array_equal(bits(pa), bits(pb)), (trait, i)


@pytest.mark.parametrize("trait", ["scaled_p10", "scaled_m30", "signed", "zero_margin", "ragged64"])
def test_fp64_families_inside_the_exact_range(monkeypatch, trait):
    """(b): gradient_f64 (given weights, then the slice-major weights a plan leaves), sync_step_f64 in both layouts, the cs64
    plans, the cs64 asynchronous iteration per call and resident, update_grad_f64 -- 1e-12, equal supports and counts"""
    pin(monkeypatch, {})
    h = hd.build(trait)
    o, eng = pair64(h.data)
    vexp = hd.vexp_of(h.data.val)
    with eng:
        for name in hd.LISTS:
            lists = hd.lists_of(trait, name)
            for rows in lists:
                assert not orb.inexact_counts(o, rows, vexp, shift64(len(rows))).any()   # every entry a whole number of grid units
                eng.set_weights(h.w)
                _check_grad(o, eng, h.w, rows)
            lr = math.ldexp(lr_of(lists), -2 * h.planted.get("k", 0))
            small = sum(len(a) for a in lists) <= 1024
            for sliced in ((False, True) if small else (False,)):
                eng.set_weights(h.w)
                if sliced:   # a plan run with lr = 0 leaves the same weights slice-major
                    p = eng.plan([lists])
                    eng.plan_run(p, 0, 1, 0.0)
                    p.destroy()
                    _check_grad(o, eng, h.w, lists[0])
                st = eng.sync_step_f64(lists, lr)
                w_o = h.w.copy()
                o.sync_step(w_o, lists, lr)
                w = eng.get_weights()
                assert st["n_active"] == o.last_stats["n_active"] and st["n_samples"] == sum(len(a) for a in lists)
                assert np.abs(w - w_o).max() <= 1e-12 * scale64(w_o), (name, sliced)
                assert np.array_equal(w != h.w, w_o != h.w)
                if trait == "signed":
                    assert not w[h.planted["private_columns"]].any()
            if small:
                eng.set_weights(h.w)
                p = eng.plan([lists])
                assert p.info()["kind"] == "column_slices_fp64"
                p.record(True)
                eng.plan_run(p, 0, 1, lr)
                eng.synchronize()
                ran(eng, "dsgd_cs64_step_kernel")
                mask, _ = p.read_record()
                p.destroy()
                assert int(mask[0][:sum(len(a) for a in lists)].sum()) == o.last_stats["n_active"]
                assert np.abs(eng.get_weights() - w_o).max() <= 1e-12 * scale64(w_o)
                # the asynchronous iteration, per call: the delta, its support, the weights
                eng.set_weights(h.w)
                d, st = eng.async_step(lists[0], lr, want_delta=True)
                ran(eng, "dsgd_cs64_async_kernel")
                w_a = h.w.copy()
                d_o = o.async_step(w_a, lists[0], lr, want_delta=True)
                assert st["n_active"] == o.last_stats["n_active"]
                assert np.array_equal(np.flatnonzero(d), np.flatnonzero(d_o)) and np.abs(d - d_o).max() <= 1e-12 * scale64(d_o)
                assert np.abs(eng.get_weights() - w_a).max() <= 1e-12 * scale64(w_a)
                # ... a peer's update (dsgd_update_grad_f64): w[key] = filt(w[key] - dv) on the keys of that delta
                keys = np.flatnonzero(d_o).astype(np.int32)
                eng.set_weights(h.w)
                eng.update_grad(keys, d_o[keys])
                want = h.w.copy()
                x = want[keys] - d_o[keys]
                want[keys] = np.where(np.abs(x) > 1e-20, x, 0.0)
                assert np.array_equal(bits(eng.get_weights()), bits(want))
        if trait == "zero_margin":
            p = h.planted
            rows = np.asarray(p["rows_a"] + p["rows_b"] + p["rows_c"], dtype=np.int32)
            eng.set_weights(h.w)
            _, st = eng.gradient_f64(rows)
            assert st["n_active"] == len(rows)
            assert not eng.forward_f64(rows).any() and np.array_equal(eng.forward_f64(rows), o.forward(h.w, rows))
            st = eng.sync_step_f64([rows[0::3].copy(), rows[1::3].copy(), rows[2::3].copy()], 0.5)
            assert st["n_active"] == len(rows)
            eng.set_weights(h.w)
            st = eng.sync_step([rows], 0.5)   # (a one-step cs64 plan inside the call)
            assert st["n_active"] == len(rows)
            eng.set_weights(h.w)
            _, st = eng.async_step(rows, 0.5)
            assert st["n_active"] == len(rows)
        # the resident asynchronous plan: the device draws the rows (oracle/hogwild_replay.hog_rows)
        eng.set_weights(h.w)
        lr = math.ldexp(0.5, -2 * h.planted.get("k", 0))
        p = eng.async_plan([(0, 3000)], 100, seed=9, positional_bug=False, first_update=0, n_updates=8)
        p.record(True)
        eng.plan_run_async(p, 0, 8, lr)
        mask, _ = p.read_record()
        w = eng.get_weights()
        ran(eng, "dsgd_cs64_async_kernel")
        p.destroy()
        w_o = h.w.copy()
        for u in range(8):
            o.async_step(w_o, hog_rows(9, 0, u, 0, 3000, 100, False), lr)
            assert int(mask[u][:100].sum()) == o.last_stats["n_active"], u
        assert np.abs(w - w_o).max() <= 1e-12 * scale64(w_o)


def test_fp64_signed_exact_sums_bit_for_bit(monkeypatch):
    """lambda = 0 on signed values with cancelling columns: each coordinate the correctly rounded exact sum (math.fsum)"""
    pin(monkeypatch, {})
    h = hd.build("signed")
    data = h.data
    o, eng = pair64(data, 0.0)
    with eng:
        for name in ("k2b700", "k1b4096"):
            idx = hd.lists_of("signed", name)[0]
            g, st = eng.gradient_f64(idx, w=h.w)
            active = [r for r in idx.tolist() if not (data.label[r] * o.row_dot(r, h.w) < 0)]
            assert st["n_active"] == len(active)
            hd.check_exact_range(data, np.asarray(active), len(idx))
            cols = np.concatenate([data.col[data.row_ptr[r]:data.row_ptr[r + 1]] for r in active])
            vals = np.concatenate([data.val[data.row_ptr[r]:data.row_ptr[r + 1]].astype(np.float64) * float(data.label[r]) for r in active])
            order = np.argsort(cols, kind="stable")
            cols, vals = cols[order], vals[order]
            want = np.zeros(data.dim + 1)
            cuts = np.flatnonzero(np.diff(cols)) + 1
            for c_, part in zip(cols[np.r_[0, cuts]], np.split(vals, cuts)):
                s = math.fsum(part.tolist())
                want[c_] = s if abs(s) > 1e-20 else 0.0
            assert (want < 0).any() and (want > 0).any()
            assert all(r in active for pair in h.planted["pairs"] for r in pair)
            assert not want[h.planted["private_columns"]].any()
            assert np.array_equal(bits(g), bits(want))


def test_fp64_outside_the_exact_range(monkeypatch):
    """(c) on wide: per coordinate within bounds.out_of_range_bound plus whole regularisers of candidate workers only
    (quantised_allowance); the planted columns (2^-42 .. 2^-46) are at or above half a unit of every fp64 grid used here
    (2^-51 at 4,096 rows) and must NOT vanish; columns whose every entry is below it must"""
    pin(monkeypatch, {})
    h = hd.build("wide")
    o, eng = pair64(h.data)
    van = set(h.planted["vanishing_columns"].tolist())
    assert hd.vexp_of(h.data.val) == 0
    with eng:
        for name in hd.LISTS:
            lists = hd.lists_of("wide", name)
            assert all(hd.outside_exact_range(h.data, rows, len(rows)) > 0 for rows in lists)   # they really ARE outside
            rows = lists[0]
            g, st = eng.gradient_f64(rows, w=h.w)
            g_o = o.gradient(h.w, rows)
            assert st["n_active"] == o.last_stats["n_active"]
            tol, cand, must, unit = orb.out_of_range_bound(o, h.w, g_o, [rows], [shift64(len(rows))], 0)
            used, _ = quantised_allowance("wide", h, g - g_o, tol, unit, cand, must, True, ("rp64 gradient", name), expect_planted=False)
            assert not g[orb.vanished(g - g_o, tol, unit, cand)[0] > 0].any()
            assert not must[list(van)].any() and not orb.vanished(g - g_o, tol, unit, cand)[0][list(van)].any()   # 2^-46 >= half a unit: they stay
            print("rp64 gradient wide %s: %d columns lost the regulariser (%d could)" % (name, used, int((cand > 0).sum())))
            legs = [("rp64", lambda lr: eng.sync_step_f64(lists, lr), [shift64(len(a)) for a in lists])]
            if sum(len(a) for a in lists) <= 1024:
                def plan_leg(lr):
                    p = eng.plan([lists])
                    assert p.info()["kind"] == "column_slices_fp64"
                    eng.synchronize()   # (the counters of whatever ran before)
                    eng.plan_run(p, 0, 1, lr)
                    st_ = eng.synchronize()
                    p.destroy()
                    ran(eng, "dsgd_cs64_step_kernel")
                    return st_
                legs.append(("cs64", plan_leg, [shift64(max(len(a) for a in lists))] * len(lists)))
            for leg, run, shifts in legs:
                lr = lr_of(lists)
                eng.set_weights(h.w)
                st = run(lr)
                w_o = h.w.copy()
                o.sync_step(w_o, lists, lr)
                assert st["n_active"] == o.last_stats["n_active"]
                tol, cand, must, unit = orb.out_of_range_bound(o, h.w, w_o, lists, shifts, 0, lr=lr)
                used, _ = quantised_allowance("wide", h, eng.get_weights() - w_o, tol, unit, cand, must, True, (leg, name), expect_planted=False)
                print("%s step wide %s: %d columns lost the regulariser (%d could)" % (leg, name, used, int((cand > 0).sum())))


def test_fp64_two_ranks_with_different_vexp(tmp_path):
    """rank 0 holds its rows times 2^10 (vexp 10), rank 1 unscaled (vexp 0): vexp_collective must put both on ONE grid --
    after every step the replicas hold the bits of one context over the union"""
    from hard_world2_worker import LAM as W_LAM, STEPS, step_lists, union_data
    from test_rccl_stub import seam_env
    from world2_common import shard_of

    wd = str(tmp_path)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "hard_world2_worker.py"), str(r), "2", wd], env=seam_env(),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-4000:])
    ranks = [dict(np.load(os.path.join(wd, "out_%d.npz" % r))) for r in range(2)]
    assert [int(ranks[r]["vexp"]) for r in range(2)] == [10, 0]
    data = union_data()
    shards = [shard_of(data, hd.N_TRAIN, r, 2) for r in range(2)]
    with dsgd_amd.Engine(data.dim, W_LAM, precision="fp64") as single:
        single.load_csr(data.row_ptr, data.col, data.val, data.label)
        single.build_dim_sparsity(hd.N_TRAIN)
        single.set_weights(np.ldexp(hd.build("signed").w, -5))
        for i in range(len(STEPS)):
            glob, lr = [], None
            for r, sh in enumerate(shards):
                lists, lr = step_lists(r, i, sh.n_train)
                glob += [(l.astype(np.int64) + sh.train_lo).astype(np.int32) for l in lists]
            st = single.sync_step_f64(glob, lr)
            w1 = single.get_weights()
            for r in range(2):
                assert np.array_equal(bits(ranks[r]["w_hist"][i]), bits(w1)), "step %d: rank %d differs from the single context" % (i, r)
                assert ranks[r]["stats"][i].tolist() == [st["n_samples"], st["n_active"]]
            assert 0 < st["n_active"] < st["n_samples"]


# ---- concentrated columns: every integer accumulator at the full scale its host rule allows ------------------------------
# tests/hard_data.py `concentrated`: column P holds y * vmax and column M holds -y * vmax in EVERY row, so from w = 0 (every
# row active) a workgroup's word for P is rows * q(vmax) and for M its negative -- with vmax = 1 exactly rows * 2^shift,
# with the largest float below 2 the same after rounding up.  Each leg reads the shift the launch reports and holds it
# against the host rule restated in hard_data.py: a leg that finds slack FAILS.  A wrapped word is 2^32 grid units off;
# nothing like that fits under the derived bound, and on vmax = 1 the two columns are asserted on BITS.
#   step 1     w = 0: active == rows listed; w[P] = -lr * mean_k(n_k * vmax), w[M] = +that (powers of two: exact)
#   steps 2-3  from the weights step 1 left, lambda = 1e-5.  Those weights classify every row with a margin (y * d =
#              -2 lr n vmax^2 + ...), so both sides must find NO active row and leave the weights alone.
#   step 4     from the NEGATED weights: every row active again at non-zero weights, the regulariser on a support that
#              holds P and M.
CONC_LR = 2.0 ** -12
CONC_LIST_SHAPES = {   # family -> (workers, rows each): powers of two, each at the edge of its family's rule
    "one_workgroup": ((1, 64),),
    "row_wise": ((1, 4096), (2, 1024)),
    "virtual_tiles": ((1, 4096), (2, 1024)),
    "column_slices_host": ((1, 1024), (2, 512)),
    "column_slices_device": ((1, 1024), (2, 512)),
}
CONC_MODES = {"default": {}, "hsplit1": {"DSGD_HSPLIT": "1"}, "bound_off": {"DSGD_FIX_BOUND": "0"}}


def device_cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def list_rows_per_workgroup(family, k, b, n_cu):
    """the rows ONE accumulator word can meet, by the family's documented rule (rows of one lane each in the virtual tiles)"""
    if family == "row_wise":     # launch_grad_mb
        return max(64, -(-b // max(1, n_cu // k)))
    if family == "virtual_tiles":   # vt_build: 64 rows a tile, workgroup g takes the 16-tile groups g, g + gx, ...
        tiles = -(-b // 64)
        gx = max(1, min(n_cu // k, -(-tiles // 16)))
        rows_of = [0] * gx
        for t in range(tiles):
            rows_of[(t // 16) % gx] += min(64, b - 64 * t)
        return max(rows_of)
    return b   # one workgroup per list / one accumulator per worker and column


def conc_pair(which, lam=LAM):
    h = hd.concentrated(which)
    o, eng = make_pair(h.data, lam, h.planted["n_train"])
    return h, o, eng


def conc_steps(o, eng, h, which, run, lists, lr, family, ranges):
    """steps 1 to 4 of the header; returns the shift step 1 reported"""
    p, m, vmax = h.planted["P"], h.planted["M"], h.planted["vmax"]
    total = sum(len(a) for a in lists)
    eng.set_weights(np.zeros(h.data.dim + 1, np.float32))
    st, _ = hard_step(o, eng, "concentrated", h, run, lists, lr, family, ranges)
    shift = eng.tuning_info()["fix_shift"]
    assert st["n_active"] == total == o.last_stats["n_active"]
    w1 = eng.get_weights()
    mean = math.fsum(len(a) * vmax for a in lists) / len(lists)
    if which == "one":
        assert np.array_equal(bits(w1[[p, m]]), bits(np.asarray([-lr * mean, lr * mean], np.float32))), (family, w1[[p, m]], lr * mean)
    for _ in range(2):
        st, _ = hard_step(o, eng, "concentrated", h, run, lists, lr, family, ranges)
        assert st["n_active"] == 0 == o.last_stats["n_active"]
    assert np.array_equal(bits(eng.get_weights()), bits(w1))
    eng.set_weights(-w1)
    st, _ = hard_step(o, eng, "concentrated", h, run, lists, lr, family, ranges)
    assert st["n_active"] == total == o.last_stats["n_active"] and orb.reg_scalar(o, -w1.astype(np.float64)) != 0.0
    return shift


@pytest.mark.parametrize("family,mode", [(f, "default") for f in LIST_FAMILIES] + [("row_wise", "hsplit1"), ("virtual_tiles", "hsplit1")])
def test_fp32_list_families_at_full_scale(monkeypatch, family, mode):
    env, how, _, kernel = LIST_FAMILIES[family]
    pin(monkeypatch, dict(env, **CONC_MODES[mode]))
    n_cu = device_cus()
    for which in hd.VMAX:
        h, o, eng = conc_pair(which)
        edges = 0
        with eng:
            assert (eng.tuning_info()["hsplit"] == 1) == (mode == "hsplit1")
            for k, b in CONC_LIST_SHAPES[family]:
                lists = hd.conc_lists(h.planted["n_train"], k, b)
                shift = conc_steps(o, eng, h, which, lambda: run_lists(eng, how, lists, CONC_LR, kernel), lists, CONC_LR, family, False)
                if family == "virtual_tiles" and mode == "hsplit1":   # (rows of up to three lanes there: no closed rule, no edge)
                    continue
                rows = list_rows_per_workgroup(family, k, b, n_cu)
                want = min(21, 30 - hd.ceil_log2(rows)) if family == "virtual_tiles" else 30 - hd.ceil_log2(rows)
                if family == "one_workgroup":
                    # dsgd_plan_kernel takes 30 - ceil(log2 B) of its sub-batch ON THE DEVICE (csrc/dsgd_batch.hpp) and the host
                    # reports the cap, which the bound above used (coarser, so weaker, than the kernel's own 24): the edge is by
                    # construction, B = 64 = 2^6 rows at 30 - 6, and is held by the bits of w[P] and w[M]
                    assert shift == hd.FIX_SHIFT_CAP and want == 24
                    shift = want
                print("%s %s %s: %d x %d rows, %d rows per workgroup, shift %d" % (family, mode, which, k, b, rows, shift))
                assert shift == want, (family, k, b, rows, shift, want)
                edges += rows << shift == 1 << 30
            assert edges > 0 or (family == "virtual_tiles" and mode == "hsplit1"), "no list length of %s ran with a full word" % family


@pytest.mark.parametrize("family,mode", [(f, m) for f in RANGE_FAMILIES for m in ("default", "bound_off")])
def test_fp32_range_families_at_full_scale(monkeypatch, family, mode):
    range_family_at_full_scale(monkeypatch, family, mode)


def test_fp32_streaming_with_a_cold_concentrated_column(monkeypatch):
    """DSGD_HSPLIT=1: P (rank 0) stays hot, M (rank 1) goes through the cold tiles and the cold partials of the streaming
    launches.  The cold words are emptied by whoever sees one at 2^28, and sixteen waves can each add the rest of a
    128-row tile before that: at the fixed shift 21 this data left the band (DSGD_ESTATE).  build_split now takes the cold
    shift from the data's cold tiles (hard_data.cold_shift_rule: 17 here), and the launch reports the coarser of its two
    grids."""
    range_family_at_full_scale(monkeypatch, "streaming", "hsplit1")


def range_family_at_full_scale(monkeypatch, family, mode):
    env, names, kernel = RANGE_FAMILIES[family]
    pin(monkeypatch, dict(env, **CONC_MODES[mode]))
    n_cu = device_cus()
    hsplit = 1 if mode == "hsplit1" else hd.HSPLIT_DEFAULT
    for which in hd.VMAX:
        h, o, eng = conc_pair(which)
        n = h.planted["n_train"]
        with eng:
            assert eng.tuning_info()["fix_bound"] == (0 if mode == "bound_off" else 1)
            for name in names:
                ranges = {"whole": [(0, n)], "halves": [(0, n // 2), (n // 2, n)]}[name]
                lists = [np.arange(a, b, dtype=np.int32) for a, b in ranges]

                def run():
                    st = eng.sync_step_ranges(ranges, CONC_LR)
                    ran(eng, kernel)
                    return st

                shift = conc_steps(o, eng, h, which, run, lists, CONC_LR, family, True)
                if family == "column_lists":
                    assert shift == 21   # 64-bit sums: the cap alone
                    continue
                rows = hd.streaming_worst_rows(h.data, ranges, n_cu, hsplit) if family == "streaming" else hd.chunk_worst_rows(h.data, ranges, n_cu, hsplit)[0]
                shift0 = hd.shift_of_rows(rows, hd.FIX_SHIFT_CAP)
                # the refinement's A on a concentrated column: every row of the worst workgroup adds ceil(vmax 2^s0 / vmax2) = 2^s0
                want = shift0 if mode == "bound_off" else hd.refined_shift(shift0, rows << shift0, rows)
                assert want == shift0
                cold, a_cold = hd.cold_shift_rule(h.data, hsplit)   # (21 with the default split: no cold entry at all)
                assert cold == (17 if mode == "hsplit1" else 21) and (a_cold >= 128 << 21) == (mode == "hsplit1")   # 128 rows of a cold tile hold M
                print("%s %s %s %s: worst workgroup %d rows, shift0 %d, cold %d, shift %d" % (family, mode, which, name, rows, shift0, cold, shift))
                assert rows > 512 and shift < 21 and shift == min(want, cold), (family, name, rows, shift0, want, cold, shift)


def test_fp32_lock_free_engine_with_one_worker_at_full_scale(monkeypatch):
    """batch = 64 = 2^6 rows at shift 30 - 6: 64 * 2^24 = 2^30, the rule of hog_launch with equality; replayed by the oracle as
    test_fp32_lock_free_engine_with_one_worker does, P and M on bits for vmax = 1"""
    pin(monkeypatch, {"DSGD_CS": "0"})
    batch, n_upd, lr = 64, 3, 2.0 ** -8
    for which in hd.VMAX:
        h, o, eng = conc_pair(which)
        n = h.planted["n_train"]
        with eng:
            eng.set_weights(np.zeros(h.data.dim + 1, np.float32))
            w_ref = np.zeros(h.data.dim + 1)
            eng.async_start([(0, n)], batch=batch, lr=lr, max_updates=n_upd, seed=77, positional_bug=False)
            eng.async_wait()
            assert eng.async_updates() == (n_upd, False)
            active = []
            for it in range(n_upd):
                o.async_step(w_ref, hog_rows(77, 0, it, 0, n, batch, False), lr)
                active.append(o.last_stats["n_active"])
            w = eng.get_weights()
            assert active == [batch, 0, 0] and w_ref[h.planted["P"]] < 0 < w_ref[h.planted["M"]]
            assert np.abs(w.astype(np.float64) - w_ref).max() <= 4 * tol32(w_ref)
            if which == "one":
                pm = [h.planted["P"], h.planted["M"]]
                assert np.array_equal(bits(w[pm]), bits(w_ref[pm].astype(np.float32))) and abs(w_ref[pm[0]]) in (lr * batch, lr)


# ---- fp64 at full scale: n * 2^(62 - ceil(log2 n)) == 2^62 at n = 2^k, on float values and on the Double twin -------------
CONC_N64 = (1, 2, 3, 1024, 1025, 4096, 4097)


def conc_engine64(which, double, lam, monkeypatch=None, fused=None):
    h = hd.concentrated(which, double=double)
    if fused is not None:
        monkeypatch.setenv("DSGD_RP64_FUSED", "1" if fused else "0")
    eng = dsgd_amd.Engine(h.data.dim, lam, precision="fp64")
    if fused is not None:
        monkeypatch.delenv("DSGD_RP64_FUSED")
    eng.load_csr(h.data.row_ptr, h.data.col, h.data.val, h.data.label)
    eng.build_dim_sparsity(h.planted["n_train"])
    assert eng.value_bits() == (64 if double else 32)
    return h, eng


def conc_exact(data, idx):
    """the correctly rounded exact sum per column (tests/test_gpu_fp64_values.py _fsum_gradient)"""
    from test_gpu_fp64_values import _fsum_gradient

    return _fsum_gradient((data.row_ptr, data.col, data.val.astype(np.float64), data.label), [int(r) for r in idx], data.dim + 1)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("which", list(hd.VMAX))
def test_fp64_exact_sums_at_full_scale(monkeypatch, which, double):
    pin(monkeypatch, {})
    h, eng = conc_engine64(which, double, 0.0)
    d, n_train, vmax, p, m = h.data, h.planted["n_train"], h.planted["vmax"], h.planted["P"], h.planted["M"]
    zero = np.zeros(d.dim + 1)
    perm = np.random.default_rng(23).permutation(n_train).astype(np.int32)
    lr = 2.0 ** -9
    with eng:
        for n in CONC_N64 + (n_train,):
            idx = perm[:n].copy()
            want = conc_exact(d, idx)
            assert want[p] == math.fsum([vmax] * n) == -want[m] and (double and which == "below2" or want[p] == n * vmax)
            g, st = eng.gradient_f64(idx, w=zero)
            assert st["n_active"] == n
            assert g[p] == math.fsum([vmax] * n) and g[m] == -g[p], (n, g[p])
            assert np.array_equal(bits(g), bits(want)), (n, np.flatnonzero(g != want)[:8])
            for other in (idx[::-1].copy(), np.random.default_rng(n).permutation(idx)):
                g2, _ = eng.gradient_f64(other, w=zero)
                assert np.array_equal(bits(g2), bits(g)), n
            # the duplicate list: one row n times, its full-scale entry in a column of rank >= RP64_HOT (plain global atomics)
            dup = np.full(n, h.planted["dup_row"], np.int32)
            gd, st = eng.gradient_f64(dup, w=zero)
            assert st["n_active"] == n and gd[h.planted["cold_column"]] == math.fsum([vmax] * n)
            assert np.array_equal(bits(gd), bits(conc_exact(d, dup)))
            # one worker's synchronous step from w = 0: w = -lr * g (a power of two: exact)
            for lists, wanted in (([idx], want), ([dup], conc_exact(d, dup))):
                eng.set_weights(zero)
                st = eng.sync_step_f64(lists, lr)
                assert st["n_active"] == n and np.array_equal(bits(eng.get_weights()), bits(0.0 - lr * wanted)), n
            if n <= 1024 and not double:   # the column-slice plan, inside its limits (float values: dsgd_plan_create refuses Double data)
                eng.set_weights(zero)
                plan = eng.plan([[idx]])
                assert plan.info()["kind"] == "column_slices_fp64"
                eng.plan_run(plan, 0, 1, lr)
                eng.synchronize()
                ran(eng, "dsgd_cs64_step_kernel")
                plan.destroy()
                assert np.array_equal(bits(eng.get_weights()), bits(0.0 - lr * want)), n
            if n <= 1024:   # the asynchronous iteration: the MEAN over the listed rows (core/Slave.scala:92-101)
                eng.set_weights(zero)
                dl, st = eng.async_step(idx, lr, want_delta=True)
                w = eng.get_weights()
                assert st["n_active"] == n and np.array_equal(w, -dl)
                assert np.abs(w + lr * want / n).max() <= 1e-12 * scale64(lr * want / n), n
                if not double:   # n equal values: the quotient is vmax again, exactly
                    ran(eng, "dsgd_cs64_async_kernel")
                    assert w[p] == -lr * vmax and w[m] == lr * vmax, (n, w[p])
    if double and which == "below2":   # both words, the high one near full scale
        assert math.fsum([vmax] * 4096) == 8192.0 - 2.0 ** -40 != 4096 * 2.0


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("double", [False, True])
def test_fp64_steps_in_one_call_at_full_scale(monkeypatch, double, fused):
    from test_gpu_fp64_steps import _served

    pin(monkeypatch, {})
    lr = 2.0 ** -9
    for which in hd.VMAX:
        h, eng = conc_engine64(which, double, 0.0, monkeypatch, fused)
        d = h.data
        perm = np.random.default_rng(29).permutation(h.planted["n_train"]).astype(np.int32)
        with eng:
            for n in CONC_N64:
                for idx in (perm[:n].copy(), np.full(n, h.planted["dup_row"], np.int32)):
                    want = conc_exact(d, idx)
                    eng.set_weights(np.zeros(d.dim + 1))
                    st = eng.sync_steps_f64(idx, np.asarray([0, n]), 1, 1, lr, per_step=True)
                    assert eng.grad_kernel_name() == _served(fused, double), (fused, eng.grad_kernel_name())
                    assert st["n_active"] == n == int(st["active_per_step"][0])
                    assert np.array_equal(bits(eng.get_weights()), bits(0.0 - lr * want)), (which, n)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("which", list(hd.VMAX))
def test_fp64_steps_at_full_scale_against_the_reference(monkeypatch, which, double):
    """steps 1 to 4 of the fp32 header at lambda = 1e-5: orc_sync_step on float values, ref_dict on the Double twin; 1e-12 *
    max(1, |ref|_inf), equal supports and active counts.  sync_step_f64 (2 x 1,024 rows, 1 x 4,096), the cs64 plan (2 x 512)."""
    from oracle import ref_dict as rd

    pin(monkeypatch, {})
    h, eng = conc_engine64(which, double, LAM)
    d, n_train, dp = h.data, h.planted["n_train"], h.data.dim + 1
    lr = 2.0 ** -9
    if double:
        rows = {}

        def sample(r):
            if r not in rows:
                b, e = int(d.row_ptr[r]), int(d.row_ptr[r + 1])
                rows[r] = (rd.Sparse({int(c): float(v) for c, v in zip(d.col[b:e], d.val[b:e])}, dp), int(d.label[r]))
            return rows[r]

        model = rd.SparseSVM(LAM, rd.dim_sparsity([sample(r) for r in range(n_train)]))
    else:
        o = orc.Oracle(d.dim, d.row_ptr, d.col, d.val, d.label, LAM)
        o.set_dim_sparsity(o.dim_sparsity(n_train))

    def ref_step(w, lists):
        """-> (weights after, active rows) from the dense float64 w"""
        if not double:
            out = w.copy()
            o.sync_step(out, lists, lr)
            return out, o.last_stats["n_active"]
        data = {int(r): sample(int(r)) for a in lists for r in a}
        ws = rd.Sparse({int(k): float(w[k]) for k in np.flatnonzero(w)}, dp)
        act = sum(1 for a in lists for r in a if not (data[int(r)][1] * data[int(r)][0].dot(ws) < 0))
        after = rd.master_sync_step(model, data, ws, [[int(r) for r in a] for a in lists], lr)
        out = np.zeros(dp)
        for k, v in after.map.items():
            out[k] = v
        return out, act

    with eng:
        if double:
            ds = np.zeros(dp)
            for k, v in model.dim_sparsity.map.items():
                ds[k] = v
            assert np.array_equal(bits(eng.get_dim_sparsity()), bits(ds))
        for k, b, planned in ((2, 1024, False), (1, 4096, False)) + (() if double else ((2, 512, True),)):   # (no plans on Double data)
            lists = hd.conc_lists(n_train, k, b, seed=1)
            total = k * b

            def step():
                if not planned:
                    return eng.sync_step_f64(lists, lr)["n_active"]
                plan = eng.plan([lists])
                assert plan.info()["kind"] == "column_slices_fp64"
                plan.record(True)
                eng.plan_run(plan, 0, 1, lr)
                eng.synchronize()
                mask, _ = plan.read_record()
                plan.destroy()
                return int(mask[0][:total].sum())

            w = np.zeros(dp)
            eng.set_weights(w)
            for leg, active in enumerate((total, 0, 0, total)):
                if leg == 3:
                    w = -w
                    eng.set_weights(w)
                w_ref, act_ref = ref_step(w, lists)
                act = step()
                w = eng.get_weights()
                assert act == act_ref == active, (k, b, leg, act, act_ref)
                assert np.array_equal(np.flatnonzero(w), np.flatnonzero(w_ref)), (k, b, leg)
                assert np.abs(w - w_ref).max() <= 1e-12 * scale64(w_ref), (k, b, leg)
            assert w[h.planted["P"]] != 0.0 and w[h.planted["M"]] != 0.0
