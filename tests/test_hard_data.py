"""The hostile-value traits of tests/hard_data.py, pinned against the oracle alone (no GPU): a later edit cannot quietly
defuse what tests/test_gpu_hard_values.py feeds the kernels.  Also: the near-gate share of every list the GPU module
uses (printed, at most 0.1 % of the rows under the RELATIVE allowance of oracle/bounds.py), the oracle's own scale
covariance bit for bit (so that statement tests kernels, not the data), and vmax2_of against the engine's frexp."""

import math

import numpy as np
import pytest

import hard_data as hd
from oracle import bounds as orb
from oracle import oracle as orc

LAM = 1e-5


def oracle_of(data, lam=LAM, n_train=hd.N_TRAIN):
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, lam)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    return o


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_base_is_one_point():
    b = hd.base()
    assert b.val.min() > 0 and b.val.max() <= 1.0 and np.diff(b.row_ptr).min() >= 1
    assert hd.vexp_of(b.val) in (0, -1)


@pytest.mark.parametrize("trait,want", [("scaled_p10", 10), ("scaled_m30", -30), ("signed", 0), ("wide", 0), ("zero_margin", 0),
                                        ("ragged64", 0)])
def test_vexp_of_every_trait(trait, want):
    h = hd.build(trait)
    assert hd.vexp_of(h.data.val) == hd.vexp_of(hd.base().val) + want if trait != "ragged64" else hd.vexp_of(h.data.val) == 0
    assert orb.vmax2_of(h.data.val) == 2.0 ** hd.vexp_of(h.data.val)
    assert np.isfinite(h.data.val).all() and (h.w.astype(np.float32).astype(np.float64) == h.w).all()


def test_vmax2_of_agrees_with_the_engines_frexp():
    """oracle/bounds.py takes ceil(log2 m) in floating point, the engine frexp (dsgd_load_csr): exact powers of two, one
    ulp above and below, and the float32 extremes the traits reach"""
    for e in list(range(-60, 41)) + [-126, -100, 100, 127]:
        p = np.float32(2.0 ** e)
        for m in (p, np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(0))):
            assert orb.vmax2_of(np.asarray([m, -m / 2], np.float32)) == 2.0 ** hd.vexp_of(np.asarray([m], np.float32)), (e, m)
    assert hd.vexp_of(np.asarray([1.0], np.float32)) == 0 and hd.vexp_of(np.asarray([1.0000001], np.float32)) == 1
    assert hd.vexp_of(np.asarray([0.99999994], np.float32)) == 0 and hd.vexp_of(np.asarray([0.5], np.float32)) == -1


@pytest.mark.parametrize("name", ["k1b100", "k3b100", "k2b700", "k1b4096"])
def test_signed_pairs_cancel_to_an_exact_zero(name):
    h = hd.build("signed")
    o = oracle_of(h.data)
    assert (h.data.val < 0).sum() > 0.4 * h.data.nnz
    priv = h.planted["private_columns"]
    assert orb.reg_scalar(o, h.w) != 0.0
    lists = hd.lists_of("signed", name)
    held = 0
    for rows in lists:
        g = o.gradient(h.w, rows)
        for ra, rb in h.planted["pairs"]:
            assert (ra in rows) == (rb in rows)
            held += ra in rows
        assert np.array_equal(bits(g[priv]), bits(np.zeros(len(priv))))   # off the support: no regulariser either
    assert held == len(h.planted["pairs"])
    # one row of a pair alone: its columns ARE in the support
    g = o.gradient(h.w, np.asarray([h.planted["pairs"][0][0]], np.int32))
    assert (g[priv[:3]] != 0).all()


def test_zero_margin_rows_sit_on_the_gate():
    h = hd.build("zero_margin")
    o = oracle_of(h.data)
    p = h.planted
    rows = p["rows_a"] + p["rows_b"] + p["rows_c"]
    for r in rows:
        assert o.row_dot(r, h.w) == 0.0
    assert {int(h.data.label[r]) for r in p["rows_a"]} == {1, -1} == {int(h.data.label[r]) for r in p["rows_b"]}
    o.gradient(h.w, np.asarray(rows, np.int32))
    assert o.last_stats["n_active"] == len(rows) and o.last_stats["n_exact_zero"] == len(rows)
    assert (h.w[p["columns_a"]] != 0).all() and (h.w[p["columns_b"]] != 0).all() and (h.w[p["columns_c"]] == 0).all()
    assert float(np.float32(2.0 ** -34)) > 1e-20 > float(np.float32(2.0 ** -34)) * 2.0 ** -34 > 0

    # the gate in three lines of numpy, with and without the product filter of math/Sparse.scala:46
    def active(filtered):
        out = []
        for r in range(hd.N_TRAIN):
            prod = h.data.val[h.data.row_ptr[r]:h.data.row_ptr[r + 1]].astype(np.float64) * h.w[h.data.col[h.data.row_ptr[r]:h.data.row_ptr[r + 1]]]
            d = float(np.where(np.abs(prod) > 1e-20, prod, 0.0).sum() if filtered else prod.sum())
            out.append(not (float(h.data.label[r]) * d < 0))
        return np.asarray(out)

    with_f, without = active(True), active(False)
    assert sorted(np.flatnonzero(with_f != without).tolist()) == sorted(p["rows_b"])
    assert with_f[p["rows_b"]].all() and not without[p["rows_b"]].any()
    o.gradient(h.w, np.arange(hd.N_TRAIN, dtype=np.int32))
    assert o.last_stats["n_active"] == int(with_f.sum())
    # gating on <= 0 instead of < 0 would switch every planted row off
    assert all(float(h.data.label[r]) * o.row_dot(r, h.w) <= 0 for r in rows)


def test_wide_entries_and_vanishing_columns():
    h = hd.build("wide")
    o = oracle_of(h.data)
    van = h.planted["vanishing_columns"]
    _, e = np.frexp(h.data.val.astype(np.float64))
    assert hd.vexp_of(h.data.val) - (e - 1).min() >= 45 and np.abs(h.data.val).min() > 1e-20
    for c in van:
        v = h.data.val[h.data.col == c]
        assert len(v) == 5 and v.max() < 2.0 ** -42 and v.min() >= 2.0 ** -46
    for name in hd.LISTS:
        n_out = 0
        g_all = np.zeros(h.data.dim + 1)
        for rows in hd.lists_of("wide", name):
            n_out += hd.outside_exact_range(h.data, rows, len(rows))
            g_all += np.abs(o.gradient(np.zeros(h.data.dim + 1), rows))   # (w = 0: every row active)
        assert n_out > 0.2 * sum(len(r) for r in hd.lists_of("wide", name))   # the lists really ARE outside the range
        assert (g_all[van] != 0).all()                    # in the oracle's support: it regularises them
    with pytest.raises(AssertionError):
        hd.check_exact_range(h.data, hd.lists_of("wide", "k1b4096")[0], 4096)
    # ... and every other trait is inside it at the lists' sizes, zero_margin's 2^-34 by its single mantissa bit
    for trait in ("signed", "ragged64", "scaled_p10", "scaled_m30"):
        d = hd.build(trait).data
        for name in hd.LISTS:
            for rows in hd.lists_of(trait, name):
                hd.check_exact_range(d, rows, len(rows))
                assert hd.outside_exact_range(d, rows, len(rows)) == 0
    z = hd.build("zero_margin")
    oz = oracle_of(z.data)
    for name in hd.LISTS:
        for rows in hd.lists_of("zero_margin", name):
            assert hd.outside_exact_range(z.data, rows, len(rows)) == sum(r in rows for r in z.planted["rows_b"])
            assert not orb.inexact_counts(oz, rows, 0, 62 - math.ceil(math.log2(len(rows)))).any()


def test_ragged64_shapes():
    h = hd.build("ragged64")
    lens = np.diff(h.data.row_ptr)
    assert (lens == 0).sum() > 500 and (lens == 1).sum() > 500 and sorted(lens[lens > 2000].tolist()) == [3000] * 4 + [8000] * 2
    assert (h.data.val == np.float32(1e-25)).sum() > 500
    for name in hd.LISTS:
        flat = np.concatenate(hd.lists_of("ragged64", name))
        assert lens[flat].max() >= 3000 and (lens[flat] == 0).any()
    assert lens[hd.lists_of("ragged64", "k1b4096")[0]].max() == 8000


@pytest.mark.parametrize("k", [10, -30])
def test_the_oracle_is_scale_covariant_bit_for_bit(k):
    """lambda = 0, X' = 2^k X, w' = 2^-k w, lr' = 2^-2k lr: g' == 2^k g and w_after' == 2^-k w_after as 64-bit patterns, and no
    quantity the absolute 1e-20 filter looks at is within a factor 1,000 of it in either frame"""
    trait = "scaled_p10" if k == 10 else "scaled_m30"
    plain, h = hd.build("plain"), hd.build(trait)
    o, o_s = oracle_of(plain.data, 0.0), oracle_of(h.data, 0.0)
    assert np.array_equal(bits(h.w), bits(np.ldexp(plain.w, -k)))
    for name in hd.LISTS:
        lists = hd.lists_of(trait, name)
        for rows in lists:
            g, n = o.gradient(plain.w, rows), o.last_stats["n_active"]
            g_s = o_s.gradient(h.w, rows)
            assert o_s.last_stats["n_active"] == n and 0 < n < len(rows)
            assert np.array_equal(bits(g_s), bits(np.ldexp(g, k)))
            for q in (g, g_s):
                assert np.abs(q[q != 0]).min() > 1e-17
            assert np.array_equal(o.forward(plain.w, rows), o_s.forward(h.w, rows))
        lr = 0.5
        w1, w1_s = plain.w.copy(), h.w.copy()
        o.sync_step(w1, lists, lr)
        o_s.sync_step(w1_s, lists, math.ldexp(lr, -2 * k))
        assert np.array_equal(bits(w1_s), bits(np.ldexp(w1, -k)))
        for q in (w1, w1_s, w1 - plain.w, w1_s - h.w):
            assert np.abs(q[q != 0]).min() > 1e-17
    for d, w in ((plain.data, plain.w), (h.data, h.w)):
        prod = np.abs(d.val.astype(np.float64) * w[d.col])
        assert np.abs(d.val).min() > 1e-17 and prod[prod != 0].min() > 1e-17


def near_share(o, w, rows, rel_eps):
    _, _, n = orb._list_profile(o, w, rows, orb.GATE_EPS, rel_eps)
    return n, len(rows)


def test_near_gate_share_of_every_list_the_gpu_module_uses(capsys):
    """rows the ORACLE places within the relative near-gate allowance (0 < |d| < rel_eps * sum |x_i w_i|, rel_eps =
    (longest row + 2) * 2^-24): at most 0.1 % of every list and range, the cap of run_sync; d == 0 is not near"""
    lines = []
    for trait in ("plain",) + hd.TRAITS:
        h = hd.build(trait)
        o = oracle_of(h.data)
        eps = orb.rel_gate_eps(o)
        assert eps == (int(np.diff(h.data.row_ptr).max()) + 2) * 2.0 ** -24
        worst = 0.0
        for name in hd.LISTS:
            for rows in hd.lists_of(trait, name):
                n, total = near_share(o, h.w, rows, eps)
                assert n <= 1e-3 * total, (trait, name, n, total)
                worst = max(worst, n / total)
        for name, ranges in hd.RANGES.items():
            for lo, hi in ranges:
                n, total = near_share(o, h.w, np.arange(lo, hi), eps)
                assert n <= 1e-3 * total, (trait, name, n, total)
                worst = max(worst, n / total)
        lines.append("near-gate share  %-12s rel_eps %.3g  worst list %.4f %%" % (trait, eps, 100 * worst))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_optional_bound_arguments_default_to_the_old_bound():
    """list_bound with its defaults against a frozen restatement of the formula it had before the optional arguments"""
    h = hd.build("plain")
    o = oracle_of(h.data)
    lists = hd.lists_of("plain", "k3b100")
    w1 = h.w.copy()
    o.sync_step(w1, lists, 0.5)
    lr, shift, k = 0.5, 23, len(lists)
    cnt, near, n_near, gabs = np.zeros(o.dim + 1), np.zeros(o.dim + 1), 0, np.zeros(o.dim + 1)
    for rows in lists:
        c, nr, n = orb._list_profile(o, h.w, rows, 1e-5)
        cnt, near, n_near = cnt + c, near + nr, n_near + n
        gabs += np.abs(o.gradient(h.w, rows))
    want = (lr / k) * (cnt * (orb.vmax2_of(o.val) * 2.0 ** (-(shift + 1))) + near)
    want += 8.0 * 2.0 ** -24 * (np.abs(w1) + np.abs(w1 - h.w)) + 1e-9
    want += 2.0 * 2.0 ** -24 * (lr / k) * gabs
    got, n = orb.list_bound(o, h.w, w1, lists, lr, shift)
    assert n == n_near and np.array_equal(got, want)
    cand, must = orb.vanishing(o, h.w, lists, [2.0 ** -24] * k)
    assert not cand.any() and not must.any()   # unit-norm rows: no column can vanish


def test_the_vanishing_term_prices_only_columns_that_can_vanish():
    """wide at a coarse fp32 grid: the planted columns (5 entries below 2^-42) MUST vanish, other columns whose few entries
    all drew a large u can -- but never one whose oracle sum exceeds the grid error; and the allowance is quantised"""
    h = hd.build("wide")
    o = oracle_of(h.data)
    rows = hd.lists_of("wide", "k1b4096")[0]
    cnt, _, _ = orb._list_profile(o, h.w, rows, 1e-5)
    half = 2.0 ** -(23 + 1)
    cand, must = orb.vanishing(o, h.w, [rows], [half])
    g0 = orb._g0(o, h.w, rows)
    assert cand.any() and (np.abs(g0[cand > 0]) <= cnt[cand > 0] * half).all() and not cand[g0 == 0].any() and (must <= cand).all()
    van = h.planted["vanishing_columns"]
    assert ((must[van] == 1) | (g0[van] == 0)).all() and must[van].any()
    s = orb.reg_scalar(o, h.w)
    assert 1e-6 < abs(s) < 1e-3     # three orders above the 1e-9 the bound grants s: the term is not a formality
    # the quantised reading: one whole regulariser on a candidate is accepted, half of one is not, one elsewhere is not
    j, i = int(np.flatnonzero(cand)[0]), int(np.flatnonzero((cand == 0) & (cnt > 0))[0])
    base = np.full(o.dim + 1, 1e-9)
    for at, amount, ok in ((j, -s, True), (j, -0.5 * s, False), (i, -s, False)):
        diff = np.zeros(o.dim + 1)
        diff[at] = amount
        assert (orb.vanished(diff, base, -s, cand)[1].max() <= 1.0) == ok


# ---- concentrated columns: the data and the reference side of tests/test_gpu_hard_values.py's full-scale legs -------------
FP64_LIST_ROWS = (1, 2, 3, 1024, 1025, 4096, 4097)


def _exact_sums(data, rows):
    """math.fsum of y * x per column over the listed rows (duplicates count)"""
    per = {}
    for r in rows:
        for p in range(int(data.row_ptr[r]), int(data.row_ptr[r + 1])):
            per.setdefault(int(data.col[p]), []).append(float(data.val[p]) * float(data.label[r]))
    return {c: math.fsum(v) for c, v in per.items()}


@pytest.mark.parametrize("which,vexp", [("one", 0), ("below2", 1)])
def test_concentrated_vexp_and_shape(which, vexp):
    h = hd.concentrated(which)
    d, n = h.data, h.planted["n_train"]
    assert hd.vexp_of(d.val) == vexp and orb.vmax2_of(d.val) == 2.0 ** vexp
    assert float(np.abs(d.val).max()) == h.planted["vmax"] == hd.VMAX[which]
    m, e = math.frexp(hd.VMAX64[which])   # the Double twin by the same rule on doubles (dsgd_load_csr_f64)
    assert (e - 1 if m == 0.5 else e) == vexp and np.abs(hd.concentrated(which, double=True).data.val).max() == hd.VMAX64[which]
    lens = np.diff(d.row_ptr)[:n]
    assert lens.min() == 2 and lens.max() == 4 and {int(y) for y in d.label[:n]} == {1, -1}
    first, y = d.row_ptr[:n], d.label[:n].astype(np.float64)
    assert (d.col[first] == hd.CONC_P).all() and (d.col[first + 1] == hd.CONC_M).all()
    assert (d.val[first] * y == h.planted["vmax"]).all() and (d.val[first + 1] * y == -h.planted["vmax"]).all()
    rest = np.abs(d.val[~np.isin(d.col, [hd.CONC_P, hd.CONC_M, hd.CONC_COLD])])
    assert rest.min() > 0 and rest.max() <= h.planted["vmax"] / 4
    # the contribution of the second vmax rounds UP to exactly 2^shift on every fp32 grid up to shift 23 (a tie to even
    # there): the bound is met with equality; at shift 24 (64 rows) it is the integer 2^24 - 1
    if which == "below2":
        for shift in range(1, 24):
            assert np.rint(np.float32(math.ldexp(h.planted["vmax"], shift - vexp))) == 2.0 ** shift
        assert math.ldexp(h.planted["vmax"], 24 - vexp) == 2.0 ** 24 - 1


@pytest.mark.parametrize("which", ["one", "below2"])
def test_concentrated_rows_are_all_active_at_zero_and_sum_in_closed_form(which):
    from oracle import ref_dict as rd

    h = hd.concentrated(which)
    d, n, vmax = h.data, h.planted["n_train"], h.planted["vmax"]
    o = oracle_of(d, n_train=n)
    rows = np.arange(n, dtype=np.int32)
    g = o.gradient(np.zeros(d.dim + 1), rows)
    assert o.last_stats["n_active"] == n
    want = _exact_sums(d, rows.tolist())
    assert g[hd.CONC_P] == math.fsum([vmax] * n) == n * vmax == want[hd.CONC_P]
    assert g[hd.CONC_M] == -math.fsum([vmax] * n) == -n * vmax == want[hd.CONC_M]
    # ref_dict: every row passes the gate at w = 0, on float and on Double values
    for double in (False, True):
        dd = hd.concentrated(which, double=double).data
        w0 = rd.Sparse({}, dd.dim + 1)
        sub = list(range(0, n, 7))
        data = {r: (rd.Sparse({int(c): float(v) for c, v in zip(dd.col[dd.row_ptr[r]:dd.row_ptr[r + 1]], dd.val[dd.row_ptr[r]:dd.row_ptr[r + 1]])},
                              dd.dim + 1), int(dd.label[r])) for r in sub}
        assert all(not (y * x.dot(w0) < 0) for x, y in data.values())
        model = rd.SparseSVM(0.0, rd.Sparse({}, dd.dim + 1))
        gs = rd.slave_gradient(model, data, w0, sub)
        v = hd.VMAX64[which] if double else vmax
        assert gs.map[hd.CONC_P] == math.fsum([v] * len(sub)) and gs.map[hd.CONC_M] == -math.fsum([v] * len(sub))


def test_concentrated_size_comes_from_the_host_rules():
    """the smallest count (in steps of 256, from the range families' dispatch floor) with shift0 < 21 in both range launches"""
    n = hd.concentrated_rows()
    d = hd.concentrated("one").data
    assert n < 30000 and n % 256 == 0
    for ranges in ([(0, n)], [(0, n // 2), (n // 2, n)]):
        ws, (wc, n_wg) = hd.streaming_worst_rows(d, ranges), hd.chunk_worst_rows(d, ranges)
        assert ws > 512 and wc > 512 and n_wg == min(ranges[0][1] - ranges[0][0], hd.N_CU * hd.FSTEP_ROWS // len(ranges)) // hd.FSTEP_ROWS
        assert hd.shift_of_rows(ws, hd.FIX_SHIFT_CAP) < 21 and hd.shift_of_rows(wc, hd.FIX_SHIFT_CAP) < 21
    if n > hd.CONC_RANGE_MIN:
        smaller = hd._conc_data("one", False, n - 256)
        assert min(hd.streaming_worst_rows(smaller, [(0, n - 256)]), hd.chunk_worst_rows(smaller, [(0, n - 256)])[0]) <= 512
    # the refinement cannot lift a concentrated column: A = rows * 2^shift0 > 2^29, so 2 A + rows > 2^30
    for rows in (513, 517, 1024, 2692, 4064):
        s0 = hd.shift_of_rows(rows, hd.FIX_SHIFT_CAP)
        assert hd.refined_shift(s0, rows << s0, rows) == s0
    assert hd.refined_shift(18, 1 << 20, 2692) == 21 and hd.refined_shift(18, (1 << 28) - 2692, 2692) == 20   # (it does lift ordinary data)
    # lowered split: M's rank 1 is at the split of 1, P's rank 0 stays hot
    r = hd.column_ranks(d)
    assert (r[hd.CONC_P], r[hd.CONC_M]) == (0, 1)
    # ... and the cold words' scale follows the cold tiles: a 128-row tile holds M 128 times (2^28 at shift 21), sixteen waves
    # twice that each: 17 is the finest shift that keeps a word below 2^30; no cold entry at the default split: 21
    for which in hd.VMAX:
        dd = hd.concentrated(which).data
        s, a = hd.cold_shift_rule(dd, 1)
        assert s == 17 and a >= 128 << 21 and 2 ** 28 + 2 ** s + 32 * (a // 16 + 256) < 2 ** 30 <= 2 ** 28 + 2 ** (s + 1) + 32 * (a // 8 + 256)
        assert hd.cold_shift_rule(dd) == (21, 0)


def test_the_duplicate_lists_column_is_cold_for_the_fp64_kernels():
    h = hd.concentrated("one")
    d = h.data
    cnt = np.bincount(d.col, minlength=d.dim + 1)
    rank = sorted(range(d.dim + 1), key=lambda c: (-cnt[c], c)).index(h.planted["cold_column"])   # count descending, ties by key
    assert rank >= hd.RP64_HOT and rank == hd.column_ranks(d)[h.planted["cold_column"]]
    b, e = int(d.row_ptr[h.planted["dup_row"]]), int(d.row_ptr[h.planted["dup_row"] + 1])
    full = np.abs(d.val[b:e]) == h.planted["vmax"]
    assert full.sum() == 1 and d.col[b:e][full][0] == h.planted["cold_column"] and cnt[h.planted["cold_column"]] == 1
    assert float(d.val[b:e][full][0]) * float(d.label[h.planted["dup_row"]]) == h.planted["vmax"]


def test_fp64_shift_is_tight_at_powers_of_two():
    for n in FP64_LIST_ROWS + (hd.concentrated_rows(),):
        s = 62 - hd.ceil_log2(n)
        assert hd.ceil_log2(n) == (math.ceil(math.log2(n)) if n > 1 else 0)
        assert n * 2 ** s <= 2 ** 62 and (n * 2 ** s == 2 ** 62) == (n & (n - 1) == 0)
        if n & (n - 1):
            assert n * 2 ** (s + 1) > 2 ** 62   # one finer would not fit
