"""-m gpu: K8, the dense logistic step, where tests/test_gpu_dense.py does not reach: several blocks per workgroup (the
path bench.py measures), exact range edges through sentinel columns, the link function bit by bit up to saturated
logits, every width, and the entry points nothing else calls.  Bounds come from tests/dense_bound.py (derived from the
kernels' operation order, shown sound and non-vacuous on the CPU by tests/test_dense_bound.py), never from the
engine's own output.  Every step is compared with the fp64 oracle started from the ENGINE's weights before that step,
so a bound covers exactly one step."""

import numpy as np
import pytest

import dense_bound as db
import dsgd_amd
import waivers
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

U = db.U
VARIANTS = pytest.mark.parametrize("variant", [0, 1])


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def engine(monkeypatch, variant, D):
    monkeypatch.setenv("DSGD_DENSE_MFMA", str(variant))
    return dsgd_amd.DenseLogistic(D)


def step_and_check(eng, X, y, lr, rb, re, variant, cu):
    """One step from the engine's current weights; weights within dw of the oracle.  Returns the Bound."""
    w0 = eng.get_weights()
    bd = db.Bound(X, y, w0, lr, rb, re, variant, db.launch_grid(variant, cu, re - rb))
    eng.step(rb, re, lr)
    err = np.abs(eng.get_weights().astype(np.float64) - bd.w_ref)
    ratio = err / np.maximum(bd.dw, 1e-300)      # (dw is 0 in an all-zero column whose weight is 0: err must be 0 too)
    print("step [%d, %d): max err / dw = %.3g, |dw|_inf = %.3g" % (rb, re, ratio.max(), bd.dw.max()))
    assert (err <= bd.dw).all(), (rb, re, int(np.argmax(ratio)), ratio.max())
    return bd


def loss_and_check(eng, X, y, rb, re, variant, family=None):
    """loss() of a range under the engine's weights: loss within what dz implies, the tally exact on the rows whose
    class round-off cannot change."""
    w = eng.get_weights()
    bd = db.Bound(X, y, w, 1.0, rb, re, variant, 1)
    loss, acc = eng.loss(rb, re)
    print("loss [%d, %d): err / dloss = %.3g" % (rb, re, abs(loss - bd.loss_ref) / bd.dloss))
    assert abs(loss - bd.loss_ref) <= bd.dloss, (loss, bd.loss_ref, bd.dloss)
    n = re - rb
    n_exc = int((~bd.certain).sum())
    assert n_exc <= 0.01 * n, n_exc
    sure = int((bd.correct & bd.certain).sum())
    got = round(acc * n)
    assert abs(acc * n - got) < 1e-6 and sure <= got <= sure + n_exc, (acc * n, sure, n_exc)
    if family:
        waivers.check(family, n_exc == 0, "%d rows with |z| <= dz" % n_exc)
    return bd


# ---- a. several blocks per workgroup, unequal counts ---------------------------------------------------------------
@VARIANTS
@pytest.mark.parametrize("D", [512, 4096])
def test_several_blocks_per_workgroup(monkeypatch, variant, D):
    """D = 512: 3 * 16 * n_cu + 8 * n_cu + 5 rows from row 3 -- every workgroup walks 3 or 4 blocks of the
    `blk += gridDim.x` loop and the last block is ragged; D = 4096: 16 * n_cu + 24 rows.  Non-zero set_weights; a
    second step over a different range and a third over 100 rows (a grid smaller than the partials the earlier steps
    left in gpart) show stale gpart rows."""
    cu = n_cu()
    X, y, w0, lr, ranges = db.case_a(D, cu)
    with engine(monkeypatch, variant, D) as eng:
        eng.load(X, y)
        eng.set_weights(w0)
        np.testing.assert_array_equal(eng.get_weights(), w0)
        for rb, re in ranges:
            step_and_check(eng, X, y, lr, rb, re, variant, cu)
        loss_and_check(eng, X, y, ranges[0][0], ranges[0][1], variant)


# ---- b. sentinel columns: exact range edges ------------------------------------------------------------------------
@VARIANTS
@pytest.mark.parametrize("rb,re", db.B_RANGES)
def test_range_edges_by_sentinel_columns(monkeypatch, variant, rb, re):
    """The last 64 columns are zero but for one 1.0 per chosen row, their weights are zero and lr = B makes lr / B
    exactly 1.0f: after one step w[s] is -r_i as the kernel computed it for an in-range sentinel row (first, last,
    either side of the 8- and 16-row block boundaries, first row of a workgroup's second block, the ragged tail) and
    exactly 0.0 for the rows just outside (row_begin - 1, row_end .. row_end + 15: opposite labels, 8x features)."""
    cu = n_cu()
    X, y, w0, lr, inside, outside = db.case_b(rb, re, variant, cu)
    with engine(monkeypatch, variant, db.B_D) as eng:
        eng.load(X, y)
        eng.set_weights(w0)
        bd = step_and_check(eng, X, y, lr, rb, re, variant, cu)
        w = eng.get_weights()
    for i, s in outside.items():
        assert w[s] == 0.0, ("row %d outside [%d, %d) reached the gradient" % (i, rb, re), w[s])
    assert rb in inside and re - 1 in inside
    for i, s in inside.items():
        assert abs(-float(w[s]) - bd.r[i - rb]) <= bd.dr[i - rb], (i, w[s], bd.r[i - rb], bd.dr[i - rb])
    # the unused sentinel columns stay zero
    used = set(inside.values()) | set(outside.values())
    assert all(w[s] == 0.0 for s in range(db.B_D - db.N_SENT, db.B_D) if s not in used)


# ---- c. link-function scan, bit level ------------------------------------------------------------------------------
def scan_values():
    mags = [1e-8, 1e-3, 0.5, 1.5, 8, 16.6, 17, 20, 30, 87, 88.7, 89, 103.9, 104.1, 110]
    z = [0.0, -0.0] + mags + [-m for m in mags] + list(np.linspace(-30.0, 30.0, 223))
    z = np.asarray(z, dtype=np.float32)          # the test's z IS the fp32 value
    zz = np.concatenate([z, z, [1.0]]).astype(np.float32)
    yy = np.concatenate([np.zeros(len(z)), np.ones(len(z)), [1.0]]).astype(np.float32)
    assert len(zz) == 511
    return zz, yy


@VARIANTS
def test_link_function_scan(monkeypatch, variant):
    """Row i has x[i, 0] = z_i and 1.0 in column i + 1; w = e_0 and lr = 511 = B.  z_i is then exact in fp32 (one
    non-zero product) and w[i + 1] after the step is -r_i exactly as the kernel computed it (every other row adds
    r * 0).  |r - r_ref| <= 4u: the argument of v_exp_f32 is z * log2e rounded, worth <= 1.5 |z| u relative in e and
    max p(1-p) |z| * 1.5u < 0.4u in p; then three operations of <= 1 ulp (<= u below 1): exp / 1 + e, reciprocal,
    subtraction.  Where the fp64 p rounds to 0 or 1 in fp32, r must be exactly -y or 1 - y (0 or -+1).  Per-row loss
    within 4u max(1, |z|): three roundings of values <= max(1, |z|) and a 1-ulp log1pf <= ln 2."""
    z, y = scan_values()
    n = len(z)
    X = np.zeros((n, 512), dtype=np.float32)
    X[:, 0] = z
    X[np.arange(n), np.arange(n) + 1] = 1.0
    w0 = np.zeros(512, dtype=np.float32)
    w0[0] = 1.0
    z64 = z.astype(np.float64)
    p = db.sigmoid(z64)
    r_ref = p - y
    loss_ref = np.maximum(z64, 0.0) + np.log1p(np.exp(-np.abs(z64))) - y * z64
    with engine(monkeypatch, variant, 512) as eng:
        eng.load(X, y)
        eng.set_weights(w0)
        per_row = [eng.loss(i, i + 1) for i in range(n)]
        eng.step(0, n, float(n))
        w = eng.get_weights()
    r = -w[1:].astype(np.float64)
    assert np.isfinite(w).all()
    err = np.abs(r - r_ref)
    k = int(np.argmax(err))
    print("link scan: max |r - r_ref| = %.3g u at z = %g, y = %g" % (err[k] / U, z[k], y[k]))
    assert (err <= 4 * U).all(), (z[k], y[k], r[k], r_ref[k], err[k] / U)
    p32 = p.astype(np.float32)
    sat = (p32 == 0.0) | (p32 == 1.0)
    assert sat.sum() >= 40      # |z| >= 20 with both labels, and the ends of the linspace
    np.testing.assert_array_equal(r[sat], p32[sat].astype(np.float64) - y[sat])
    loss = np.array([l for l, _ in per_row])
    lerr = np.abs(loss - loss_ref) / (4 * U * np.maximum(1.0, np.abs(z64)))
    k = int(np.argmax(lerr))
    print("link scan: max loss err = %.3g of the bound at z = %g, y = %g" % (lerr[k], z[k], y[k]))
    assert np.isfinite(loss).all() and (lerr <= 1.0).all(), (z[k], y[k], loss[k], loss_ref[k])
    tally = np.array([a for _, a in per_row])
    np.testing.assert_array_equal(tally, ((z > 0) == (y > 0.5)).astype(np.float64))   # z = +-0 predicts class 0


# ---- d. every width -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,D", [(v, D) for v in (0, 1) for D in db.D_WIDTHS[v]])
def test_every_width(monkeypatch, variant, D):
    """zpart[wave] is summed over D/512 (VALU) or D/256 (MFMA) waves: every count, not only powers of two.  Logits
    of sigma ~ 10, 37 rows from row 3, two steps, loss on a sub-range; the tally is exact on the rows with
    |z_ref| > dz[i] and at most 1 % of rows may be excluded."""
    cu = n_cu()
    X, y, w0, lr = db.case_d(D)
    with engine(monkeypatch, variant, D) as eng:
        eng.load(X, y)
        eng.set_weights(w0)
        for rb, re in db.D_RANGES:
            step_and_check(eng, X, y, lr, rb, re, variant, cu)
        bd = loss_and_check(eng, X, y, db.D_LOSS[0], db.D_LOSS[1], variant, family="dense_edges:tally_of_certain_rows")
        assert 5.0 < bd.z.std() < 20.0


# ---- e. entry points ------------------------------------------------------------------------------------------------
def small(n, D, seed):
    X, y, w = db._make(n, D, seed, 1.0)
    return X, y, w


@VARIANTS
def test_prof_counts_step_launches(monkeypatch, variant):
    X, y, w = small(64, 512, 1)
    with engine(monkeypatch, variant, 512) as eng:
        eng.load(X, y)
        assert eng.prof(True) == (0.0, 0)
        for k in range(5):
            eng.step(0, 64, 1.0)
        eng.loss(0, 64)                      # evaluation launches are not counted
        ms, n = eng.prof(False)
        assert n == 5 and ms > 0
        assert eng.prof(False) == (0.0, 0)
        eng.step(0, 64, 1.0)                 # profiling off: nothing recorded
        assert eng.prof(False) == (0.0, 0)


@VARIANTS
def test_prof_crosses_the_event_pool(monkeypatch, variant):
    """4,100 eight-row steps: the pool of 4,096 event pairs fills, is collected and re-used; none may be lost."""
    X, y, w = small(64, 512, 2)
    with engine(monkeypatch, variant, 512) as eng:
        eng.load(X, y)
        eng.prof(True)
        for k in range(4100):
            b = 8 * (k % 8)
            eng.step(b, b + 8, 0.01)
        ms, n = eng.prof(False)
        assert n == 4100 and ms > 0
        assert eng.prof(False) == (0.0, 0)
        assert np.isfinite(eng.get_weights()).all()


@VARIANTS
def test_reload_continues_like_a_fresh_engine(monkeypatch, variant):
    D = 1024
    Xs, ys, w = small(100, D, 3)
    Xl, yl, _ = small(300, D, 4)
    with engine(monkeypatch, variant, D) as eng, engine(monkeypatch, variant, D) as fresh:
        eng.generate(200, seed=5)
        eng.step(0, 200, 2.0)
        w1 = eng.get_weights()
        assert np.abs(w1).max() > 0
        eng.load(Xs, ys)                     # smaller
        np.testing.assert_array_equal(eng.get_weights(), w1)        # weights survive the reload
        with pytest.raises(IndexError):
            eng.step(0, 200, 2.0)            # the old range
        with pytest.raises(IndexError):
            eng.loss(100, 101)
        np.testing.assert_array_equal(eng.get_weights(), w1)
        fresh.load(Xs, ys)
        fresh.set_weights(w1)
        for e in (eng, fresh):
            e.step(0, 100, 2.0)
            e.step(7, 93, 2.0)
        np.testing.assert_array_equal(eng.get_weights(), fresh.get_weights())
        assert eng.loss(0, 100) == fresh.loss(0, 100)
        w2 = eng.get_weights()
        eng.load(Xl, yl)                     # larger
        np.testing.assert_array_equal(eng.get_weights(), w2)
        with pytest.raises(IndexError):
            eng.step(0, 301, 2.0)
        fresh.load(Xl, yl)
        for e in (eng, fresh):
            e.step(100, 300, 2.0)            # rows the smaller shard never had
            e.step(0, 300, 2.0)
        np.testing.assert_array_equal(eng.get_weights(), fresh.get_weights())
        assert eng.loss(0, 300) == fresh.loss(0, 300)
        assert not np.array_equal(eng.get_weights(), w2)


def test_refusals_change_nothing(monkeypatch):
    monkeypatch.setenv("DSGD_DENSE_MFMA", "1")
    with pytest.raises(dsgd_amd.DsgdError) as ei:
        dsgd_amd.DenseLogistic(4608)         # one wave per 256 columns: at most 4096 on the matrix cores
    assert ei.value.code == -7 and "4096" in str(ei.value)   # DSGD_EUNSUPPORTED
    with dsgd_amd.DenseLogistic(4096):
        pass
    monkeypatch.setenv("DSGD_DENSE_MFMA", "0")
    with dsgd_amd.DenseLogistic(4608):
        pass
    for variant in (0, 1):
        monkeypatch.setenv("DSGD_DENSE_MFMA", str(variant))
        for D in (0, 256, 8704):
            with pytest.raises(ValueError):
                dsgd_amd.DenseLogistic(D)
        X, y, w = small(40, 512, 6)
        with dsgd_amd.DenseLogistic(512) as eng:
            eng.load(X, y)
            eng.set_weights(w)
            eng.step(0, 40, 1.0)
            w1 = eng.get_weights()
            before = eng.loss(0, 40)
            bad = y.copy()
            bad[17] = 0.5
            with pytest.raises(ValueError, match="17"):
                eng.load(X, bad)             # refused before anything is released
            for rb, re in ((5, 5), (9, 3)):
                with pytest.raises(ValueError):
                    eng.loss(rb, re)
            for rb, re in ((-1, 4), (0, 41), (40, 41), (100, 200)):
                with pytest.raises(IndexError):
                    eng.loss(rb, re)
                with pytest.raises(IndexError):
                    eng.step(rb, re, 1.0)
            np.testing.assert_array_equal(eng.get_weights(), w1)
            assert eng.loss(0, 40) == before     # data and weights as they were


@VARIANTS
def test_generator_is_counter_based(monkeypatch, variant):
    """A row's content depends on (seed, row, column) alone: not on n_rows, hence not on the generating grid
    (min(n_rows, 8 n_cu) workgroups: 1,000 against 2,048 on 256 CUs).  Seeds differ in x and label noise and share
    the planted separator."""
    D = 1024
    w = np.random.default_rng(8).normal(size=D).astype(np.float32)
    with engine(monkeypatch, variant, D) as eng:
        eng.set_weights(w)
        eng.generate(1000, seed=0)
        a = eng.loss(0, 1000)
        part = [eng.loss(b, b + 100) for b in range(0, 1000, 100)]
        eng.generate(5000, seed=0)
        assert eng.loss(0, 1000) == a
        assert [eng.loss(b, b + 100) for b in range(0, 1000, 100)] == part
        tail = eng.loss(1000, 2000)
        assert tail != a                     # other rows, other content
        eng.generate(1000, seed=1)
        assert eng.loss(0, 1000) != a
        # train on seed 0, evaluate on a seed-1 shard: the same separator
        eng.set_weights(np.zeros(D, dtype=np.float32))
        eng.generate(16384, seed=0)
        for ep in range(3):
            for b in range(0, 16384, 2048):
                eng.step(b, b + 2048, 8.0)
        eng.generate(4096, seed=1)
        l1, a1 = eng.loss(0, 4096)
        assert l1 < np.log(2.0) - 0.005 and a1 > 0.7, (l1, a1)
