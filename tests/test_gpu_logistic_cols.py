"""The logistic model's whole-split steps by column lists on the GPU (include/dsgd.h "WHOLE-SPLIT STEPS BY COLUMN LISTS", DESIGN.md
3.13): Engine.lg_sync_steps_ranges against a SECOND context on the same data and start weights stepped by the unchanged
lg_sync_step_ranges.  Both forms add the same 64-bit integers, so every comparison is of bits, never within a tolerance.

Not reached here: the decline to the row form (2^31 entries or positions, no memory) cannot be produced at test size on the GPU
and no knob or compiled-in seam forces it.  The decision itself is checked on the CPU (tests/cpp/lg_cols_host_test.cpp: 2^31 - 1
is laid out, 2^31 is declined), and what a declined call runs is lg_launch, the existing row form that every test here uses as
its yardstick."""

import ctypes as C

import numpy as np
import pytest

import dsgd_amd
import logistic_cases as cases
from dsgd_amd import _lib

pytestmark = pytest.mark.gpu

COLS, ROWS = "dsgd_lg_cgrad_kernel", "dsgd_lg_grad_range_kernel"
LR = 2.0 ** -6   # (a worker's gradient is a SUM over its rows)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f64bits(x):
    return np.float64(x).view(np.uint64)


def engine_of(csr, dim, lam):
    eng = dsgd_amd.Engine(dim, lam)
    eng.load_csr(*csr)
    return eng


def step_both(cols, rows, ranges, n_steps, lr, w=None):
    """the new call on `cols`, the loop of single steps on `rows`, from w (None: from what each holds); asserts equal stats and
    weight bits and returns the weights"""
    if w is not None:
        cols.set_weights(w)
        rows.set_weights(w)
    st = cols.lg_sync_steps_ranges(ranges, n_steps, lr)
    assert cols.grad_kernel_name() == COLS
    for _ in range(n_steps):
        st_rows = rows.lg_sync_step_ranges(ranges, lr)
    assert rows.grad_kernel_name() == ROWS
    n = sum(b - a for a, b in ranges)
    assert st == st_rows == {"n_samples": n, "n_active": n}
    w_cols, w_rows = cols.get_weights(), rows.get_weights()
    diff = int(np.count_nonzero(bits(w_cols) != bits(w_rows)))
    print("%d ranges, %d rows, %d steps: %d of %d weights differ" % (len(ranges), n, n_steps, diff, w_cols.size))
    assert diff == 0
    return w_cols


def same_loss(cols, rows, a, b):
    """lg_loss_acc from the |w'|^2 words the last finish left, on both sides"""
    got, want = cols.lg_loss_acc(a, b), rows.lg_loss_acc(a, b)
    assert f64bits(got[0]) == f64bits(want[0]) and got[1] == want[1], (got, want)


@pytest.fixture(scope="module")
def pair():
    d = cases.data()
    with engine_of(cases.csr(d), d.dim, cases.LAM) as cols, engine_of(cases.csr(d), d.dim, cases.LAM) as rows:
        yield cols, rows


RANGE_SETS = {
    "whole": [(0, 4096)],                                   # the hot columns span several shares: the cut-column atomics run
    "uneven": [(0, 700), (700, 764), (764, 765)],           # uneven workers, a one-row worker
    "one_row": [(77, 78)],
    "k16": [(256 * i, 256 * (i + 1)) for i in range(16)],
    "overlap": [(0, 3000), (1000, 4096)],                   # lg_check_ranges accepts overlapping workers: each sums its own rows
}


@pytest.mark.parametrize("n_steps", [1, 5])
@pytest.mark.parametrize("name", list(RANGE_SETS))
def test_steps_are_bit_equal_to_the_row_form(pair, name, n_steps):
    cols, rows = pair
    if name == "whole":   # the premise: the hottest column alone holds more entries than the largest share, so shares begin inside it
        assert np.bincount(cases.data().col).max() > 2048
    step_both(cols, rows, RANGE_SETS[name], n_steps, LR, cases.weights(1.0))
    same_loss(cols, rows, 0, cases.N)


def share_of(n_ent, n_cu):
    """csrc/dsgd_lg_cols_host.hpp: lgc_share"""
    s = -(-n_ent // (n_cu * 8))
    return min(2048, max(256, -(-s // 256) * 256))


def test_every_round_count_of_a_share():
    """The 4,096-row sets stay at the smallest share (256 entries: ONE round of 64 per wave).  At the MI355X's 256 compute
    units a wave walks 2 rounds from 524,289 entries on and 8 from 3,670,017 on, so 50,000 rows it is: 12,000 of them as one
    range (2 rounds), 17,000, 24,000, 31,000 and 38,000 (3, 4, 5 and 6: the loop is unrolled to LGC_NU = 8 with `u < rounds`
    guards, every count between takes its own way through them), two uneven workers (7) and the whole set (8, the largest
    share)."""
    import hard_data as hd

    d = dsgd_amd.synth.generate(50000, seed=5)
    csr = (d.row_ptr, d.col, d.val, d.label)
    cases_ = ([(0, 12000)], [(0, 17000)], [(0, 24000)], [(0, 31000)], [(0, 38000)], [(0, 20000), (20000, 45000)], [(0, 50000)])
    assert [share_of(sum(int(d.row_ptr[b] - d.row_ptr[a]) for a, b in r), hd.N_CU) // 256 for r in cases_] == [2, 3, 4, 5, 6, 7, 8]
    with engine_of(csr, d.dim, cases.LAM) as cols, engine_of(csr, d.dim, cases.LAM) as rows:
        for ranges in cases_:
            step_both(cols, rows, ranges, 2, 2.0 ** -10, cases.weights(1.0))
            same_loss(cols, rows, 0, 50000)


@pytest.mark.parametrize("split", ["one", "three"])
def test_row_shapes_and_saturation(split):
    """the hand-built CSR of tests/test_gpu_logistic.py: an empty row, 1, 64, 65 and 2,100 non-zeros, and the SAT_W rows whose
    coefficients are -+0 (q = 0) and -y"""
    import test_gpu_logistic as tgl

    csr, w, n_shape, sat0 = tgl._hand()
    n = len(csr[3])
    ranges = [(0, n)] if split == "one" else [(0, 5), (5, n_shape), (n_shape, n)]
    with engine_of(csr, tgl.HD, 0.0) as cols, engine_of(csr, tgl.HD, 0.0) as rows:
        w1 = step_both(cols, rows, ranges, 1, 0.25, w)
        assert np.isfinite(w1).all() and not np.array_equal(bits(w1), bits(w))
        same_loss(cols, rows, 0, n)
        step_both(cols, rows, ranges, 3, 0.25)
        same_loss(cols, rows, 0, n)
        step_both(cols, rows, [(0, 1)], 2, 0.25)   # the empty row alone: one padding entry, q = 0
        same_loss(cols, rows, 0, n)


def test_hostile_feature_values():
    """the generators of tests/test_gpu_hard_values.py: scaled, signed, wide, zero-margin and ragged rows, one range of 2,048 rows"""
    import test_gpu_hard_values as thv

    for trait in thv.ORACLE_TRAITS:
        h = thv.hd.build(trait)
        d = h.data
        csr = (d.row_ptr, d.col, d.val, d.label)
        assert d.n_rows >= 2048
        with engine_of(csr, d.dim, thv.LAM) as cols, engine_of(csr, d.dim, thv.LAM) as rows:
            step_both(cols, rows, [(0, 2048)], 2, 2.0 ** -8, h.w.astype(np.float32))
            same_loss(cols, rows, 0, 2048)


def test_the_accumulators_are_left_clean(pair):
    cols, rows = pair
    lists, lr = cases.step_cases()["3 workers 100/37/1"]
    idx = cases.gradient_lists()["100 (row thrice)"]
    step_both(cols, rows, RANGE_SETS["whole"], 2, LR, cases.weights(1.0))
    out = []
    for eng in (cols, rows):   # a list step and a gradient behind it: both read every accumulator word
        st = eng.lg_sync_step(lists, lr)
        g, gst = eng.lg_gradient(idx)
        out.append((st, eng.get_weights(), g, gst))
    assert out[0][0] == out[1][0] and out[0][3] == out[1][3]
    assert np.array_equal(bits(out[0][1]), bits(out[1][1])) and np.array_equal(bits(out[0][2]), bits(out[1][2]))
    step_both(cols, rows, RANGE_SETS["uneven"], 1, LR)   # ... and the column lists again behind the row kernels
    same_loss(cols, rows, 0, cases.N)


def test_the_cache_keeps_evicts_and_follows_a_reload():
    d = cases.data()
    w = cases.weights(1.0)
    with engine_of(cases.csr(d), d.dim, cases.LAM) as cols, engine_of(cases.csr(d), d.dim, cases.LAM) as rows:
        first = [(0, 1000), (1000, 2000)]
        w1 = step_both(cols, rows, first, 1, LR, w)
        w2 = step_both(cols, rows, first, 1, LR, w)        # the cached layout: the same bits
        assert np.array_equal(bits(w1), bits(w2))
        for i in range(1, 10):                              # nine other configurations: the first one has made room by now
            step_both(cols, rows, [(i, 500 + 7 * i), (600, 1200 + i)], 1, LR, w)
        w3 = step_both(cols, rows, first, 2, LR, w)         # laid out again
        assert not np.array_equal(bits(w3), bits(w1))
        # other rows under the same ranges: the layout of the old ones must not serve
        d2 = dsgd_amd.synth.generate(3000, seed=12)
        csr2 = (d2.row_ptr, d2.col, d2.val, d2.label)
        assert not np.array_equal(d2.col[:1000], d.col[:1000])
        cols.load_csr(*csr2)
        rows.load_csr(*csr2)
        w4 = step_both(cols, rows, first, 1, LR, w)
        assert not np.array_equal(bits(w4), bits(w1))
        same_loss(cols, rows, 0, 3000)
        with engine_of(csr2, d2.dim, cases.LAM) as fresh:   # ... and it is what a context that never saw the old rows gives
            fresh.set_weights(w)
            fresh.lg_sync_steps_ranges(first, 1, LR)
            assert np.array_equal(bits(fresh.get_weights()), bits(w4))


def test_refusals_leave_the_context_alone(pair):
    cols, rows = pair
    w = cases.weights(1.0)
    cols.set_weights(w)
    lib, ctx = cols._lib, cols._ctx
    z = C.c_int64

    def both(rb, re_, k, n_steps=1):
        """the codes of the new call and of the single step on the same arguments"""
        a, b = (z * len(rb))(*rb), (z * len(re_))(*re_)
        return lib.dsgd_lg_sync_steps_ranges(ctx, a, b, k, z(n_steps), 0.5, None), lib.dsgd_lg_sync_step_ranges(ctx, a, b, k, 0.5, None)

    assert lib.dsgd_lg_sync_steps_ranges(ctx, (z * 1)(0), (z * 1)(10), 1, z(0), 0.5, None) == _lib.EINVAL      # no steps
    assert np.array_equal(bits(cols.get_weights()), bits(w))
    assert lib.dsgd_lg_sync_steps_ranges(ctx, (z * 1)(0), (z * 1)(10), 1, z(-1), 0.5, None) == _lib.EINVAL
    assert np.array_equal(bits(cols.get_weights()), bits(w))
    for args, code in ((([5], [5], 1), _lib.EINVAL),                  # an empty range
                       (([9], [3], 1), _lib.EINVAL),                  # a reversed one
                       (([0, 7], [5, 7], 2), _lib.EINVAL),            # an empty worker among two
                       (([0], [5], 0), _lib.EINVAL),                  # no workers
                       (([0], [cases.N + 1], 1), _lib.ERANGE),        # beyond the data
                       (([-1], [5], 1), _lib.ERANGE)):
        assert both(*args) == (code, code), (args, lib.dsgd_last_error())
        assert np.array_equal(bits(cols.get_weights()), bits(w)), args
    # the context is as it was: the next call is the one a context without the refusals makes
    step_both(cols, rows, RANGE_SETS["uneven"], 1, LR, w)
    same_loss(cols, rows, 0, cases.N)


def test_refused_states():
    d = cases.data()
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:                      # no data loaded
        for f in (lambda: eng.lg_sync_steps_ranges([(0, 5)], 1, 0.5), lambda: eng.lg_sync_step_ranges([(0, 5)], 0.5)):
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                f()
            assert ei.value.code == _lib.ESTATE
    with dsgd_amd.Engine(d.dim, cases.LAM, precision="fp64") as eng:    # an fp64 context
        eng.load_csr(*cases.csr(d))
        w = eng.get_weights()
        for f in (lambda: eng.lg_sync_steps_ranges([(0, 5)], 1, 0.5), lambda: eng.lg_sync_step_ranges([(0, 5)], 0.5)):
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                f()
            assert ei.value.code == _lib.EUNSUPPORTED
        assert np.array_equal(eng.get_weights(), w)
    with engine_of(cases.csr(d), d.dim, cases.LAM) as eng:              # the lock-free engine running
        eng.set_weights(cases.weights(1.0))
        eng.build_dim_sparsity(cases.N)
        eng.async_start([(0, cases.N)], batch=100, lr=0.5, max_updates=4_000_000, seed=1, positional_bug=True)
        try:
            for f in (lambda: eng.lg_sync_steps_ranges([(0, 5)], 1, 0.5), lambda: eng.lg_sync_step_ranges([(0, 5)], 0.5)):
                with pytest.raises(dsgd_amd.DsgdError) as ei:
                    f()
                assert ei.value.code == _lib.ESTATE
        finally:
            eng.async_stop()
        assert eng.lg_sync_steps_ranges([(0, 10)], 2, 0.5) == {"n_samples": 10, "n_active": 10}   # usable afterwards
        assert eng.grad_kernel_name() == COLS
