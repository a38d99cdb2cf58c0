"""-m gpu: the fp64 mode on Double feature values (dsgd_load_csr_f64; csrc/dsgd_rp64.hpp) against the Double oracle
oracle/ref_dict.py (Python floats; oracle/oracle.py holds float32 values).

Shapes: D = 3,000 (ranks on both sides of the 1,024 hot ranks kept in LDS), about 2,000 rows of 0 - 40 entries (shorter
and longer than the 16 lanes of a row), one row of 700 entries, empty and one-entry rows, values m * 2^e with full 53-bit
mantissas of both signs.

Bounds: the column sums are exact integers on the device (two 64-bit words per column), so inside the stated exact range
(e >= vexp - (42 - ceil(log2 n)); the data spans 8 binades) a gradient differs from ref_dict's only by the rounding order
of x . w and w . ds and by ref_dict's per-add rounding: max|dw| <= 1e-12 * max(1, |w|_inf), the bound of
tests/test_gpu_fp64_requests.py, with equal supports and active counts.  With lambda = 0 a coordinate is the correctly
rounded exact sum: bit for bit math.fsum.

The communicator of the refusal test is real RCCL with one rank, as tests/test_gpu_fp64_world2.py attaches it."""

import ctypes as C
import math
import os

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from oracle import ref_dict as rd
from oracle import ref_loader
from oracle.backend import OracleBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

D = 3000
DP = D + 1
N_ROWS = 2000
N_TRAIN = 1600
LAM = 1e-5
NEVER = lambda losses: False
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = [(2901 + 2 * i, 2902 + 2 * i) for i in range(6)]   # (a, b): x = {a: 1 + 2^-30, b: 1}, y = -1


def _make(float_values=False):
    """-> row_ptr, col, val (float64), label; the first 2 * len(PLANTED) rows after row 9 are planted."""
    rng = np.random.default_rng(5)
    p = 1.0 / (np.arange(1, 2901) + 10.0)
    p /= p.sum()
    rows = []
    for i in range(N_ROWS):
        n = 700 if i == 3 else (0 if i % 97 == 5 else (1 if i % 89 == 7 else int(rng.integers(0, 41))))
        cols = np.sort(rng.choice(np.arange(1, 2901), size=n, replace=False, p=p))
        vals = rng.standard_normal(n) * np.exp2(rng.integers(-7, 1, size=n))   # full mantissas, both signs, 8 binades
        rows.append((cols, vals, 1 if rng.random() < 0.5 else -1))
    for t, (a, b) in enumerate(PLANTED):   # decisive rows: inactive in Double, active once x is rounded to float
        rows[10 + t] = (np.asarray([a, b]), np.asarray([1.0 + 2.0 ** -30, 1.0]), -1)
    row_ptr = np.zeros(N_ROWS + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(r[0]) for r in rows])
    col = np.concatenate([r[0] for r in rows]).astype(np.int32)
    val = np.concatenate([r[1] for r in rows]).astype(np.float64)
    if float_values:
        val = val.astype(np.float32).astype(np.float64)
    label = np.asarray([r[2] for r in rows], np.int8)
    return row_ptr, col, val, label


_CACHE = {}


def _csr(float_values=False):
    if float_values not in _CACHE:
        _CACHE[float_values] = _make(float_values)
    return _CACHE[float_values]


def _ref_data(row_ptr, col, val, label, size=DP):
    return [(rd.Sparse({int(c): float(v) for c, v in zip(col[row_ptr[i]:row_ptr[i + 1]], val[row_ptr[i]:row_ptr[i + 1]])}, size),
             int(label[i])) for i in range(len(label))]


def _ref(float_values=False, n_train=N_TRAIN, lam=LAM):
    key = ("ref", float_values, n_train, lam)
    if key not in _CACHE:
        data = _ref_data(*_csr(float_values))
        _CACHE[key] = (data, rd.SparseSVM(lam, rd.dim_sparsity(data[:n_train])))
    return _CACHE[key]


def _dense(sp, dp=DP):
    out = np.zeros(dp)
    for k, v in sp.map.items():
        out[k] = v
    return out


def _sparse(w):
    return rd.Sparse({int(k): float(w[k]) for k in np.flatnonzero(w)}, len(w))


def _engine(csr, lam=LAM, n_train=N_TRAIN, as_float=False, dim=D):
    row_ptr, col, val, label = csr
    eng = dsgd_amd.Engine(dim, lam, precision="fp64")
    eng.load_csr(row_ptr, col, val.astype(np.float32) if as_float else val, label)
    eng.build_dim_sparsity(n_train)
    return eng


def _scale(v):
    return max(1.0, float(np.abs(v).max()))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _active(model, data, w, idx):
    return sum(1 for i in idx if not (data[i][1] * data[i][0].dot(w) < 0))


def _decisive_w():
    rng = np.random.default_rng(3)
    w = np.zeros(DP)
    ks = rng.choice(np.arange(1, 2901), 800, replace=False)
    w[ks] = rng.normal(scale=0.1, size=800)
    for a, b in PLANTED:
        w[a], w[b] = 1.0, -1.0
    return w


def _tallies(preds, labels):
    c = [0, 0, 0]
    for p_, y in zip(preds, labels):
        c[0 if p_ == y else (1 if p_ == 0 else 2)] += 1
    return c


def test_decisive_rows_follow_the_doubles():
    """1: rows whose gate the float rounding of x flips -- Double data decides them as ref_dict does, float data does not"""
    csr = _csr()
    data, model = _ref()
    w = _decisive_w()
    ws = _sparse(w)
    idx = np.arange(0, 400, dtype=np.int32)
    g_ref = _dense(rd.slave_gradient(model, data, ws, idx.tolist()))
    pred_ref = rd.slave_forward(model, data, ws, idx.tolist())
    act_ref = _active(model, data, ws, idx.tolist())
    planted = list(range(10, 10 + len(PLANTED)))
    with _engine(csr) as eng:
        assert eng.value_bits() == 64
        eng.set_weights(w)
        g, st = eng.gradient_f64(idx)
        pred = eng.forward_f64(idx)
        _, _, counts = eng.loss_acc(0, 400)
    assert st["n_active"] == act_ref
    assert np.array_equal(np.flatnonzero(g), np.flatnonzero(g_ref))
    assert np.abs(g - g_ref).max() <= 1e-12 * _scale(g_ref)
    assert np.array_equal(pred, np.asarray(pred_ref, np.float64))
    assert counts == _tallies(pred_ref, csr[3][:400])
    assert all(pred[r] == -1.0 for r in planted)   # x . w = 2^-30 > 0
    # the negative control: the same rows as floats differ on exactly the planted rows
    with _engine(csr, as_float=True) as eng32:
        assert eng32.value_bits() == 32
        eng32.set_weights(w)
        g32, st32 = eng32.gradient_f64(idx)
        pred32 = eng32.forward_f64(idx)
    assert st32["n_active"] == act_ref + len(PLANTED)
    assert np.flatnonzero(pred32 != pred).tolist() == planted and all(pred32[r] == 0.0 for r in planted)
    for a, b in PLANTED:   # active there: y * x = -x lands on both columns
        assert abs((g32[a] - g[a]) + 1.0) < 1e-3 and abs((g32[b] - g[b]) + 1.0) < 1e-3   # (-x, and s where the support grew)


def _fsum_gradient(csr, idx, dp=DP):
    row_ptr, col, val, label = csr
    per = {}
    for r in idx:
        for p in range(row_ptr[r], row_ptr[r + 1]):
            if abs(val[p]) > 1e-20:
                per.setdefault(int(col[p]), []).append(float(val[p]) * float(label[r]))
    want = np.zeros(dp)
    for c_, part in per.items():
        s = math.fsum(part)
        want[c_] = s if abs(s) > 1e-20 else 0.0
    return want


def test_exact_sums_bit_for_bit_and_order_free():
    """2: lambda = 0, w = 0 (every row active): each coordinate is the correctly rounded exact sum, whatever the order"""
    csr = _csr()
    perm = np.random.default_rng(11).permutation(N_ROWS).astype(np.int32)
    with _engine(csr, lam=0.0) as eng:
        eng.set_weights(np.zeros(DP))
        for n in (1, 2, 64, 65, 1024, 1025, 2000):   # both sides of the shift's steps
            idx = perm[:n]
            g, st = eng.gradient_f64(idx)
            assert st["n_active"] == n
            assert np.array_equal(_bits(g), _bits(_fsum_gradient(csr, idx.tolist()))), n
        idx = perm[:1025]
        g, _ = eng.gradient_f64(idx)
        for other in (idx[::-1], np.random.default_rng(2).permutation(idx)):
            g2, _ = eng.gradient_f64(np.ascontiguousarray(other))
            assert np.array_equal(_bits(g), _bits(g2))
        dup = np.concatenate([idx[:300], idx[:300]])
        gd, _ = eng.gradient_f64(dup)
        gd2, _ = eng.gradient_f64(np.ascontiguousarray(np.repeat(idx[:300], 2)))
        assert np.array_equal(_bits(gd), _bits(gd2))
        assert np.array_equal(_bits(gd), _bits(_fsum_gradient(csr, dup.tolist())))


def test_a_cancelled_column_stays_off_the_support():
    """2: full-mantissa pairs +v (y = +1) and +v (y = -1) on one column: the low words alone sum past 2^32, the total is
    exactly 0 -- no support, no regulariser -- while the other columns get s"""
    rng = np.random.default_rng(8)
    vals = (1.0 + rng.random(8)) * 2.0 ** -14   # 52-bit mantissas 14 binades under the data's largest: 12 bits below the high word's unit
    rows, labels = [], []
    for v in vals:   # one-entry rows on column 7, in cancelling pairs
        rows += [([7], [v]), ([7], [v])]
        labels += [1, -1]
    for i in range(40):
        cols = np.sort(rng.choice(np.arange(8, 200), size=12, replace=False))
        rows.append((cols.tolist(), rng.standard_normal(12).tolist()))
        labels.append(1 if i % 2 else -1)
    row_ptr = np.zeros(len(rows) + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(r[0]) for r in rows])
    col = np.concatenate([r[0] for r in rows]).astype(np.int32)
    val = np.concatenate([r[1] for r in rows]).astype(np.float64)
    csr = (row_ptr, col, val, np.asarray(labels, np.int8))
    # what the kernel adds for the planted entries: v = +-x * 2^(S - vexp); every fraction is non-zero, so both words are
    # used, and a pair's low words sum to exactly 2^32 (f and 1 - f): 8 pairs put 8 * 2^32 into LO against -8 in HI
    vexp = math.frexp(float(np.abs(val).max()))[1]
    shift = 62 - math.ceil(math.log2(len(rows)))
    scaled = [float(v) * 2.0 ** (shift - vexp) for v in vals]
    assert all(x != math.floor(x) for x in scaled)
    lo_sum = sum(round((x - math.floor(x)) * 2.0 ** 32) + round((-x - math.floor(-x)) * 2.0 ** 32) for x in scaled)
    assert lo_sum == 8 * 2 ** 32 and sum(math.floor(x) + math.floor(-x) for x in scaled) == -8
    data = _ref_data(*csr, size=301)
    model = rd.SparseSVM(1e-3, rd.dim_sparsity(data))
    w = np.zeros(301)
    w[8:200] = rng.normal(scale=1e-3, size=192)   # (small: most rows stay active; column 7 has no weight: d = 0, active)
    idx = np.arange(len(rows), dtype=np.int32)
    g_ref = _dense(rd.slave_gradient(model, data, _sparse(w), idx.tolist()), 301)
    with _engine(csr, lam=1e-3, n_train=len(rows), dim=300) as eng:
        eng.set_weights(w)
        g, st = eng.gradient_f64(idx)
    s = 1e-3 * 2.0 * _sparse(w).dot(model.dim_sparsity)
    assert abs(s) > 1e-20 and g[7] == 0.0 and g_ref[7] == 0.0
    assert np.array_equal(np.flatnonzero(g), np.flatnonzero(g_ref))
    assert np.abs(g - g_ref).max() <= 1e-12 * _scale(g_ref)


@pytest.mark.parametrize("below", [0, 1])
def test_the_last_exact_binade(below):
    """2: n = 4 rows, vexp = 1 (|x| <= 2): entries of exponent e = vexp - (42 - 2) = -39 with all 53 bits are exact; one
    binade below the error is within one grid unit 2^(vexp - 60 - 32) per entry"""
    e = -39 - below
    rng = np.random.default_rng(4 + below)
    m = 1.0 + rng.integers(0, 2 ** 52, size=4).astype(np.float64) * 2.0 ** -52
    m[0] = 1.0 + 2.0 ** -52   # (the last bit set)
    small = m * 2.0 ** e * np.asarray([1, -1, 1, 1])
    row_ptr = np.asarray([0, 2, 3, 4, 5], np.int64)
    col = np.asarray([1, 2, 2, 2, 2], np.int32)
    val = np.asarray([1.5, small[0], small[1], small[2], small[3]])
    label = np.asarray([1, 1, -1, 1], np.int8)
    csr = (row_ptr, col, val, label)
    with _engine(csr, lam=0.0, n_train=4, dim=4) as eng:
        eng.set_weights(np.zeros(5))
        g, _ = eng.gradient_f64(np.arange(4, dtype=np.int32))
    want = _fsum_gradient(csr, range(4), 5)
    assert g[1] == 1.5
    if not below:
        assert np.array_equal(_bits(g), _bits(want))
    else:
        assert abs(g[2] - want[2]) <= 4 * 2.0 ** (1 - 60 - 32)


def test_float_representable_values_give_the_float_calls_bits():
    """3: values a float holds, loaded as doubles on one engine and as floats on its twin: bit-identical throughout"""
    csr = _csr(float_values=True)
    rng = np.random.default_rng(21)
    w = _decisive_w()
    with _engine(csr) as a, _engine(csr, as_float=True) as b:
        assert (a.value_bits(), b.value_bits()) == (64, 32)
        assert np.array_equal(_bits(a.get_dim_sparsity()), _bits(b.get_dim_sparsity()))
        idx = rng.integers(0, N_TRAIN, size=777).astype(np.int32)
        for e in (a, b):
            e.set_weights(w)
        ga, sa = a.gradient_f64(idx)
        gb, sb = b.gradient_f64(idx)
        assert sa == sb and np.array_equal(_bits(ga), _bits(gb))
        for k, n in ((3, 100), (6, 100), (3, N_TRAIN)):
            split = host.split_vanilla(N_TRAIN, k)
            for e in (a, b):
                e.set_weights(np.zeros(DP))
            for _ in range(20):
                lists = [rng.permutation(np.asarray(r))[:n].astype(np.int32) for r in split]
                assert a.sync_step_f64(lists, 0.5) == b.sync_step_f64(lists, 0.5)
            assert np.array_equal(_bits(a.get_weights()), _bits(b.get_weights())), (k, n)
        for _ in range(5):
            idx = rng.integers(0, N_TRAIN, size=100).astype(np.int32)
            da, sa = a.async_step(idx, 0.3, want_delta=True)
            db, sb = b.async_step(idx, 0.3, want_delta=True)
            assert sa == sb and np.array_equal(_bits(da), _bits(db))
        assert np.array_equal(_bits(a.get_weights()), _bits(b.get_weights()))
        all_rows = np.arange(N_ROWS, dtype=np.int32)
        assert np.array_equal(a.forward_f64(all_rows), b.forward_f64(all_rows))
        assert a.loss_acc(N_TRAIN, N_ROWS) == b.loss_acc(N_TRAIN, N_ROWS)


def test_double_data_on_slice_major_weights_gives_the_float_calls_bits():
    """3: Double data can meet slice-major weights: a plan made on float data outlives load_csr with doubles (plans are
    refused only at their creation there) and its run leaves the weights in the column slices' layout.  The row-parallel
    calls behind it read and update that layout; on values a float holds they give the float-data twin's bits"""
    csr = _csr(float_values=True)
    row_ptr, col, val, label = csr
    rng = np.random.default_rng(71)
    split = host.split_vanilla(N_TRAIN, 3)
    steps = [[rng.permutation(np.asarray(r))[:100].astype(np.int32) for r in split] for _ in range(2)]
    idx = rng.integers(0, N_TRAIN, size=777).astype(np.int32)
    lists = [rng.permutation(np.asarray(r))[:150].astype(np.int32) for r in split]
    w0 = _decisive_w()
    with _engine(csr, as_float=True) as a, _engine(csr, as_float=True) as b:
        pa, pb = a.plan(steps), b.plan(steps)
        a.load_csr(row_ptr, col, val, label)   # the doubles; the plan stays
        a.build_dim_sparsity(N_TRAIN)
        assert (a.value_bits(), b.value_bits()) == (64, 32)
        for e, p in ((a, pa), (b, pb)):
            e.set_weights(w0)
            e.plan_run(p, 0, 2, 0.5)   # (reads the values as floats on both: the same steps)
            e.synchronize()
        ga, sa = a.gradient_f64(idx)   # w = NULL right after a plan run: the slice-major weights
        gb, sb = b.gradient_f64(idx)
        assert sa == sb and np.array_equal(_bits(ga), _bits(gb))
        assert a.sync_step_f64(lists, 0.5) == b.sync_step_f64(lists, 0.5)
        da, sa = a.async_step(idx[:100], 0.3, want_delta=True)
        db, sb = b.async_step(idx[:100], 0.3, want_delta=True)
        assert sa == sb and np.array_equal(_bits(da), _bits(db))
        wa, wb = a.get_weights(), b.get_weights()
        assert np.array_equal(_bits(wa), _bits(wb)) and not np.array_equal(_bits(wa), _bits(w0))
        pa.destroy()
        pb.destroy()


@pytest.mark.parametrize("k,n", [(3, 100), (5, 37)])
def test_sync_steps_against_ref_dict(k, n):
    """4: 20 steps of sync_step_f64 on the doubles against ref_dict.master_sync_step"""
    data, model = _ref()
    rng = np.random.default_rng(31 + k)
    split = host.split_vanilla(N_TRAIN, k)
    w_ref = rd.Sparse({}, DP)
    with _engine(_csr()) as eng:
        assert np.array_equal(_bits(eng.get_dim_sparsity()), _bits(_dense(model.dim_sparsity)))
        eng.set_weights(np.zeros(DP))
        for step in range(20):
            lists = [rng.permutation(np.asarray(r))[:n].astype(np.int32) for r in split]
            act = sum(_active(model, data, w_ref, l.tolist()) for l in lists)
            w_ref = rd.master_sync_step(model, data, w_ref, [l.tolist() for l in lists], 0.5)
            st = eng.sync_step_f64(lists, 0.5)
            w = eng.get_weights()
            wr = _dense(w_ref)
            assert st["n_active"] == act and st["n_samples"] == k * n
            assert np.array_equal(np.flatnonzero(w), np.flatnonzero(wr)), step
            assert np.abs(w - wr).max() <= 1e-12 * _scale(wr), step


def test_async_steps_against_ref_dict():
    """4: 20 async_step_f64 iterations with their deltas, dense and sparse, against ref_dict.async_step"""
    data, model = _ref()
    rng = np.random.default_rng(41)
    w_ref = rd.Sparse({}, DP)
    with _engine(_csr()) as eng:
        eng.set_weights(np.zeros(DP))
        for it in range(20):
            idx = rng.integers(0, N_TRAIN, size=100 if it % 3 else 33).astype(np.int32)
            act = _active(model, data, w_ref, idx.tolist())
            w_ref, upd = rd.async_step(model, data, w_ref, idx.tolist(), 0.3)
            if it % 2:
                keys, vals, st = eng.async_step_sparse(idx, 0.3)
                delta = np.zeros(DP)
                delta[keys] = vals
                assert np.all(np.diff(keys) > 0) and np.all(np.abs(vals) > 1e-20)
            else:
                delta, st = eng.async_step(idx, 0.3, want_delta=True)
            w, wr, dr = eng.get_weights(), _dense(w_ref), _dense(upd)
            assert st["n_active"] == act and st["n_samples"] == len(idx)
            assert np.array_equal(np.flatnonzero(delta), np.flatnonzero(dr)), it
            assert np.abs(delta - dr).max() <= 1e-12 * _scale(dr), it
            assert np.array_equal(np.flatnonzero(w), np.flatnonzero(wr)), it
            assert np.abs(w - wr).max() <= 1e-12 * _scale(wr), it


def _refused(call):
    with pytest.raises(_lib.DsgdError) as e:
        call()
    assert e.value.code == _lib.EUNSUPPORTED, e.value


def test_refusals_and_state():
    """5: what Double data refuses is refused with nothing changed; float data brings everything back"""
    csr = _csr()
    row_ptr, col, val, label = csr
    rng = np.random.default_rng(51)
    split = host.split_vanilla(N_TRAIN, 3)
    steps = [[rng.permutation(np.asarray(r))[:100].astype(np.int32) for r in split] for _ in range(2)]
    w0 = _decisive_w()
    with _engine(csr) as eng:
        eng.set_weights(w0)
        g0, _ = eng.gradient_f64(steps[0][0])
        _refused(lambda: eng.plan(steps))
        _refused(lambda: eng.plan_from_seed(host.JavaRandom(0).seed, [(r.start, r.stop) for r in split], 200, 100))
        _refused(lambda: eng.async_plan([(r.start, r.stop) for r in split], 100, n_updates=4))
        _refused(lambda: eng.comm_init_f64(b"\0" * _lib.UNIQUE_ID_BYTES, 1, 0))
        out = C.c_void_p(12345)   # *out untouched
        offs = np.asarray([0, 100], np.int64)
        rc = eng._lib.dsgd_plan_create(eng._ctx, _lib.ptr(steps[0][0]), _lib.ptr(offs), C.c_int64(1), C.c_int32(1), C.byref(out))
        assert rc == _lib.EUNSUPPORTED and out.value == 12345
        assert eng.value_bits() == 64
        assert np.array_equal(_bits(eng.get_weights()), _bits(w0))
        g1, _ = eng.gradient_f64(steps[0][0])   # the next call works, on the same data and weights
        assert np.array_equal(_bits(g0), _bits(g1))
        # float values again: value_bits = 32, plans accepted
        eng.load_csr(row_ptr, col, val.astype(np.float32), label)
        eng.build_dim_sparsity(N_TRAIN)
        assert eng.value_bits() == 32
        p = eng.plan(steps)
        eng.plan_run(p, 0, 2, 0.5)
        eng.synchronize()
        p.destroy()
    with dsgd_amd.Engine(D, LAM) as e32:   # an fp32 context
        rc = e32._lib.dsgd_load_csr_f64(e32._ctx, C.c_int64(N_ROWS), _lib.ptr(row_ptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(label))
        assert rc == _lib.ESTATE
        assert e32.value_bits() == 32


def test_load_csr_f64_is_refused_under_a_communicator():
    """5: a communicator attached (one rank), float data loaded: Double data is refused, nothing changes, the next call works"""
    row_ptr, col, val, label = _csr()
    lists = [np.arange(k * 100, k * 100 + 100, dtype=np.int32) for k in range(3)]
    w0 = _decisive_w()
    with _engine(_csr(), as_float=True) as eng:
        eng.comm_init_f64(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        try:
            eng.set_weights(w0)
            _refused(lambda: eng.load_csr(row_ptr, col, val, label))
            assert eng.value_bits() == 32 and eng.n_rows == N_ROWS
            assert np.array_equal(_bits(eng.get_weights()), _bits(w0))
            st = eng.sync_step_f64(lists, 0.5)   # the float data is still there
            assert st["n_samples"] == 300
        finally:
            eng.comm_destroy()
        eng.load_csr(row_ptr, col, val, label)   # without the communicator the doubles load
        assert eng.value_bits() == 64


class _RefDictOracle:
    """ref_dict behind the surface oracle.backend.OracleBackend drives (sync_step, loss_acc)"""

    def __init__(self, data, model, dim):
        self.data, self.model, self.dim, self.lam = data, model, dim, model.lam
        self.last_stats = {"min_abs_margin": 0.0, "n_active": 0}

    def sync_step(self, w, lists, lr):
        ws = _sparse(w)
        self.last_stats = {"min_abs_margin": 0.0, "n_active": sum(_active(self.model, self.data, ws, [int(i) for i in l]) for l in lists)}
        w[:] = _dense(rd.master_sync_step(self.model, self.data, ws, [[int(i) for i in l] for l in lists], lr), len(w))

    def loss_acc(self, w, lo, hi):
        ws = _sparse(w)
        part = self.data[lo:hi]
        preds = [self.model.forward(ws, x) for x, _ in part]
        c = _tallies(preds, [y for _, y in part])
        n = float(hi - lo)
        return self.lam * float(np.sum(w * w)) + (c[1] + 2.0 * c[2]) / n, c[0] / n, c, 0.0


def _fit(backend, epochs=2):
    m = host.MasterSync(backend, N_TRAIN, N_ROWS, node_count=3, rnd=host.JavaRandom(0))
    s = m.fit(np.zeros(DP), epochs, 100, 0.5, NEVER)
    return m, s


def test_master_sync_fit_on_double_data():
    """5: 2 epochs of 3 x 100 through host.MasterSync: the plans are refused, the steps run through sync_step_f64"""
    data, model = _ref()
    ref, s_ref = _fit(OracleBackend(_RefDictOracle(data, model, D)))
    with _engine(_csr()) as eng:
        m, s = _fit(eng)
        w = eng.get_weights()
    assert m.steps_run == ref.steps_run
    assert m.accs == ref.accs and m.test_accs == ref.test_accs
    assert np.abs(w - s_ref.grad).max() <= 1e-12 * _scale(s_ref.grad)


def test_master_async_fit_raises_on_double_data():
    with _engine(_csr()) as eng:
        m = host.MasterAsync(eng, N_TRAIN, N_ROWS, node_count=3)
        with pytest.raises(NotImplementedError, match="Double feature values"):
            m.fit(np.zeros(DP), 1, 100, 0.5, NEVER, 100, 0.9)


def test_from_text_to_one_epoch():
    """6: the LYRL2004 sample: text -> doubles -> one epoch of 3 x 100 on the GPU, against ref_dict fed by ref_loader"""
    folder = os.path.join(ROOT, "tests", "golden", "lyrl2004_sample")
    data = dsgd_amd.rcv1.load(folder, full=True)
    rp, col, val, lab, _ = ref_loader.rcv1(folder, full=True)
    assert data.val64.dtype == np.float64 and data.n_rows == len(lab)
    n_rows = data.n_rows
    n_train = int(n_rows * 0.8)
    dp = data.dim + 1
    ref = _ref_data(rp, col, val, lab, dp)
    model = rd.SparseSVM(LAM, rd.dim_sparsity(ref[:n_train]))
    split = host.split_vanilla(n_train, 3)
    batch = min(100, min(len(r) for r in split))
    rng = np.random.default_rng(61)
    w_ref = rd.Sparse({}, dp)
    with dsgd_amd.Engine(data.dim, LAM, precision="fp64") as eng:
        eng.load_csr(data.row_ptr, data.col, data.val64, data.label)
        assert eng.value_bits() == 64
        eng.build_dim_sparsity(n_train)
        eng.set_weights(np.zeros(dp))
        for _ in range(4):   # (24 documents: 19 train rows, splits of 7, 7, 5)
            perms = [rng.permutation(np.asarray(r)) for r in split]
            lists = [p_[:batch].astype(np.int32) for p_ in perms]
            w_ref = rd.master_sync_step(model, ref, w_ref, [l.tolist() for l in lists], 0.5)
            eng.sync_step_f64(lists, 0.5)
        w = eng.get_weights()
    wr = _dense(w_ref, dp)
    assert np.array_equal(np.flatnonzero(w), np.flatnonzero(wr))
    assert np.abs(w - wr).max() <= 1e-12 * _scale(wr)
