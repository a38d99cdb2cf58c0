"""-m gpu: resident ROW-PARALLEL plans of the fp64 mode (dsgd_plan_create_rp64_n, dsgd_plan_create_from_seed_rp64,
dsgd_async_plan_create_rp64; include/dsgd.h "THE FP64 MODE", ROW-PARALLEL PLANS; csrc/dsgd_rp64.hpp).

The yardstick is always code from before these plans existed, never the plan path itself: Engine.sync_steps_f64,
Engine.async_step (dsgd_async_step_f64), csrc/jrand.c through host.epoch_lists, and oracle/ref_dict.py.  Every comparison
with sync_steps_f64 / async_step_f64 is on BITS: the column sums are integers, so nothing depends on the order of the adds
or on how a run is cut into calls.

Data: synth.generate(4000, seed=5, dim=1000), 3,200 train rows.  Double data: the same rows with every value times
(1 + k * 2^-40), k a small per-entry integer -- no value is float-representable.  Weights: 300 random coordinates of
scale 0.1, the manner of tests/test_gpu_fp64_values.py's _decisive_w (restated here): margins far from zero.

Against ref_dict the bound is the one tests/test_gpu_fp64_values.py uses for the asynchronous step: equal supports and
max|w - w_ref| <= 1e-12 * max(1, |w_ref|_inf)."""

import ctypes as C
import math

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from oracle import ref_dict as rd

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
LR = 0.5
DIM = 1000
N_ROWS, N_TRAIN = 4000, 3200
NEVER = lambda losses: False
_CACHE = {}


def _data(dim=DIM, n_rows=N_ROWS):
    """-> (Csr with float values, the Double values)"""
    key = ("data", dim, n_rows)
    if key not in _CACHE:
        d = dsgd_amd.synth.generate(n_rows, seed=5, dim=dim)
        k = np.random.default_rng(13).integers(1, 64, size=len(d.val))
        val64 = d.val.astype(np.float64) * (1.0 + k * 2.0 ** -40)
        assert np.all(val64.astype(np.float32).astype(np.float64) != val64)   # no value is a float
        _CACHE[key] = (d, val64)
    return _CACHE[key]


def _engine(double, dim=DIM, n_rows=N_ROWS, n_train=N_TRAIN, precision="fp64", rounded=False):
    """rounded: the Double values rounded to float (the negative control's data)"""
    d, val64 = _data(dim, n_rows)
    eng = dsgd_amd.Engine(d.dim, LAM, precision=precision)
    val = val64 if double else (val64.astype(np.float32) if rounded else d.val)
    eng.load_csr(d.row_ptr, d.col, val, d.label)
    eng.build_dim_sparsity(n_train)
    return eng


def _decisive_w(dim=DIM):
    rng = np.random.default_rng(3)
    w = np.zeros(dim + 1)
    ks = rng.choice(np.arange(1, dim + 1), min(300, dim), replace=False)
    w[ks] = rng.normal(scale=0.1, size=len(ks))
    return w


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _scale(v):
    return max(1.0, float(np.abs(v).max()))


def _flat(steps):
    lists = [np.asarray(a, np.int32) for s in steps for a in s]
    offs = np.zeros(len(lists) + 1, np.int64)
    offs[1:] = np.cumsum([len(a) for a in lists])
    return np.concatenate(lists), offs, len(steps), len(steps[0])


def _steps(n_steps, k, n, n_train=N_TRAIN, seed=17):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, n_train, size=n).astype(np.int32) for _ in range(k)] for _ in range(n_steps)]


def _ref_dict(double):
    """(data, model) of oracle/ref_dict.py over the float or the Double values"""
    key = ("ref", double)
    if key not in _CACHE:
        d, val64 = _data()
        val = val64 if double else d.val.astype(np.float64)
        data = [(rd.Sparse({int(c): float(v) for c, v in zip(d.col[d.row_ptr[i]:d.row_ptr[i + 1]], val[d.row_ptr[i]:d.row_ptr[i + 1]])},
                           d.dim + 1), int(d.label[i])) for i in range(d.n_rows)]
        _CACHE[key] = (data, rd.SparseSVM(LAM, rd.dim_sparsity(data[:N_TRAIN])))
    return _CACHE[key]


def _sparse(w):
    return rd.Sparse({int(k): float(w[k]) for k in np.flatnonzero(w)}, len(w))


def _dense(sp, dp):
    out = np.zeros(dp)
    for k, v in sp.map.items():
        out[k] = v
    return out


def _code(call):
    try:
        call()
    except _lib.DsgdError as e:
        return e.code
    return _lib.OK


def _plan_vs_steps(steps, double, dim=DIM, n_rows=N_ROWS, n_train=N_TRAIN, cuts=None):
    """a row-parallel plan of `steps` against sync_steps_f64 on the same lists from the same weights: bits and statistics"""
    idx, offs, n_steps, k = _flat(steps)
    w0 = _decisive_w(dim)
    with _engine(double, dim, n_rows, n_train) as ref:
        ref.set_weights(w0)
        st_ref = ref.sync_steps_f64(idx, offs, n_steps, k, LR)
        w_ref = ref.get_weights()
    assert not np.array_equal(_bits(w_ref), _bits(w0)) and st_ref["n_active"] > 0
    with _engine(double, dim, n_rows, n_train) as eng:
        eng.set_weights(w0)
        p = eng.plan(steps, rp64=True)
        assert p.info()["kind"] == "row_parallel_fp64" and p.info()["slices"] == 0
        for a, b in (cuts or [(0, n_steps)]):
            eng.plan_run(p, a, b, LR)
        st = eng.synchronize()
        assert eng.grad_kernel_name() == ("dsgd_rp64v_grad_kernel" if double else "dsgd_rp64_grad_kernel")
        w = eng.get_weights()
        p.destroy()
    assert st == st_ref
    assert np.array_equal(_bits(w), _bits(w_ref))
    return w


@pytest.mark.parametrize("k,n,n_steps", [(5, 40, 12), (2, 1100, 4)])
def test_beyond_the_column_slices_limits_on_bits(k, n, n_steps):
    """1: more than 4 workers; more than 1,024 rows per step (float data)"""
    steps = _steps(n_steps, k, n)
    with _engine(False) as eng:   # (what the existing creator says to these lists)
        assert _code(lambda: eng.plan(steps)) == _lib.EUNSUPPORTED
    _plan_vs_steps(steps, False)


def test_beyond_the_lds_limit_on_bits():
    """1: dim = 50,416 at 4 workers, the model tests/test_gpu_fp64.py shows being refused"""
    steps = [[((np.arange(50) * 7 + 11 * j + 3 * s) % 480).astype(np.int32) for j in range(4)] for s in range(2)]
    with _engine(False, 50416, 600, 480) as eng:
        assert _code(lambda: eng.plan(steps)) == _lib.EUNSUPPORTED
    _plan_vs_steps(steps, False, 50416, 600, 480)


def test_double_data_cut_into_calls_and_the_negative_control():
    """2: 3 x 100 x 20 on Double data; [0, 7) + [7, 20); the float-rounded copy differs"""
    steps = _steps(20, 3, 100)
    w = _plan_vs_steps(steps, True)
    w_cut = _plan_vs_steps(steps, True, cuts=[(0, 7), (7, 20)])
    assert np.array_equal(_bits(w), _bits(w_cut))
    with _engine(False, rounded=True) as eng:
        eng.set_weights(_decisive_w())
        p = eng.plan(steps, rp64=True)
        eng.plan_run(p, 0, 20, LR)
        eng.synchronize()
        w_rounded = eng.get_weights()
        p.destroy()
    assert not np.array_equal(_bits(w), _bits(w_rounded))   # the doubles are read


def test_slice_major_weights_on_entry():
    """3: a column-slice plan leaves the weights slice-major; the row-parallel plan behind it reads and writes them there"""
    first, then = _steps(3, 3, 100, seed=5), _steps(5, 3, 100, seed=6)
    got = []
    for rp in (True, False):
        with _engine(False) as eng:
            eng.set_weights(_decisive_w())
            p = eng.plan(first)
            assert p.info()["kind"] == "column_slices_fp64"
            eng.plan_run(p, 0, 3, LR)
            if rp:
                q = eng.plan(then, rp64=True)
                eng.plan_run(q, 0, 5, LR)
                st = eng.synchronize()
                assert st["n_samples"] == 3 * 300 + 5 * 300
                q.destroy()
            else:
                eng.synchronize()
                eng.sync_steps_f64(*_flat(then), LR)
            p.destroy()
            got.append(eng.get_weights())
    assert np.array_equal(_bits(got[0]), _bits(got[1]))


def _lcg_steps(a, b, limit):
    """raw values java.util.Random draws between its internal states a and b"""
    n = 0
    while a != b:
        a = (a * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        n += 1
        assert n <= limit
    return n


def test_lists_drawn_by_the_device_on_double_data():
    """4: plan_from_seed(rp64=True): the lists, the generator's state and the draw count are the host's; the epoch on bits"""
    split = host.split_vanilla(N_TRAIN, 3)
    max_samples = max(len(r) for r in split)
    rnd = host.JavaRandom(0)
    state0 = rnd.seed
    idx_h, offs_h, n_h = host.epoch_lists(rnd, split, max_samples, 100)
    w0 = _decisive_w()
    with _engine(True) as eng:
        assert _code(lambda: eng.plan_from_seed(state0, split, max_samples, 100)) == _lib.EUNSUPPORTED   # (the existing creator)
        eng.set_weights(w0)
        p, n_d, state_d, draws = eng.plan_from_seed(state0, split, max_samples, 100, rp64=True)
        assert p.info()["kind"] == "row_parallel_fp64"
        idx_d, offs_d = eng.plan_lists(p)
        assert n_d == n_h and np.array_equal(offs_d, offs_h[:n_h * 3 + 1]) and np.array_equal(idx_d, idx_h[:offs_h[n_h * 3]])
        assert state_d == rnd.seed
        assert draws == _lcg_steps(state0, rnd.seed, 4 * n_h * N_TRAIN)
        eng.plan_run(p, 0, n_d, LR)
        st = eng.synchronize()
        p.destroy()
        w = eng.get_weights()
    with _engine(True) as ref:
        ref.set_weights(w0)
        st_ref = ref.sync_steps_f64(idx_h[:offs_h[n_h * 3]], offs_h[:n_h * 3 + 1], n_h, 3, LR)
        assert st == st_ref
        assert np.array_equal(_bits(w), _bits(ref.get_weights()))


def test_asynchronous_plans():
    """5: async_plan(rp64=True) on Double data: the existing creator's lists, the bits of the async_step_f64 loop; on float data
    with a batch of 1,100 rows against ref_dict.async_step"""
    split = [(r.start, r.stop) for r in host.split_vanilla(N_TRAIN, 3)]
    w0 = _decisive_w()
    with _engine(False) as f32:
        old = f32.async_plan(split, 100, seed=9, n_updates=12)
        idx_old, offs_old = f32.plan_lists(old)
        old.destroy()
    with _engine(True) as eng:
        assert _code(lambda: eng.async_plan(split, 100, seed=9, n_updates=12)) == _lib.EUNSUPPORTED
        eng.set_weights(w0)
        p = eng.async_plan(split, 100, seed=9, n_updates=12, rp64=True)
        idx, offs = eng.plan_lists(p)
        assert np.array_equal(idx, idx_old) and np.array_equal(offs, offs_old)
        eng.plan_run_async(p, 0, 5, 0.3)
        eng.plan_run_async(p, 5, 12, 0.3)
        st = eng.synchronize()
        p.destroy()
        w = eng.get_weights()
    with _engine(True) as ref:
        ref.set_weights(w0)
        act = 0
        for u in range(12):
            _, s_u = ref.async_step(idx[offs[u]:offs[u + 1]], 0.3)
            act += s_u["n_active"]
        assert st == {"n_samples": 1200, "n_active": act}
        assert np.array_equal(_bits(w), _bits(ref.get_weights()))
    # float data, a batch beyond the column slices' 1,024 rows: dsgd_rp64_finish_async_kernel
    data, model = _ref_dict(False)
    with _engine(False) as eng:
        assert _code(lambda: eng.async_plan(split, 1100, seed=4, n_updates=4)) == _lib.EUNSUPPORTED
        eng.set_weights(w0)
        p = eng.async_plan(split, 1100, seed=4, n_updates=4, rp64=True)
        idx, offs = eng.plan_lists(p)
        w_ref = _sparse(w0)
        for u in range(4):
            eng.plan_run_async(p, u, u + 1, 0.3)
            eng.synchronize()
            w_ref, _ = rd.async_step(model, data, w_ref, [int(i) for i in idx[offs[u]:offs[u + 1]]], 0.3)
            w, wr = eng.get_weights(), _dense(w_ref, DIM + 1)
            assert np.array_equal(np.flatnonzero(w), np.flatnonzero(wr)), u
            assert np.abs(w - wr).max() <= 1e-12 * _scale(wr), u
        p.destroy()


def test_the_record_on_double_data():
    """6: the record changes no bit of the weights; per step its popcount, every bit against ref_dict, s_used, and a second run"""
    steps = _steps(6, 3, 100, seed=23)
    idx, offs, n_steps, k = _flat(steps)
    data, model = _ref_dict(True)
    w0 = _decisive_w()
    with _engine(True) as ref:
        ref.set_weights(w0)
        act_ref = ref.sync_steps_f64(idx, offs, n_steps, k, LR, per_step=True)["active_per_step"].tolist()
        w_ref = ref.get_weights()
    with _engine(True) as eng:
        ds = eng.get_dim_sparsity()
        eng.set_weights(w0)
        p = eng.plan(steps, rp64=True)
        p.record(True)
        assert p.info()["record_words"] == (300 + 31) // 32
        before = []
        for t in range(n_steps):   # (step by step: the weights in front of every step)
            before.append(eng.get_weights())
            eng.plan_run(p, t, t + 1, LR)
            eng.synchronize()
        assert eng.grad_kernel_name() == "dsgd_rp64v_grad_rec_kernel"
        assert np.array_equal(_bits(eng.get_weights()), _bits(w_ref))   # on or off: the same bits
        mask, s_used = p.read_record()
        assert mask.shape == (n_steps, 32 * ((300 + 31) // 32))
        checked = 0
        for t in range(n_steps):
            assert int(mask[t].sum()) == act_ref[t] and not mask[t][300:].any(), t
            ws = _sparse(before[t])
            rows = [int(i) for lst in steps[t] for i in lst]
            for r, i in enumerate(rows):
                margin = data[i][1] * data[i][0].dot(ws)
                if abs(margin) > 1e-9:
                    checked += 1
                    assert bool(mask[t][r]) == (not margin < 0), (t, r, margin)
            s = LAM * 2.0 * math.fsum(float(a) * float(b) for a, b in zip(before[t], ds))
            ulp = float(np.spacing(np.float32(abs(s))))
            assert abs(float(s_used[t]) - float(np.float32(s))) <= ulp, (t, s, s_used[t])
        assert checked == n_steps * 300   # decisive weights: the cap on the margin hid no row
        # a step run again overwrites its record: step 0 from the weights behind the run decides other rows than from w0
        eng.plan_run(p, 0, 1, LR)
        eng.synchronize()
        mask2, s2 = p.read_record(0, 1)
        ws = _sparse(w_ref)
        want = [not (data[int(i)][1] * data[int(i)][0].dot(ws) < 0) for lst in steps[0] for i in lst]
        assert mask2[0][:300].tolist() == want and not mask2[0][300:].any()
        assert mask2[0][:300].tolist() != mask[0][:300].tolist() and s2[0] != s_used[0]
        p.record(False)
        p.destroy()


def test_refusals_change_nothing():
    """7"""
    lib = _lib.load()
    steps = _steps(2, 2, 50)
    idx, offs, n_steps, k = _flat(steps)
    with _engine(False, precision="fp32") as e32:
        assert _code(lambda: e32.plan(steps, rp64=True)) == _lib.ESTATE
        split = [(r.start, r.stop) for r in host.split_vanilla(N_TRAIN, 3)]
        assert _code(lambda: e32.async_plan(split, 100, rp64=True)) == _lib.ESTATE
        assert _code(lambda: e32.plan_from_seed(host.JavaRandom(0).seed, host.split_vanilla(N_TRAIN, 3), 1067, 100, rp64=True)) == _lib.ESTATE
    with _engine(True) as eng:
        w0 = _decisive_w()
        eng.set_weights(w0)
        sentinel = 0x5A5A5A5A

        def raw(idx_, n_idx, offs_, n_steps_, k_, with_out=True):
            h = C.c_void_p(sentinel)
            rc = lib.dsgd_plan_create_rp64_n(eng._ctx, _lib.ptr(idx_), C.c_int64(n_idx), _lib.ptr(offs_), C.c_int64(n_steps_), C.c_int32(k_),
                                             C.byref(h) if with_out else None)
            assert h.value == sentinel   # *out untouched
            return rc

        empty = offs.copy()
        empty[2] = empty[1]
        down = offs.copy()
        down[2] = down[1] - 1
        short = offs.copy()
        short[-1] -= 1
        bad = idx.copy()
        bad[-1] = N_ROWS
        for what, rc, want in (("an empty list", raw(idx, len(idx), empty, n_steps, k), _lib.EINVAL),
                               ("offsets decrease", raw(idx, len(idx), down, n_steps, k), _lib.EINVAL),
                               ("offsets end early", raw(idx, len(idx), short, n_steps, k), _lib.EINVAL),
                               ("row == n_rows", raw(bad, len(idx), offs, n_steps, k), _lib.ERANGE),
                               ("null out", raw(idx, len(idx), offs, n_steps, k, with_out=False), _lib.EINVAL)):
            assert rc == want, what
            assert np.array_equal(_bits(eng.get_weights()), _bits(w0)), what
        p = eng.plan(steps, rp64=True)
        assert _code(lambda: eng.plan_run_async(p, 0, 1, 0.3)) == _lib.EINVAL
        assert np.array_equal(_bits(eng.get_weights()), _bits(w0))
        # the existing creators refuse Double data as before
        assert _code(lambda: eng.plan(steps)) == _lib.EUNSUPPORTED
        assert _code(lambda: eng.async_plan([(0, N_TRAIN)], 100)) == _lib.EUNSUPPORTED
        assert _code(lambda: eng.plan_from_seed(host.JavaRandom(0).seed, host.split_vanilla(N_TRAIN, 3), 1067, 100)) == _lib.EUNSUPPORTED
        # ... and the context is usable: the plan runs, and is sync_steps_f64
        eng.plan_run(p, 0, n_steps, LR)
        eng.synchronize()
        p.destroy()
        w = eng.get_weights()
    with _engine(True) as ref:
        ref.set_weights(w0)
        ref.sync_steps_f64(idx, offs, n_steps, k, LR)
        assert np.array_equal(_bits(w), _bits(ref.get_weights()))


def test_reload():
    """8: a plan made on float data serves the Double copy loaded behind it; lists beyond a shorter load: DSGD_ERANGE, then again"""
    d, val64 = _data()
    steps = _steps(4, 3, 100, seed=31)   # (rows up to 3,199)
    idx, offs, n_steps, k = _flat(steps)
    w0 = _decisive_w()
    with _engine(True) as fresh:
        fresh.set_weights(w0)
        q = fresh.plan(steps, rp64=True)
        fresh.plan_run(q, 0, n_steps, LR)
        fresh.synchronize()
        q.destroy()
        w_fresh = fresh.get_weights()
    with _engine(False) as eng:
        p = eng.plan(steps, rp64=True)
        eng.load_csr(d.row_ptr, d.col, val64, d.label)
        eng.build_dim_sparsity(N_TRAIN)
        eng.set_weights(w0)
        eng.plan_run(p, 0, n_steps, LR)
        eng.synchronize()
        assert eng.grad_kernel_name() == "dsgd_rp64v_grad_kernel"
        assert np.array_equal(_bits(eng.get_weights()), _bits(w_fresh))
        # 1,000 rows: the plan indexes beyond them
        assert int(idx.max()) >= 1000
        nnz = int(d.row_ptr[1000])
        eng.load_csr(d.row_ptr[:1001], d.col[:nnz], val64[:nnz], d.label[:1000])
        eng.build_dim_sparsity(800)
        eng.set_weights(w0)
        assert _code(lambda: eng.plan_run(p, 0, n_steps, LR)) == _lib.ERANGE
        assert np.array_equal(_bits(eng.get_weights()), _bits(w0))
        # the full data back: it runs again
        eng.load_csr(d.row_ptr, d.col, val64, d.label)
        eng.build_dim_sparsity(N_TRAIN)
        eng.set_weights(w0)
        eng.plan_run(p, 0, n_steps, LR)
        eng.synchronize()
        assert np.array_equal(_bits(eng.get_weights()), _bits(w_fresh))
        p.destroy()


def _fit_sync(eng):
    m = host.MasterSync(eng, N_TRAIN, N_ROWS, node_count=3, rnd=host.JavaRandom(0))
    m.fit(np.zeros(DIM + 1), 2, 100, 0.5, NEVER)
    return m


def test_host_mirrors(monkeypatch):
    """9: DSGD_F64_RP_PLANS=1 -- MasterSync.fit through one device-drawn row-parallel plan per epoch, the bits of the
    DSGD_F64_STEPS=1 run; MasterAsync.fit on Double data, the bits of the async_step_f64 loop; unset: it raises as before"""
    monkeypatch.delenv("DSGD_F64_RP_PLANS", raising=False)
    monkeypatch.setenv("DSGD_F64_STEPS", "1")
    with _engine(True) as eng:
        m_ref = _fit_sync(eng)
        w_ref = eng.get_weights()
    monkeypatch.delenv("DSGD_F64_STEPS", raising=False)
    monkeypatch.setenv("DSGD_F64_RP_PLANS", "1")
    with _engine(True) as eng:
        seeded, batched = [], []
        real_seed, real_steps = eng.plan_from_seed, eng.sync_steps_f64
        eng.plan_from_seed = lambda *a, **kw: (seeded.append(kw.get("rp64", False)), real_seed(*a, **kw))[1]
        eng.sync_steps_f64 = lambda *a, **kw: (batched.append(1), real_steps(*a, **kw))[1]
        m = _fit_sync(eng)
        assert seeded.count(True) == 2 and not batched
        assert m.steps_run == m_ref.steps_run and m.accs == m_ref.accs and m.test_accs == m_ref.test_accs
        assert np.array_equal(_bits(eng.get_weights()), _bits(w_ref))
    # MasterAsync: 24 updates of 3 workers x 100 rows, a loss check every 8
    with _engine(True) as eng:
        lists = []
        real_plan = eng.async_plan

        def spy(*a, **kw):
            plan = real_plan(*a, **kw)
            lists.append((kw.get("rp64", False), kw["first_update"]) + tuple(eng.plan_lists(plan)))
            return plan

        eng.async_plan = spy
        ma = host.MasterAsync(eng, N_TRAIN, N_ROWS, node_count=3)
        state = ma.fit(np.zeros(DIM + 1), 1, 100, 0.5, NEVER, 8, 0.9, seed=2, max_steps=24)
        assert state.updates == 24 and len(lists) == 1 and lists[0][0] is True and lists[0][1] == 0
        w = eng.get_weights()
    with _engine(True) as ref:
        ref.set_weights(np.zeros(DIM + 1))
        _, _, idx, offs = lists[0]
        for u in range(24):
            ref.async_step(idx[offs[u]:offs[u + 1]], 0.5)
        assert np.array_equal(_bits(w), _bits(ref.get_weights()))
    monkeypatch.delenv("DSGD_F64_RP_PLANS", raising=False)
    with _engine(True) as eng:
        with pytest.raises(NotImplementedError, match="Double feature values"):
            host.MasterAsync(eng, N_TRAIN, N_ROWS, node_count=3).fit(np.zeros(DIM + 1), 1, 100, 0.5, NEVER, 8, 0.9, max_steps=24)
