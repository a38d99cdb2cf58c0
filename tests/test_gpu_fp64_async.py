"""-m gpu: the fp64 asynchronous iteration (dsgd_cs64_async_kernel, include/dsgd.h "THE FP64 MODE") against the fp64
oracle's orc_async_step.

Strict, no waivers: the engine's per-step sums are exact and only the summation order of x.w and w.ds differs from the
oracle's (~1e-16 relative), so no gate decision may differ and the weights agree within 1e-12 * max(1, |w|inf)."""

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from oracle import oracle as orc
from oracle.hogwild_replay import hog_rows, margins

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
LR = 0.5


def _pair(data, n_train, precision="fp64"):
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    eng = dsgd_amd.Engine(data.dim, LAM, precision=precision)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(n_train)
    return o, eng


def _tol(w):
    return 1e-12 * max(1.0, float(np.abs(w).max()))


def _split(n_train, k):
    return [(r.start, r.stop) for r in host.split_vanilla(n_train, k)]


def _lists(split, batch, seed, first, n, bug=False):
    K = len(split)
    return [hog_rows(seed, u % K, u // K, split[u % K][0], split[u % K][1] - split[u % K][0], batch, bug)
            for u in range(first, first + n)]


def _active(o, w, rows):
    """The oracle's gate decisions of a step's rows at weights w (core/ml/SparseSVM.scala:27-28)."""
    return o.label[rows].astype(np.float64) * margins(o, w, rows) >= 0


@pytest.mark.parametrize("batch", [1, 7, 100, 960])
def test_per_call_steps_against_the_oracle(batch):
    data = dsgd_amd.synth.generate(20000, seed=21)
    n_train = 16000
    o, eng = _pair(data, n_train)
    rng = np.random.default_rng(batch)
    w0 = np.zeros(data.dim + 1)
    w0[0] = 1e-21   # (key 0 is in no row's support: |w| <= 1e-20 there, the oracle's filt(w - 0) zeroes it)
    w_o = w0.copy()
    with eng:
        eng.set_weights(w0)
        for it in range(30):
            idx = rng.permutation(n_train)[:batch].astype(np.int32)
            d, st = eng.async_step(idx, LR, want_delta=True)
            d_o = o.async_step(w_o, idx, LR, want_delta=True)
            assert st["n_active"] == o.last_stats["n_active"] and st["n_samples"] == batch, it
            assert d.dtype == np.float64
            assert np.abs(d - d_o).max() <= _tol(d_o), it
            assert np.array_equal(np.flatnonzero(d), np.flatnonzero(d_o)), it
        w = eng.get_weights()
        assert eng.grad_kernel_name() == "dsgd_cs64_async_kernel"
    assert w[0] == 0.0 and w_o[0] == 0.0
    assert np.abs(w - w_o).max() <= _tol(w_o)


def test_update_grad_f64():
    data = dsgd_amd.synth.generate(4000, seed=22)
    _, eng = _pair(data, 3200)
    D = data.dim
    with eng:
        w0 = np.zeros(D + 1)
        w0[[1, 2, 3, 10]] = [0.25, 1e-19, -7.0, 2.0]
        eng.set_weights(w0)
        # exact cancellation, a result below 1e-20, an ordinary one, a key that was zero
        eng.update_grad(np.array([1, 2, 3, 11]), np.array([0.25, 9.5e-20, 1.5, -4e-3]))
        assert 0.0 < 1e-19 - 9.5e-20 <= 1e-20
        want = w0.copy()
        want[1] = 0.0
        want[2] = 0.0
        want[3] = -7.0 - 1.5
        want[11] = 4e-3
        w = eng.get_weights()
        assert np.array_equal(w, want) and w[1] == 0.0 and w[2] == 0.0
        before = w.copy()
        for keys, vals, code in (([4, 4], [1.0, 2.0], _lib.EINVAL), ([0, D + 1], [1.0, 1.0], _lib.ERANGE), ([-1], [1.0], _lib.ERANGE)):
            with pytest.raises(_lib.DsgdError) as ei:
                eng.update_grad(np.array(keys), np.array(vals))
            assert ei.value.code == code
            assert np.array_equal(eng.get_weights().view(np.uint64), before.view(np.uint64))
        # on slice-major weights (kept between plan runs) the update lands where it does on rank-ordered ones
        p = eng.async_plan(_split(3200, 1), 10, seed=1, positional_bug=False, first_update=0, n_updates=3)
        keys, vals = np.array([7, 3, 0]), np.array([0.5, -0.25, 1e-3])
        eng.plan_run_async(p, 0, 3, LR)
        eng.update_grad(keys, vals)                  # (the weights are slice-major here)
        after_sliced = eng.get_weights()
        eng.set_weights(before)
        eng.plan_run_async(p, 0, 3, LR)
        mid = eng.get_weights()                      # (rank order again)
        eng.update_grad(keys, vals)
        after = eng.get_weights()
        p.destroy()
        exp = mid.copy()
        for k_, v_ in zip(keys, vals):
            x = mid[k_] - v_
            exp[k_] = x if abs(x) > 1e-20 else 0.0
        assert np.array_equal(after, exp)
        assert np.array_equal(after_sliced.view(np.uint64), after.view(np.uint64))
    with dsgd_amd.Engine(data.dim, LAM) as e32:
        lib = e32._lib
        k = np.array([1], dtype=np.int32)
        v = np.array([1.0])
        assert lib.dsgd_update_grad_f64(e32._ctx, _lib.ptr(k), _lib.ptr(v), _lib.C.c_int64(1)) == _lib.ESTATE
        assert lib.dsgd_async_step_f64(e32._ctx, _lib.ptr(k), _lib.C.c_int64(1), _lib.C.c_double(0.5), None, None) == _lib.ESTATE
        assert lib.dsgd_plan_run_async_f64(e32._ctx, None, _lib.C.c_int64(0), _lib.C.c_int64(0), _lib.C.c_double(0.5)) == _lib.EINVAL
        with pytest.raises(_lib.DsgdError) as ei:
            e32.async_plan([(0, 100)], 10)
        assert ei.value.code == _lib.ESTATE


def test_three_replicas_gossip_bit_identical():
    data = dsgd_amd.synth.generate(23149, seed=0)
    n_train = int(23149 * 0.8)
    split = _split(n_train, 3)
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    reps = []
    for _ in range(3):
        _, e = _pair(data, n_train)
        reps.append(e)
    w_ref = np.zeros(data.dim + 1)
    seed = 5
    try:
        for u in range(300):
            k = u % 3
            rows = hog_rows(seed, k, u // 3, split[k][0], split[k][1] - split[k][0], 100, False)
            d, _ = reps[k].async_step(rows, LR, want_delta=True)
            for j in range(3):
                if j != k:
                    reps[j].update_grad(np.flatnonzero(d), d[d != 0])
            o.async_step(w_ref, rows, LR)
        ws = [e.get_weights() for e in reps]
    finally:
        for e in reps:
            e.close()
    assert np.array_equal(ws[0].view(np.uint64), ws[1].view(np.uint64))
    assert np.array_equal(ws[0].view(np.uint64), ws[2].view(np.uint64))
    assert np.abs(ws[0] - w_ref).max() <= _tol(w_ref)


@pytest.mark.parametrize("K,batch,bug", [(1, 100, False), (3, 100, True), (4, 1, False), (2, 960, False)])
def test_device_lists_equal_hog_rows(K, batch, bug):
    data = dsgd_amd.synth.generate(23149, seed=0)
    n_train = int(23149 * 0.8)
    split = _split(n_train, K)
    _, eng = _pair(data, n_train)
    with eng:
        for first, n in ((0, 2 * K + 1), (K + 1, 3 * K + 2)):   # (the second starts in the middle of a round)
            p = eng.async_plan(split, batch, seed=77, positional_bug=bug, first_update=first, n_updates=n)
            assert p.n_workers == 1 and p.info()["kind"] == "column_slices_fp64"
            idx, offsets = eng.plan_lists(p)
            p.destroy()
            assert list(offsets) == [batch * i for i in range(n + 1)]
            want = np.concatenate(_lists(split, batch, 77, first, n, bug))
            assert np.array_equal(idx, want)


def _replay(o, w, lists, mask=None):
    """The oracle's sequential replay; with `mask` (the engine's record) every gate decision is compared first."""
    for t, rows in enumerate(lists):
        if mask is not None:
            assert np.array_equal(mask[t, :len(rows)], _active(o, w, rows)), "step %d: a gate decision differs" % t
        o.async_step(w, rows, LR)
    return w


def test_resident_runs():
    n_rows = 23149
    n_train = int(n_rows * 0.8)
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    split = _split(n_train, 3)
    o, eng = _pair(data, n_train)
    _, eng2 = _pair(data, n_train)
    n = 2000
    with eng, eng2:
        p = eng.async_plan(split, 100, seed=3, positional_bug=False, first_update=0, n_updates=n)
        p.record(True)
        eng.plan_run_async(p, 0, 700, LR)            # [0, a) + [a, b) ...
        eng.plan_run_async(p, 700, n, LR)
        mask, _ = p.read_record()
        w = eng.get_weights()
        assert eng.grad_kernel_name() == "dsgd_cs64_async_kernel"
        p2 = eng2.async_plan(split, 100, seed=3, positional_bug=False, first_update=0, n_updates=n)
        eng2.plan_run_async(p2, 0, n, LR)            # ... against one run [0, b) on a second context
        w2 = eng2.get_weights()
        idx, offsets = eng2.plan_lists(p2)
        p.destroy()
        p2.destroy()
        # the same lists through the per-call entry
        eng2.set_weights(np.zeros(data.dim + 1))
        for t in range(300):
            eng2.async_step(idx[offsets[t]:offsets[t + 1]], LR)
        w_call = eng2.get_weights()
        eng2.set_weights(np.zeros(data.dim + 1))
        p3 = eng2.async_plan(split, 100, seed=3, positional_bug=False, first_update=0, n_updates=300)
        eng2.plan_run_async(p3, 0, 300, LR)
        w_res = eng2.get_weights()
        p3.destroy()
    assert np.array_equal(w.view(np.uint64), w2.view(np.uint64))
    assert np.array_equal(w_call.view(np.uint64), w_res.view(np.uint64))
    w_o = _replay(o, np.zeros(data.dim + 1), _lists(split, 100, 3, 0, n), mask)
    assert np.abs(w - w_o).max() <= _tol(w_o)


def test_plan_of_several_workers_is_refused_by_the_async_run():
    data = dsgd_amd.synth.generate(4000, seed=23)
    _, eng = _pair(data, 3200)
    with eng:
        p = eng.plan([[np.arange(0, 10, dtype=np.int32), np.arange(10, 20, dtype=np.int32)]])
        with pytest.raises(_lib.DsgdError) as ei:
            eng.plan_run_async(p, 0, 1, LR)
        assert ei.value.code == _lib.EINVAL
        p.destroy()
        with pytest.raises(_lib.DsgdError) as ei:
            eng.async_plan([(0, 3200)], 1025)
        assert ei.value.code == _lib.EUNSUPPORTED
        with pytest.raises(_lib.DsgdError) as ei:
            eng.async_plan([(0, 4001)], 10)
        assert ei.value.code == _lib.ERANGE


def test_master_async_fit_fp64_against_the_oracle():
    """host.MasterAsync.fit on an fp64 engine, application.conf's sizes (N = 23,149, 3 workers x 100, lr 0.5), one
    epoch's budget, never stopping early: the zero-lag schedule replayed by the oracle."""
    n_rows = 23149
    n_train = int(n_rows * 0.8)
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    o, eng = _pair(data, n_train)
    check_every, leak, seed = 2000, 0.9, 0
    with eng:
        m = host.MasterAsync(eng, n_train, n_rows, 3)
        s = m.fit(np.zeros(data.dim + 1), 1, 100, LR, lambda losses: False, check_every, leak, seed=seed, positional_bug=True)
    steps = n_train
    assert s.updates == steps
    split = _split(n_train, 3)
    w = np.zeros(data.dim + 1)
    losses, accs, best_l, best_w = [], [], float("inf"), w.copy()
    for u0 in range(0, steps + 1, check_every):
        l, a, _, _ = o.loss_acc(w, n_train, n_rows)
        pl, pa = (losses[0], accs[0]) if losses else (l, a)
        l, a = leak * l + (1 - leak) * pl, leak * a + (1 - leak) * pa
        if best_l > l:
            best_l, best_w = l, w.copy()
        losses.insert(0, l)
        accs.insert(0, a)
        n = min(check_every, steps - u0)
        if n <= 0:
            break
        _replay(o, w, _lists(split, 100, seed, u0, n, True))
    if steps % check_every:
        l, a, _, _ = o.loss_acc(w, n_train, n_rows)
        l, a = leak * l + (1 - leak) * losses[0], leak * a + (1 - leak) * accs[0]
        if best_l > l:
            best_l, best_w = l, w.copy()
        losses.insert(0, l)
        accs.insert(0, a)
    assert m.test_accs == accs
    assert len(m.test_losses) == len(losses)
    for x, y in zip(m.test_losses, losses):
        assert abs(x - y) <= 1e-12 * max(1.0, abs(y))
    assert np.abs(s.grad - best_w).max() <= _tol(best_w)


def test_rcv1_size_20000_updates_no_decision_differs():
    n_rows = 804414
    n_train = int(n_rows * 0.8)
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    split = _split(n_train, 3)
    o, eng = _pair(data, n_train)
    n = 20000
    with eng:
        p = eng.async_plan(split, 100, seed=9, positional_bug=False, first_update=0, n_updates=n)
        p.record(True)
        eng.plan_run_async(p, 0, n, LR)
        mask, _ = p.read_record()
        w = eng.get_weights()
        p.destroy()
    w_o = _replay(o, np.zeros(data.dim + 1), _lists(split, 100, 9, 0, n), mask)
    assert np.abs(w - w_o).max() <= _tol(w_o)


def test_fp32_hogwild_untouched_by_an_fp64_async_neighbour():
    data = dsgd_amd.synth.generate(20000, seed=15)
    n_train = 16000

    def hog_run():
        _, e = _pair(data, n_train, precision="fp32")
        with e:
            e.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
            e.async_start([(0, n_train)], batch=100, lr=LR, max_updates=300, seed=4, positional_bug=False)
            e.async_wait()
            e.async_stop()
            return e.get_weights()

    alone = hog_run()
    _, e64 = _pair(data, n_train)
    with e64:
        p = e64.async_plan(_split(n_train, 3), 100, seed=4, positional_bug=False, first_update=0, n_updates=3000)
        e64.plan_run_async(p, 0, 3000, LR)
        beside = hog_run()
        e64.synchronize()
        p.destroy()
    assert np.array_equal(alone.view(np.uint32), beside.view(np.uint32))
