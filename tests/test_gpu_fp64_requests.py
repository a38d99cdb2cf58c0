"""-m gpu: the fp64 mode's request / response gradient and steps of any size (dsgd_gradient_f64, dsgd_sync_step_f64,
dsgd_forward_f64; csrc/dsgd_rp64.hpp) against the fp64 oracle.

The column sums are exact 64-bit integers on the device, so inside the stated exact range the results differ from the
oracle only by the rounding order of x . w and w . ds and by the oracle's per-add rounding: 1e-12 relative, no gate
decision differs.  With lambda = 0 each coordinate is the correctly rounded exact sum, bit for bit math.fsum."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from hard_data import check_exact_range as _check_exact_range   # (with its complement, outside_exact_range)
from oracle import oracle as orc
from oracle_backend import OracleBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
NEVER = lambda losses: False   # (no early stop: every epoch runs)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DATA = {}


def _data(n_rows):
    if n_rows not in _DATA:
        _DATA.clear()   # (one data set at a time: the full size is 60 M non-zeros)
        _DATA[n_rows] = dsgd_amd.synth.generate(n_rows, seed=0)
    return _DATA[n_rows]


def _pair(data, n_train, lam=LAM, precision="fp64"):
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, lam)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    eng = dsgd_amd.Engine(data.dim, lam, precision=precision)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(n_train)
    return o, eng


def _random_w(dim, seed=1):
    rng = np.random.default_rng(seed)
    w = np.zeros(dim + 1)
    w[rng.choice(np.arange(1, dim + 1), 3000, replace=False)] = rng.normal(scale=0.1, size=3000)
    return w


def _scale(v):
    return max(1.0, float(np.abs(v).max()))


def _check_grad(o, eng, w, idx):
    g, st = eng.gradient_f64(idx)
    g_o = o.gradient(w, idx)
    assert g.dtype == np.float64 and st["n_samples"] == len(idx)
    assert st["n_active"] == o.last_stats["n_active"]
    assert np.array_equal(np.flatnonzero(g), np.flatnonzero(g_o))
    assert np.abs(g - g_o).max() <= 1e-12 * _scale(g_o)
    return g


@pytest.mark.parametrize("n", [1, 100, 960, 4096, 65536])
def test_gradient_f64_against_the_oracle(n):
    data = _data(100000)
    n_train = 80000
    o, eng = _pair(data, n_train)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, n_train, size=n).astype(np.int32)
    with eng:
        w = _random_w(data.dim)
        eng.set_weights(w)
        _check_grad(o, eng, w, idx)
        # the weights a 20-step fp64 plan leaves (slice-major on the device)
        eng.set_weights(np.zeros(data.dim + 1))
        split = host.split_vanilla(n_train, 3)
        steps = [[rng.permutation(np.asarray(r))[:100].astype(np.int32) for r in split] for _ in range(20)]
        p = eng.plan(steps)
        eng.plan_run(p, 0, 20, 0.5)
        w_o = np.zeros(data.dim + 1)
        for lists in steps:
            o.sync_step(w_o, lists, 0.5)
        g = _check_grad(o, eng, w_o, idx)
        w_now = eng.get_weights()
        assert np.abs(w_now - w_o).max() <= 1e-12 * _scale(w_o)
        g2, _ = eng.gradient_f64(idx, w=w_now)
        assert np.array_equal(g.view(np.uint64), g2.view(np.uint64))
        p.destroy()


def test_gradient_f64_of_a_whole_split_at_full_size():
    """one worker's whole split at N = 804,414 with 3 workers: 214,511 rows"""
    data = _data(804414)
    n_train = int(804414 * 0.8)
    split = host.split_vanilla(n_train, 3)
    idx = np.asarray(split[0], dtype=np.int32)
    assert len(idx) == 214511
    o, eng = _pair(data, n_train)
    with eng:
        for w in (_random_w(data.dim), np.zeros(data.dim + 1)):
            eng.set_weights(w)
            _check_grad(o, eng, w, idx)


@pytest.mark.parametrize("n", [100, 4096])
def test_exact_sums_bit_for_bit(n):
    """lambda = 0: s = 0, g = g0 -- each coordinate the correctly rounded sum of the active rows' y * x (math.fsum)"""
    data = _data(100000)
    o, eng = _pair(data, 80000, lam=0.0)
    rng = np.random.default_rng(7 + n)
    idx = rng.integers(0, 80000, size=n).astype(np.int32)
    w = _random_w(data.dim, seed=9)
    with eng:
        eng.set_weights(w)
        g, st = eng.gradient_f64(idx)
    active = [r for r in idx.tolist() if not (data.label[r] * o.row_dot(r, w) < 0)]
    assert st["n_active"] == len(active)
    _check_exact_range(data, np.asarray(active), n)
    cols = np.concatenate([data.col[data.row_ptr[r]:data.row_ptr[r + 1]] for r in active])
    vals = np.concatenate([data.val[data.row_ptr[r]:data.row_ptr[r + 1]].astype(np.float64) * float(data.label[r]) for r in active])
    order = np.argsort(cols, kind="stable")
    cols, vals = cols[order], vals[order]
    want = np.zeros(data.dim + 1)
    bounds = np.flatnonzero(np.diff(cols)) + 1
    for c_, part in zip(cols[np.r_[0, bounds]], np.split(vals, bounds)):
        s = math.fsum(part.tolist())
        want[c_] = s if abs(s) > 1e-20 else 0.0
    assert np.array_equal(g.view(np.uint64), want.view(np.uint64))


def test_order_independence_bit_for_bit():
    data = _data(100000)
    o, eng = _pair(data, 80000)
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 80000, size=3000).astype(np.int32)
    w = _random_w(data.dim, seed=4)
    with eng:
        eng.set_weights(w)
        g, _ = eng.gradient_f64(idx)
        for other in (idx[::-1].copy(), rng.permutation(idx)):
            g2, _ = eng.gradient_f64(other)
            assert np.array_equal(g.view(np.uint64), g2.view(np.uint64))
        dup = np.concatenate([idx, idx[:500]])   # duplicates count twice, as in the oracle
        gd = _check_grad(o, eng, w, dup)
        gd2, _ = eng.gradient_f64(rng.permutation(dup))
        assert np.array_equal(gd.view(np.uint64), gd2.view(np.uint64))


def test_weights_in_either_layout():
    data = _data(100000)
    o, eng = _pair(data, 80000)
    rng = np.random.default_rng(5)
    split = host.split_vanilla(80000, 3)
    steps = [[rng.permutation(np.asarray(r))[:100].astype(np.int32) for r in split] for _ in range(20)]
    idx = rng.integers(0, 80000, size=500).astype(np.int32)
    lists = [rng.integers(0, 80000, size=700).astype(np.int32) for _ in range(5)]
    with eng:
        p = eng.plan(steps)
        eng.plan_run(p, 0, 20, 0.5)
        g_sliced, _ = eng.gradient_f64(idx)            # w = NULL right after a plan run: the slice-major weights
        eng.sync_step_f64(lists, 0.5)                  # ... and a step on them
        w_after_sliced = eng.get_weights()
        # the same from rank order
        eng.set_weights(np.zeros(data.dim + 1))
        eng.plan_run(p, 0, 20, 0.5)
        w_plan = eng.get_weights()
        g_rank, _ = eng.gradient_f64(idx, w=w_plan)
        assert np.array_equal(g_sliced.view(np.uint64), g_rank.view(np.uint64))
        eng.sync_step_f64(lists, 0.5)
        assert np.array_equal(w_after_sliced.view(np.uint64), eng.get_weights().view(np.uint64))
        p.destroy()
        # a call with w leaves exactly those weights resident
        w = _random_w(data.dim, seed=8)
        eng.gradient_f64(idx, w=w)
        assert np.array_equal(eng.get_weights().view(np.uint64), w.view(np.uint64))


@pytest.mark.parametrize("k,rows", [(6, 100), (3, 2000), (3, None)])
def test_sync_step_f64_against_the_oracle(k, rows):
    """20 steps each; rows = None: every worker's whole split at N = 23,149"""
    n_rows = 23149
    n_train = int(n_rows * 0.8)
    data = _data(n_rows)
    o, eng = _pair(data, n_train)
    rng = np.random.default_rng(k)
    split = host.split_vanilla(n_train, k)
    w_o = np.zeros(data.dim + 1)
    with eng:
        for _ in range(20):
            lists = [rng.permutation(np.asarray(r))[:rows].astype(np.int32) for r in split]
            st = eng.sync_step_f64(lists, 0.5)
            o.sync_step(w_o, lists, 0.5)
            assert st["n_active"] == o.last_stats["n_active"]
            assert st["n_samples"] == sum(len(a) for a in lists)
        w = eng.get_weights()
    assert np.abs(w - w_o).max() <= 1e-12 * _scale(w_o)


def test_sync_step_f64_matches_the_plan_path_at_3x100():
    n_rows = 23149
    n_train = int(n_rows * 0.8)
    data = _data(n_rows)
    _, eng = _pair(data, n_train)
    rng = np.random.default_rng(11)
    split = host.split_vanilla(n_train, 3)
    steps = [[rng.permutation(np.asarray(r))[:100].astype(np.int32) for r in split] for _ in range(20)]
    with eng:
        p = eng.plan(steps)
        p.record(True)
        eng.plan_run(p, 0, 20, 0.5)
        mask, _ = p.read_record()
        w_plan = eng.get_weights()
        p.destroy()
        eng.set_weights(np.zeros(data.dim + 1))
        actives = [eng.sync_step_f64(lists, 0.5)["n_active"] for lists in steps]
        w = eng.get_weights()
    plan_actives = [int(mask[s_].sum()) for s_ in range(20)]   # (the gate bits of each step)
    assert actives == plan_actives
    assert np.abs(w - w_plan).max() <= 1e-12 * _scale(w_plan)


def _fit(backend, n_train, n_rows, k, batch, epochs):
    m = host.MasterSync(backend, n_train, n_rows, node_count=k, rnd=host.JavaRandom(0))
    s = m.fit(np.zeros(backend.dp), epochs, batch, 0.5, NEVER)
    return m, s


@pytest.mark.parametrize("k,batch", [(6, 100), (3, 2000), (3, 10000)])
def test_master_sync_fit_beyond_the_plans(k, batch):
    """3 epochs of host.MasterSync.fit at N = 23,149, JavaRandom(0): the plans are refused, the steps run through
    sync_step_f64 (3 x 10,000: batch >= split, the whole split per step)"""
    n_rows = 23149
    n_train = int(n_rows * 0.8)
    data = _data(n_rows)
    o, eng = _pair(data, n_train)
    ref, s_ref = _fit(OracleBackend(o), n_train, n_rows, k, batch, 3)
    with eng:
        m, s = _fit(eng, n_train, n_rows, k, batch, 3)
        w = eng.get_weights()
    assert m.steps_run == ref.steps_run
    assert m.accs == ref.accs and m.test_accs == ref.test_accs
    for a, b in zip(m.losses + m.test_losses, ref.losses + ref.test_losses):
        assert abs(a - b) <= 1e-12 * abs(b)
    assert np.abs(w - s_ref.grad).max() <= 1e-9 * _scale(s_ref.grad)


def test_errors_and_forward():
    data = _data(23149)
    o, eng = _pair(data, 18519)
    idx = np.arange(0, 18519, 5, dtype=np.int32)
    with eng:
        w = _random_w(data.dim, seed=12)
        eng.set_weights(w)
        w_set = eng.get_weights()
        calls = [(lambda: eng.gradient_f64(np.zeros(0, np.int32)), _lib.EINVAL),
                 (lambda: eng.sync_step_f64([], 0.5), _lib.EINVAL),
                 (lambda: eng.sync_step_f64([idx[:10], np.zeros(0, np.int32)], 0.5), _lib.EINVAL),
                 (lambda: eng.gradient_f64(np.asarray([3, 23149], np.int32), w=np.ones(data.dim + 1)), _lib.ERANGE),
                 (lambda: eng.sync_step_f64([idx[:10], np.asarray([-1], np.int32)], 0.5), _lib.ERANGE),
                 (lambda: eng.forward_f64(np.asarray([5, 99999], np.int32), w=np.ones(data.dim + 1)), _lib.ERANGE)]
        for call, code in calls:
            with pytest.raises(_lib.DsgdError) as ei:
                call()
            assert ei.value.code == code, str(ei.value)
        assert "Cannot sum an empty list of vectors" in str(_raises(calls[0][0]))
        assert np.array_equal(eng.get_weights().view(np.uint64), w_set.view(np.uint64))
        pred = eng.forward_f64(idx)
        assert pred.dtype == np.float64 and np.array_equal(pred, o.forward(w_set, idx))
        w2 = _random_w(data.dim, seed=13)
        assert np.array_equal(eng.forward_f64(idx, w=w2), o.forward(w2, idx))
        assert np.array_equal(eng.get_weights().view(np.uint64), w2.view(np.uint64))
        assert len(eng.forward_f64(np.zeros(0, np.int32))) == 0
    with dsgd_amd.Engine(data.dim, LAM) as e32:   # fp32 contexts: DSGD_ESTATE
        e32.load_csr(data.row_ptr, data.col, data.val, data.label)
        e32.build_dim_sparsity(18519)
        for call in (lambda: e32.gradient_f64(idx), lambda: e32.sync_step_f64([idx], 0.5), lambda: e32.forward_f64(idx)):
            with pytest.raises(_lib.DsgdError) as ei:
                call()
            assert ei.value.code == _lib.ESTATE


def _raises(fn):
    try:
        fn()
    except _lib.DsgdError as e:
        return e
    raise AssertionError("no error")


def test_wire_worker_over_an_fp64_engine():
    pytest.importorskip("grpc")
    from dsgd_amd import wire

    data = _data(23149)
    o, eng = _pair(data, 18519)
    with eng:
        worker = wire.SlaveWorker(eng, data.dim).start()
        try:
            stub = wire.Stub(wire.new_channel("127.0.0.1", worker.port), "Slave")
            M = wire.messages()
            rng = np.random.default_rng(21)
            w = _random_w(data.dim, seed=21) + 0.0
            w[w != 0] += 1e-12   # Double values no float32 holds
            idx = rng.permutation(18519)[:400].astype(np.int32)
            reply = stub.Gradient(M["GradientRequest"](weights=wire.to_sparse(w, data.dim), samples=idx.tolist()))
            g_o = o.gradient(w, idx)
            got = np.zeros(data.dim + 1)
            for kk, v in reply.gradUpdate.map.items():
                got[kk] = v
            assert sorted(reply.gradUpdate.map.keys()) == np.flatnonzero(g_o).tolist()
            assert np.abs(got - g_o).max() <= 1e-12 * _scale(g_o)
            fr = stub.Forward(M["ForwardRequest"](weights=wire.to_sparse(w, data.dim), samples=idx.tolist()))
            assert list(fr.predictions) == o.forward(w, idx).tolist()
        finally:
            worker.stop()


@pytest.mark.parametrize("env", [{"DSGD_NODE_COUNT": "6"}, {"DSGD_BATCH_SIZE": "5000"}])
def test_train_fp64_beyond_the_plans(env):
    e = dict(os.environ, DSGD_MAX_EPOCHS="2", **env)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--synthetic", "23149", "--precision", "fp64"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=e, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "final test accuracy" in proc.stdout
