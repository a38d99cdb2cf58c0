"""-m gpu: the fp64 mode (DSGD_F_FP64, csrc/dsgd_cs64.hpp) against the fp64 oracle.

The engine's fp64 context follows the reference's trajectory: the per-worker sums are exact on both sides, only the
summation order of x.w and w.ds differs (~1e-16 relative), so no gate decision may differ and the weights agree at fp64
rounding.  Every check is strict: no waivers."""

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from oracle import oracle as orc
from oracle import ref_dict as rd
from oracle import sync_replay
from oracle_backend import OracleBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
NEVER = lambda losses: False   # (no early stop: every epoch runs)


def _pair(data, n_train, precision="fp64"):
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(n_train))
    eng = dsgd_amd.Engine(data.dim, LAM, precision=precision)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(n_train)
    return o, eng


def _steps(rng, n_train, k, rows, n_steps):
    """n_steps steps of k workers, `rows` rows per step in all (as even as the split allows), Master.scala:184."""
    split = rd.split_vanilla(n_train, k)
    per = [rows // k + (1 if j < rows % k else 0) for j in range(k)]
    return [[rng.permutation(np.asarray(r))[:b].astype(np.int32) for r, b in zip(split, per)] for _ in range(n_steps)]


def _scale(w):
    return max(1.0, float(np.abs(w).max()))


def test_precision_and_dim_sparsity_bit_for_bit():
    data = dsgd_amd.synth.generate(20000, seed=3)
    o, eng = _pair(data, 16000)
    with eng:
        assert eng.precision == "fp64" and eng.precision_bits() == 64
        ds = eng.build_dim_sparsity(16000)
        assert ds.dtype == np.float64
        assert np.array_equal(ds, o.dim_sparsity(16000))
        w32 = eng.get_weights_f32()
        assert w32.dtype == np.float32 and not w32.any()
    with dsgd_amd.Engine(data.dim, LAM) as e32:
        assert e32.precision_bits() == 32
        assert e32._lib.dsgd_get_weights_f64(e32._ctx, _lib.ptr(np.zeros(data.dim + 1))) == _lib.ESTATE


@pytest.mark.parametrize("k,rows", [(1, 1), (1, 100), (3, 300), (4, 800), (4, 960), (2, 74)])
def test_steps_against_the_oracle(k, rows):
    """20-step plans, one launch each: the recorded active count of every step equals the oracle's, the final weights agree
    at fp64 rounding.  (4 x 960: near the layout's 1,024 slots of one slice -- a step of 1,024 rows of these ~75 non-zeros
    needs a few more and is refused when the plan is created.)"""
    data = dsgd_amd.synth.generate(20000, seed=11)
    n_train = 16000
    o, eng = _pair(data, n_train)
    rng = np.random.default_rng(k * 1000 + rows)
    steps = _steps(rng, n_train, k, rows, 20)
    with eng:
        p = eng.plan(steps)
        assert p.info()["kind"] == "column_slices_fp64"
        p.record(True)
        eng.plan_run(p, 0, 20, 0.5)
        eng.synchronize()
        assert eng.grad_kernel_name() == "dsgd_cs64_step_kernel"
        mask, _ = p.read_record()
        w = eng.get_weights()
        p.destroy()
    w_o = np.zeros(data.dim + 1)
    for t, lists in enumerate(steps):
        o.sync_step(w_o, lists, 0.5)
        assert int(mask[t][:rows].sum()) == o.last_stats["n_active"], t
    assert np.abs(w - w_o).max() <= 1e-12 * _scale(w_o)


def test_narrow_model_and_the_lds_boundary():
    rng = np.random.default_rng(5)
    data = dsgd_amd.synth.generate(4000, seed=5, dim=1000)
    o, eng = _pair(data, 3200)
    steps = _steps(rng, 3200, 3, 300, 10)
    with eng:
        p = eng.plan(steps)
        eng.plan_run(p, 0, 10, 0.5)
        w = eng.get_weights()
        p.destroy()
    w_o = np.zeros(data.dim + 1)
    for lists in steps:
        o.sync_step(w_o, lists, 0.5)
    assert np.abs(w - w_o).max() <= 1e-12 * _scale(w_o)
    # the widest model include/dsgd.h states for 4 workers runs; one feature more is refused when the plan is created
    lists = [[np.arange(j * 50, j * 50 + 50, dtype=np.int32) for j in range(4)]]
    for dim, ok in ((50415, True), (50416, False)):
        with dsgd_amd.Engine(dim, LAM, precision="fp64") as e:
            if ok:
                e.plan(lists).destroy()
            else:
                with pytest.raises(_lib.DsgdError) as ei:
                    e.plan(lists)
                assert ei.value.code == _lib.EUNSUPPORTED and "LDS" in str(ei.value)
    wide = dsgd_amd.synth.generate(600, seed=6, dim=50415)
    ow, ew = _pair(wide, 500)
    with ew:
        p = ew.plan(lists)
        ew.plan_run(p, 0, 1, 0.5)
        w = ew.get_weights()
        p.destroy()
    w_o = np.zeros(wide.dim + 1)
    ow.sync_step(w_o, lists[0], 0.5)
    assert np.abs(w - w_o).max() <= 1e-12 * _scale(w_o)


def test_bit_reproducibility():
    data = dsgd_amd.synth.generate(20000, seed=12)
    rng = np.random.default_rng(1)
    steps = _steps(rng, 16000, 3, 300, 20)

    def run(parts):
        _, e = _pair(data, 16000)
        with e:
            p = e.plan(steps)
            for a, b in parts:
                e.plan_run(p, a, b, 0.5)
            w = e.get_weights()
            p.destroy()
        return w

    w1 = run([(0, 20)])
    assert np.array_equal(w1.view(np.uint64), run([(0, 7), (7, 20)]).view(np.uint64))
    assert np.array_equal(w1.view(np.uint64), run([(0, 20)]).view(np.uint64))
    # a one-step dsgd_sync_step against the equivalent plan
    _, e1 = _pair(data, 16000)
    _, e2 = _pair(data, 16000)
    with e1, e2:
        st = e1.sync_step(steps[0], 0.5)
        p = e2.plan(steps[:1])
        e2.plan_run(p, 0, 1, 0.5)
        assert np.array_equal(e1.get_weights().view(np.uint64), e2.get_weights().view(np.uint64))
        assert st["n_samples"] == 300 and 0 <= st["n_active"] <= 300
        p.destroy()


def _fit(backend, n_train, n_rows, k, batch, epochs, record=None):
    m = host.MasterSync(backend, n_train, n_rows, node_count=k, rnd=host.JavaRandom(0))
    s = m.fit(np.zeros(backend.dp), epochs, batch, 0.5, NEVER)
    return m, s


@pytest.mark.parametrize("k,batch", [(3, 100), (4, 200)])
def test_shipped_configurations_ten_epochs(k, batch):
    """application.conf (full = false: N = 23,149, 80 % train, lr 0.5, 3 x 100) and kube/config-sync.yaml (4 x 200),
    10 epochs of host.MasterSync.fit over the fp64 engine and over the oracle, the same java.util.Random(0)."""
    n_rows = 23149
    n_train = int(n_rows * 0.8)
    data = dsgd_amd.synth.generate(n_rows, seed=0)
    o, eng = _pair(data, n_train)
    ob = OracleBackend(o)
    ref, s_ref = _fit(ob, n_train, n_rows, k, batch, 10)
    with eng:
        m, s = _fit(eng, n_train, n_rows, k, batch, 10)
        w = eng.get_weights()
    assert m.accs == ref.accs and m.test_accs == ref.test_accs
    for a, b in zip(m.losses + m.test_losses, ref.losses + ref.test_losses):
        assert abs(a - b) <= 1e-12 * abs(b)
    assert np.abs(w - s_ref.grad).max() <= 1e-9 * _scale(s_ref.grad)


def _replay_epoch(n_rows, k, batch, seed=0):
    """One epoch through the engine's plan with the record on, replayed by the oracle with the engine's own decisions."""
    n_train = int(n_rows * 0.8)
    data = dsgd_amd.synth.generate(n_rows, seed=seed)
    o, eng = _pair(data, n_train)
    split = host.split_vanilla(n_train, k)
    idx, offsets, n_steps = host.epoch_lists(host.JavaRandom(0), split, max(len(r) for r in split), batch)
    steps = [[idx[offsets[s_ * k + j]:offsets[s_ * k + j + 1]] for j in range(k)] for s_ in range(n_steps)]
    with eng:
        p = eng.plan_flat(idx, offsets, n_steps, k)
        p.record(True)
        eng.plan_run(p, 0, n_steps, 0.5)
        mask, _ = p.read_record()
        w = eng.get_weights()
        _, _, counts = eng.loss_acc(n_train, n_rows)
        p.destroy()
    w_r = np.zeros(data.dim + 1)
    stats = sync_replay.replay(o, w_r, steps, 0.5, mask)
    return stats, w, w_r, counts, o.loss_acc(w_r, n_train, n_rows)[2]


@pytest.mark.parametrize("k,batch", [(3, 100), (4, 200)])
def test_shipped_configurations_one_epoch_of_the_full_split(k, batch):
    """N = 804,414, one epoch: where the fp32 engine meets a near-gate row (3 x 100: step 1,252, max |dw| 0.47)."""
    stats, w, w_r, counts, counts_r = _replay_epoch(804414, k, batch)
    assert stats["first_divergent_step"] is None
    assert np.abs(w - w_r).max() <= 1e-9 * _scale(w_r)
    assert list(counts) == list(counts_r)


def test_shipped_configuration_replay_at_23149():
    stats, w, w_r, _, _ = _replay_epoch(23149, 3, 100)
    assert stats["first_divergent_step"] is None
    assert np.abs(w - w_r).max() <= 1e-12 * _scale(w_r)


def test_evaluation_with_fp64_weights():
    data = dsgd_amd.synth.generate(20000, seed=13)
    o, eng = _pair(data, 16000)
    rng = np.random.default_rng(2)
    steps = _steps(rng, 16000, 3, 300, 20)
    with eng:
        p = eng.plan(steps)
        eng.plan_run(p, 0, 20, 0.5)
        w = eng.get_weights()
        p.destroy()
        assert np.array_equal(eng.get_weights_f32(), w.astype(np.float32))
        loss, acc, counts = eng.loss_acc(0, 20000)
        loss_o, acc_o, counts_o, _ = o.loss_acc(w, 0, 20000)
        assert list(counts) == list(counts_o) and acc == acc_o
        assert abs(loss - loss_o) <= 1e-12 * abs(loss_o)
        idx = np.arange(0, 20000, 7, dtype=np.int32)
        assert np.array_equal(eng.forward(idx), o.forward(w, idx).astype(np.float32))


def test_unsupported_entries_change_nothing():
    data = dsgd_amd.synth.generate(20000, seed=14)
    _, eng = _pair(data, 16000)
    with eng:
        w0 = np.random.default_rng(3).normal(scale=0.01, size=data.dim + 1)
        eng.set_weights(w0)
        w_set = eng.get_weights()
        calls = [lambda: eng.sync_step_ranges([(0, 5000), (5000, 10000)], 0.5),
                 lambda: eng.gradient(np.arange(10)),
                 lambda: eng.async_start([(0, 8000), (8000, 16000)], 10, 0.5, 100),
                 lambda: eng.comm_init(b"\0" * _lib.UNIQUE_ID_BYTES, 1, 0),
                 lambda: eng.plan([[np.arange(j, j + 2, dtype=np.int32) for j in range(0, 10, 2)]]),   # K = 5
                 lambda: eng.plan([[np.arange(1025, dtype=np.int32)]])]                                # 1,025 rows
        for call in calls:
            with pytest.raises(_lib.DsgdError) as ei:
                call()
            assert ei.value.code == _lib.EUNSUPPORTED, str(ei.value)
        assert np.array_equal(eng.get_weights().view(np.uint64), w_set.view(np.uint64))


def test_fp32_context_untouched_by_an_fp64_neighbour():
    data = dsgd_amd.synth.generate(20000, seed=15)
    steps = _steps(np.random.default_rng(4), 16000, 3, 300, 10)

    def fp32_run():
        _, e = _pair(data, 16000, precision="fp32")
        with e:
            p = e.plan(steps)
            e.plan_run(p, 0, 10, 0.5)
            w = e.get_weights()
            p.destroy()
        return w

    alone = fp32_run()
    _, e64 = _pair(data, 16000)
    with e64:
        p64 = e64.plan(steps)
        e64.plan_run(p64, 0, 10, 0.5)
        beside = fp32_run()
        e64.synchronize()
        p64.destroy()
    assert np.array_equal(alone.view(np.uint32), beside.view(np.uint32))
