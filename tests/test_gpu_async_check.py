"""-m gpu: the consistent loss check of the asynchronous path (dsgd_async_check / _keep / _weights; csrc/dsgd_snapshot.hpp).
Loss, accuracy, tallies, weights and update window of a check describe ONE snapshot of the weights: on a context at rest
the check IS dsgd_loss_acc + dsgd_get_weights, bit for bit; beside the running lock-free engine the snapshot a check
handed out reproduces the check's tallies and loss on the context at rest afterwards."""

import time

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

N_ROWS, N_TRAIN, LAM = 6000, 4800, 1e-5   # the test range: 1,200 rows, below 4,096 -- dsgd_loss_acc is row-wise there too


@pytest.fixture(scope="module")
def data():
    return dsgd_amd.synth.generate(N_ROWS, seed=44)


def engine_of(data, precision="fp32"):
    eng = dsgd_amd.Engine(data.dim, LAM, precision=precision)
    eng.load_csr(data.row_ptr, data.col, data.val, data.label)
    eng.build_dim_sparsity(N_TRAIN)
    return eng


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def code_of(fn):
    with pytest.raises(dsgd_amd.DsgdError) as ei:
        fn()
    return ei.value.code


def random_weights(dim, seed):
    return (np.random.default_rng(seed).normal(size=dim + 1) * 0.05).astype(np.float32)


def test_quiet_context_the_check_is_loss_acc_and_get_weights(data):
    with engine_of(data) as eng:
        eng.set_weights(random_weights(data.dim, 1))
        loss_ref, acc_ref, counts_ref = eng.loss_acc(N_TRAIN, N_ROWS)
        loss, acc, counts, window = eng.async_check(N_TRAIN, N_ROWS)
        print("quiet: loss %r vs %r, acc %r vs %r, counts %r vs %r, window %r" % (loss, loss_ref, acc, acc_ref, counts, counts_ref, window))
        assert counts == counts_ref and sum(counts) == N_ROWS - N_TRAIN
        assert loss == loss_ref and acc == acc_ref              # (doubles: bit for bit)
        assert np.array_equal(bits(eng.async_check_weights(0)), bits(eng.get_weights()))
        u, running = eng.async_updates()
        assert window == (u, u) and not running
        # the check left the cached scalars dirty, not wrong: the synchronous path goes on as if it had not been there
        assert eng.loss_acc(N_TRAIN, N_ROWS) == (loss_ref, acc_ref, counts_ref)


def test_one_worker_run_to_its_budget(data):
    with engine_of(data) as eng:
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        eng.async_start([(0, N_TRAIN)], batch=100, lr=0.5, max_updates=60, seed=5, positional_bug=True)
        eng.async_wait()
        loss, acc, counts, window = eng.async_check(N_TRAIN, N_ROWS)
        assert window == (60, 60) and eng.async_updates() == (60, False)
        assert np.array_equal(bits(eng.async_check_weights(0)), bits(eng.get_weights()))
        assert (loss, acc, counts) == eng.loss_acc(N_TRAIN, N_ROWS)
        assert np.abs(eng.get_weights()).max() > 0


def test_four_workers_running_every_check_is_of_its_own_snapshot(data):
    max_updates = 4_000_000   # a safety bound: the engine ends by itself after some 15 s
    with engine_of(data) as eng:
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        split = [(r.start, r.stop) for r in host.split_vanilla(N_TRAIN, 4)]
        eng.async_start(split, batch=100, lr=0.5, max_updates=max_updates, seed=3, positional_bug=True)
        checks, snaps = [], []
        try:
            checks.append(eng.async_check(N_TRAIN, N_ROWS))
            u_now, running = eng.async_updates()
            # a check that had waited for the engine would come back to a finished one
            assert running and u_now < max_updates, (u_now, running)
            snaps.append(eng.async_check_weights(0))
            time.sleep(0.02)
            checks.append(eng.async_check(N_TRAIN, N_ROWS))
            snaps.append(eng.async_check_weights(0))
            eng.async_check_keep()
            time.sleep(0.02)
            checks.append(eng.async_check(N_TRAIN, N_ROWS))
            snaps.append(eng.async_check_weights(0))
            best = eng.async_check_weights(1)
        finally:
            eng.async_stop()
        final, running = eng.async_updates()
        assert not running
        print("windows %r, final %d" % ([c[3] for c in checks], final))
        assert np.array_equal(bits(best), bits(snaps[1]))          # the kept one, after the third check has run
        assert not np.array_equal(bits(snaps[0]), bits(snaps[2]))  # the engine did move
        prev_lo = prev_hi = 0
        for (loss, acc, counts, (lo, hi)), v in zip(checks, snaps):
            assert 0 <= lo <= hi <= final and lo >= prev_lo and hi >= prev_hi, (lo, hi, prev_lo, prev_hi, final)
            prev_lo, prev_hi = lo, hi
            # the snapshot is what was evaluated: on the context at rest it gives the check's tallies and loss
            loss_q, acc_q, counts_q = eng.loss_acc(N_TRAIN, N_ROWS, w=v)
            print("check at [%d, %d]: loss %r vs %r, counts %r vs %r" % (lo, hi, loss, loss_q, counts, counts_q))
            assert counts == counts_q and loss == loss_q and acc == acc_q
        assert eng.async_check_weights(1).tobytes() == best.tobytes()   # (still there behind the stop and the loss_acc calls)


class Recording:
    """The engine behind the backend interface, with every check's raw result and the keeps on record."""

    def __init__(self, eng):
        self.eng, self.checks, self.kept = eng, [], []

    def async_check(self, a, b):
        r = self.eng.async_check(a, b)
        self.checks.append(r)
        return r

    def async_check_keep(self):
        self.kept.append(len(self.checks) - 1)
        self.eng.async_check_keep()

    def get_weights(self):
        raise AssertionError("fit read the live weights although DSGD_ASYNC_SNAPSHOT=1")

    def __getattr__(self, name):
        return getattr(self.eng, name)


def test_master_async_fit_returns_the_weights_its_best_loss_is_of(data, monkeypatch):
    """What test_master_async_fit_four_workers_learns_and_stops_at_the_budget cannot say: the GradState's weights HAVE the
    loss the best check computed.  The raw loss of that check (on record; the leaky average is also undone as
    test_gpu_host.py:180-182 undoes it -- that direction rounds, so it is held to 1e-12) equals loss_acc of st.grad."""
    monkeypatch.setenv("DSGD_ASYNC_SNAPSHOT", "1")
    leak = 0.9
    with engine_of(data) as eng:
        rec = Recording(eng)
        m = host.MasterAsync(rec, N_TRAIN, N_ROWS, node_count=4)
        st = m.fit(np.zeros(data.dim + 1), max_epoch=1, batch_size=100, learning_rate=0.5,
                   stopping_criterion=lambda losses: False, check_every=100, leak_loss_coef=leak, max_steps=1500,
                   positional_bug=True)
        assert rec.checks and rec.kept and len(rec.checks) == len(m.test_losses)
        i = rec.kept[-1]
        smooth = m.test_losses[::-1]
        assert smooth[i] == min(smooth) == st.loss
        raw_best = rec.checks[i][0]
        loss_q, acc_q, counts_q = eng.loss_acc(N_TRAIN, N_ROWS, w=st.grad)
        undone = smooth[i] if i == 0 else (smooth[i] - (1 - leak) * smooth[i - 1]) / leak
        print("best check %d of %d: raw %r, undone %r, loss_acc(st.grad) %r" % (i, len(smooth), raw_best, undone, loss_q))
        assert raw_best == loss_q and rec.checks[i][2] == counts_q and rec.checks[i][1] == acc_q
        assert abs(undone - loss_q) <= 1e-12
        # the leaky average forwards, in fit's own arithmetic, is exact
        assert smooth[i] == leak * loss_q + (1 - leak) * (smooth[i - 1] if i else loss_q)
        assert 100 <= st.updates <= 1500 + 3 and np.isfinite(st.grad).all()


def test_refusals(data):
    with engine_of(data, precision="fp64") as eng:
        assert code_of(lambda: eng.async_check(N_TRAIN, N_ROWS)) == _lib.EUNSUPPORTED
        assert code_of(eng.async_check_keep) == _lib.ESTATE
    with engine_of(data) as eng:
        assert code_of(eng.async_check_keep) == _lib.ESTATE
        assert code_of(lambda: eng.async_check_weights(0)) == _lib.ESTATE
        assert code_of(lambda: eng.async_check_weights(1)) == _lib.ESTATE
        assert code_of(lambda: eng.async_check(N_TRAIN, N_TRAIN)) == _lib.EINVAL
        assert code_of(lambda: eng.async_check(N_TRAIN, N_ROWS + 1)) == _lib.ERANGE
        assert code_of(lambda: eng.async_check(-1, N_ROWS)) == _lib.ERANGE
        assert code_of(lambda: eng.async_check_weights(2)) == _lib.EINVAL
        assert code_of(eng.async_check_keep) == _lib.ESTATE            # (the refused checks left nothing)
        eng.async_check(N_TRAIN, N_ROWS)
        assert code_of(lambda: eng.async_check_weights(1)) == _lib.ESTATE   # a check, but nothing kept
        eng.async_check_keep()
        eng.async_check_weights(1)
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)          # the internal column order goes: both dropped
        assert code_of(lambda: eng.async_check_weights(0)) == _lib.ESTATE
        assert code_of(lambda: eng.async_check_weights(1)) == _lib.ESTATE
        assert code_of(eng.async_check_keep) == _lib.ESTATE
        # a communicator, even of one rank: dsgd_loss_acc is the call that sums over ranks
        w = eng.get_weights()
        eng.comm_init(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        assert code_of(lambda: eng.async_check(N_TRAIN, N_ROWS)) == _lib.EUNSUPPORTED
        assert np.array_equal(bits(eng.get_weights()), bits(w))
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        assert code_of(lambda: eng.async_check(0, 10)) == _lib.ESTATE       # no data
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        assert code_of(lambda: eng.async_check(0, 10)) == _lib.ESTATE       # no dimSparsity


def test_reload_a_fresh_check_works_again(data):
    other = dsgd_amd.synth.generate(5000, seed=45)
    with engine_of(data) as eng:
        eng.set_weights(random_weights(data.dim, 2))
        eng.async_check(N_TRAIN, N_ROWS)
        eng.async_check_keep()
        eng.load_csr(other.row_ptr, other.col, other.val, other.label)
        eng.build_dim_sparsity(4000)
        w = random_weights(data.dim, 3)
        eng.set_weights(w)
        loss, acc, counts, window = eng.async_check(4000, 5000)
        assert (loss, acc, counts) == eng.loss_acc(4000, 5000)
        assert np.array_equal(bits(eng.async_check_weights(0)), bits(eng.get_weights()))
        assert code_of(lambda: eng.async_check_weights(1)) == _lib.ESTATE   # the kept one belonged to the old order
        eng.async_check_keep()
        assert np.array_equal(bits(eng.async_check_weights(1)), bits(eng.get_weights()))
