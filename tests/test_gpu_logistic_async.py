"""GPU: the logistic model's asynchronous iteration (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS; csrc/dsgd_logistic.hpp:
dsgd_lg_async_finish_kernel, dsgd_lg_update_kernel; csrc/dsgd_lg_cs_async.hpp: dsgd_lg_cs_async_kernel).

Per call against the fp64 reference tests/logistic_async_ref.py inside tests/logistic_async_bound.py (derived from the operation
order; tests/test_logistic_async_bound.py shows what it is worth on these very lists), and EXACTLY on the host: float32(float64(w) -
delta) is the new weight, bit for bit.  Bit equalities wherever the order is the same: one row against the synchronous step of one
worker, a peer that applies the delta, a plan against the per-call sequence, split runs against whole runs.  The slice form is held
to its own bound and to its own determinism.  Only well-formed plans run: the abort path is not driven here.

The refusal under a communicator runs on real RCCL at world = 1, as tests/test_gpu_logistic_ranks.py attaches one."""

import functools

import numpy as np
import pytest

import dsgd_amd
import logistic_async_bound as ab
import logistic_async_cases as ac
import logistic_async_ref as aref
import logistic_bound as lb
import logistic_cases as cases
import logistic_hard_cases as hard
import logistic_ref as ref
from dsgd_amd import _lib, host

pytestmark = pytest.mark.gpu

LAM = cases.LAM
LR = ac.LR
N2 = 2000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine(csr, dim, lam=LAM, **kw):
    eng = dsgd_amd.Engine(dim, lam, **kw)
    eng.load_csr(*csr)
    return eng


@pytest.fixture(scope="module")
def eng():
    with engine(cases.csr(), cases.data().dim) as e:
        yield e


@functools.lru_cache(maxsize=None)
def data2():
    d = dsgd_amd.synth.generate(N2, seed=13)
    return (d.row_ptr, d.col, d.val, d.label), d.dim


def one_update_against_the_reference(e, csr, w0, idx, lr, lam, n_rows, what):
    e.set_weights(w0)
    delta, st = e.lg_async_step(idx, lr, want_delta=True)
    w1 = e.get_weights()
    assert st["n_samples"] == st["n_active"] == len(idx), (what, st)
    assert e.grad_kernel_name() == "dsgd_lg_grad_kernel"
    dw, dd, w_ref, d_ref = ab.dstep(csr, w0, idx, lr, lam)
    ew, ed = np.abs(w1.astype(np.float64) - w_ref), np.abs(delta - d_ref)
    print("%s: worst |w - ref| / bound = %.3f, |delta - ref| / bound = %.3f" % (what, float(np.max(ew / dw)), float(np.max(ed / dd))))
    assert np.all(ew <= dw) and np.all(ed <= dd), what
    # exactly, on the host: the one rounding to float, every coordinate
    assert np.array_equal(bits((np.asarray(w0, dtype=np.float32).astype(np.float64) - delta).astype(np.float32)), bits(w1)), what
    # the evaluation behind it reads the |w'|^2 words the finish left
    loss, acc = e.lg_loss_acc(0, n_rows)
    want = ref.loss_acc(csr, w1.astype(np.float64), 0, n_rows, lam)
    assert abs(loss - want[0]) <= lb.dloss(csr, w1, 0, n_rows, lam), what
    unsure = int(np.count_nonzero(np.abs(want[3]) <= lb.dz(csr, w1)[:n_rows]))
    assert abs(acc - want[1]) * n_rows <= unsure, what
    return w1, delta


# ---- 1. per call, against the reference ----
PER_CALL = [("logits 1", n) for n in ac.lists()] + [("tiny", "100"), ("logits 8", "17")]


@pytest.mark.parametrize("wname,lname", PER_CALL)
def test_one_update_inside_the_bound_and_exact_on_the_host(eng, wname, lname):
    one_update_against_the_reference(eng, cases.csr(), ac.weight_sets()[wname], ac.lists()[lname], LR, LAM, cases.N, "%s, %s rows" % (wname, lname))


@pytest.mark.parametrize("dim", ac.WIDTHS)
def test_hard_widths(dim):
    c = hard.width(dim)
    with engine(c.csr, dim, c.lam) as e:
        for name, idx in ac.width_lists(dim).items():
            w1, delta = one_update_against_the_reference(e, c.csr, c.w, idx, LR, c.lam, hard.W_ROWS, "dim %d, %s rows" % (dim, name))
            if dim in hard.W_FULL and name == "37":   # the row of every key: the columns of the edge ranks moved by data
                rank = lb.ranks_of(c.csr, dim + 1)
                for r in hard.W_EDGE_RANKS[dim]:
                    k = int(np.where(rank == r)[0][0])
                    assert delta[k] != LR * ((2.0 * c.lam) * float(c.w[k])), (dim, r)   # (more than the regulariser alone)


# ---- 2. one row: the synchronous step of one worker, bit for bit ----
def test_one_row_is_the_synchronous_step(eng):
    w0 = cases.weights(1.0)
    for r in (0, 7, 1234, 4095):
        eng.set_weights(w0)
        eng.lg_async_step([r], LR)
        a = eng.get_weights()
        eng.set_weights(w0)
        eng.lg_sync_step([[r]], LR)
        assert np.array_equal(bits(a), bits(eng.get_weights())), r
        assert np.any(bits(a) != bits(w0))


# ---- 3. the |w|^2 words ----
def test_norm_words_after_an_update_and_after_a_peers_update(eng):
    w0 = cases.weights(1.0)
    eng.set_weights(w0)
    delta, _ = eng.lg_async_step(ac.lists()["100"], LR, want_delta=True)
    la = eng.lg_loss_acc(0, cases.N)
    eng.set_weights(eng.get_weights())
    assert la == eng.lg_loss_acc(0, cases.N)
    eng.lg_update_grad(np.arange(len(w0), dtype=np.int32), delta)   # (after an evaluation that left fresh words: they must go stale)
    lb_ = eng.lg_loss_acc(0, cases.N)
    eng.set_weights(eng.get_weights())
    assert lb_ == eng.lg_loss_acc(0, cases.N) and lb_ != la
    eng.lg_update_grad(np.zeros(0, dtype=np.int32), np.zeros(0))     # nnz == 0: a no-op
    assert lb_ == eng.lg_loss_acc(0, cases.N)


# ---- 4. three replicas that gossip every delta ----
def test_three_replicas_and_a_plan_stay_bit_identical():
    csr, dim = data2()
    dp = dim + 1
    split = aref.split_vanilla(1600, 3)
    lists = aref.schedule_lists(split, 100, 9, True, 0, 6)
    w0 = (np.random.default_rng(1).standard_normal(dp) * 0.05).astype(np.float32)
    keys = np.arange(dp, dtype=np.int32)
    with engine(csr, dim) as a, engine(csr, dim) as b, engine(csr, dim) as c, engine(csr, dim) as solo:
        reps = [a, b, c]
        for e in reps + [solo]:
            e.set_weights(w0)
        for u, idx in enumerate(lists):
            delta, _ = reps[u % 3].lg_async_step(idx, LR, want_delta=True)
            for j in range(3):
                if j != u % 3:
                    reps[j].lg_update_grad(keys[::-1] if u % 2 else keys, delta[::-1] if u % 2 else delta)   # (any key order)
            ws = [e.get_weights() for e in reps]
            assert np.array_equal(bits(ws[0]), bits(ws[1])) and np.array_equal(bits(ws[0]), bits(ws[2])), u
        flat = np.concatenate(lists)
        offs = np.arange(7, dtype=np.int64) * 100
        plan = solo.lg_plan_flat(flat, offs, 6, 1)
        solo.plan_run_async_lg(plan, 0, 6, LR)
        st = solo.synchronize()
        assert st["n_samples"] == st["n_active"] == 600
        plan.destroy()
        assert np.array_equal(bits(solo.get_weights()), bits(ws[0])) and np.any(bits(ws[0]) != bits(w0))
        # keys are checked on the host first: nothing moves
        for bad_keys, code in (([0, 5, 5], _lib.EINVAL), ([0, dp, 1], _lib.ERANGE), ([-1, 2, 3], _lib.ERANGE)):
            with pytest.raises(_lib.DsgdError) as ei:
                a.lg_update_grad(np.asarray(bad_keys, dtype=np.int32), np.ones(3))
            assert ei.value.code == code
            assert np.array_equal(bits(a.get_weights()), bits(ws[0]))


# ---- 5. plans, row form ----
@pytest.mark.parametrize("bug,first,batch", [(1, 0, 16), (0, 0, 16), (1, 37, 16), (0, 5, 1), (1, 0, 1030)])
def test_device_drawn_lists_are_the_schedule(bug, first, batch):
    csr, dim = data2()
    split = aref.split_vanilla(1600, 3)
    with engine(csr, dim) as e:
        plan = e.lg_async_plan(split, batch, seed=77, positional_bug=bool(bug), first_update=first, n_updates=11)
        assert plan.info()["kind"] == "logistic"
        idx, offs = e.plan_lists(plan)
        plan.destroy()
    want = aref.schedule_lists(split, batch, 77, bug, first, 11)
    assert np.array_equal(offs, np.arange(12) * batch) and np.array_equal(idx, np.concatenate(want))


def test_whole_split_per_call_and_a_callers_plan_give_the_same_bits():
    csr, dim = data2()
    split = aref.split_vanilla(1600, 3)
    n_up = 9
    lists = aref.schedule_lists(split, 16, 3, True, 4, n_up)
    w0 = np.zeros(dim + 1, dtype=np.float32)
    with engine(csr, dim) as e:
        plan = e.lg_async_plan(split, 16, seed=3, positional_bug=True, first_update=4, n_updates=n_up)
        e.set_weights(w0)
        e.plan_run_async_lg(plan, 0, n_up, LR)
        assert e.synchronize()["n_samples"] == 16 * n_up
        whole = e.get_weights()
        la = e.lg_loss_acc(0, N2)            # (the last finish left the |w'|^2 words)
        e.set_weights(whole)
        assert la == e.lg_loss_acc(0, N2)
        for cuts in ((1,), (3, 4, 8)):
            e.set_weights(w0)
            at = 0
            for cut in cuts + (n_up,):
                e.plan_run_async_lg(plan, at, cut, LR)
                at = cut
            e.plan_run_async_lg(plan, 2, 2, LR)   # (an empty range changes nothing)
            e.synchronize()
            assert np.array_equal(bits(e.get_weights()), bits(whole)), cuts
        plan.destroy()
        e.set_weights(w0)
        for idx in lists:
            e.lg_async_step(idx, LR)
        assert np.array_equal(bits(e.get_weights()), bits(whole)) and np.any(whole != 0)
        # a caller's one-worker plan, its lists of unequal lengths
        own = [lists[0], lists[1][:5], lists[2][:1], np.concatenate(lists[3:6])]
        mine = e.lg_plan_flat(np.concatenate(own), np.concatenate([[0], np.cumsum([len(x) for x in own])]).astype(np.int64), len(own), 1)
        e.set_weights(w0)
        e.plan_run_async_lg(mine, 0, len(own), LR)
        e.synchronize()
        got = e.get_weights()
        e.set_weights(w0)
        for idx in own:
            e.lg_async_step(idx, LR)
        assert np.array_equal(bits(e.get_weights()), bits(got))
        # dsgd_plan_run on the same plan keeps meaning the synchronous step
        e.set_weights(w0)
        e.plan_run(mine, 0, len(own), LR)
        e.synchronize()
        sync = e.get_weights()
        e.set_weights(w0)
        for idx in own:
            e.lg_sync_step([idx], LR)
        assert np.array_equal(bits(e.get_weights()), bits(sync)) and np.any(bits(sync) != bits(got))
        mine.destroy()


# ---- 6. plans, slice form ----
def test_slices_deterministic_split_and_inside_their_bound():
    csr, dim = data2()
    split = aref.split_vanilla(1600, 3)
    n_up = 50
    lists = aref.schedule_lists(split, 100, 21, True, 0, n_up)
    w0 = np.zeros(dim + 1, dtype=np.float32)
    with engine(csr, dim) as e:
        plan = e.lg_async_plan(split, 100, seed=21, positional_bug=True, first_update=0, n_updates=n_up, slices=True)
        info = plan.info()
        assert info["kind"] == "logistic_column_slices" and info["slices"] == 16, info
        idx, _ = e.plan_lists(plan)
        assert np.array_equal(idx, np.concatenate(lists))
        runs = []
        for cuts in ((), (), (1, 20, 49)):
            e.set_weights(w0)
            at = 0
            for cut in cuts + (n_up,):
                e.plan_run_async_lg(plan, at, cut, LR)
                at = cut
            st = e.synchronize()
            assert st["n_samples"] == st["n_active"] == 100 * n_up and e.grad_kernel_name() == "dsgd_lg_cs_async_kernel"
            runs.append(e.get_weights())
        assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.array_equal(bits(runs[0]), bits(runs[2]))
        la = e.lg_loss_acc(0, N2)                 # straight behind the run: |w|^2 is computed, not taken from stale words
        e.set_weights(runs[0])
        assert la == e.lg_loss_acc(0, N2)
        # every coordinate after 50 updates within the carried slice bound of the fp64 reference
        w_ref, E = w0.astype(np.float64), np.zeros(dim + 1)
        for lst in lists:
            E, _, w_ref, _ = ab.dstep(csr, w_ref, lst, LR, LAM, E, slices=True)
        err = np.abs(runs[0].astype(np.float64) - w_ref)
        print("slices, 50 updates of 100 rows: worst err / carried bound = %.3f" % float(np.max(err / E)))
        assert np.all(err <= E) and np.any(runs[0] != 0)
        # the synchronous run of the same plan is another arithmetic: dsgd_plan_run keeps its meaning
        e.set_weights(w0)
        e.plan_run(plan, 0, 3, LR)
        e.synchronize()
        assert e.grad_kernel_name() == "dsgd_lg_cs_step_kernel"
        plan.destroy()
        with pytest.raises(_lib.DsgdError) as ei:                      # a batch beyond the slices' 1,024 rows is refused at creation
            e.lg_async_plan(split, 1025, n_updates=2, slices=True)
        assert ei.value.code == _lib.EUNSUPPORTED
        e.lg_async_plan(split, 1025, n_updates=2).destroy()           # (the row form takes any batch)
    c = hard.width(300000)                                             # 3 words of LDS per column: 16 slices cannot hold it
    with engine(c.csr, c.dim, c.lam) as wide:
        with pytest.raises(_lib.DsgdError) as ei:
            wide.lg_async_plan([(0, 300), (300, 600)], 16, n_updates=2, slices=True)
        assert ei.value.code == _lib.EUNSUPPORTED
        wide.lg_async_plan([(0, 300), (300, 600)], 16, n_updates=2).destroy()


@functools.lru_cache(maxsize=None)
def narrow():
    """1,100 rows of 8 entries over 128 keys: whatever the ranking, a row has at most 8 entries in a slice -- one slot -- so a step of
    1,024 rows is at most 1,024 slots and 8 columns per row in every slice: inside the slice builder's limits BY CONSTRUCTION.  (On
    the synthetic rows of ~75 entries a step of 1,024 rows declines to the row form as soon as one row has 17 entries in one slice.)"""
    rng = np.random.default_rng(31)
    n, dp, k = 1100, 128, 8
    col = np.concatenate([np.sort(rng.choice(dp, size=k, replace=False)) for _ in range(n)]).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, size=n * k).astype(np.float32)
    label = rng.choice(np.array([-1, 1], dtype=np.int8), size=n)
    return (np.arange(n + 1, dtype=np.int64) * k, col, val, label), dp - 1


def test_the_largest_batch_runs_on_the_slices():
    csr, dim = narrow()
    split = aref.split_vanilla(1050, 3)
    lr = 2.0 ** -2
    lists = aref.schedule_lists(split, 1024, 6, False, 0, 3)
    w0 = (np.random.default_rng(4).standard_normal(dim + 1) * 0.25).astype(np.float32)
    with engine(csr, dim, 1e-3) as e:
        plan = e.lg_async_plan(split, 1024, seed=6, positional_bug=False, first_update=0, n_updates=3, slices=True)
        info = plan.info()
        assert info["kind"] == "logistic_column_slices" and info["slices"] == 16 and info["device_built"], info
        e.set_weights(w0)
        e.plan_run_async_lg(plan, 0, 3, lr)
        assert e.synchronize()["n_samples"] == 3072 and e.grad_kernel_name() == "dsgd_lg_cs_async_kernel"
        got = e.get_weights()
        plan.destroy()
    w_ref, E = w0.astype(np.float64), np.zeros(dim + 1)
    for lst in lists:
        E, _, w_ref, _ = ab.dstep(csr, w_ref, lst, lr, 1e-3, E, slices=True)
    err = np.abs(got.astype(np.float64) - w_ref)
    print("slices, 3 updates of 1,024 rows: worst err / carried bound = %.3f" % float(np.max(err / E)))
    assert np.all(err <= E) and np.any(bits(got) != bits(w0))


# ---- 7. refusals: nothing enqueued, nothing changed ----
def test_refusals_leave_the_weights():
    csr, dim = data2()
    w0 = (np.random.default_rng(2).standard_normal(dim + 1) * 0.05).astype(np.float32)
    rows = np.arange(32, dtype=np.int32)
    offs2 = np.array([0, 16, 32], dtype=np.int64)
    with engine(csr, dim) as e:
        e.set_weights(w0)
        two = e.lg_plan_flat(rows, offs2, 1, 2)
        svm = e.plan([[rows[:16], rows[16:]]])
        for call, code in ((lambda: e.plan_run_async_lg(two, 0, 1, LR), _lib.EINVAL), (lambda: e.plan_run_async_lg(svm, 0, 1, LR), _lib.EUNSUPPORTED),
                           (lambda: e.lg_async_step(np.zeros(0, dtype=np.int32), LR), _lib.EINVAL),
                           (lambda: e.lg_async_step([N2], LR), _lib.ERANGE),
                           (lambda: e.lg_async_plan([(0, N2 + 1)], 4), _lib.ERANGE)):
            with pytest.raises(_lib.DsgdError) as ei:
                call()
            assert ei.value.code == code
            assert np.array_equal(bits(e.get_weights()), bits(w0))
        two.destroy()
        svm.destroy()
    with engine(csr, dim, precision="fp64") as e64:
        e64.set_weights(w0.astype(np.float64))
        for call in (lambda: e64.lg_async_step(rows, LR), lambda: e64.lg_update_grad(rows, np.ones(32)), lambda: e64.lg_async_plan([(0, 100)], 4),
                     lambda: e64.lg_async_plan([(0, 100)], 4, slices=True)):
            with pytest.raises(_lib.DsgdError) as ei:
                call()
            assert ei.value.code == _lib.EUNSUPPORTED
        assert np.array_equal(e64.get_weights(), w0.astype(np.float64))


def test_refusals_under_a_communicator_of_comm_init_lg():
    """real RCCL, one rank: the schedule is one process's, so all five entry points are refused while it is attached"""
    csr, dim = data2()
    w0 = (np.random.default_rng(3).standard_normal(dim + 1) * 0.05).astype(np.float32)
    rows = np.arange(16, dtype=np.int32)
    with engine(csr, dim) as e:
        e.set_weights(w0)
        mine = e.lg_plan_flat(rows, np.array([0, 16], dtype=np.int64), 1, 1)
        e.comm_init_lg(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        try:
            for call in (lambda: e.lg_async_step(rows, LR), lambda: e.lg_update_grad(rows, np.ones(16)), lambda: e.lg_async_plan([(0, 100)], 4),
                         lambda: e.lg_async_plan([(0, 100)], 4, slices=True), lambda: e.plan_run_async_lg(mine, 0, 1, LR)):
                with pytest.raises(_lib.DsgdError) as ei:
                    call()
                assert ei.value.code == _lib.EUNSUPPORTED
                assert np.array_equal(bits(e.get_weights()), bits(w0))
        finally:
            e.comm_destroy()
        e.plan_run_async_lg(mine, 0, 1, LR)   # local again
        assert e.synchronize()["n_samples"] == 16 and np.any(bits(e.get_weights()) != bits(w0))
        mine.destroy()


# ---- 8. the mirror ----
@pytest.mark.parametrize("slices", [False, True])
def test_logistic_async_fit_follows_the_reference_replay(slices):
    csr, dim = data2()
    n_train, K, batch, steps, every, leak = 1600, 3, 16, 240, 50, 0.5
    w0 = np.zeros(dim + 1, dtype=np.float32)
    never = lambda losses: False
    E_at = {0: np.zeros(dim + 1)}

    def carry(u, w, idx):
        E_at[u + 1] = ab.dstep(csr, w, idx, LR, LAM, E_at[u], slices=slices)[0]

    want = aref.fit(csr, w0, n_train, N2, K, 1, batch, LR, LAM, never, every, leak, seed=4, max_steps=steps, on_update=carry)
    with engine(csr, dim) as e:
        m = host.LogisticAsync(e, n_train, N2, K, slices=slices)
        m.CHUNK = 100   # (several plans in 240 updates)
        state = m.fit(w0, 1, batch, LR, never, every, leak, seed=4, max_steps=steps)
        if slices:
            assert e.grad_kernel_name() == "dsgd_lg_cs_async_kernel"
    assert state.updates == want["updates"] == steps and m.checks == want["checks"] == 6
    best = int(np.argmin(want["test_losses"][::-1]))
    assert int(np.argmin(m.test_losses[::-1])) == best and state.loss == min(m.test_losses)
    E = E_at[want["check_at"][best]]
    err = np.abs(state.grad.astype(np.float64) - want["best_w"])
    print("mirror (slices=%s): best at check %d, worst err / carried bound = %.3f" % (slices, best, float(np.max(err / np.maximum(E, 1e-300)))))
    assert np.all(err <= E)
