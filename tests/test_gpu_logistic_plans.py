"""GPU: resident logistic plans, device-drawn lists, the several-ranges evaluation and the training mirror (include/dsgd.h "THE
LOGISTIC MODEL": RESIDENT PLANS, dsgd_lg_loss_acc_ranges; host.LogisticSync).

What is new is held to what was there: a plan's steps to the bits of dsgd_lg_sync_steps and of dsgd_lg_sync_step on the same
lists (and ONE step to the fp64 reference tests/logistic_ref.py within tests/logistic_bound.py's dw, exactly as
tests/test_gpu_logistic.py holds dsgd_lg_sync_step: no new tolerance), the device-drawn lists to csrc/jrand.c's entry for entry,
every range of dsgd_lg_loss_acc_ranges to the bits of dsgd_lg_loss_acc on that range alone, the mirror's figures to calls made
by hand.  Shapes: 600 rows (row 7 emptied), lists of 1 .. 100 rows; 20,000 rows where the evaluation's persistent workgroups
must take a second pass (more than 64 rows per workgroup of at most 256)."""

import ctypes as C
import functools

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_ref as ref
from dsgd_amd import _lib, host

pytestmark = pytest.mark.gpu

LAM = 1e-5
LR = 2.0 ** -3
N = 600
EMPTY_ROW = 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dbits(pairs):
    return np.asarray(pairs, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def data(n=N, seed=13):
    """n synthetic rows; row 7 has no entry."""
    d = dsgd_amd.synth.generate(n, seed=seed)
    a, b = int(d.row_ptr[EMPTY_ROW]), int(d.row_ptr[EMPTY_ROW + 1])
    row_ptr = d.row_ptr.copy()
    row_ptr[EMPTY_ROW + 1:] -= b - a
    return dsgd_amd.synth.Csr(d.dim, row_ptr, np.delete(d.col, np.s_[a:b]), np.delete(d.val, np.s_[a:b]), d.label)


def csr_of(d):
    return (d.row_ptr, d.col, d.val, d.label)


def engine(d=None, **kw):
    d = d or data()
    eng = dsgd_amd.Engine(d.dim, LAM, **kw)
    eng.load_csr(*csr_of(d))
    return eng


@functools.lru_cache(maxsize=None)
def steps_of(K, n_steps=4):
    """n_steps steps x K workers.  Worker k of step t lists LENS[(t + k) % 5] rows: the lengths 1, 3 and 17 meet in one step (three
    shifts); a 1-row list; the 3-row lists name a row twice; the 17-row lists (two workgroups of 16 rows) start with the empty row."""
    lens = (1, 3, 17, 37, 100)
    rng = np.random.default_rng(100 + K)
    steps = []
    for t in range(n_steps):
        lists = []
        for k in range(K):
            n = lens[(t + k) % 5]
            a = rng.integers(0, N, size=n).astype(np.int32)
            if n == 3:
                a[2] = a[0]
            if n == 17:
                a[0] = EMPTY_ROW
            lists.append(a)
        steps.append(lists)
    return steps


def flat_of(steps):
    lists = [a for s in steps for a in s]
    return np.concatenate(lists), np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)


def zeros(d):
    return np.zeros(d.dim + 1, dtype=np.float32)


# ---- 1. a plan's steps are the calls' steps ----
def test_plan_steps_equal_the_call_steps():
    d = data()
    with engine() as eng:
        for K in (1, 3, 5):   # (5 after 3 on one context: the accumulators regrow past their capacity of 4)
            steps = steps_of(K)
            n = len(steps)
            idx, offs = flat_of(steps)
            total = len(idx)
            # the calls that were there: all steps in one call, and step by step
            eng.set_weights(zeros(d))
            eng.lg_sync_steps(idx, offs, n, K, LR)
            w_steps = eng.get_weights()
            eng.lg_sync_steps(idx, offs, n, K, LR)
            w_twice = eng.get_weights()
            eng.set_weights(zeros(d))
            for s in steps:
                eng.lg_sync_step(s, LR)
            assert np.array_equal(bits(eng.get_weights()), bits(w_steps)), K
            assert np.any(w_steps != 0) and not np.array_equal(bits(w_steps), bits(w_twice))
            # the plan
            plan = eng.lg_plan(steps)
            try:
                info = plan.info()
                assert info["kind"] == "logistic" and info["slices"] == info["slot_stride"] == info["row_stride"] == info["col_list_stride"] == 0
                got_idx, got_offs = eng.plan_lists(plan)
                assert np.array_equal(got_idx, idx) and np.array_equal(got_offs, offs)
                eng.set_weights(zeros(d))
                eng.plan_run(plan, 0, n, LR)
                st = eng.synchronize()
                assert st["n_samples"] == st["n_active"] == total, (K, st)
                assert np.array_equal(bits(eng.get_weights()), bits(w_steps)), K
                # ... a second time: its lists twice
                eng.plan_run(plan, 0, n, LR)
                assert np.array_equal(bits(eng.get_weights()), bits(w_twice)), K
                assert eng.synchronize()["n_samples"] == total
                # ... in two parts
                eng.set_weights(zeros(d))
                eng.plan_run(plan, 0, 2, LR)
                eng.plan_run(plan, 2, n, LR)
                st = eng.synchronize()
                assert st["n_samples"] == st["n_active"] == total
                assert np.array_equal(bits(eng.get_weights()), bits(w_steps)), K
                # ... and an empty range of steps changes nothing
                eng.plan_run(plan, 1, 1, LR)
                assert eng.synchronize()["n_samples"] == 0
                assert np.array_equal(bits(eng.get_weights()), bits(w_steps))
                assert eng.grad_kernel_name() == "dsgd_lg_grad_kernel"
            finally:
                plan.destroy()
        eng.synchronize()
        assert eng.cache_trim(0) == 0   # (the launch stream is idle) the plans' blocks went back to the cache, and leave it


# ---- 2. one step of a plan against the fp64 reference, within the derived bound of dsgd_lg_sync_step ----
def test_a_one_step_plan_within_dw():
    d = data()
    csr = csr_of(d)
    lists = steps_of(3)[0]   # 1, 3 and 17 rows
    more = steps_of(5)[2]    # 17, 37, 100, 1, 3 rows
    with engine() as eng:
        for ls, w0 in ((lists, zeros(d)), (more, None)):
            if w0 is not None:
                eng.set_weights(w0)
            w_before = eng.get_weights()
            plan = eng.lg_plan([ls])
            eng.plan_run(plan, 0, 1, LR)
            plan.destroy()
            w_gpu = eng.get_weights()
            err = np.abs(w_gpu.astype(np.float64) - ref.sync_step(csr, w_before, ls, LR, LAM))
            bound = lb.dw(csr, w_before, ls, LR, LAM)
            print("one-step plan of %d workers: max err/bound %.3f" % (len(ls), float(np.max(err / bound))))
            assert np.all(err <= bound)


# ---- 3. lists the device draws ----
@pytest.mark.parametrize("n_splits,batch", [(3, 100), (2, 7)])
def test_device_drawn_lists(n_splits, batch):
    d = data()
    n_train = 300
    split = host.split_vanilla(n_train, n_splits)
    max_samples = max(len(r) for r in split)
    rnd = host.JavaRandom(0)
    seed0 = rnd.seed
    idx, offs, n_steps = host.epoch_lists(rnd, split, max_samples, batch, native=True)   # csrc/jrand.c
    assert n_steps == len(range(0, max_samples, batch)) and (batch != 7 or offs[-1] - offs[-2] == max_samples % 7)
    with engine() as eng, engine() as other:
        plan, got_steps, state, draws = eng.lg_plan_from_seed(seed0, split, max_samples, batch)
        try:
            assert plan.info()["kind"] == "logistic"
            got_idx, got_offs = eng.plan_lists(plan)
            assert got_steps == n_steps and np.array_equal(got_offs, offs) and np.array_equal(got_idx, idx)
            assert state == rnd.seed
            # what dsgd_plan_create_from_seed returns for the same arguments, on a second context
            p2, steps2, state2, draws2 = other.plan_from_seed(seed0, split, max_samples, batch)
            p2.destroy()
            assert (got_steps, state, draws) == (steps2, state2, draws2)
            eng.set_weights(zeros(d))
            eng.plan_run(plan, 0, n_steps, LR)
            st = eng.synchronize()
            assert st["n_samples"] == st["n_active"] == len(idx) == plan.n_samples
            w_dev = eng.get_weights()
        finally:
            plan.destroy()
        hp = eng.lg_plan_flat(idx, offs, n_steps, len(split))   # the same lists, drawn by the host
        eng.set_weights(zeros(d))
        eng.plan_run(hp, 0, n_steps, LR)
        hp.destroy()
        assert np.array_equal(bits(eng.get_weights()), bits(w_dev)) and np.any(w_dev != 0)
        # a batch beyond the device form: refused, the state as it was
        sb = np.asarray([r.start for r in split], dtype=np.int64)
        se = np.asarray([r.stop for r in split], dtype=np.int64)
        st64, h, ns, dr = C.c_uint64(seed0), C.c_void_p(), C.c_int64(-1), C.c_int64(-1)
        rc = eng._lib.dsgd_plan_create_from_seed_lg(eng._ctx, C.byref(st64), _lib.ptr(sb), _lib.ptr(se), len(sb), max_samples, 1025, C.byref(h),
                                                    C.byref(ns), C.byref(dr))
        assert rc == _lib.EUNSUPPORTED and st64.value == seed0 and not h.value
        assert np.array_equal(bits(eng.get_weights()), bits(w_dev))


# ---- 4. several ranges in one launch ----
BIG = 20000   # 64 * n_cu + 65 <= 16,449 rows at n_cu <= 256: the whole set takes every workgroup through a second pass


def test_ranges_evaluation_gives_the_bits_of_single_calls():
    d = data(BIG, seed=17)
    rng = np.random.default_rng(3)
    steps = [[rng.integers(0, BIG, size=n).astype(np.int32) for n in (100, 37, 64)] for _ in range(3)]
    ranges = [(11, 12), (100, 164), (200, 265), (0, BIG), (5000, 9000), (7000, 12000), (300, 1300), (300, 1300)]
    sixteen = [(i * 7, i * 7 + n) for i, n in enumerate((1, 64, 65, 128, 129, 4095, 4096, 4097, 2, 63, 1000, BIG - 100, 16384, 16385, 16449, 3))]
    assert len(sixteen) == 16 and all(b <= BIG for _, b in sixteen)
    with engine(d) as eng:
        plan = eng.lg_plan(steps)
        eng.set_weights(zeros(d))
        eng.plan_run(plan, 0, 3, LR)
        after_run = eng.lg_loss_acc_ranges(ranges)           # |w|^2 from the plan's last finish
        assert eng.synchronize()["n_samples"] == 3 * 201
        w = eng.get_weights()
        assert np.any(w != 0)
        eng.set_weights(w)
        after_set = eng.lg_loss_acc_ranges(ranges)           # |w|^2 from dsgd_lg_nsq_kernel
        assert np.array_equal(dbits(after_run), dbits(after_set))
        single = [eng.lg_loss_acc(a, b) for a, b in ranges]
        assert np.array_equal(dbits(after_run), dbits(single)), (after_run, single)
        assert after_run[6] == after_run[7] and 0.0 < after_run[3][0] < np.inf and 0.0 < after_run[3][1] < 1.0
        got16 = eng.lg_loss_acc_ranges(sixteen)
        assert np.array_equal(dbits(got16), dbits([eng.lg_loss_acc(a, b) for a, b in sixteen]))
        assert np.array_equal(dbits(eng.lg_loss_acc_ranges([(0, BIG)])), dbits(single[3:4]))   # one range alone
        # with w passed in (which then replaces the resident weights, as in dsgd_lg_loss_acc)
        w2 = (w * np.float32(0.5)).astype(np.float32)
        passed = eng.lg_loss_acc_ranges(ranges, w=w2)
        assert np.array_equal(bits(eng.get_weights()), bits(w2))
        assert np.array_equal(dbits(passed), dbits([eng.lg_loss_acc(a, b, w=w2) for a, b in ranges]))
        assert not np.array_equal(dbits(passed), dbits(after_run))
        # the plan still runs behind it, and the SVM's calls are undisturbed by the evaluation's counters
        eng.plan_run(plan, 0, 1, LR)
        assert eng.synchronize()["n_samples"] == 201
        plan.destroy()


# ---- 5. refusals leave everything as it was ----
def test_refusals_leave_the_weights_and_the_context():
    d = data()
    steps = steps_of(3)
    idx, offs = flat_of(steps)
    w = (np.random.default_rng(1).standard_normal(d.dim + 1) * 0.01).astype(np.float32)
    with engine() as eng:
        eng.set_weights(w)
        plan = eng.lg_plan(steps)
        lib, ctx = eng._lib, eng._ctx
        z = C.c_int64
        h = C.c_void_p()
        loss, acc = np.zeros(17), np.zeros(17)
        rb, re_ = np.arange(17, dtype=np.int64), np.arange(17, dtype=np.int64) + 5
        bad = idx.copy()
        bad[5] = N
        neg = idx.copy()
        neg[0] = -1
        empty = offs.copy()
        empty[2] = empty[1]
        p = _lib.ptr
        calls = [
            (_lib.EUNSUPPORTED, lambda: lib.dsgd_plan_run_f64(ctx, plan.handle, z(0), z(1), C.c_double(0.5))),
            (_lib.EUNSUPPORTED, lambda: lib.dsgd_plan_run_async_f64(ctx, plan.handle, z(0), z(1), C.c_double(0.5))),
            (_lib.EUNSUPPORTED, lambda: lib.dsgd_plan_record(ctx, plan.handle, 1)),
            (_lib.EUNSUPPORTED, lambda: lib.dsgd_plan_read_record(ctx, plan.handle, z(0), z(1), None, None, None)),
            (_lib.ERANGE, lambda: lib.dsgd_plan_create_lg_n(ctx, p(bad), z(len(bad)), p(offs), z(4), 3, C.byref(h))),
            (_lib.ERANGE, lambda: lib.dsgd_plan_create_lg_n(ctx, p(neg), z(len(neg)), p(offs), z(4), 3, C.byref(h))),
            (_lib.EINVAL, lambda: lib.dsgd_plan_create_lg_n(ctx, p(idx), z(len(idx)), p(empty), z(4), 3, C.byref(h))),
            (_lib.EINVAL, lambda: lib.dsgd_plan_create_lg_n(ctx, p(idx), z(len(idx) - 1), p(offs), z(4), 3, C.byref(h))),
            (_lib.EINVAL, lambda: lib.dsgd_plan_create_lg_n(ctx, p(idx), z(len(idx)), p(offs), z(0), 3, C.byref(h))),
            (_lib.EINVAL, lambda: lib.dsgd_plan_create_lg_n(ctx, None, z(len(idx)), p(offs), z(4), 3, C.byref(h))),
            (_lib.EINVAL, lambda: lib.dsgd_plan_run(ctx, plan.handle, z(0), z(5), C.c_float(0.5))),   # steps outside the plan
            (_lib.EINVAL, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(rb), p(re_), 17, p(loss), p(acc))),
            (_lib.EINVAL, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(rb), p(re_), 0, p(loss), p(acc))),
            (_lib.EINVAL, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(re_), p(rb), 2, p(loss), p(acc))),   # reversed
            (_lib.EINVAL, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(rb), p(rb), 1, p(loss), p(acc))),    # empty
            (_lib.EINVAL, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(rb), p(re_), 2, None, None)),
            (_lib.ERANGE, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(rb), p(re_ + N), 2, p(loss), p(acc))),
            (_lib.ERANGE, lambda: lib.dsgd_lg_loss_acc_ranges(ctx, None, p(rb - 1), p(re_), 2, p(loss), p(acc))),
        ]
        for i, (code, f) in enumerate(calls):
            assert f() == code, (i, code, lib.dsgd_last_error())
            assert not h.value, i
            assert np.array_equal(bits(eng.get_weights()), bits(w)), i
        assert not loss.any() and not acc.any()
        # dimSparsity was never set: the plan runs all the same
        eng.plan_run(plan, 0, len(steps), LR)
        assert eng.synchronize()["n_active"] == len(idx)
        w1 = eng.get_weights()
        assert not np.array_equal(bits(w1), bits(w))
        # a reload to fewer rows: the plan's lists no longer fit -- refused at the run, the weights as they were; under data
        # that holds its rows again it runs
        small = d.rows(0, 100)
        eng.load_csr(*csr_of(small))
        w2 = eng.get_weights()
        with pytest.raises(dsgd_amd.DsgdError) as ei:
            eng.plan_run(plan, 0, len(steps), LR)
        assert ei.value.code == _lib.ERANGE
        with pytest.raises(dsgd_amd.DsgdError) as ei:
            plan.info()
        assert ei.value.code == _lib.ERANGE
        assert np.array_equal(bits(eng.get_weights()), bits(w2))
        assert eng.synchronize()["n_samples"] == 0
        with pytest.raises(dsgd_amd.DsgdError) as ei:
            eng.lg_loss_acc_ranges([(0, 50), (50, 101)])
        assert ei.value.code == _lib.ERANGE
        eng.load_csr(*csr_of(d))
        eng.set_weights(w)
        eng.plan_run(plan, 0, len(steps), LR)
        assert np.array_equal(bits(eng.get_weights()), bits(w1))
        plan.destroy()
    with engine(precision="fp64") as eng:   # an fp64 context: no logistic plan is made, nothing is evaluated
        for f in (lambda: eng.lg_plan(steps), lambda: eng.lg_plan_from_seed(host.JavaRandom(0).seed, [range(0, 100)], 100, 10),
                  lambda: eng.lg_loss_acc_ranges([(0, 5)])):
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                f()
            assert ei.value.code == _lib.EUNSUPPORTED
    with dsgd_amd.Engine(d.dim, LAM) as eng:   # no data loaded
        for f in (lambda: eng.lg_plan(steps), lambda: eng.lg_loss_acc_ranges([(0, 5)])):
            with pytest.raises(dsgd_amd.DsgdError) as ei:
                f()
            assert ei.value.code == _lib.ESTATE


# ---- 6. the mirror ----
def test_logistic_sync_mirror():
    d = data()
    n_train, K, batch, lr = 300, 3, 100, 0.5
    out = []
    for device_lists in (True, False):
        with engine() as eng:
            m = host.LogisticSync(eng, n_train, N, K, rnd=host.JavaRandom(0), device_lists=device_lists)
            state = m.fit(zeros(d), 2, batch, lr, lambda losses: False)
            assert m.device_drawn_epochs == (2 if device_lists else 0) and m.steps_run == 2 and state.updates == 2
            assert state.loss == m.losses[0] and m.local_loss() == m.losses[0] and m.local_accuracy(test=True) == m.test_accs[0]
            proba = m.predict_proba(np.arange(5, dtype=np.int32))
            assert np.array_equal(proba, eng.lg_predict_proba(np.arange(5, dtype=np.int32))) and np.all((proba > 0) & (proba < 1))
            assert m.metrics.snapshot() is not None
            out.append((state.grad.copy(), list(m.losses), list(m.accs), list(m.test_losses), list(m.test_accs), m.rnd.seed))
    dev, hst = out
    assert np.array_equal(bits(dev[0]), bits(hst[0])) and np.any(dev[0] != 0)
    assert dev[1:] == hst[1:]
    # by hand: the same stream, the calls that were there
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(n_train, K)
    with engine() as eng:
        eng.set_weights(zeros(d))
        losses, accs, tlosses, taccs = [], [], [], []
        for _ in range(2):
            idx, offs, n_steps = host.epoch_lists(rnd, split, 100, batch)
            eng.lg_sync_steps(idx, offs, n_steps, K, lr)
            l, a = eng.lg_loss_acc(0, n_train)
            tl, ta = eng.lg_loss_acc(n_train, N)
            losses.insert(0, l), accs.insert(0, a), tlosses.insert(0, tl), taccs.insert(0, ta)
        assert np.array_equal(bits(eng.get_weights()), bits(dev[0]))
        assert (losses, accs, tlosses, taccs, rnd.seed) == dev[1:]
        seed_after_one = host.JavaRandom(0)
        host.epoch_lists(seed_after_one, split, 100, batch)
        # early stopping on the test's criterion: after the first epoch's test loss; the epoch laid out ahead is dropped and
        # the stream stands where one epoch leaves it
        for device_lists in (True, False):
            seen = []
            m = host.LogisticSync(eng, n_train, N, K, rnd=host.JavaRandom(0), device_lists=device_lists)
            state = m.fit(zeros(d), 5, batch, lr, lambda tl_: seen.append(list(tl_)) or len(tl_) >= 1)
            assert state.updates == 1 and seen == [[], [tlosses[1]]] and m.test_losses == [tlosses[1]] and m.losses == [losses[1]]
            assert m.rnd.seed == seed_after_one.seed
            eng.synchronize()
            assert eng.cache_trim(0) == 0   # (the launch stream is idle) also the dropped plan's blocks are back
