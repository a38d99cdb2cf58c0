"""GPU: logistic plans on column slices (include/dsgd.h "THE LOGISTIC MODEL": COLUMN SLICES; csrc/dsgd_lg_cs.hpp).

The slice form's x.w is a sum of 16 slice partials, so its weights are NOT the row form's bits and nothing here asks for that.
What is asked: every coordinate after every step within the carried dw of tests/logistic_cs_bound.py against the fp64 reference
tests/logistic_ref.py (the bound is derived from the kernel's order; tests/test_logistic_cs_bound.py shows what it is worth);
bit equalities wherever the order is the same (one run against split runs, again from the same weights, caller lists against
device-drawn ones; the saturated sets whose answers are exact); plan code 7 and the row form's bits wherever the slices decline;
and a context left as any other logistic call leaves it.  Shapes: 2,000 synthetic rows at the real D, hand-built rows whose
place in the slices is known at dp = 64, 100 and 400."""

import functools

import numpy as np
import pytest

import dsgd_amd
import hard_data as hd
import logistic_bound as lb
import logistic_cs_bound as cb
import logistic_hard_cases as cases
import logistic_ref as ref
from dsgd_amd import _lib, host

pytestmark = pytest.mark.gpu

LAM = 1e-5
LR = 2.0 ** -3
N = 2000
KERNEL = "dsgd_lg_cs_step_kernel"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def data(n=N, seed=13):
    return dsgd_amd.synth.generate(n, seed=seed)


def csr_of(d):
    return (d.row_ptr, d.col, d.val, d.label)


def engine(csr=None, dim=None, lam=LAM):
    if csr is None:
        csr, dim = csr_of(data()), data().dim
    eng = dsgd_amd.Engine(dim, lam)
    eng.load_csr(*csr)
    return eng


@functools.lru_cache(maxsize=None)
def steps_of(lens, n_steps, seed=5, n=N):
    rng = np.random.default_rng([seed, len(lens), n_steps])
    return [[rng.integers(0, n, size=m).astype(np.int32) for m in lens] for _ in range(n_steps)]


def flat_of(steps):
    lists = [a for s in steps for a in s]
    return np.concatenate(lists), np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)


def slice_plan(eng, steps):
    plan = eng.lg_plan(steps, slices=True)
    info = plan.info()
    assert info["kind"] == "logistic_column_slices" and info["slices"] == 16 and info["device_built"] and info["threads"] == 512, info
    return plan


def hold_to_reference(eng, csr, steps, lr, lam, w0, what):
    """every coordinate after every step (plan_run(s, s + 1)) within the carried dw of the fp64 reference; returns the weights"""
    plan = slice_plan(eng, steps)
    try:
        eng.set_weights(w0)
        w_ref, E = np.asarray(w0, dtype=np.float64), np.zeros(len(w0))
        worst = 0.0
        for s, lists in enumerate(steps):
            eng.plan_run(plan, s, s + 1, lr)
            st = eng.synchronize()
            assert st["n_samples"] == st["n_active"] == sum(len(a) for a in lists), (what, s, st)
            assert eng.grad_kernel_name() == KERNEL
            E = cb.dw(csr, w_ref, lists, lr, lam, E)
            w_ref = ref.sync_step(csr, w_ref, lists, lr, lam)
            w = eng.get_weights()
            err = np.abs(w.astype(np.float64) - w_ref)
            worst = max(worst, float(np.max(err / E)))
            assert np.all(err <= E), (what, s, float(np.max(err / E)))
        print("%s: worst err / carried dw over %d steps = %.3f" % (what, len(steps), worst))
        return eng.get_weights()
    finally:
        plan.destroy()


# ---- 1. the shapes, each held to the reference on every coordinate after every step ----
SHAPES = {"3 x 100 x 20": ((100, 100, 100), 20), "4 x 200 x 5": ((200, 200, 200, 200), 5), "1 x 1": ((1,), 3),
          "6 uneven": ((1, 7, 100, 16, 33, 250), 3)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_against_the_fp64_reference(name):
    lens, n_steps = SHAPES[name]
    d = data()
    with engine() as eng:
        w = hold_to_reference(eng, csr_of(d), steps_of(lens, n_steps), LR, LAM, np.zeros(d.dim + 1, dtype=np.float32), name)
        assert np.any(w != 0)


# ---- 2. rows whose place in the slices is known: several slots in one slice, one slice only, empty, listed twice, by two workers;
#         narrow models whose slices end in padding (dp = 64: four columns and four of padding; dp = 100: slices of 7 and 6) ----
@pytest.mark.parametrize("dp", [64, 100, 400])
def test_designed_rows_and_narrow_models(dp):
    csr, steps, w0 = cb.designed(dp)
    row_ptr = csr[0]
    _, sl = cb.slice_of(csr, dp)
    per2 = np.bincount(sl[row_ptr[2]:row_ptr[3]], minlength=16)
    assert np.count_nonzero(per2) == 1 and (per2.max() == 20 if dp == 400 else per2.max() >= 4)
    with engine(csr, dp - 1, 0.05) as eng:
        w = hold_to_reference(eng, csr, list(steps), 0.25, 0.05, w0, "designed rows, dp = %d" % dp)
        # the honest emulation of the slice order is the kernel's order: the same bits
        emu = cb.Emu(csr, w0)
        for lists in steps:
            emu.step(lists, 0.25, 0.05)
        assert np.array_equal(bits(w), bits(emu.w)), int(np.count_nonzero(bits(w) != bits(emu.w)))


# ---- 3. hostile values; saturated sets with exact answers ----
@pytest.mark.parametrize("trait", hd.TRAITS)
def test_hostile_values(trait):
    case = cases.hostile(trait)
    lists, lr = case.step
    with engine(case.csr, case.dim, case.lam) as eng:
        hold_to_reference(eng, case.csr, [list(lists), list(lists)], lr, case.lam, case.w, "hostile " + trait)


@pytest.mark.parametrize("n", cases.BROAD_N)
@pytest.mark.parametrize("vmax", list(hd.VMAX))
def test_saturated_sets_are_exact(n, vmax):
    case = cases.exact_case("broad", n, vmax)
    lists, w1 = case.expect.step["all"]
    with engine(case.csr, case.dim, 0.0) as eng:
        plan = slice_plan(eng, [lists])
        eng.set_weights(case.w)
        eng.plan_run(plan, 0, 1, case.lr)
        eng.synchronize()
        assert np.array_equal(bits(eng.get_weights()), bits(w1))
        eng.plan_run(plan, 0, 1, case.lr)   # ... and the second step over all rows as one worker
        eng.synchronize()
        assert np.array_equal(bits(eng.get_weights()), bits(case.expect.whole[1]))
        plan.destroy()


# ---- 4. determinism: bit equalities ----
def test_one_run_split_runs_a_second_run_and_device_drawn_lists():
    d = data()
    steps = steps_of((100, 100, 100), 8)
    w0 = np.zeros(d.dim + 1, dtype=np.float32)
    with engine() as eng:
        plan = slice_plan(eng, steps)
        eng.set_weights(w0)
        eng.plan_run(plan, 0, 8, LR)
        st = eng.synchronize()
        assert st["n_samples"] == st["n_active"] == 2400
        w_one = eng.get_weights()
        for cut in (1, 3, 7):
            eng.set_weights(w0)
            eng.plan_run(plan, 0, cut, LR)
            eng.plan_run(plan, cut, 8, LR)
            eng.synchronize()
            assert np.array_equal(bits(eng.get_weights()), bits(w_one)), cut
        eng.set_weights(w0)
        eng.plan_run(plan, 0, 8, LR)
        eng.plan_run(plan, 4, 4, LR)   # (an empty range changes nothing)
        assert eng.synchronize()["n_samples"] == 2400
        assert np.array_equal(bits(eng.get_weights()), bits(w_one))
        plan.destroy()
        # a device-drawn plan against a caller-list plan of the lists read back from it
        split = host.split_vanilla(1600, 3)
        drawn, n_steps, state, _ = eng.lg_plan_from_seed(host.JavaRandom(0).seed, split, max(len(r) for r in split), 100, slices=True)
        plain, n_plain, state_plain, _ = eng.lg_plan_from_seed(host.JavaRandom(0).seed, split, max(len(r) for r in split), 100)
        assert drawn.info()["kind"] == "logistic_column_slices" and plain.info()["kind"] == "logistic"
        assert (n_steps, state) == (n_plain, state_plain)
        idx, offs = eng.plan_lists(drawn)
        idx_plain, offs_plain = eng.plan_lists(plain)
        assert np.array_equal(idx, idx_plain) and np.array_equal(offs, offs_plain)
        plain.destroy()
        eng.set_weights(w0)
        eng.plan_run(drawn, 0, n_steps, LR)
        eng.synchronize()
        w_drawn = eng.get_weights()
        mine = eng.lg_plan_flat(idx, offs, n_steps, 3, slices=True)
        assert mine.info()["kind"] == "logistic_column_slices"
        eng.set_weights(w0)
        eng.plan_run(mine, 0, n_steps, LR)
        eng.synchronize()
        assert np.array_equal(bits(eng.get_weights()), bits(w_drawn)) and np.any(w_drawn != 0)
        drawn.destroy()
        mine.destroy()


# ---- 5. declines: plan code 7 and the bits of the plan made without `slices` ----
def decline_case(name):
    if name == "K = 7":
        return csr_of(data()), data().dim, steps_of((20,) * 7, 2)
    if name == "a step of 1,025 rows":
        return csr_of(data()), data().dim, steps_of((1000, 25), 2)
    csr, steps, _ = cb.designed(63)
    return csr, 62, list(steps[:2])


@pytest.mark.parametrize("name", ["K = 7", "a step of 1,025 rows", "dp = 63"])
def test_declines_run_the_row_form(name):
    csr, dim, steps = decline_case(name)
    idx, offs = flat_of(steps)
    got = []
    for slices in (True, False):
        with engine(csr, dim) as eng:
            plan = eng.lg_plan_flat(idx, offs, len(steps), len(steps[0]), slices=slices)
            info = plan.info()
            assert info["kind"] == "logistic" and info["slices"] == 0, (name, info)
            eng.set_weights(np.zeros(dim + 1, dtype=np.float32))
            eng.plan_run(plan, 0, len(steps), LR)
            st = eng.synchronize()
            assert st["n_samples"] == st["n_active"] == len(idx)
            assert eng.grad_kernel_name() == "dsgd_lg_grad_kernel"
            got.append(eng.get_weights())
            plan.destroy()
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.any(got[0] != 0)


# ---- 6. the state a slice run leaves ----
def test_evaluation_and_following_steps_see_a_clean_context():
    d = data()
    steps = steps_of((100, 100, 100), 3)
    lists = steps_of((50, 70), 1, seed=9)[0]
    with engine() as eng, engine() as fresh:
        plan = slice_plan(eng, steps)
        eng.set_weights(np.zeros(d.dim + 1, dtype=np.float32))
        eng.plan_run(plan, 0, 3, LR)
        eng.synchronize()
        la = eng.lg_loss_acc(0, N)                  # straight behind the run: |w|^2 is computed, not taken from stale words
        w = eng.get_weights()
        fresh.set_weights(w)
        assert la == fresh.lg_loss_acc(0, N)
        # a gradient, then a list step, behind another run: the shared accumulators were left clean
        eng.plan_run(plan, 0, 3, LR)
        eng.synchronize()
        fresh.set_weights(eng.get_weights())
        g, _ = eng.lg_gradient(lists[0])
        g_fresh, _ = fresh.lg_gradient(lists[0])
        assert np.array_equal(bits(g), bits(g_fresh))
        eng.plan_run(plan, 1, 2, LR)
        eng.synchronize()
        fresh.set_weights(eng.get_weights())
        eng.lg_sync_step(lists, LR)
        fresh.lg_sync_step(lists, LR)
        assert np.array_equal(bits(eng.get_weights()), bits(fresh.get_weights()))
        assert eng.lg_loss_acc(0, N) == fresh.lg_loss_acc(0, N)
        # refused as a code-7 plan is
        for call in (lambda: plan.record(True), lambda: plan.read_record(0, 1)):
            with pytest.raises(_lib.DsgdError) as e:
                call()
            assert e.value.code == -7
        plan.destroy()


def test_svm_and_logistic_slice_plans_share_a_context():
    d = data()
    n_train = 1600
    svm_steps = steps_of((100, 100, 100), 4, seed=21, n=n_train)
    lg_steps = steps_of((100, 100, 100), 4, seed=22, n=n_train)
    w0 = np.zeros(d.dim + 1, dtype=np.float32)

    def ctx():
        e = engine()
        e.build_dim_sparsity(n_train)
        return e

    with ctx() as both, ctx() as only_svm, ctx() as only_lg:
        p_svm, p_lg = both.plan(svm_steps), slice_plan(both, lg_steps)
        q_svm, q_lg = only_svm.plan(svm_steps), slice_plan(only_lg, lg_steps)
        assert p_svm.info()["kind"] == q_svm.info()["kind"] == "column_slices"
        both.set_weights(w0)
        w = w0
        for rnd in range(3):   # in turn, each from the weights the other left: the tags run on, the exchange buffer is one
            both.plan_run(p_svm, 0, 4, 0.5)
            both.synchronize()
            only_svm.set_weights(w)
            only_svm.plan_run(q_svm, 0, 4, 0.5)
            only_svm.synchronize()
            w = only_svm.get_weights()
            assert both.grad_kernel_name() == "dsgd_cs_step_kernel"
            both.plan_run(p_lg, 0, 4, LR)
            st = both.synchronize()
            assert st["n_samples"] == st["n_active"] == 1200 and both.grad_kernel_name() == KERNEL
            only_lg.set_weights(w)
            only_lg.plan_run(q_lg, 0, 4, LR)
            only_lg.synchronize()
            w = only_lg.get_weights()
            assert np.array_equal(bits(both.get_weights()), bits(w)), rnd
        for p in (p_svm, p_lg, q_svm, q_lg):
            p.destroy()


def test_a_plan_that_outlives_a_load():
    d, other, small = data(), data(N, 14), data(500, 15)
    steps = steps_of((100, 100, 100), 2)
    idx, offs = flat_of(steps)
    got = []
    for slices in (True, False):
        with engine() as eng:
            plan = eng.lg_plan_flat(idx, offs, 2, 3, slices=slices)
            eng.load_csr(*csr_of(small))           # rows the lists leave: DSGD_ERANGE, nothing ran
            with pytest.raises(_lib.DsgdIndexError):
                eng.plan_run(plan, 0, 2, LR)
            eng.load_csr(*csr_of(other))           # other rows that hold the lists: the layout is stale, the row form runs
            assert plan.info()["kind"] == "logistic"
            eng.set_weights(np.zeros(d.dim + 1, dtype=np.float32))
            eng.plan_run(plan, 0, 2, LR)
            assert eng.synchronize()["n_samples"] == 600
            assert eng.grad_kernel_name() == "dsgd_lg_grad_kernel"
            got.append(eng.get_weights())
            plan.destroy()
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.any(got[0] != 0)


# ---- 7. the training mirror ----
def test_logistic_sync_on_slices_follows_the_reference_trajectory():
    d = data()
    csr = csr_of(d)
    n_train, K, batch, epochs = 1600, 3, 100, 2
    w0 = np.zeros(d.dim + 1, dtype=np.float32)
    never = lambda losses: False
    states = {}
    for slices in (True, False):
        with engine() as eng:
            m = host.LogisticSync(eng, n_train, N, K, rnd=host.JavaRandom(0), slices=slices)
            m.fit(w0, epochs, batch, LR, never)
            states[slices] = (m.rnd.seed, m.steps_run, m.device_drawn_epochs)
            if slices:
                losses, test_losses = list(m.losses), list(m.test_losses)
    assert states[True] == states[False] and states[True][2] == epochs
    # the fp64 trajectory over the same lists, the weights' bound carried through every step
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(n_train, K)
    w_ref, E = np.zeros(d.dim + 1), np.zeros(d.dim + 1)
    row_ptr, col, val, _ = lb._csr(csr)
    rows = np.repeat(np.arange(N), np.diff(row_ptr))
    for ep in range(epochs):
        idx, offs, n_steps = host.epoch_lists(rnd, split, max(len(r) for r in split), batch)
        for s in range(n_steps):
            lists = [idx[offs[s * K + k]:offs[s * K + k + 1]] for k in range(K)]
            E = cb.dw(csr, w_ref, lists, LR, LAM, E)
            w_ref = ref.sync_step(csr, w_ref, lists, LR, LAM)
        # |dl/dd| <= 1: a row's loss moves by at most sum_j |x_ij| E_j; lambda |w|^2 by at most lambda sum (2 |w_j| + E_j) E_j
        per_row = np.bincount(rows, weights=np.abs(val.astype(np.float64)) * E[col], minlength=N)
        nsq = LAM * float(np.sum((2.0 * np.abs(w_ref) + E) * E))
        for (a, b), got in (((0, n_train), losses[epochs - 1 - ep]), ((n_train, N), test_losses[epochs - 1 - ep])):
            want = ref.loss_acc(csr, w_ref, a, b, LAM)[0]
            bound = lb.dloss(csr, w_ref, a, b, LAM) + float(np.mean(per_row[a:b])) + nsq
            print("epoch %d rows [%d, %d): |loss - ref| / bound = %.3f" % (ep, a, b, abs(got - want) / bound))
            assert abs(got - want) <= bound
    assert rnd.seed == states[True][0]
