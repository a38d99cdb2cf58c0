"""-m gpu: the dense model's index lists, resident plans and per-row probabilities (include/dsgd.h "INDEX LISTS").

The block structure of the list kernels depends on list POSITIONS only and a row's z on the row and w only, so every
list step has an exact twin in the range form -- which tests/test_gpu_dense_edges.py already holds to the fp64 oracle.
The tests here therefore assert `==` on raw float bits; tests/test_dense_list_abi.py shows on the CPU that the lists
used (tests/dense_lists.py) make those equalities sensitive to every indexing mistake it seeds."""

import numpy as np
import pytest

import dense_bound as db
import dense_lists as dl
import dsgd_amd
from conftest import has_gpu
from oracle import dense_ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

VARIANTS = pytest.mark.parametrize("variant", [0, 1])
EINVAL, ERANGE, ESTATE = -1, -2, -3


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def engine(monkeypatch, variant, D):
    monkeypatch.setenv("DSGD_DENSE_MFMA", str(variant))
    return dsgd_amd.DenseLogistic(D)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what=None):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=str(what))


# ---- 1. a contiguous list is the range ---------------------------------------------------------------------------------
@VARIANTS
@pytest.mark.parametrize("D", [512, 4096])
def test_contiguous_list_is_the_range(monkeypatch, variant, D):
    cu = n_cu()
    big = dl.big_len(D, cu)
    X, y, w0 = dl.shard(D, big + 8)
    spans = [(rb, rb + n) for rb in (0, 5) for n in dl.LENGTHS] if D == 512 else []
    spans += [(3, 3 + big)]
    with engine(monkeypatch, variant, D) as eng:
        eng.load(X, y)
        for rb, re in spans:
            eng.set_weights(w0)
            eng.step(rb, re, 4.0)
            want = eng.get_weights()
            assert not np.array_equal(want, w0)
            eng.set_weights(w0)
            eng.step_list(np.arange(rb, re), 4.0)
            same_bits(eng.get_weights(), want, (rb, re))


# ---- 2. any list is the range step on permuted data --------------------------------------------------------------------
def list_against_permuted_data(monkeypatch, variant, D, n_rows, todo):
    """Engine A holds (X, y) and steps over each list; engine B holds (X[idx], y[idx]) and steps over [0, n)."""
    X, y, w0 = dl.shard(D, n_rows)
    with engine(monkeypatch, variant, D) as A, engine(monkeypatch, variant, D) as B:
        A.load(X, y)
        for idx, idx2 in todo:
            A.set_weights(w0)
            A.step_list(idx, 4.0)
            wa = A.get_weights()
            B.load(X[idx], y[idx])
            B.set_weights(w0)
            B.step(0, len(idx), 4.0)
            same_bits(wa, B.get_weights(), (D, len(idx)))
            assert not np.array_equal(wa, w0)
            if idx2 is not None:          # a second step, from the weights the first left
                A.step_list(idx2, 4.0)
                B.load(X[idx2], y[idx2])
                B.step(0, len(idx2), 4.0)
                same_bits(A.get_weights(), B.get_weights(), (D, len(idx), "second step"))


@VARIANTS
@pytest.mark.parametrize("kind", dl.KINDS)
def test_any_list_is_the_range_step_on_permuted_data(monkeypatch, variant, kind):
    cu = n_cu()
    by_shard = {}
    for D, n_rows, k, n in dl.cases(cu):
        if k == kind and not (variant and D > 4096):
            idx = dl.make_list(kind, n, n_rows)
            idx2 = dl.step2_list(n_rows) if n in (dl.WIDE_N, 17) else None
            by_shard.setdefault((D, n_rows), []).append((idx, idx2))
    widths = {D for D, _ in by_shard}
    assert widths == {D for D in dl.WIDTHS if not (variant and D > 4096)}
    for (D, n_rows), todo in by_shard.items():
        list_against_permuted_data(monkeypatch, variant, D, n_rows, todo)


# ---- 3. plans ----------------------------------------------------------------------------------------------------------
def plan_lists(cu):
    lens = [1, 8, 9, 100, 17, 3 * 8 * 2 * cu + 5]
    n_rows = dl.big_len(512, cu) + 8
    kinds = ["perm", "perm", "reverse", "repeat", "perm", "perm"]
    return n_rows, [dl.make_list(k, n, n_rows, seed=3 + i) for i, (k, n) in enumerate(zip(kinds, lens))]


@VARIANTS
def test_plan_run_is_its_steps_however_it_is_cut(monkeypatch, variant):
    cu = n_cu()
    n_rows, lists = plan_lists(cu)
    X, y, w0 = dl.shard(512, n_rows)
    out = {}
    for how in ("whole", "calls", "cut"):
        with engine(monkeypatch, variant, 512) as eng:
            eng.load(X, y)
            eng.set_weights(w0)
            if how == "calls":
                for idx in lists:
                    eng.step_list(idx, 2.0)
            else:
                plan = eng.plan(lists)
                assert plan.n_steps == 6
                assert eng.prof(True) == (0.0, 0)
                for a, b in ([(0, 6)] if how == "whole" else [(0, 2), (2, 3), (3, 6)]):
                    eng.plan_run(plan, a, b, 2.0)
                ms, n = eng.prof(False)
                assert n == 6 and ms > 0            # every plan step is counted
                eng.plan_run(plan, 3, 3, 2.0)       # an empty step range: nothing happens
                plan.destroy()
                plan.destroy()                      # (idempotent)
            out[how] = eng.get_weights()
    assert not np.array_equal(out["whole"], w0)
    same_bits(out["whole"], out["calls"])
    same_bits(out["whole"], out["cut"])


@VARIANTS
def test_back_to_back_list_steps_each_use_their_own_list(monkeypatch, variant):
    """No synchronise between the calls: the second list must not land in the staging buffer under the first's copy."""
    X, y, w0 = dl.shard(512, dl.SMALL_ROWS)
    l1, l2 = dl.make_list("perm", 37, dl.SMALL_ROWS, seed=1), dl.make_list("reverse", 37, dl.SMALL_ROWS)
    assert not np.array_equal(l1, l2)
    with engine(monkeypatch, variant, 512) as eng, engine(monkeypatch, variant, 512) as ref:
        for e in (eng, ref):
            e.load(X, y)
            e.set_weights(w0)
        assert eng.prof(True) == (0.0, 0)
        eng.step_list(l1, 2.0)
        eng.step_list(l2, 2.0)
        assert eng.prof(False)[1] == 2              # list steps are counted as range steps are
        plan = ref.plan([l1, l2])
        ref.plan_run(plan, 0, 2, 2.0)
        same_bits(eng.get_weights(), ref.get_weights())
        # the object releases the plan it still owns when it closes


@VARIANTS
def test_plan_crosses_the_event_pool(monkeypatch, variant):
    """4,100 one-block steps with profiling on: the pool of 4,096 event pairs fills inside ONE plan_run, is collected and
    re-used; the weights are those of the same list steps issued one by one, unprofiled."""
    X, y, w0 = dl.shard(512, dl.SMALL_ROWS)
    rng = np.random.default_rng(5)
    lists = [rng.permutation(dl.SMALL_ROWS)[:8].astype(np.int32) for _ in range(4100)]
    with engine(monkeypatch, variant, 512) as eng, engine(monkeypatch, variant, 512) as ref:
        for e in (eng, ref):
            e.load(X, y)
            e.set_weights(w0)
        plan = eng.plan(lists)
        eng.prof(True)
        eng.plan_run(plan, 0, 4100, 0.01)
        ms, n = eng.prof(False)
        assert n == 4100 and ms > 0
        for idx in lists:
            ref.step_list(idx, 0.01)
        w = eng.get_weights()
        assert np.isfinite(w).all() and not np.array_equal(w, w0)
        same_bits(w, ref.get_weights())
        plan.destroy()


# ---- 4. probabilities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,D", [(0, 512), (1, 512), (0, 4096), (1, 4096), (0, 8192)])
def test_probabilities_of_a_list_and_of_a_range(monkeypatch, variant, D):
    X, y, w, _ = db.case_d(D)           # 45 rows, logits of sigma ~ 10
    N = len(y)
    idx = np.concatenate([dl.make_list("perm", 37, N), dl.make_list("longer", 5, N)])
    bd = db.Bound(X, y, w, 1.0, 0, N, variant, 1)
    with engine(monkeypatch, variant, D) as eng:
        eng.load(X, y)
        eng.set_weights(w)
        p = eng.predict_proba(0, N)
        same_bits(eng.predict_proba(), p)
        same_bits(eng.predict_proba(idx=idx), p[idx])
        same_bits(eng.predict_proba(3, 40), p[3:40])
        np.testing.assert_array_equal(eng.get_weights(), w)       # forward only
    err = np.abs(p.astype(np.float64) - db.sigmoid(bd.z))
    print("predict_proba D = %d: max err / dr = %.3g" % (D, (err / bd.dr).max()))
    assert 5.0 < bd.z.std() < 20.0
    assert (err <= bd.dr).all(), (int(np.argmax(err / bd.dr)), (err / bd.dr).max())


@VARIANTS
def test_probabilities_at_zero_and_saturated_logits(monkeypatch, variant):
    z = np.array([0.0, -0.0, 110.0, -110.0] * 5, dtype=np.float32)[:19]     # 19 rows: two blocks, ragged
    X = np.zeros((len(z), 512), dtype=np.float32)
    X[:, 0] = z
    w = np.zeros(512, dtype=np.float32)
    w[0] = 1.0
    want = np.where(z == 0, 0.5, np.where(z > 0, 1.0, 0.0)).astype(np.float32)
    with engine(monkeypatch, variant, 512) as eng:
        eng.load(X, np.zeros(len(z), dtype=np.float32))
        eng.set_weights(w)
        same_bits(eng.predict_proba(), want)
        rev = np.arange(len(z) - 1, -1, -1)
        same_bits(eng.predict_proba(idx=rev), want[rev])


# ---- 5. list loss ------------------------------------------------------------------------------------------------------
@VARIANTS
@pytest.mark.parametrize("kind", ["perm", "longer"])
def test_list_loss(monkeypatch, variant, kind):
    cu = n_cu()
    n_rows = dl.SMALL_ROWS if kind == "longer" else dl.big_len(512, cu) + 8
    n = 17 if kind == "longer" else 2 * 16 * cu + 21      # several workgroups, a ragged tail
    X, y, w0 = dl.shard(512, n_rows)
    idx = dl.make_list(kind, n, n_rows)
    bd = db.Bound(X[idx], y[idx], w0, 1.0, 0, len(idx), variant, 1)
    loss_ref, _, _ = dense_ref.loss_grad(X[idx], y[idx], w0)
    with engine(monkeypatch, variant, 512) as A, engine(monkeypatch, variant, 512) as B:
        A.load(X, y)
        A.set_weights(w0)
        B.load(X[idx], y[idx])
        B.set_weights(w0)
        loss, acc = A.loss_list(idx)
        loss_b, acc_b = B.loss(0, len(idx))
        np.testing.assert_array_equal(A.get_weights(), w0)
    print("loss_list %s: err / dloss = %.3g" % (kind, abs(loss - loss_ref) / bd.dloss))
    assert acc * len(idx) == acc_b * len(idx) and abs(acc * len(idx) - round(acc * len(idx))) < 1e-6
    assert abs(loss - loss_ref) <= bd.dloss, (loss, loss_ref, bd.dloss)


# ---- 6. refusals change nothing ----------------------------------------------------------------------------------------
def refused(code, call, *args, match=None):
    with pytest.raises(dsgd_amd.DsgdError) as ei:
        call(*args)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    if match:
        for m in match:
            assert m in str(ei.value), str(ei.value)


@VARIANTS
def test_refusals_change_nothing(monkeypatch, variant):
    N = dl.SMALL_ROWS
    X, y, w0 = dl.shard(512, N)
    good = dl.make_list("perm", 17, N)
    with engine(monkeypatch, variant, 512) as eng:
        for call, args in ((eng.step_list, (good, 1.0)), (eng.loss_list, (good,)), (eng.predict_proba, (0, 4)),
                           (lambda: eng.predict_proba(idx=good), ()), (eng.plan, ([good],))):
            refused(ESTATE, call, *args)                 # before any data
        eng.load(X, y)
        eng.set_weights(w0)
        eng.step_list(good, 1.0)
        w1 = eng.get_weights()
        calls = 0
        for bad in (N, -1):
            for at in (0, 8, 16):                        # first, middle, last position
                idx = good.copy()
                idx[at] = bad
                match = ("idx[%d]" % at, "= %d " % bad)
                refused(ERANGE, eng.step_list, idx, 1.0, match=match)
                refused(ERANGE, eng.loss_list, idx, match=match)
                refused(ERANGE, lambda: eng.predict_proba(idx=idx), match=match)
                refused(ERANGE, eng.plan, [good, idx], match=("idx[%d]" % (17 + at),))
                assert isinstance(pytest.raises(IndexError, eng.step_list, idx, 1.0).value, dsgd_amd.DsgdError)
                calls += 5
        empty = np.zeros(0, dtype=np.int32)
        refused(EINVAL, eng.step_list, empty, 1.0)       # n = 0
        refused(EINVAL, eng.loss_list, empty)
        refused(EINVAL, lambda: eng.predict_proba(idx=empty))
        refused(EINVAL, eng.plan, [good, empty, good])   # an empty step in a plan
        refused(EINVAL, eng.plan, [])
        refused(EINVAL, eng.plan_flat, np.concatenate([good, good]), [0, 20, 17, 34])    # decreasing offsets
        refused(EINVAL, eng.plan_flat, np.concatenate([good, good]), [0, 17, 30])        # do not end at n_idx
        refused(EINVAL, eng.plan_flat, np.concatenate([good, good]), [1, 17, 34])        # do not start at 0
        with pytest.raises(ValueError):
            eng.predict_proba(5, 5)
        with pytest.raises(IndexError):
            eng.predict_proba(0, N + 1)
        plan = eng.plan([good, good[::-1].copy()])
        for a, b in ((-1, 1), (0, 3), (2, 1)):
            refused(EINVAL, eng.plan_run, plan, a, b, 1.0)       # bad step ranges
        with engine(monkeypatch, variant, 512) as other:
            other.load(X, y)
            with pytest.raises(ValueError):
                other.plan_run(plan, 0, 1, 1.0)                  # a plan belongs to its object
        same_bits(eng.get_weights(), w1)
        eng.load(X, y)                                           # the same rows again: the plan is stale all the same
        refused(ESTATE, eng.plan_run, plan, 0, 2, 1.0)
        same_bits(eng.get_weights(), w1)
        plan.destroy()
        assert calls == 30
        # ... and the next valid calls work, from the weights as they were
        with engine(monkeypatch, variant, 512) as ref:
            ref.load(X, y)
            ref.set_weights(w1)
            for e in (eng, ref):
                e.step_list(good, 1.0)
                p2 = e.plan([good[::-1].copy()])
                e.plan_run(p2, 0, 1, 1.0)
            same_bits(eng.get_weights(), ref.get_weights())
            assert not np.array_equal(eng.get_weights(), w1)
            assert eng.loss_list(good)[1] == ref.loss_list(good)[1]


# ---- 7. a communicator of one rank -------------------------------------------------------------------------------------
def test_communicator_of_one_rank_changes_nothing_for_lists_and_plans():
    N = dl.SMALL_ROWS
    X, y, w0 = dl.shard(512, N)
    lists = [dl.make_list(k, n, N, seed=2) for k, n in (("perm", 37), ("repeat", 16), ("longer", 9))]
    out = []
    for with_comm in (False, True):
        with dsgd_amd.DenseLogistic(512) as eng:
            if with_comm:
                eng.comm_init(dsgd_amd.Engine.comm_unique_id(), 1, 0)
            eng.load(X, y)
            eng.set_weights(w0)
            for idx in lists:
                eng.step_list(idx, 2.0)
            plan = eng.plan(lists)
            eng.plan_run(plan, 0, 3, 2.0)
            eng.synchronize()
            out.append(eng.get_weights())
    assert not np.array_equal(out[0], w0)
    same_bits(out[0], out[1])


# ---- 8. addresses beyond 32 bits ---------------------------------------------------------------------------------------
def test_addresses_beyond_32_bits(monkeypatch):
    """D = 8192 (VALU only), 262,160 generated rows = 8.0 GiB: row 131,072 starts at BYTE offset 2^32 and row 262,144 at
    ELEMENT offset 2^31 -- the smallest shape at which a 32-bit row offset in the list indexing goes wrong."""
    import torch

    D, N = 8192, 262160
    free, _ = torch.cuda.mem_get_info()
    assert free > 9.0e9, "needs about 8.6 GB of device memory, %.1f GB free" % (free / 1e9)
    w0 = (np.random.default_rng(11).normal(size=D)).astype(np.float32)
    with engine(monkeypatch, 0, D) as eng:
        eng.generate(N, seed=3)
        for rb, re in ((131072 - 20, 131072 + 21), (262144 - 21, N)):
            eng.set_weights(w0)
            eng.step(rb, re, 4.0)
            want = eng.get_weights()
            assert not np.array_equal(want, w0)
            eng.set_weights(w0)
            eng.step_list(np.arange(rb, re), 4.0)
            same_bits(eng.get_weights(), want, (rb, re))
        eng.set_weights(w0)
        p = eng.predict_proba(0, N)
        assert 0.05 < p.std() and np.isfinite(p).all()
        low, mid, high = np.arange(7, 20), np.arange(131072 - 6, 131072 + 7), np.arange(262144 - 6, 262144 + 7)
        mixed = np.stack([low, high, mid], axis=1).reshape(-1)     # 39 positions: below, above both lines, between
        same_bits(eng.predict_proba(idx=mixed), p[mixed])
        assert len(np.unique(bits(p[mixed]))) > 30
