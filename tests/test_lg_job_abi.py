"""The boundary of the logistic model's Master.fit across ranks (include/dsgd.h "THE LOGISTIC MODEL", ACROSS RANKS:
dsgd_plan_create_from_seed_job_lg, dsgd_lg_eval_job; host.LogisticSync(ranks=...), host.logistic_rank_rows) without a GPU: the
library exports the two entry points, the header declares them, the binding lists them, the refusals that need no device write
nothing, the new kernel is in the gfx950 code object without scratch or LDS, and the mirror makes the calls it should -- over a
scripted backend that records them."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dsgd_amd
from conftest import ROOT
from dsgd_amd import _lib, host
from test_abi import _kernel_notes

NAMES = ("dsgd_plan_create_from_seed_job_lg", "dsgd_lg_eval_job")
HEADER = open(os.path.join(ROOT, "include", "dsgd.h")).read()


def test_library_exports_the_two_entry_points_and_the_binding_lists_them():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dsgd_\w+)", nm))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
    assert re.search(r"\bint dsgd_lg_eval_job\(dsgd_ctx\* ctx, const float\* w", HEADER)
    assert re.search(r"\bint dsgd_plan_create_from_seed_job_lg\(dsgd_ctx\* ctx, uint64_t\* jstate, const int64_t\* job_len", HEADER)
    assert lib.dsgd_abi_version() == 1
    for method in ("lg_plan_from_seed_job", "lg_eval_job"):
        assert callable(getattr(dsgd_amd.Engine, method)), method
    assert callable(host.logistic_rank_rows)


def test_the_header_states_the_contracts():
    lg = HEADER[HEADER.index("THE LOGISTIC MODEL on the resident CSR rows"):]
    across = lg[lg.index(" * ACROSS RANKS (dsgd_comm_init_lg"):lg.index(" * DISTRIBUTED AND SAMPLED EVALUATION")]
    for words in ("dsgd_plan_create_from_seed_job_lg", "dsgd_lg_eval_job (COLLECTIVE)", "rank * n_local + j", "bit for bit what dsgd_lg_predict_ranges",
                  "ONE in-place ncclAllReduce(int64, sum)", "DSGD_ESTATE", "There is no column-slice twin"):
        assert words in across, words
    limits = lg[lg.index(" * LIMITS (out of scope"):lg.index(" * dsgd_lg_gradient: one worker's")]
    assert "dsgd_plan_create_from_seed_job_lg" in limits and "dsgd_lg_eval_job" in limits
    assert "ranks=(world, rank)" in host.LogisticSync.__doc__ and "which no rank holds" in host.LogisticSync.__doc__


def test_refusals_that_need_no_device_write_nothing():
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cnt = np.full(6, -1, dtype=np.int64)
    rl = np.full(2, -1.0)
    rb, re_ = (C.c_int64 * 2)(0, 4), (C.c_int64 * 2)(4, 8)
    loss, acc, K = C.c_double(-1), C.c_double(-1), C.c_int32(-1)
    for k in (2, 0, 257):   # a null context, whatever else is right or wrong
        assert lib.dsgd_lg_eval_job(None, None, rb, re_, k, p(cnt), p(rl), C.byref(loss), C.byref(acc), C.byref(K)) == _lib.EINVAL
    assert b"null context" in lib.dsgd_last_error()
    state = C.c_uint64(0x1234567890AB)
    jl = np.asarray([10, 10], dtype=np.int64)
    sb = np.asarray([0], dtype=np.int64)
    h = C.c_void_p(0)
    n_steps, draws = C.c_int64(-1), C.c_int64(-1)
    assert lib.dsgd_plan_create_from_seed_job_lg(None, C.byref(state), p(jl), 2, 0, 1, p(sb), 10, 5, C.byref(h), C.byref(n_steps),
                                                 C.byref(draws)) == _lib.EINVAL
    assert (loss.value, acc.value, K.value) == (-1, -1, -1) and (cnt == -1).all() and (rl == -1.0).all()
    assert state.value == 0x1234567890AB and not h.value and (n_steps.value, draws.value) == (-1, -1)


def test_the_fold_kernel_is_in_the_code_object_without_scratch_or_lds(tmp_path):
    notes = _kernel_notes(tmp_path)
    kn = {k: v for k, v in notes.items() if "dsgd_lg_eval_fold_kernel" in k}
    assert len(kn) == 1, sorted(kn)
    v = next(iter(kn.values()))
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] <= 32, v
    assert sum("dsgd_lg_predict_ranges_kernel" in k for k in notes) == 1   # the evaluation's launch is the one there was


# ---- host.logistic_rank_rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_train,n_rows,K,world", [(10, 14, 4, 2), (23, 31, 6, 3), (18519, 23149, 3, 1)])
def test_logistic_rank_rows_against_split_vanilla(n_train, n_rows, K, world):
    split = host.split_vanilla(n_train, K)
    tsplit = host.split_vanilla(n_rows - n_train, world)
    assert len(split) == K and len(tsplit) == world
    k = K // world
    seen = []
    for r in range(world):
        rows = host.logistic_rank_rows(n_train, n_rows, K, world, r)
        assert rows.dtype == np.int64
        want = [i for g in split[r * k:(r + 1) * k] for i in g] + [n_train + i for i in tsplit[r]]
        assert rows.tolist() == want
        seen.extend(want)
    assert sorted(seen) == list(range(n_rows))   # every row of the job is one rank's, once


# ---- host.LogisticSync(ranks=...) over a scripted backend ------------------------------------------------------------------
N_TRAIN, N_ROWS, K, WORLD, BATCH = 1000, 1300, 4, 2, 100


class FakePlan:
    def __init__(self, n_samples):
        self.n_samples = n_samples

    def destroy(self):
        pass


class Scripted:
    """Records every call.  refuse_job: lg_plan_from_seed_job answers DSGD_EUNSUPPORTED (-7), nothing drawn."""

    lg_predict_max_ranges = 256

    def __init__(self, refuse_job=False):
        self.calls = []
        self.refuse_job = refuse_job

    def set_weights(self, w):
        pass

    def get_weights(self):
        return np.zeros(4, dtype=np.float32)

    def synchronize(self):
        return {"n_samples": 0, "n_active": 0}

    def lg_plan_from_seed_job(self, jstate, job_lens, first, split_begins, max_samples, batch_size):
        self.calls.append(("lg_plan_from_seed_job", int(jstate), [int(x) for x in job_lens], int(first), [int(x) for x in split_begins],
                           int(max_samples), int(batch_size)))
        if self.refuse_job:
            raise _lib.DsgdError(_lib.EUNSUPPORTED, "scripted: outside the device form")
        rnd = host.JavaRandom(0)   # (what the device draws: ONE stream over all the job's workers)
        rnd.seed = int(jstate)
        begins = np.concatenate([[0], np.cumsum(job_lens)])
        _, offsets, n_steps = host.epoch_lists(rnd, [range(int(begins[i]), int(begins[i + 1])) for i in range(len(job_lens))], max_samples, batch_size)
        return FakePlan(int(offsets[-1])), n_steps, rnd.seed, 0

    def lg_plan_from_seed(self, *a, **k):
        raise AssertionError("the one-process form is not the ranks'")

    def lg_plan_flat(self, idx, offsets, n_steps, n_workers, **kw):
        assert np.asarray(idx).dtype == np.int32 and not kw
        self.calls.append(("lg_plan_flat", np.asarray(idx).copy(), np.asarray(offsets).copy(), int(n_steps), int(n_workers)))
        return FakePlan(int(offsets[-1]))

    def plan_run(self, plan, b, e, lr):
        self.calls.append(("plan_run", int(b), int(e), float(lr)))

    def lg_eval_job(self, ranges, w=None):
        self.calls.append(("lg_eval_job", [tuple(int(x) for x in r) for r in ranges], w))
        n = len(ranges)
        return np.zeros((n * WORLD, 3), np.int64), np.zeros(n * WORLD), 0.5 + n / 16.0, 0.25 + n / 16.0

    def lg_loss_acc_ranges(self, ranges, w=None):   # (the one-process mirror's evaluation)
        self.calls.append(("lg_loss_acc_ranges", [tuple(r) for r in ranges]))
        return [(0.5, 0.5)] * len(ranges)

    def lg_predict_ranges(self, ranges, w=None, want_proba=False):
        self.calls.append(("lg_predict_ranges", [tuple(r) for r in ranges], w))
        total = sum(b - a for a, b in ranges)
        return np.zeros(total, np.int8), None, np.zeros((len(ranges), 3), np.int64), np.zeros(len(ranges)), 0.625, 0.75


def mirror(backend, rank, seed=5, **kw):
    return host.LogisticSync(backend, N_TRAIN, N_ROWS, K, rnd=host.JavaRandom(seed), ranks=(WORLD, rank), **kw)


def never(losses):
    return False


LOCAL_TRAIN = [(0, 250), (250, 500)]
LOCAL_TEST = (500, 650)


@pytest.mark.parametrize("rank", [0, 1])
def test_the_flow_of_an_epoch_under_ranks(rank):
    b = Scripted()
    m = mirror(b, rank)
    m.fit(np.zeros(4, np.float32), 2, BATCH, 0.5, never)
    names = [c[0] for c in b.calls]
    # epoch 1: the job plan, the collective run, the prefetch, the two evaluations; epoch 2 (the last): no prefetch
    assert names == ["lg_plan_from_seed_job", "plan_run", "lg_plan_from_seed_job", "lg_eval_job", "lg_eval_job", "plan_run", "lg_eval_job", "lg_eval_job"]
    first = b.calls[0]
    assert first[1] == host.JavaRandom(5).seed and first[2] == [250] * 4 and first[3] == rank * 2 and first[4] == [0, 250] and first[5:] == (250, BATCH)
    assert b.calls[1] == ("plan_run", 0, 3, 0.5)
    assert b.calls[3][1] == LOCAL_TRAIN and b.calls[4][1] == [LOCAL_TEST] and b.calls[3][2] is None
    assert m.losses == [0.625, 0.625] and m.test_losses == [0.5625, 0.5625] and m.accs == [0.375] * 2 and m.test_accs == [0.3125] * 2
    assert m.steps_run == 6 and m.device_drawn_epochs == 2
    # the stream ends where one process's ends: two epochs of the job's K workers
    one = host.LogisticSync(Scripted(), N_TRAIN, N_ROWS, K, rnd=host.JavaRandom(5), device_lists=False)
    one.fit(np.zeros(4, np.float32), 2, BATCH, 0.5, never)
    assert m.rnd.seed == one.rnd.seed != host.JavaRandom(5).seed


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("how", ["refused", "off"])
def test_the_fall_back_draws_the_whole_job_and_keeps_the_window(rank, how):
    b = Scripted(refuse_job=True)
    m = mirror(b, rank, **({"device_lists": False} if how == "off" else {}))
    m.fit(np.zeros(4, np.float32), 2, BATCH, 0.5, never)
    names = [c[0] for c in b.calls]
    asked = ["lg_plan_from_seed_job"] if how == "refused" else []   # (refused once: the host draws from there on)
    assert names == asked + ["lg_plan_flat", "plan_run", "lg_plan_flat", "lg_eval_job", "lg_eval_job", "plan_run", "lg_eval_job", "lg_eval_job"]
    assert m.device_drawn_epochs == 0 and not m.device_lists
    split = host.split_vanilla(N_TRAIN, K)
    rnd = host.JavaRandom(5)
    k = K // WORLD
    for call in [c for c in b.calls if c[0] == "lg_plan_flat"]:
        idx, offsets, n_steps = host.epoch_lists(rnd, split, 250, BATCH)   # the job's epoch, from the same stream
        _, got_idx, got_offs, got_steps, got_workers = call
        assert (got_steps, got_workers) == (n_steps, k) == (3, 2) and len(got_offs) == n_steps * k + 1 and got_offs[0] == 0
        for s in range(n_steps):
            for j in range(k):
                g = s * K + rank * k + j
                want = idx[offsets[g]:offsets[g + 1]] - split[rank * k + j].start + LOCAL_TRAIN[j][0]   # entry for entry, as local rows
                got = got_idx[got_offs[s * k + j]:got_offs[s * k + j + 1]]
                assert np.array_equal(got, want) and got.min() >= LOCAL_TRAIN[j][0] and got.max() < LOCAL_TRAIN[j][1]
    assert m.rnd.seed == rnd.seed
    one = host.LogisticSync(Scripted(), N_TRAIN, N_ROWS, K, rnd=host.JavaRandom(5), device_lists=False)
    one.fit(np.zeros(4, np.float32), 2, BATCH, 0.5, never)
    assert m.rnd.seed == one.rnd.seed


def test_a_stopped_fit_gives_the_prefetched_epochs_draws_back():
    b = Scripted()
    m = mirror(b, 0)
    m.fit(np.zeros(4, np.float32), 5, BATCH, 0.5, lambda losses: len(losses) >= 1)   # stops behind epoch 1; epoch 2 was prefetched
    one = host.LogisticSync(Scripted(), N_TRAIN, N_ROWS, K, rnd=host.JavaRandom(5), device_lists=False, prefetch=False)
    one.fit(np.zeros(4, np.float32), 1, BATCH, 0.5, never)
    assert m.rnd.seed == one.rnd.seed and m.steps_run == 3


def test_the_other_methods_under_ranks():
    b = Scripted()
    m = mirror(b, 1)
    w = np.ones(4, dtype=np.float32)
    assert m.distributed_loss_and_accuracy(w) == (0.625, 0.375)
    assert b.calls[-1] == ("lg_eval_job", LOCAL_TRAIN, w)
    assert m.distributed_loss() == 0.625 and m.distributed_accuracy() == 0.375
    assert m.local_loss(test=True) == 0.5625 and b.calls[-1][1] == [LOCAL_TEST]
    rows, classes = m.predict()
    assert b.calls[-1][0] == "lg_predict_ranges" and b.calls[-1][1] == LOCAL_TRAIN
    assert np.array_equal(rows, np.arange(500, 1000)) and len(classes) == 500     # this rank's rows, the job's numbers
    seed = m.rnd.seed
    n = len(b.calls)
    for fn in (m.local_sampled_loss, m.local_sampled_accuracy):
        for test in (False, True):
            with pytest.raises(ValueError, match="no rank holds"):
                fn(10, test=test)
    assert len(b.calls) == n and m.rnd.seed == seed     # nothing was asked, nothing was drawn


def test_refusals_of_the_constructor():
    b = Scripted()
    mk = lambda n_train, n_rows, node_count, ranks, **kw: host.LogisticSync(b, n_train, n_rows, node_count, ranks=ranks, **kw)
    with pytest.raises(ValueError, match="k x 2"):      # a K that is not k x world
        mk(N_TRAIN, N_ROWS, 3, (2, 0))
    with pytest.raises(ValueError, match="k x 4"):
        mk(N_TRAIN, N_ROWS, 2, (4, 0))
    assert len(host.split_vanilla(9, 4)) == 3           # a short split: ceil(9 / 4) = 3 rows per group, three groups
    with pytest.raises(ValueError, match="3 groups, not 4"):
        mk(9, 20, 4, (2, 0))
    assert len(host.split_vanilla(9, 4)) == 3 and len(host.split_vanilla(3, 2)) == 2 and len(host.split_vanilla(5, 4)) == 3
    with pytest.raises(ValueError, match="3 slices, not 4"):   # ... of the test rows
        mk(1000, 1005, 4, (4, 0))
    with pytest.raises(ValueError, match="column slices do not span ranks"):
        mk(N_TRAIN, N_ROWS, K, (2, 0), slices=True)
    with pytest.raises(ValueError):
        mk(N_TRAIN, N_ROWS, K, (2, 2))
    with pytest.raises(ValueError):
        host.logistic_rank_rows(9, 20, 4, 2, 0)
    assert b.calls == []
    # the default leaves today's mirror as it is
    m = host.LogisticSync(b, N_TRAIN, N_ROWS, 3)
    assert m.ranks is None
    m.distributed_loss()
    assert b.calls[-1][0] == "lg_predict_ranges"
