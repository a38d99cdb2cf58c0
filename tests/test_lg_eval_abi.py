"""The boundary of the logistic model's distributed and sampled evaluation (include/dsgd.h "THE LOGISTIC MODEL", DISTRIBUTED AND
SAMPLED EVALUATION: dsgd_lg_predict_ranges, dsgd_lg_loss_acc_list, dsgd_lg_loss_acc_sampled) without a GPU: the library exports
the three entry points, the header declares them, the ctypes binding lists them, the refusals that need no device write nothing,
both kernels are in the gfx950 code object without scratch, and host.LogisticSync's new methods make the calls they should --
over a scripted backend that records them."""

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

NAMES = ("dsgd_lg_predict_ranges", "dsgd_lg_loss_acc_list", "dsgd_lg_loss_acc_sampled")
HEADER = open(os.path.join(ROOT, "include", "dsgd.h")).read()


def test_library_exports_the_three_entry_points_and_the_binding_lists_them():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.HIP_LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dsgd_\w+)", nm))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
        assert re.search(r"\bint %s\(dsgd_ctx\* ctx, const float\* w" % name, HEADER), name
    assert lib.dsgd_abi_version() == 1
    for method in ("lg_predict_ranges", "lg_loss_acc_list", "lg_loss_acc_sampled"):
        assert callable(getattr(dsgd_amd.Engine, method)), method
    assert dsgd_amd.Engine.lg_predict_max_ranges == 256


def test_the_header_states_the_contracts_and_the_limits_shrank():
    lg = HEADER[HEADER.index("THE LOGISTIC MODEL on the resident CSR rows"):]
    sec = lg[lg.index(" * DISTRIBUTED AND SAMPLED EVALUATION"):lg.index(" * LIMITS (out of scope")]
    for words in ("the bits of dsgd_lg_loss_acc on range r alone", "the bits of dsgd_lg_predict over the same rows", "the bits of dsgd_lg_loss_acc(b, e)",
                  "the bits of dsgd_lg_loss_acc_list on idx_out", "*jstate untouched", "n_ranges < 1 or > 256", "ranges that overlap", "DSGD_ERANGE",
                  "LOCAL: no collective is entered"):
        assert words in sec, words
    limits = lg[lg.index(" * LIMITS (out of scope"):lg.index(" * dsgd_lg_gradient: one worker's")]
    assert "no predict_ranges" not in limits and "no distributed or sampled evaluation" not in limits
    assert "no evaluation summed over the ranks" in limits and "no fp64 contexts" in limits
    assert "no distributed or sampled evaluation" not in host.LogisticSync.__doc__


def test_refusals_that_need_no_device_write_nothing():
    lib = _lib.load()
    idx = np.arange(4, dtype=np.int32)
    out = np.full(4, 7, dtype=np.int32)
    cls = np.full(8, 7, dtype=np.int8)
    proba = np.full(8, 7.0, dtype=np.float32)
    cnt = np.full(6, -1, dtype=np.int64)
    rl = np.full(2, -1.0)
    rb, re_ = (C.c_int64 * 2)(0, 4), (C.c_int64 * 2)(4, 8)
    loss, acc = C.c_double(-1), C.c_double(-1)
    counts = (C.c_int64 * 3)(-1, -1, -1)
    n, draws = C.c_int64(-1), C.c_int64(-1)
    state = C.c_uint64(0x1234567890AB)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # a null context, whatever else is right or wrong
    for k in (2, 0, 257):
        assert lib.dsgd_lg_predict_ranges(None, None, rb, re_, k, p(cls), p(proba), p(cnt), p(rl), C.byref(loss), C.byref(acc)) == _lib.EINVAL
    assert b"null context" in lib.dsgd_last_error()
    for count in (4, 0, -1):   # n < 1
        assert lib.dsgd_lg_loss_acc_list(None, None, p(idx), count, C.byref(loss), C.byref(acc), counts) == _lib.EINVAL
    assert lib.dsgd_lg_loss_acc_list(None, None, None, 4, C.byref(loss), C.byref(acc), counts) == _lib.EINVAL
    for st in (C.byref(state), None):   # a null jstate
        assert lib.dsgd_lg_loss_acc_sampled(None, None, st, 0, 4, 2, C.byref(loss), C.byref(acc), counts, p(out), C.byref(n), C.byref(draws)) == _lib.EINVAL
    assert lib.dsgd_lg_loss_acc_sampled(None, None, C.byref(state), 0, 4, 0, C.byref(loss), C.byref(acc), counts, p(out), C.byref(n),
                                        C.byref(draws)) == _lib.EINVAL
    assert loss.value == -1 and acc.value == -1 and list(counts) == [-1, -1, -1] and (n.value, draws.value) == (-1, -1)
    assert (out == 7).all() and (cls == 7).all() and (proba == 7.0).all() and (cnt == -1).all() and (rl == -1.0).all()
    assert state.value == 0x1234567890AB


def test_both_kernels_are_in_the_code_object_without_scratch(tmp_path):
    notes = _kernel_notes(tmp_path)
    for name in ("dsgd_lg_predict_ranges_kernel", "dsgd_lg_eval_list_kernel"):
        kn = {k: v for k, v in notes.items() if name in k}
        assert len(kn) == 1, (name, sorted(kn))
        v = next(iter(kn.values()))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0        # (all of the LDS is the launch's: the tile, the tallies, the sums, the table)
        assert v["vgpr_count"] <= 128, (name, v)         # 1024-lane workgroups: four waves per SIMD
    # the siblings they are modelled on are still there, once each
    for name in ("dsgd_lg_eval_kernel", "dsgd_lg_eval_ranges_kernel", "dsgd_lg_predict_kernel"):
        assert sum(name in k for k in notes) == 1, name


# ---- host.LogisticSync over a scripted backend -----------------------------------------------------------------------------
N_TRAIN, N_ROWS = 1000, 1300


class Scripted:
    """Records every call; the figures are functions of the arguments, so that two routes can be compared."""

    lg_predict_max_ranges = 256

    def __init__(self, refuse_device=False):
        self.calls = []
        self.refuse_device = refuse_device

    def lg_predict_ranges(self, ranges, w=None, want_proba=False):
        self.calls.append(("lg_predict_ranges", [tuple(r) for r in ranges], w, want_proba))
        total = sum(b - a for a, b in ranges)
        cls = (np.arange(total) % 3 - 1).astype(np.int8)
        return cls, None, np.zeros((len(ranges), 3), np.int64), np.zeros(len(ranges)), 0.625, 0.75

    def lg_loss_acc_list(self, idx, w=None):
        idx = np.asarray(idx)
        assert idx.dtype == np.int32
        self.calls.append(("lg_loss_acc_list", idx.copy()))
        return float(idx.sum()) / 1e6, float(idx[0]) / 1e4, [len(idx), 0, 0]

    def lg_loss_acc_sampled(self, jstate, lo, hi, k, w=None, want_idx=False):
        self.calls.append(("lg_loss_acc_sampled", int(jstate), lo, hi, k))
        if self.refuse_device:
            raise _lib.DsgdError(_lib.EUNSUPPORTED, "scripted: outside the device form")
        rnd = host.JavaRandom(0)
        rnd.seed = int(jstate)
        idx = (host.sampled_list(rnd, hi - lo, k) + np.int32(lo)).astype(np.int32)   # (what the device draws: the same stream)
        return float(idx.sum()) / 1e6, float(idx[0]) / 1e4, [len(idx), 0, 0], rnd.seed, hi - lo - 1


def master(backend, node_count=3, seed=5):
    return host.LogisticSync(backend, N_TRAIN, N_ROWS, node_count, rnd=host.JavaRandom(seed))


def test_distributed_methods_make_one_call_over_the_splits():
    b = Scripted()
    m = master(b)
    split = host.split_vanilla(N_TRAIN, 3)
    rows, classes = m.predict()
    assert [c[0] for c in b.calls] == ["lg_predict_ranges"]
    assert b.calls[0][1] == [(r.start, r.stop) for r in split] and b.calls[0][2] is None
    assert rows.dtype == np.int64 and np.array_equal(rows, np.arange(N_TRAIN)) and classes.dtype == np.int8 and len(classes) == N_TRAIN
    w = np.ones(4, dtype=np.float32)
    assert m.distributed_loss_and_accuracy(w) == (0.625, 0.75)
    assert len(b.calls) == 2 and b.calls[1][2] is w            # one more call, with the weights handed over
    assert m.distributed_loss() == 0.625 and m.distributed_accuracy() == 0.75
    assert [c[0] for c in b.calls] == ["lg_predict_ranges"] * 4
    assert m.rnd.seed == host.JavaRandom(5).seed               # the distributed calls draw nothing


def test_more_than_256_splits_is_a_value_error():
    b = Scripted()
    many = lambda k: host.LogisticSync(b, k, k + 10, k)   # (one row per split: vanilla yields k of them)
    assert len(host.split_vanilla(257, 257)) == 257
    with pytest.raises(ValueError):
        many(257).predict()
    with pytest.raises(ValueError):
        many(257).distributed_loss()
    assert b.calls == []
    many(256).predict()
    assert len(b.calls) == 1 and len(b.calls[0][1]) == 256


@pytest.mark.parametrize("test", [False, True])
def test_sampled_chain_device_leg_on_and_off(monkeypatch, test):
    lo, hi = (N_TRAIN, N_ROWS) if test else (0, N_TRAIN)
    results = {}
    for route, env, refuse in (("host", "0", False), ("device", "1", False), ("refused", "1", True)):
        monkeypatch.setenv("DSGD_SAMPLED_DEVICE", env)
        b = Scripted(refuse_device=refuse)
        m = master(b)
        loss = m.local_sampled_loss(100, test=test)
        acc = m.local_sampled_accuracy(40, test=test)      # a second call: a second, different sample from where the first left
        results[route] = (loss, acc, m.rnd.seed, [c[0] for c in b.calls])
        for c in b.calls:
            if c[0] == "lg_loss_acc_list":
                assert c[1].min() >= lo and c[1].max() < hi and len(set(c[1].tolist())) == len(c[1])
            else:
                assert c[2:4] == (lo, hi)
    assert results["host"][3] == ["lg_loss_acc_list"] * 2
    assert results["device"][3] == ["lg_loss_acc_sampled"] * 2
    assert results["refused"][3] == ["lg_loss_acc_sampled", "lg_loss_acc_list"] * 2
    # the same numbers and the same generator state whichever side drew
    assert results["host"][:3] == results["device"][:3] == results["refused"][:3]
    # ... and the state is the one a whole shuffle of the window, twice, leaves
    rnd = host.JavaRandom(5)
    first = host.sampled_list(rnd, hi - lo, 100) + lo
    second = host.sampled_list(rnd, hi - lo, 40) + lo
    assert results["host"][2] == rnd.seed
    assert results["host"][0] == float(first.sum()) / 1e6 and results["host"][1] == float(second[0]) / 1e4
    # the device leg is off by default
    monkeypatch.delenv("DSGD_SAMPLED_DEVICE")
    b = Scripted()
    master(b).local_sampled_loss(10, test=test)
    assert [c[0] for c in b.calls] == ["lg_loss_acc_list"]


def test_sampled_calls_raise_while_a_prefetched_plan_is_pending_and_on_an_empty_sample(monkeypatch):
    monkeypatch.delenv("DSGD_SAMPLED_DEVICE", raising=False)
    b = Scripted()
    m = master(b)
    m._pending = {"plan": None, "seed_before": m.rnd.seed}
    seed = m.rnd.seed
    with pytest.raises(RuntimeError):
        m.local_sampled_loss(10)
    with pytest.raises(RuntimeError):
        m.local_sampled_accuracy(10, test=True)
    m._pending = None
    with pytest.raises(ValueError):
        m.local_sampled_loss(0)
    assert b.calls == [] and m.rnd.seed == seed      # nothing was asked, nothing was drawn
    assert m.local_sampled_loss(10) is not None
    # an error that is no refusal goes up, and the device drew nothing

    class Broken(Scripted):
        def lg_loss_acc_sampled(self, *a, **k):
            raise _lib.DsgdError(_lib.ESTATE, "scripted: the engine is running")

    monkeypatch.setenv("DSGD_SAMPLED_DEVICE", "1")
    m2 = master(Broken())
    with pytest.raises(_lib.DsgdError):
        m2.local_sampled_loss(10)
    assert m2.rnd.seed == host.JavaRandom(5).seed
