"""Distributed evaluation on the device (-m gpu): Engine.predict_ranges (dsgd_predict_ranges / _f64; csrc/dsgd_predict.hpp)
-- the forward passes of all workers' splits and their exact tallies in ONE launch (core/Master.scala:61-98) -- in an fp32
context and in fp64 contexts on float and on Double feature values.

What is asserted, and why it can be exact: a row's prediction and its tally are decided on one x . w, computed with the
routine the context's evaluation kernel uses, and the forward kernels add the same products in the same order; so the
predictions equal Engine.forward / forward_f64 entry for entry and the per-range counts equal Engine.loss_acc's.  Against
the fp64 oracle the predictions are compared on every row whose oracle margin |x . w| is at least GATE_EPS = 1e-5 (the
gate band of tests/test_gpu_parity.py); rows without a non-zero are compared exactly (0 == 0), and the excluded share must
stay within 0.1 % of the rows.  On the data below (seed 20, L2-normalised rows, normal weights) the oracle alone excludes
NO row (checked on the CPU): five margins are exactly 0, the empty rows, and the smallest other one is 3.3e-4.

Data: 2,003 rows over D = 3,000 columns (the row-wise evaluation stages 1,024 weights in LDS for calls below 4,096 rows,
so columns fall on both sides of the tile; DSGD_HSPLIT = 512 puts the streams' split below D as well), Zipfian columns,
five rows without a non-zero, one row of 300 entries (more than G x UNR = 256 at the widest group), labels of both signs.
"""

import ctypes as C
import os

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import host
from oracle import oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

GATE_EPS = 1e-5          # tests/test_gpu_parity.py
N, N_TRAIN, D, LAM = 2003, 1800, 3000, 1e-5
EMPTY_ROWS = (0, 258, 777, 1799, 2002)
LONG_ROW = 1234
# lengths 1, 257 and the rest, plus one empty range; then the same rows as a single range
SPLITS = [(0, 1), (1, 258), (258, 258), (258, N)]
KINDS = ("fp32", "fp64", "fp64v")


def make_data(seed=20):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, D + 1) ** 1.1
    p /= p.sum()
    row_ptr, col, val = [0], [], []
    for i in range(N):
        n = 0 if i in EMPTY_ROWS else (300 if i == LONG_ROW else int(rng.integers(1, 60)))
        keys = np.sort(rng.choice(D, size=n, replace=False, p=p if n < 100 else None)) + 1   # 1-based feature ids
        v = rng.normal(size=n)
        if n:
            v /= np.linalg.norm(v)
        col.extend(keys.tolist())
        val.extend(v.tolist())
        row_ptr.append(len(col))
    label = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=N)
    return (np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float64), label,
            rng.normal(size=D + 1))


@pytest.fixture(scope="module")
def data():
    return make_data()


@pytest.fixture(scope="module")
def engines(data):
    """One context per kind, data loaded, dimSparsity built, and the oracle over the values that context holds."""
    row_ptr, col, val64, label, _ = data
    old = os.environ.get("DSGD_HSPLIT")
    os.environ["DSGD_HSPLIT"] = "512"   # (read when a context is created)
    out = {}
    try:
        for kind in KINDS:
            val = val64 if kind == "fp64v" else val64.astype(np.float32)
            eng = dsgd_amd.Engine(D, LAM, precision="fp32" if kind == "fp32" else "fp64")
            eng.load_csr(row_ptr, col, val, label)
            eng.build_dim_sparsity(N_TRAIN)
            assert eng.value_bits() == (64 if kind == "fp64v" else 32)
            o = orc.Oracle(D, row_ptr, col, val.astype(np.float64), label, LAM)
            o.set_dim_sparsity(o.dim_sparsity(N_TRAIN))
            out[kind] = (eng, o)
    finally:
        if old is None:
            del os.environ["DSGD_HSPLIT"]
        else:
            os.environ["DSGD_HSPLIT"] = old
    yield out
    for eng, _ in out.values():
        eng.close()


@pytest.fixture(scope="module")
def oracle_side(data, engines):
    """Per kind: the weights as the context holds them, the oracle's predictions, margins and tallies -- computed once."""
    w_norm = data[4]
    out = {}
    for kind, (_, o) in engines.items():
        w = w_norm.astype(np.float32).astype(np.float64) if kind == "fp32" else w_norm
        out[kind] = {"w": w, "pred": o.forward(w, np.arange(N)), "margin": np.abs([o.row_dot(i, w) for i in range(N)]),
                     "loss_acc": o.loss_acc(w, 0, N)}
    return out


def set_w(eng, kind, w):
    eng.set_weights(np.asarray(w, dtype=np.float32 if kind == "fp32" else np.float64))


def forward_of(eng, kind, rows):
    return eng.forward(rows) if kind == "fp32" else eng.forward_f64(rows)


def host_counts(pred, label):
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    return [int(np.count_nonzero((pred != 0) & (pred == label))), int(np.count_nonzero(pred == 0)),
            int(np.count_nonzero((pred != 0) & (pred != label)))]


def rows_of(ranges):
    return np.concatenate([np.arange(b, e, dtype=np.int32) for b, e in ranges])


@pytest.mark.parametrize("ranges", [SPLITS, [(0, N)]], ids=["four_ranges", "single_range"])
@pytest.mark.parametrize("kind", KINDS)
def test_predictions_and_tallies_come_from_one_dot(engines, oracle_side, data, kind, ranges):
    eng, _ = engines[kind]
    label = data[3]
    ref = oracle_side[kind]
    set_w(eng, kind, ref["w"])
    pred, counts, loss, acc = eng.predict_ranges(ranges)
    rows = rows_of(ranges)
    assert pred.dtype == np.int8 and len(pred) == len(rows) == N and counts.shape == (len(ranges), 3)
    assert set(np.unique(pred).tolist()) <= {-1, 0, 1}
    assert (pred[np.isin(rows, EMPTY_ROWS)] == 0).all()            # a row with no non-zeros predicts 0
    # entry for entry the forward kernel's predictions
    assert np.array_equal(pred.astype(np.float64), np.asarray(forward_of(eng, kind, rows), dtype=np.float64))
    # per range the evaluation kernel's tallies; the host's recount from the returned bytes gives the same numbers
    off = 0
    for k, (b, e) in enumerate(ranges):
        if e == b:
            assert counts[k].tolist() == [0, 0, 0]
            continue
        assert counts[k].tolist() == eng.loss_acc(b, e)[2], (k, b, e)
        assert counts[k].tolist() == host_counts(pred[off:off + e - b], label[b:e]), (k, b, e)
        off += e - b
    l_ref, a_ref, c_ref = eng.loss_acc(0, N)                         # (the splits are adjacent: their union is one range)
    assert counts.sum(axis=0).tolist() == c_ref and loss == l_ref and acc == a_ref
    # the oracle: equal wherever its margin is outside the gate band; empty rows are 0 == 0 and not excluded
    near = (ref["margin"] < GATE_EPS) & ~np.isin(np.arange(N), EMPTY_ROWS)
    print("%s: %d rows within %.0e of the gate, smallest non-zero margin %.3e" % (
        kind, int(near.sum()), GATE_EPS, ref["margin"][ref["margin"] > 0].min()))
    assert near.sum() <= 0.001 * N
    keep = ~near[rows]
    assert np.array_equal(pred[keep].astype(np.float64), ref["pred"][rows][keep])
    if not near.any():
        o_loss, o_acc, o_counts, _ = ref["loss_acc"]
        assert counts.sum(axis=0).tolist() == list(o_counts) and acc == o_acc
        # the tallies are exact; |w|^2 is a sum of D + 1 squares in the context's precision: (D + 1) roundings at the most
        nsq = float((ref["w"] ** 2).sum())
        assert abs(loss - o_loss) <= LAM * nsq * (D + 1) * 2.0 ** (-24 if kind == "fp32" else -53)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_weights(engines, kind):
    eng, _ = engines[kind]
    zero = np.zeros(D + 1, dtype=np.float32 if kind == "fp32" else np.float64)
    for ranges in (SPLITS, [(0, N)]):
        pred, counts, loss, acc = eng.predict_ranges(ranges, w=zero)   # (w given: the float form on fp32, the _f64 form otherwise)
        assert not pred.any() and len(pred) == N
        assert counts.tolist() == [[0, e - b, 0] for b, e in ranges]
        assert loss == 1.0 and acc == 0.0                                # the reference's first two log lines (Main.scala:75-78)
    assert not eng.get_weights().any()                                   # w replaced the resident weights


@pytest.mark.parametrize("kind", KINDS)
def test_given_weights_equal_resident_weights(engines, oracle_side, kind):
    eng, _ = engines[kind]
    w = oracle_side[kind]["w"]
    set_w(eng, kind, np.zeros(D + 1))
    given = eng.predict_ranges(SPLITS, w=w.astype(np.float32) if kind == "fp32" else w)
    resident = eng.predict_ranges(SPLITS)
    assert np.array_equal(given[0], resident[0]) and np.array_equal(given[1], resident[1]) and given[2:] == resident[2:]
    assert np.array_equal(eng.get_weights(), w.astype(np.float32) if kind == "fp32" else w)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_change_nothing(engines, oracle_side, kind):
    eng, _ = engines[kind]
    w = oracle_side[kind]["w"]
    set_w(eng, kind, w)
    before = eng.get_weights().copy()
    other = np.ones(D + 1, dtype=np.float32 if kind == "fp32" else np.float64)   # would replace the weights if a refused call got that far
    lists = [np.arange(k * 50, (k + 1) * 50, dtype=np.int32) for k in range(3)]

    def refused(exc, ranges, w_arg=other):
        with pytest.raises(exc):
            eng.predict_ranges(ranges, w=w_arg)
        assert np.array_equal(eng.get_weights(), before)

    refused(ValueError, [(0, 100), (99, 200)])            # overlapping ranges
    refused(ValueError, [(0, 100), (300, 400), (50, 60)])   # ... in any order
    refused(ValueError, [(10, 5)])                         # begin > end
    refused(ValueError, [(5, 5), (9, 9)])                  # no rows at all
    refused(ValueError, [])                                # no ranges
    refused(IndexError, [(0, 10), (N - 1, N + 1)])         # a row beyond the data
    refused(IndexError, [(-1, 10)])
    refused(ValueError, [(i, i + 1) for i in range(257)])  # K = 257
    if kind != "fp32":                                     # a float w through the float form on an fp64 context
        rb, re_ = (C.c_int64 * 1)(0), (C.c_int64 * 1)(10)
        pred = np.zeros(10, dtype=np.int8)
        w32 = np.ones(D + 1, dtype=np.float32)
        rc = eng._lib.dsgd_predict_ranges(eng._ctx, w32.ctypes.data_as(C.c_void_p), rb, re_, 1,
                                          pred.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == dsgd_amd._lib.EINVAL
        assert np.array_equal(eng.get_weights(), before)
    else:                                                  # the Double form needs an fp64 context
        with pytest.raises(dsgd_amd.DsgdError):
            rb, re_ = (C.c_int64 * 1)(0), (C.c_int64 * 1)(10)
            pred = np.zeros(10, dtype=np.int8)
            dsgd_amd._lib.check(eng._lib.dsgd_predict_ranges_f64(eng._ctx, None, rb, re_, 1, pred.ctypes.data_as(C.c_void_p),
                                                                 None, None, None))
        assert np.array_equal(eng.get_weights(), before)
    # K = 256 is served, and the context goes on working: a step, then an evaluation that agrees with loss_acc again
    pred, counts, _, _ = eng.predict_ranges([(i, i + 1) for i in range(256)])
    assert len(pred) == 256 and counts.shape == (256, 3) and (counts.sum(axis=1) == 1).all()
    st = eng.sync_step(lists, 0.5)
    assert st["n_samples"] == 150
    assert not np.array_equal(eng.get_weights(), before)
    _, counts, loss, acc = eng.predict_ranges(SPLITS)
    l_ref, a_ref, c_ref = eng.loss_acc(0, N)
    assert counts.sum(axis=0).tolist() == c_ref and loss == l_ref and acc == a_ref


@pytest.mark.parametrize("kind", KINDS)
def test_masters_distributed_loss_and_accuracy_equal_the_local_ones(engines, oracle_side, kind):
    eng, _ = engines[kind]
    set_w(eng, kind, oracle_side[kind]["w"])
    for master in (host.MasterSync(eng, N_TRAIN, N, node_count=3), host.MasterAsync(eng, N_TRAIN, N, node_count=3)):
        assert master.distributed_loss() == eng.loss_acc(0, N_TRAIN)[0]
        assert master.distributed_accuracy() == eng.loss_acc(0, N_TRAIN)[1]
        rows, pred = master.predict()
        assert rows.tolist() == list(range(N_TRAIN)) and pred.dtype == np.int8
        assert np.array_equal(pred.astype(np.float64), np.asarray(forward_of(eng, kind, rows.astype(np.int32)), dtype=np.float64))
    m = host.MasterSync(eng, N_TRAIN, N, node_count=3)
    assert m.distributed_loss() == m.local_loss() and m.distributed_accuracy() == m.local_accuracy()


# ---- more rows than lane groups: the persistent loop, the carried counters, the flush at a range boundary ----------------
# The fp32 launch holds at most n_cu workgroups of 1,024 / G groups (G >= 8: 32,768 groups on 256 CUs), the fp64 launch at
# most 8 * n_cu workgroups of 16 groups (32,768 again).  With 40,003 rows every launch has groups that own two or more
# ordinals t, t + n_groups, ..., and the ranges below are cut so that a group's successive ordinals fall into different
# ranges (and, ranges 3 and 5, into the same one): lengths 5, 0, 19,995, 13,003, 3, 6,997 -- given out of row order, so
# the range-major order of the reply is not the row order.  From 4,096 rows on the fp32 launch stages the full weight tile
# (40,960 of D + 1 = 47,237 weights: columns on both sides).
BIG_N = 40003
BIG_RANGES = [(20000, 33003), (0, 5), (7, 7), (5, 20000), (33003, 33006), (33006, BIG_N)]


@pytest.fixture(scope="module")
def big():
    data = dsgd_amd.synth.generate(BIG_N, seed=41)
    # Double values that no float holds: every value times (1 + u * 2^-24)
    val64 = data.val.astype(np.float64) * (1.0 + (np.random.default_rng(4).random(data.nnz) * 2.0 - 1.0) * 2.0 ** -24)
    return data, val64, np.random.default_rng(6).normal(size=data.dim + 1)


@pytest.mark.parametrize("kind", KINDS)
def test_groups_that_own_several_rows_across_ranges(big, kind):
    data, val64, w = big
    with dsgd_amd.Engine(data.dim, LAM, precision="fp32" if kind == "fp32" else "fp64") as eng:
        eng.load_csr(data.row_ptr, data.col, val64 if kind == "fp64v" else data.val, data.label)
        eng.build_dim_sparsity(BIG_N)
        set_w(eng, kind, w)
        rows = rows_of(BIG_RANGES)
        assert len(rows) == BIG_N and len(np.unique(rows)) == BIG_N
        fwd = np.asarray(forward_of(eng, kind, rows), dtype=np.float64)   # the reference: one group per listed row, no carry
        pred, counts, loss, acc = eng.predict_ranges(BIG_RANGES)
        assert np.array_equal(pred.astype(np.float64), fwd)
        off = 0
        for k, (b, e) in enumerate(BIG_RANGES):
            # per range: the host's recount from FORWARD's predictions and the labels
            assert counts[k].tolist() == host_counts(fwd[off:off + e - b], data.label[b:e]), (k, b, e)
            # ... and the evaluation kernel's tallies wherever it is the row-wise kernel that computes them (fp64: always;
            # fp32: ranges below 4,096 rows -- beyond, dsgd_loss_acc streams the split matrix in another summation order)
            if e > b and (kind != "fp32" or e - b < 4096):
                assert counts[k].tolist() == eng.loss_acc(b, e)[2], (k, b, e)
            off += e - b
        total = counts.sum(axis=0)
        assert total.sum() == BIG_N and acc == total[0] / BIG_N
        nsq = float((np.asarray(eng.get_weights(), dtype=np.float64) ** 2).sum())
        assert abs(loss - (LAM * nsq + (total[1] + 2.0 * total[2]) / BIG_N)) <= LAM * nsq * (data.dim + 1) * 2.0 ** (-24 if kind == "fp32" else -53)
        # the same rows as ONE range in row order: the same bytes, permuted back
        pred1, counts1, _, _ = eng.predict_ranges([(0, BIG_N)])
        assert np.array_equal(pred1[rows], pred) and counts1[0].tolist() == total.tolist()
