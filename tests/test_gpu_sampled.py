"""Sampled evaluation on the device (-m gpu): Engine.loss_acc_list and Engine.loss_acc_sampled (dsgd_loss_acc_list /
dsgd_loss_acc_sampled and their _f64 forms; csrc/dsgd_eval_list.hpp) -- Master.localSampledLoss / localSampledAccuracy
(core/Master.scala:109-118) -- in an fp32 context and in fp64 contexts on float and on Double feature values.

What is asserted, and why it can be exact: a listed row is decided on the x . w that dsgd_predict_ranges decides it on,
which is the forward kernels' (tests/test_gpu_predict.py), so the tallies of a list equal the tallies folded on the host
from Engine.forward / forward_f64 over that list, and those of idx = lo .. hi - 1 equal Engine.loss_acc(lo, hi) (fp32:
below 4,096 rows, the condition include/dsgd.h states).  The sampled form draws its list with the device's trace of the
reference's random stream: list, generator state and draw count equal csrc/jrand.c's (dsgd_jrand_shuffle), entry for entry.
Against the fp64 oracle the class of a row is compared wherever the oracle's margin |x . w| is at least GATE_EPS = 1e-5.

Data: the generator of tests/test_gpu_predict.py (copied): 2,003 rows over D = 3,000 columns, DSGD_HSPLIT = 512, five rows
without a non-zero, one row of 300 entries, labels of both signs, normal weights.
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
KINDS = ("fp32", "fp64", "fp64v")
EUNSUPPORTED, ESTATE, EINVAL, ERANGE = dsgd_amd._lib.EUNSUPPORTED, dsgd_amd._lib.ESTATE, dsgd_amd._lib.EINVAL, dsgd_amd._lib.ERANGE


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
    """One context per kind, data loaded, dimSparsity built, the weights set, and the oracle over the values it holds."""
    row_ptr, col, val64, label, w_norm = data
    old = os.environ.get("DSGD_HSPLIT")
    os.environ["DSGD_HSPLIT"] = "512"   # (read when a context is created)
    out = {}
    try:
        for kind in KINDS:
            val = val64 if kind == "fp64v" else val64.astype(np.float32)
            eng = dsgd_amd.Engine(D, LAM, precision="fp32" if kind == "fp32" else "fp64")
            eng.load_csr(row_ptr, col, val, label)
            eng.build_dim_sparsity(N_TRAIN)
            o = orc.Oracle(D, row_ptr, col, val.astype(np.float64), label, LAM)
            w = w_norm.astype(np.float32).astype(np.float64) if kind == "fp32" else w_norm
            set_w(eng, kind, w)
            out[kind] = (eng, o, w)
    finally:
        if old is None:
            del os.environ["DSGD_HSPLIT"]
        else:
            os.environ["DSGD_HSPLIT"] = old
    yield out
    for eng, _, _ in out.values():
        eng.close()


@pytest.fixture(scope="module")
def forward_all(engines):
    """Per kind: the forward kernel's predictions of every row under the module's weights -- computed once, never changed."""
    return {kind: np.asarray(forward_of(eng, kind, np.arange(N, dtype=np.int32)), dtype=np.int64) for kind, (eng, _, _) in engines.items()}


def set_w(eng, kind, w):
    eng.set_weights(np.asarray(w, dtype=np.float32 if kind == "fp32" else np.float64))


def forward_of(eng, kind, rows):
    return eng.forward(rows) if kind == "fp32" else eng.forward_f64(rows)


def host_counts(pred, label):
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    return [int(np.count_nonzero((pred != 0) & (pred == label))), int(np.count_nonzero(pred == 0)),
            int(np.count_nonzero((pred != 0) & (pred != label)))]


@pytest.fixture(scope="module")
def lam_nsq(engines, forward_all, data):
    """Per kind lambda |w|^2 as dsgd_loss_acc takes it, under the module's weights: the loss of ONE correctly classified
    row is lambda |w|^2 + 0 / 1, the product itself."""
    out = {}
    for kind, (eng, _, _) in engines.items():
        row = int(np.flatnonzero(forward_all[kind] == data[3])[0])
        loss, _, counts = eng.loss_acc(row, row + 1)
        assert counts == [1, 0, 0]
        out[kind] = loss
    return out


def jrand_shuffle(state, length):
    """(shuffled 0 .. length - 1, state after, raw values consumed) by csrc/jrand.c"""
    lib = host._host_lib()
    assert lib is not None, "lib/libdsgd_host.so is not built"
    buf = np.arange(length, dtype=np.int32)
    st = C.c_uint64(state)
    draws = lib.dsgd_jrand_shuffle(C.byref(st), buf.ctypes.data_as(C.c_void_p), C.c_int64(length))
    return buf, int(st.value), int(draws)


def lists_under_test():
    rng = np.random.default_rng(5)
    every = np.arange(N, dtype=np.int32)
    repeats = np.asarray([EMPTY_ROWS[1]] * 3 + [LONG_ROW] * 2 + [5, 5, 6, 1999, LONG_ROW - 1, EMPTY_ROWS[1] + 1], dtype=np.int32)
    out = {"in_order": every, "permutation": rng.permutation(N).astype(np.int32), "repeats": repeats}
    for n in (1, 63, 64, 65, 4097):   # (4,097: by tiling -- from 4,096 entries on the fp32 launch stages the large weight tile)
        out["len%d" % n] = np.resize(rng.permutation(N).astype(np.int32), n)
    return out


LISTS = lists_under_test()


# ---- 1. the list form against forward: exact ----
@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("kind", KINDS)
def test_list_tallies_equal_the_forward_kernels(engines, forward_all, lam_nsq, data, kind, name):
    eng, _, w = engines[kind]
    label, idx = data[3], LISTS[name]
    want = host_counts(forward_all[kind][idx], label[idx])
    loss, acc, counts = eng.loss_acc_list(idx)
    assert counts == want and sum(counts) == len(idx)
    # include/dsgd.h: loss = lambda |w|^2 + (c1 + 2 c2) / n, acc = c0 / n -- the same operations on the same doubles
    n = float(len(idx))
    assert loss == lam_nsq[kind] + (float(want[1]) + 2.0 * float(want[2])) / n and acc == float(want[0]) / n
    # an explicit w (of the context's own width) replaces the resident weights and gives the same answer
    set_w(eng, kind, np.zeros(D + 1))
    wv = np.asarray(w, dtype=np.float32 if kind == "fp32" else np.float64)
    assert eng.loss_acc_list(idx, w=wv) == (loss, acc, counts)
    assert np.array_equal(eng.get_weights(), wv)


# ---- 2. the list form against dsgd_loss_acc: exact ----
@pytest.mark.parametrize("kind", KINDS)
def test_list_of_a_range_equals_loss_acc(engines, kind):
    eng, _, _ = engines[kind]
    for lo, hi in ((0, N), (0, N_TRAIN), (N_TRAIN, N), (1234, 1235), (257, 258 + 64)):
        assert eng.loss_acc_list(np.arange(lo, hi, dtype=np.int32)) == eng.loss_acc(lo, hi), (lo, hi)


# ---- 3. the list form against the fp64 oracle ----
@pytest.mark.parametrize("kind", KINDS)
def test_classes_against_the_oracle(engines, data, kind):
    eng, o, w = engines[kind]
    label = data[3].astype(np.int64)
    pred = np.asarray(o.forward(w, np.arange(N)), dtype=np.int64)
    margin = np.abs([o.row_dot(i, w) for i in range(N)])
    empty = np.isin(np.arange(N), EMPTY_ROWS)
    near = (margin < GATE_EPS) & ~empty
    print("%s: %d rows within %.0e of the gate" % (kind, int(near.sum()), GATE_EPS))
    assert near.sum() <= 0.001 * N
    # the class of a row, from a list of that row alone: 0 = p == y, 1 = p == 0, 2 = p == -y
    got = np.asarray([int(np.argmax(eng.loss_acc_list(np.asarray([i], dtype=np.int32))[2])) for i in range(N)])
    want = np.where(pred == 0, 1, np.where(pred == label, 0, 2))
    assert (got[empty] == 1).all() and (want[empty] == 1).all()
    assert np.array_equal(got[~near], want[~near])
    # ... and the tallies of the whole list are the oracle's where no row is excluded
    if not near.any():
        assert eng.loss_acc_list(np.arange(N, dtype=np.int32))[2] == [int(c) for c in o.loss_acc(w, 0, N)[2]]


# ---- 4. the sampled form against csrc/jrand.c: entry for entry ----
def check_sampled(eng, state, lo, hi, k):
    length = hi - lo
    shuffled, state_after, draws = jrand_shuffle(state, length)
    n = min(k, length)
    want_idx = (shuffled[:n] + lo).astype(np.int32)
    loss, acc, counts, st, dr, idx = eng.loss_acc_sampled(state, lo, hi, k, want_idx=True)
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx), (lo, hi, k)
    assert (st, dr) == (state_after, draws), (lo, hi, k)
    assert (loss, acc, counts) == eng.loss_acc_list(want_idx), (lo, hi, k)
    assert eng.loss_acc_sampled(state, lo, hi, k) == (loss, acc, counts, st, dr)   # (without the list: the same numbers)
    return st, dr


@pytest.mark.parametrize("window", [(0, N_TRAIN), (N_TRAIN, N)], ids=["train", "test"])
@pytest.mark.parametrize("kind", KINDS)
def test_sampled_equals_jrand(engines, kind, window):
    eng, _, _ = engines[kind]
    lo, hi = window
    length = hi - lo
    state = host.JavaRandom(11).seed
    for k in [k for k in (1, 2, 1023, 1024, 1025) if k <= length] + [length, length + 7]:   # (where they fit the window)
        state, _ = check_sampled(eng, state, lo, hi, k)   # (every case continues the stream of the one before)


@pytest.mark.parametrize("kind", KINDS)
def test_sampled_small_and_power_of_two_windows(engines, kind):
    eng, _, _ = engines[kind]
    state = host.JavaRandom(3).seed
    # one row: nothing is drawn, that row is evaluated
    loss, acc, counts, st, dr, idx = eng.loss_acc_sampled(state, 700, 701, 5, want_idx=True)
    assert (st, dr, idx.tolist()) == (state, 0, [700])
    assert (loss, acc, counts) == eng.loss_acc_list(np.asarray([700], dtype=np.int32))
    # two rows: one draw
    assert check_sampled(eng, state, 700, 702, 2)[1] == 1
    assert check_sampled(eng, state, 700, 702, 1)[1] == 1
    # 1,024 rows: the first draw's bound is a power of two (nextInt's other branch)
    for k in (1, 100, 1024):
        check_sampled(eng, state, 500, 500 + 1024, k)


# ---- 5. rejections ----
@pytest.fixture(scope="module")
def wide():
    """Rows with one non-zero each, as many as the largest window a test asks for plus one."""
    n, d = (1 << 20) + 1, 1000
    eng = dsgd_amd.Engine(d, LAM)
    i = np.arange(n)
    eng.load_csr(np.arange(n + 1, dtype=np.int64), (i % d + 1).astype(np.int32), np.where(i % 3 == 0, -1.0, 1.0).astype(np.float32),
                 np.where(i % 2 == 0, -1, 1).astype(np.int8))
    eng.build_dim_sparsity(n)
    eng.set_weights(np.linspace(-1.0, 1.0, d + 1).astype(np.float32))
    yield eng, n
    eng.close()


def test_rejections_inside_the_shuffle(wide):
    eng, _ = wide
    length, k = 300000, 5000
    state = host.JavaRandom(2024).seed
    shuffled, state_after, draws = jrand_shuffle(state, length)
    assert draws > length - 1, "the host reports no rejection for this seed: the test would be vacuous (expected len^2 / 2^33 = 10)"
    loss, acc, counts, st, dr, idx = eng.loss_acc_sampled(state, 0, length, k, want_idx=True)
    assert np.array_equal(idx, shuffled[:k]) and (st, dr) == (state_after, draws)
    assert (loss, acc, counts) == eng.loss_acc_list(shuffled[:k])
    # two sampled calls, then a device-drawn plan from the running state: the stream is the host's throughout
    rnd = host.JavaRandom(0)
    rnd.seed = state
    running = state
    for kk in (777, 2048):
        want = host.sampled_list(rnd, length, kk, native=True)
        *_, running, _, idx = eng.loss_acc_sampled(running, 0, length, kk, want_idx=True)
        assert np.array_equal(idx, want) and running == rnd.seed
    plan, n_steps, after, _ = eng.plan_from_seed_job(running, [length], 0, [0], 3000, 1000)
    try:
        got_idx, got_off = eng.plan_lists(plan)
        want_idx, want_off, want_steps = host.epoch_lists(rnd, [range(0, length)], 3000, 1000, native=True)
        assert n_steps == want_steps == 3 and after == rnd.seed
        assert np.array_equal(got_off, want_off) and np.array_equal(got_idx, want_idx)
    finally:
        plan.destroy()


# ---- 6. refusals: nothing drawn, nothing written ----
def raw_sampled(eng, fn, w, state, lo, hi, k):
    """The C call with sentinels in every output: (rc, state after, outputs untouched?)"""
    st = C.c_uint64(state)
    loss, acc = C.c_double(-7.0), C.c_double(-7.0)
    counts = (C.c_int64 * 3)(-7, -7, -7)
    idx = np.full(max(1, min(max(k, 1), 4096)), -7, dtype=np.int32)
    n, draws = C.c_int64(-7), C.c_int64(-7)
    rc = getattr(eng._lib, fn)(eng._ctx, None if w is None else w.ctypes.data_as(C.c_void_p), C.byref(st), lo, hi, k, C.byref(loss),
                               C.byref(acc), counts, idx.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(draws))
    untouched = (loss.value, acc.value, list(counts), n.value, draws.value) == (-7.0, -7.0, [-7] * 3, -7, -7) and (idx == -7).all()
    return rc, int(st.value), untouched


def raw_list(eng, fn, w, idx):
    loss, acc = C.c_double(-7.0), C.c_double(-7.0)
    counts = (C.c_int64 * 3)(-7, -7, -7)
    idx = np.asarray(idx, dtype=np.int32)
    rc = getattr(eng._lib, fn)(eng._ctx, None if w is None else w.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), len(idx),
                               C.byref(loss), C.byref(acc), counts)
    return rc, (loss.value, acc.value, list(counts)) == (-7.0, -7.0, [-7] * 3)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(engines, kind):
    eng, _, w = engines[kind]
    before = eng.get_weights().copy()
    state = host.JavaRandom(9).seed
    own = "dsgd_loss_acc_sampled" if kind == "fp32" else "dsgd_loss_acc_sampled_f64"
    own_list = "dsgd_loss_acc_list" if kind == "fp32" else "dsgd_loss_acc_list_f64"
    other = np.ones(D + 1, dtype=np.float32 if kind == "fp32" else np.float64)   # would replace the weights if a refused call got that far
    for (lo, hi, k), code in (((0, 100, 0), EINVAL), ((0, 100, -3), EINVAL), ((50, 50, 10), EINVAL), ((60, 50, 10), EINVAL),
                              ((N - 10, N + 1, 5), ERANGE), ((-1, 10, 5), ERANGE)):
        assert raw_sampled(eng, own, other, state, lo, hi, k) == (code, state, True), (lo, hi, k)
        assert np.array_equal(eng.get_weights(), before)
    for bad in ([3, -1, 4], [3, N, 4], [N]):
        assert raw_list(eng, own_list, None, bad) == (ERANGE, True), bad
    with pytest.raises(IndexError):
        eng.loss_acc_list([0, N])
    with pytest.raises(ValueError):
        eng.loss_acc_list([])
    if kind != "fp32":   # a float w through the float forms on an fp64 context
        w32 = np.ones(D + 1, dtype=np.float32)
        assert raw_sampled(eng, "dsgd_loss_acc_sampled", w32, state, 0, 100, 10) == (EINVAL, state, True)
        assert raw_list(eng, "dsgd_loss_acc_list", w32, [1, 2, 3]) == (EINVAL, True)
    else:                # the Double forms need an fp64 context
        assert raw_sampled(eng, "dsgd_loss_acc_sampled_f64", None, state, 0, 100, 10) == (ESTATE, state, True)
        assert raw_list(eng, "dsgd_loss_acc_list_f64", None, [1, 2, 3]) == (ESTATE, True)
    assert np.array_equal(eng.get_weights(), before)
    # the context goes on working
    assert eng.loss_acc_list(np.arange(N, dtype=np.int32)) == eng.loss_acc(0, N)


def test_window_beyond_the_device_form(wide):
    eng, n = wide
    state = host.JavaRandom(1).seed
    assert n == (1 << 20) + 1
    assert raw_sampled(eng, "dsgd_loss_acc_sampled", None, state, 0, n, 1000) == (EUNSUPPORTED, state, True)
    with pytest.raises(dsgd_amd.DsgdError) as e:
        eng.loss_acc_sampled(state, 0, n, 1000)
    assert e.value.code == EUNSUPPORTED
    # 2^20 rows are served (the largest bitmap of the trace)
    loss, acc, counts, st, dr, idx = eng.loss_acc_sampled(state, 1, n, 1500, want_idx=True)
    shuffled, state_after, draws = jrand_shuffle(state, n - 1)
    assert np.array_equal(idx, shuffled[:1500] + 1) and (st, dr) == (state_after, draws)


def test_refused_while_the_lock_free_engine_runs(engines):
    eng, _, w = engines["fp32"]
    state = host.JavaRandom(1).seed
    eng.async_start([(0, N_TRAIN)], batch=10, lr=1e-3, max_updates=1 << 40)
    try:
        assert raw_sampled(eng, "dsgd_loss_acc_sampled", None, state, 0, 100, 10) == (ESTATE, state, True)
        assert raw_list(eng, "dsgd_loss_acc_list", None, [1, 2, 3]) == (ESTATE, True)
    finally:
        eng.async_stop()
        set_w(eng, "fp32", w)   # (the module's weights, for whatever runs next)


# ---- 7. the mirrors on the device ----
class Withhold:
    """An Engine without some of its methods (the chain's later links)."""

    def __init__(self, eng, *names):
        self._eng, self._names = eng, names

    def __getattr__(self, name):
        if name in self._names:
            raise AttributeError(name)
        return getattr(self._eng, name)


@pytest.mark.parametrize("kind", KINDS)
def test_mirrors_three_routes(engines, data, kind, monkeypatch):
    eng, _, _ = engines[kind]
    label = data[3]
    results = {}
    for route in ("device", "list", "forward"):
        monkeypatch.setenv("DSGD_SAMPLED_DEVICE", "1" if route == "device" else "0")
        backend = {"device": eng, "list": Withhold(eng, "loss_acc_sampled"), "forward": Withhold(eng, "loss_acc_sampled", "loss_acc_list")}[route]
        got = []
        for cls in (host.MasterSync, host.MasterAsync):
            m = cls(backend, N_TRAIN, N, node_count=3, rnd=host.JavaRandom(77))
            m.labels = label
            got.append((m.local_sampled_loss(500), m.local_sampled_accuracy(500), m.local_sampled_loss(300, test=True),
                        m.local_sampled_accuracy(10 ** 6, test=True), m.rnd.seed))
        assert got[0] == got[1]
        results[route] = got[0]
    assert results["device"] == results["list"]
    assert results["list"][1] == results["forward"][1] and results["list"][3:] == results["forward"][3:]
    # the loss of the third route takes |w|^2 from the host's sum over get_weights() in fp64, the device sums in the
    # context's precision: dp + 2 roundings of relative size u at most, on a term lambda |w|^2
    u = 2.0 ** -24 if kind == "fp32" else 2.0 ** -53
    nsq = float(np.sum(np.asarray(eng.get_weights(), dtype=np.float64) ** 2))
    for a, b in ((results["list"][0], results["forward"][0]), (results["list"][2], results["forward"][2])):
        print("%s: loss by list %.17g, by forward and fold %.17g" % (kind, a, b))
        assert abs(a - b) <= LAM * nsq * (D + 3) * u + 4 * np.finfo(np.float64).eps * abs(a)
