"""host.MasterSync / MasterAsync .local_sampled_loss / .local_sampled_accuracy (core/Master.scala:109-118) over the oracle
backend, without a GPU: the numbers against an independent restatement written here, the random stream against
scala_shuffle and csrc/jrand.c, its continuity into fit's lists, and the refusals."""

import numpy as np
import pytest

import dsgd_amd
from dsgd_amd import host
from oracle import oracle as orc
from oracle_backend import OracleBackend

N_ROWS, N_TRAIN, LAM, SEED = 400, 320, 1e-3, 17


@pytest.fixture(scope="module")
def problem():
    data = dsgd_amd.synth.generate(N_ROWS, seed=31)
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(N_TRAIN))
    w = np.random.default_rng(3).normal(size=data.dim + 1)
    pred = np.asarray(o.forward(w, np.arange(N_ROWS)), dtype=np.float64)   # the oracle's per-row predictions, once
    return data, o, w, pred


def master_of(cls, problem, backend=None, seed=SEED):
    data, o, w, _ = problem
    if backend is None:
        backend = OracleBackend(o)
        backend.set_weights(w)
    m = cls(backend, N_TRAIN, N_ROWS, node_count=3, rnd=host.JavaRandom(seed))
    m.labels = np.asarray(data.label)
    return m


def restated(problem, rnd, k, test):
    """(loss, accuracy) of ONE sample each, as Master.scala:109-118 states them: shuffle the window's indices, take k, map
    them to the rows, fold the model's loss / count the correct predictions."""
    data, _, w, pred = problem
    lo, hi = (N_TRAIN, N_ROWS) if test else (0, N_TRAIN)
    rows = [lo + p for p in host.scala_shuffle(range(hi - lo), rnd)[:k]]
    y = np.asarray(data.label, dtype=np.float64)[rows]
    nsq = 0.0
    for v in w[np.abs(w) > host.SPARSE_EPSILON]:
        nsq += float(v) * float(v)
    hinge = sum(max(0.0, 1.0 - float(a) * float(b)) for a, b in zip(y, pred[rows]))
    return LAM * nsq + hinge / len(rows), sum(1 for a, b in zip(y, pred[rows]) if a == b) / len(rows)


@pytest.mark.parametrize("cls", [host.MasterSync, host.MasterAsync])
@pytest.mark.parametrize("test", [False, True], ids=["train", "test"])
def test_sampled_loss_and_accuracy_equal_the_restatement(problem, cls, test):
    length = N_ROWS - N_TRAIN if test else N_TRAIN
    m = master_of(cls, problem)
    rnd = host.JavaRandom(SEED)
    for k in (1, length - 1, length, length + 5):
        want_loss = restated(problem, rnd, k, test)[0]
        got = m.local_sampled_loss(k, test=test)
        assert got == want_loss and m.rnd.seed == rnd.seed, k
        want_acc = restated(problem, rnd, k, test)[1]          # (a second shuffle: another sample)
        assert m.local_sampled_accuracy(k, test=test) == want_acc and m.rnd.seed == rnd.seed, k
    snap = m.metrics.snapshot() if hasattr(m, "metrics") else None
    if snap is not None:
        assert len(snap["histograms"]["master.sampled.loss.duration"]) == 4
        assert len(snap["histograms"]["master.sampled.accuracy.duration"]) == 4


def test_jrand_route_and_scala_shuffle_route_give_the_same_list_and_state():
    assert host._host_lib() is not None, "lib/libdsgd_host.so is not built"
    for length, k in ((1, 1), (2, 1), (2, 5), (1024, 100), (4097, 4097), (70000, 33)):
        a, b = host.JavaRandom(5), host.JavaRandom(5)
        la, lb = host.sampled_list(a, length, k, native=True), host.sampled_list(b, length, k, native=False)
        assert la.dtype == lb.dtype == np.int32 and np.array_equal(la, lb) and len(la) == min(k, length)
        assert a.seed == b.seed
        c = host.JavaRandom(5)
        assert lb.tolist() == host.scala_shuffle(range(length), c)[:k] and c.seed == b.seed


def test_the_stream_continues_through_the_checks_into_fit(problem):
    m = master_of(host.MasterSync, problem)
    rnd = host.JavaRandom(SEED)
    loss = m.local_sampled_loss(50)
    acc = m.local_sampled_accuracy(50)
    split = host.split_vanilla(N_TRAIN, 3)
    got = host.epoch_lists(m.rnd, split, 200, 100)
    # one Python generator: two shuffles of the train window, then the epoch's per-batch shuffles
    first = host.scala_shuffle(range(N_TRAIN), rnd)[:50]
    second = host.scala_shuffle(range(N_TRAIN), rnd)[:50]
    assert first != second
    want = host.epoch_lists(rnd, split, 200, 100, native=False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] == 2
    assert m.rnd.seed == rnd.seed
    # ... and the two numbers are those of the two different samples
    again = host.JavaRandom(SEED)
    assert loss == restated(problem, again, 50, False)[0]
    assert acc == restated(problem, again, 50, False)[1]


class Refusing:
    """A backend whose device draw and list form refuse as the library does: DsgdError with code EUNSUPPORTED."""

    def __init__(self, inner):
        self._inner, self.calls = inner, []

    def loss_acc_sampled(self, jstate, lo, hi, k, w=None, want_idx=False):
        self.calls.append("sampled")
        raise dsgd_amd.DsgdError(dsgd_amd._lib.EUNSUPPORTED, "windows up to 2^20 rows")

    def loss_acc_list(self, idx, w=None):
        self.calls.append("list")
        raise dsgd_amd.DsgdError(dsgd_amd._lib.EUNSUPPORTED, "refused")

    def __getattr__(self, name):
        return getattr(self._inner, name)


def test_a_refusal_falls_through_with_equal_results_and_state(problem, monkeypatch):
    monkeypatch.setenv("DSGD_SAMPLED_DEVICE", "1")
    plain = master_of(host.MasterSync, problem)
    want = (plain.local_sampled_loss(40), plain.local_sampled_accuracy(40, test=True), plain.rnd.seed)
    be = OracleBackend(problem[1])
    be.set_weights(problem[2])
    refusing = Refusing(be)
    m = master_of(host.MasterSync, problem, backend=refusing)
    assert (m.local_sampled_loss(40), m.local_sampled_accuracy(40, test=True), m.rnd.seed) == want
    assert refusing.calls == ["sampled", "list"] * 2       # every link was tried, in order, once per check
    # with the knob off the device draw is not tried
    monkeypatch.setenv("DSGD_SAMPLED_DEVICE", "0")
    refusing.calls.clear()
    m.local_sampled_loss(5)
    assert refusing.calls == ["list"]
    # an error that is no refusal is not swallowed
    class Broken(Refusing):
        def loss_acc_list(self, idx, w=None):
            raise dsgd_amd.DsgdError(dsgd_amd._lib.ESTATE, "async computation running")
    with pytest.raises(dsgd_amd.DsgdError):
        master_of(host.MasterSync, problem, backend=Broken(be)).local_sampled_loss(5)


@pytest.mark.parametrize("cls", [host.MasterSync, host.MasterAsync])
def test_an_empty_sample_raises_and_draws_nothing(problem, cls):
    m = master_of(cls, problem)
    before = m.rnd.seed
    for k in (0, -3):
        with pytest.raises(ValueError):
            m.local_sampled_loss(k)
        with pytest.raises(ValueError):
            m.local_sampled_accuracy(k, test=True)
    assert m.rnd.seed == before


def test_a_pending_prefetch_raises(problem):
    m = master_of(host.MasterSync, problem)
    before = m.rnd.seed
    m._pending = {"seed_before": before, "plan": None}     # what fit's prefetch holds while an epoch runs
    with pytest.raises(RuntimeError):
        m.local_sampled_loss(10)
    with pytest.raises(RuntimeError):
        m.local_sampled_accuracy(10)
    assert m.rnd.seed == before
    m._pending = None
    m.local_sampled_loss(10)
    assert m.rnd.seed != before
