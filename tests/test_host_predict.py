"""host.MasterSync / MasterAsync .predict, .distributed_loss, .distributed_accuracy (core/Master.scala:61-98) without a
GPU: over a small numpy backend that offers `forward` only (one ForwardRequest per split, the fold on the host), against
the dict-based restatement of the reference (oracle/ref_dict.py): the known-answer rows of SURVEY.md 8(c) and a 60-row
synthetic set, node_count in {1, 3, 4}."""

import numpy as np
import pytest

from dsgd_amd import host
from oracle import ref_dict as rd
from test_oracle_golden import KAT_ROWS

LAM = 0.1


class ForwardOnlyBackend:
    """Rows as {key: value} dicts; forward(idx, w) = -signum(x . w) with the products filtered at 1e-20 and added in
    ascending key order (math/Sparse.scala:20-31, :108-118).  No predict_ranges, no loss_acc: what a recording or wire
    backend offers the mirrors."""

    def __init__(self, rows, dim, lam):
        self.rows, self.dim, self.lam = rows, dim, lam
        self.label = np.asarray([y for _, y in rows], dtype=np.int8)
        self.w = np.zeros(dim + 1)
        self.requests = []

    def set_weights(self, w):
        self.w = np.asarray(w, dtype=np.float64).copy()

    def get_weights(self):
        return self.w.copy()

    def forward(self, idx, w=None):
        if w is not None:
            self.set_weights(w)   # the ForwardRequest carries the weights (core/Slave.scala:129-140)
        self.requests.append(np.asarray(idx).copy())
        out = np.zeros(len(idx))
        for t, i in enumerate(idx):
            d = 0.0
            for k in sorted(self.rows[i][0]):
                p = self.rows[i][0][k] * float(self.w[k])
                if abs(p) > 1e-20:
                    d = d + p
            out[t] = -1.0 if d > 0 else (1.0 if d < 0 else 0.0)
        return out


def synth_rows(n=60, dim=12, seed=5):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        if i in (7, 31):   # rows without a non-zero: x . w = 0 whatever w is
            rows.append(({}, 1 if i == 7 else -1))
            continue
        keys = rng.choice(np.arange(1, dim + 1), size=int(rng.integers(1, 6)), replace=False)
        v = rng.normal(size=len(keys))
        v /= np.linalg.norm(v)
        rows.append(({int(k): float(x) for k, x in zip(keys, v)}, int(rng.choice([-1, 1]))))
    return rows, dim


def oracle_side(rows, dim, n_train, w):
    data = [(rd.Sparse(dict(m), dim), y) for m, y in rows]
    model = rd.SparseSVM(LAM, rd.dim_sparsity(data[:n_train]))
    ws = rd.Sparse({k: float(v) for k, v in enumerate(w) if v != 0}, dim)
    train = data[:n_train]
    return (rd.slave_forward(model, data, ws, range(n_train)), rd.local_loss(model, ws, train), rd.local_accuracy(model, ws, train))


CASES = [("kat", KAT_ROWS, 6, 6), ("synth60", *synth_rows(), 60), ("synth60_short_last_split", *synth_rows(), 58)]


@pytest.mark.parametrize("node_count", [1, 3, 4])
@pytest.mark.parametrize("name,rows,dim,n_train", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("master", [host.MasterSync, host.MasterAsync], ids=["sync", "async"])
def test_mirrors_equal_the_reference_restatement(master, name, rows, dim, n_train, node_count):
    rng = np.random.default_rng(11)
    w_rand = np.zeros(dim + 1)
    w_rand[1:] = rng.normal(size=dim)
    split = host.split_vanilla(n_train, node_count)
    if name == "kat" and node_count == 4:
        assert len(split) == 3          # node_count exceeds the groups `grouped` yields (ceil(6 / 4) = 2 rows each)
    if name == "synth60_short_last_split" and node_count in (3, 4):
        assert len(split[-1]) < len(split[0])
    for w in (np.zeros(dim + 1), w_rand):
        be = ForwardOnlyBackend(rows, dim, LAM)
        m = master(be, n_train, len(rows), node_count)
        pred_ref, loss_ref, acc_ref = oracle_side(rows, dim, n_train, w)
        got_rows, got_pred = m.predict(w)
        # one ForwardRequest per split, over exactly the split's rows, in split order
        assert [r.tolist() for r in be.requests] == [list(s) for s in split]
        assert got_rows.tolist() == list(range(n_train))
        assert got_pred.tolist() == [float(p) for p in pred_ref]
        assert set(got_pred.tolist()) <= {-1.0, 0.0, 1.0}
        assert m.distributed_loss(w) == loss_ref
        assert m.distributed_accuracy(w) == acc_ref
        if not w.any():   # the reference's first two log lines (Main.scala:75-78)
            assert m.distributed_loss(w) == 1.0 and m.distributed_accuracy(w) == 0.0
        # weights=None evaluates what the backend holds
        assert m.distributed_loss() == loss_ref and m.predict()[1].tolist() == got_pred.tolist()


def test_empty_rows_predict_zero_and_count_as_loss_one():
    rows, dim = synth_rows()
    be = ForwardOnlyBackend(rows, dim, LAM)
    w = np.ones(dim + 1)
    _, pred = host.MasterSync(be, 60, 60, 3).predict(w)
    assert pred[7] == 0 and pred[31] == 0 and np.count_nonzero(pred == 0) == 2


class RangesBackend:
    """A backend with predict_ranges: the mirrors must take everything from ONE call of it per question."""

    lam = LAM

    def __init__(self):
        self.calls = []

    def predict_ranges(self, ranges, w=None):
        self.calls.append((list(ranges), w))
        n = sum(e - b for b, e in ranges)
        return np.ones(n, dtype=np.int8), np.zeros((len(ranges), 3), dtype=np.int64), 0.25, 0.75

    def forward(self, idx, w=None):
        raise AssertionError("forward must not be asked when predict_ranges is offered")


@pytest.mark.parametrize("master", [host.MasterSync, host.MasterAsync], ids=["sync", "async"])
def test_a_backend_with_predict_ranges_serves_all_three(master):
    be = RangesBackend()
    m = master(be, 10, 12, 3)
    rows, pred = m.predict()
    assert rows.tolist() == list(range(10)) and pred.dtype == np.int8 and len(pred) == 10
    assert m.distributed_loss() == 0.25 and m.distributed_accuracy() == 0.75
    assert [c[0] for c in be.calls] == [[(0, 4), (4, 8), (8, 10)]] * 3 and all(c[1] is None for c in be.calls)
