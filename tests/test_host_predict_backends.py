"""The mirrors' predict / distributed_loss / distributed_accuracy (core/Master.scala:61-98) over the backends the project
ships that have no predict_ranges: the oracle backend (forward per split, the labels from the master) and wire.WireBackend
(the reference's own fan-out: one Forward RPC per split and slave, the labels from the backend), both against the oracle's
loss_acc over the train rows."""

import numpy as np
import pytest

import dsgd_amd
from dsgd_amd import host
from oracle import oracle as orc
from oracle_backend import OracleBackend

N_ROWS, N_TRAIN, LAM = 300, 241, 1e-5


@pytest.fixture(scope="module")
def case():
    data = dsgd_amd.synth.generate(N_ROWS, seed=33)
    o = orc.Oracle(data.dim, data.row_ptr, data.col, data.val, data.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(N_TRAIN))
    w = np.random.default_rng(2).normal(size=data.dim + 1)
    loss, acc, _, _ = o.loss_acc(w, 0, N_TRAIN)
    return data, o, w, o.forward(w, np.arange(N_TRAIN)), loss, acc


def check(master, case, node_count):
    data, _, w, pred_ref, loss_ref, acc_ref = case
    rows, pred = master.predict(w)
    assert rows.tolist() == list(range(N_TRAIN)) and np.array_equal(pred, pred_ref)
    # the tallies are integers; |w|^2 is added in another order than the oracle's: a few roundings of a sum of D + 1 squares
    tol = LAM * float(w @ w) * (data.dim + 1) * 2.0 ** -53
    assert abs(master.distributed_loss(w) - loss_ref) <= tol and master.distributed_accuracy(w) == acc_ref
    assert master.distributed_loss_and_accuracy() == (master.distributed_loss(), master.distributed_accuracy())   # resident weights
    zero = np.zeros(data.dim + 1)
    assert master.distributed_loss(zero) == 1.0 and master.distributed_accuracy(zero) == 0.0


@pytest.mark.parametrize("master", [host.MasterSync, host.MasterAsync], ids=["sync", "async"])
@pytest.mark.parametrize("node_count", [1, 3, 4])
def test_oracle_backend_with_the_masters_labels(case, master, node_count):
    data, o = case[0], case[1]
    m = master(OracleBackend(o), N_TRAIN, N_ROWS, node_count)
    with pytest.raises(ValueError, match="labels"):   # neither the master nor this backend holds labels: said so, nothing asked
        m.distributed_loss(case[2])
    m.labels = data.label
    check(m, case, node_count)


def test_label_sources():
    class B:
        lam = 0.0

        def get_weights(self):
            return np.zeros(3)

        def forward(self, idx, w=None):
            return np.asarray([-1.0, 1.0, 0.0, 1.0])[np.asarray(idx)]

    y = np.asarray([-1, -1, 1, 1])
    for attr, value in (("labels", y), ("label", y), ("labels", lambda rows: y[rows])):   # array, array, method
        b = B()
        setattr(b, attr, value)
        assert host.MasterSync(b, 4, 4, 2).distributed_loss_and_accuracy() == ((0 + 2 + 1 + 0) / 4, 2 / 4)
    m = host.MasterSync(B(), 4, 4, 2)
    m.labels = -y                                       # the master's own labels come first
    assert m.distributed_accuracy() == 1 / 4


def test_wire_backend_fans_forward_out_over_its_slaves(case):
    pytest.importorskip("grpc")
    from dsgd_amd import wire

    data, o = case[0], case[1]
    k = 3
    service = wire.MasterService(expected_nodes=k).start()
    workers = [wire.SlaveWorker(OracleBackend(o), data.dim, master=("127.0.0.1", service.port)).start() for _ in range(k)]
    try:
        assert service.ready.wait(5)
        stubs = [wire.Stub(wire.new_channel("127.0.0.1", w.port), "Slave") for w in workers]
        for master in (host.MasterSync, host.MasterAsync):
            for node_count in (1, 2, 3):   # (the reference splits over workers.size: never more splits than slaves)
                before = [w.metrics.snapshot()["counters"].get("slave.sync.forward", 0) for w in workers]
                m = master(wire.WireBackend(stubs, data.dim, LAM, data.label), N_TRAIN, N_ROWS, node_count)
                m.predict(case[2])
                after = [w.metrics.snapshot()["counters"].get("slave.sync.forward", 0) for w in workers]
                split = host.split_vanilla(N_TRAIN, node_count)   # split j was served by slave j, per sample counted
                assert [a - b for a, b in zip(after, before)] == [len(r) for r in split] + [0] * (k - len(split))
                check(m, case, node_count)
        with pytest.raises(ValueError, match="slaves"):
            host.MasterSync(wire.WireBackend(stubs[:2], data.dim, LAM, data.label), N_TRAIN, N_ROWS, 3).predict()
    finally:
        for w in workers:
            w.stop()
        service.stop()
