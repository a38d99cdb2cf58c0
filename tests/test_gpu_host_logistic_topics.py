"""host.LogisticTopics on the GPU: 3 topics, at most 2 epochs of 3 x 100 steps, the stopping rule per topic.  Each topic's
GradState must be the bits of host.LogisticSync alone on an engine whose labels are that topic's plane, from the same seed."""

import numpy as np
import pytest

import dsgd_amd
import logistic_cases as cases
from dsgd_amd import host

pytestmark = pytest.mark.gpu

N_TRAIN = 3276


def test_each_topic_is_logistic_sync_alone():
    d = cases.data()
    n = d.n_rows
    rng = np.random.default_rng(31)
    P = np.ascontiguousarray(np.stack([d.label, np.ones(n, np.int8), rng.choice(np.array([-1, 1], np.int8), size=n)]), dtype=np.int8)
    T, dp = 3, d.dim + 1
    W0 = np.zeros((T, dp), dtype=np.float32)
    stop = host.EarlyStopping.target(0.5)      # (the all +1 plane gets there after one epoch, the random plane never does)
    with dsgd_amd.Engine(d.dim, cases.LAM) as eng:
        eng.load_csr(*cases.csr(d))
        eng.lg_topics_set(P)
        m = host.LogisticTopics(eng, N_TRAIN, n, 3, rnd=host.JavaRandom(0))
        states = m.fit(W0, 2, 100, 0.5, stop)
    assert len(states) == T
    for t in range(T):
        with dsgd_amd.Engine(d.dim, cases.LAM) as one:
            one.load_csr(d.row_ptr, d.col, d.val, P[t])
            s = host.LogisticSync(one, N_TRAIN, n, 3, rnd=host.JavaRandom(0))
            want = s.fit(W0[t], 2, 100, 0.5, stop)
        got = states[t]
        print("topic %d: updates %d, loss %r" % (t, got.updates, got.loss))
        assert got.updates == want.updates, t
        assert np.array_equal(np.asarray(got.grad, np.float32).view(np.uint32), np.asarray(want.grad, np.float32).view(np.uint32)), t
        assert np.float64(got.loss).view(np.uint64) == np.float64(want.loss).view(np.uint64), (t, got.loss, want.loss)
        assert m.test_losses[t][:: -1][:want.updates] == s.test_losses[::-1]
    assert states[1].updates == 1 and states[2].updates == 2     # the rule fired per topic
