"""No GPU needed: host.LogisticTopics against a scripted backend -- the call sequence of an epoch (ONE lg_topics_sync_steps over
epoch_lists' lists from the one JavaRandom, then ONE lg_topics_loss_acc each over train and test) and the stopping rule applied
per topic: a topic's GradState is taken when its own rule first fires, the others go on."""

import numpy as np
import pytest

from dsgd_amd import host


class Scripted:
    """test losses per epoch and topic from a script; the weights count the epochs (topic t holds t + epochs / 10)"""

    def __init__(self, T, dp, test_losses):
        self.T, self.dp, self.script = T, dp, test_losses
        self.calls, self.epochs, self.W = [], 0, None

    def lg_topics_set_weights(self, W):
        self.calls.append(("set_weights", W.shape))
        self.W = np.array(W, dtype=np.float32)

    def lg_topics_get_weights(self):
        self.calls.append(("get_weights",))
        return self.W.copy()

    def lg_topics_sync_steps(self, idx, offsets, n_steps, n_workers, lr):
        self.calls.append(("sync_steps", np.array(idx), np.array(offsets), n_steps, n_workers, lr))
        self.epochs += 1
        self.W = self.W + np.float32(0.1)

    def lg_topics_loss_acc(self, lo, hi):
        self.calls.append(("loss_acc", lo, hi))
        test = lo > 0
        row = self.script[self.epochs - 1]
        return (np.array(row, dtype=np.float64) if test else np.array(row, dtype=np.float64) + 100.0), np.full(self.T, 0.5)


def test_call_sequence_and_per_topic_stopping():
    T, dp = 3, 5
    script = [[0.9, 0.4, 0.9], [0.9, 0.1, 0.3], [0.9, 0.0, 0.0]]     # topic 1 reaches 0.5 after epoch 1, topic 2 after epoch 2, topic 0 never
    b = Scripted(T, dp, script)
    m = host.LogisticTopics(b, 60, 80, 3, rnd=host.JavaRandom(0))
    W0 = np.arange(T, dtype=np.float32)[:, None] * np.ones((1, dp), dtype=np.float32)
    states = m.fit(W0, 3, 10, 0.25, host.EarlyStopping.target(0.5))
    assert [s.updates for s in states] == [3, 1, 2]
    for t, s in enumerate(states):
        assert np.allclose(s.grad, t + 0.1 * s.updates) and s.grad.dtype == np.float32     # the weights as they were when the rule fired
        assert s.loss == script[s.updates - 1][t] + 100.0 and s.end is not None            # the newest TRAIN loss then
    kinds = [c[0] for c in b.calls]
    assert kinds == ["set_weights"] + ["sync_steps", "loss_acc", "loss_acc", "get_weights"] * 3
    assert [c[1:] for c in b.calls if c[0] == "loss_acc"] == [(0, 60), (60, 80)] * 3
    # the lists are epoch_lists' from the one stream: three epochs drawn one after the other
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(60, 3)
    for c in [c for c in b.calls if c[0] == "sync_steps"]:
        idx, offs, n_steps = host.epoch_lists(rnd, split, 20, 10)
        assert n_steps == c[3] == 2 and c[4] == 3 and c[5] == 0.25
        assert np.array_equal(c[1], idx) and np.array_equal(c[2], offs)
    assert m.rnd.seed == rnd.seed and m.steps_run == 6
    assert m.test_losses[1] == [0.0, 0.1, 0.4]                                             # newest first; the finished topic was stepped on


def test_no_epoch_and_an_epoch_that_runs_dry():
    b = Scripted(2, 4, [[0.0, 0.0]])
    m = host.LogisticTopics(b, 60, 80, 3)
    W0 = np.ones((2, 4), dtype=np.float32)
    states = m.fit(W0, 0, 10, 0.25, host.EarlyStopping.target(0.5))
    assert [s.updates for s in states] == [0, 0] and all(s.loss is None for s in states) and [c[0] for c in b.calls] == ["set_weights"]
    assert np.array_equal(states[0].grad, W0[0])
    with pytest.raises(ValueError):
        host.LogisticTopics(b, 80, 80, 3)
    with pytest.raises(ValueError, match="empty list of vectors"):    # 61 rows on 3 workers: 21, 21, 19 -- the third batch finds worker 2 empty
        host.LogisticTopics(Scripted(2, 4, [[1.0, 1.0]] * 3), 61, 80, 3).fit(W0, 1, 10, 0.25, host.EarlyStopping.target(0.5))
