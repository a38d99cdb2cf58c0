"""The fp64 reference of the logistic model's ASYNCHRONOUS iteration (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS;
core/Slave.scala:79-111, 177-185; core/MasterAsync.scala:32-178), built on tests/logistic_ref.py.  Nothing of the kernels' order:

    one update   r = (sum_{i in list} c_i x_i) / n + 2 lambda w,   delta = lr r,   w <- w - delta       (ONE worker's list of n rows)
    a peer       w[k] <- w[k] - dv[k]
    the run      the ZERO-LAG schedule: update u is worker u mod K at its iteration u div K, its rows what the lock-free engine's
                 worker draws there (oracle/hogwild_replay.hog_rows); every update is seen by all workers before the next one
    the master   a loss check before the first update and after every `check_every` updates: the test loss and accuracy folded
                 into a leaky average, the best weights kept, the stopping criterion asked newest first, the end at max_steps
"""

import numpy as np

import logistic_ref as ref
from oracle.hogwild_replay import hog_rows


def async_step(csr, w, idx, lr, lam):
    """(w', delta) of one update over the listed rows, float64."""
    w = np.asarray(w, dtype=np.float64)
    g, _ = ref.data_sum(csr, w, idx)
    r = g / float(len(idx)) + 2.0 * lam * w
    delta = lr * r
    return w - delta, delta


def update_grad(w, keys, vals):
    w = np.asarray(w, dtype=np.float64).copy()
    w[np.asarray(keys, dtype=np.int64)] -= np.asarray(vals, dtype=np.float64)
    return w


def split_vanilla(n, k):
    size = -(-n // k)
    return [(b, min(n, b + size)) for b in range(0, n, size)]


def schedule_lists(split, batch, seed, positional_bug, first_update, n_updates):
    """The lists of updates [first_update, first_update + n_updates): one int32 array of `batch` rows each."""
    K = len(split)
    out = []
    for u in range(first_update, first_update + n_updates):
        b, e = split[u % K]
        out.append(hog_rows(seed, u % K, u // K, b, e - b, batch, positional_bug=bool(positional_bug)))
    return out


def fit(csr, w0, n_train, n_rows, node_count, max_epoch, batch, lr, lam, stop, check_every, leak, seed=0, positional_bug=True, max_steps=None,
        step=async_step, loss_acc=None, on_update=None):
    """MasterAsync.fit on the zero-lag schedule.  `step(csr, w, idx, lr, lam) -> (w', delta)` and `loss_acc(w) -> (loss, acc)` may
    be replaced (a backend under test).  Returns a dict: best_w, best_loss, updates, test_losses / test_accs (newest first),
    checks, check_at (the update counts at which a check was taken)."""
    split = split_vanilla(n_train, node_count)
    steps = n_train * max_epoch if max_steps is None else max_steps
    if loss_acc is None:
        loss_acc = lambda w: ref.loss_acc(csr, w, n_train, n_rows, lam)[:2]
    w = np.asarray(w0, dtype=np.float64).copy()
    best_w, best_loss = w.copy(), float("inf")
    losses, accs, check_at = [], [], []
    updates = 0
    while True:
        cl, ca = loss_acc(w)
        pl = losses[0] if losses else cl
        pa = accs[0] if accs else ca
        loss = leak * cl + (1 - leak) * pl
        acc = leak * ca + (1 - leak) * pa
        losses.insert(0, loss)
        accs.insert(0, acc)
        check_at.append(updates)
        if best_loss > loss:
            best_loss, best_w = loss, w.copy()
        if stop(losses) or updates >= steps:
            break
        target = min(steps, updates + check_every)
        while updates < target:
            idx = schedule_lists(split, batch, seed, positional_bug, updates, 1)[0]
            if on_update is not None:
                on_update(updates, w, idx)
            w, _ = step(csr, w, idx, lr, lam)
            updates += 1
    return {"best_w": best_w, "best_loss": best_loss, "updates": updates, "test_losses": losses, "test_accs": accs, "checks": len(losses),
            "check_at": check_at, "w": w}
