"""The data, weights and lists that tests/test_logistic_bound.py (CPU) and tests/test_gpu_logistic.py (GPU) share: the CPU
test shows the bound's worth for exactly the lists the GPU tests step."""

import functools

import numpy as np

import logistic_ref as ref

N = 4096
SEED = 11
LAM = 1e-5
LR = 0.5


@functools.lru_cache(maxsize=None)
def data():
    import dsgd_amd

    return dsgd_amd.synth.generate(N, seed=SEED)


def csr(d=None):
    d = d or data()
    return (d.row_ptr, d.col, d.val, d.label)


@functools.lru_cache(maxsize=None)
def weights(scale, seed=3):
    """float32 weights whose logits x . w have standard deviation `scale` over the rows."""
    d = data()
    w = np.random.default_rng(seed).standard_normal(d.dim + 1)
    w = (w * (scale / np.std(ref.dots(csr(d), w)))).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def step_cases():
    """name -> (the workers' lists of one step, lr): 3 workers of unequal lengths; 1 x 4,097 (longer than the rows: one is named
    twice).  A worker's gradient is a SUM over its rows, so the long list steps with a smaller lr (both are floats exactly)."""
    rng = np.random.default_rng(5)
    three = [rng.permutation(N)[:n].astype(np.int32) for n in (100, 37, 1)]
    p = rng.permutation(N).astype(np.int32)
    return {"3 workers 100/37/1": (three, LR), "1 x 4097": ([np.concatenate([p, p[:1]])], 2.0 ** -6)}


@functools.lru_cache(maxsize=None)
def gradient_lists():
    """name -> one worker's list: 1, 17, 100 and 4,097 positions (16 rows per 256 lanes: 17 and 4,097 leave a ragged last pass),
    a row named three times, a list longer than n_rows."""
    rng = np.random.default_rng(9)
    p = rng.permutation(N).astype(np.int32)
    return {"1": p[:1], "17": p[1:18], "100 (row thrice)": np.concatenate([p[18:116], p[18:19], p[18:19]]),
            "4097 (> n_rows)": np.concatenate([p, p[7:8]])}
