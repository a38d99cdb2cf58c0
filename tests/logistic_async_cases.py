"""The lists and weights that tests/test_logistic_async_bound.py (CPU, emulated) and tests/test_gpu_logistic_async.py (GPU) share:
the CPU test shows the bound's worth -- and that the reference itself is inside it -- for exactly what the GPU tests run."""

import functools

import numpy as np

import logistic_cases as cases
import logistic_hard_cases as hard

LR = 0.5                      # (a float exactly: dsgd_lg_sync_step's float lr and the double lr here are the same number)
TINY = 2.0 ** -20             # logits of this deviation: |w| far below |delta|, so a delta rounded to float early shows
LENS = (1, 2, 17, 100, 1025)  # one group, two, a ragged pass, the reference's batch, beyond the slices' 1,024 rows


@functools.lru_cache(maxsize=None)
def lists():
    """name -> one worker's list on logistic_cases.data(); the 100-row list names one row three times"""
    rng = np.random.default_rng(23)
    p = rng.permutation(cases.N).astype(np.int32)
    out, at = {}, 0
    for n in LENS:
        a = p[at:at + n].copy()
        at += n
        if n == 100:
            a[-2:] = a[0]
        a.setflags(write=False)
        out[str(n)] = a
    return out


def weight_sets():
    return {"logits 1": cases.weights(1.0), "logits 8": cases.weights(8.0), "tiny": cases.weights(TINY)}


# the hard widths: 2 columns; the LDS head's last word and the first column beyond it (ranks 2,047 / 2,048); one and two
# workgroups of the finish (256 / 257 columns)
WIDTHS = (1, 255, 256, 2047, 2048)


def width_lists(dim):
    """name -> list on logistic_hard_cases.width(dim): its 17 rows, and a 37-row list that (at the widths which have one) names the
    row of EVERY key: more than 64 non-zeros, past the registers of RowRegs, and data on the columns of the edge ranks"""
    c = hard.width(dim)
    long = np.array(c.step[0][1])
    if dim in hard.W_FULL:
        long[0] = hard.W_FULL_ROW
    long.setflags(write=False)
    return {"17": c.grad_lists["17"], "37": long}
