"""The fp64 mode on Double feature values (dsgd_load_csr_f64) next to the same calls on the same data rounded to float:
the two value types of the one row-parallel family (csrc/dsgd_rp64.hpp).

One GPU run, one JSON line, over N = 804,414 synthetic RCV1-like rows (80 % train, 3 workers' splits).  The generator's
values are float by construction, so the Double data set is made here: every value times (1 + u * 2^-24), u uniform in
[-1, 1) -- the low 29 mantissa bits filled, as a text file's values have them; the float data set is that rounded.
  gradient   us per gradient_f64 call for n = 100, 4,096 and 65,536 rows, on doubles and on floats, their ratio, and the
             second-word atomics of the call: the entries of its active rows whose scaled value x * 2^(S - vexp) is no
             integer (counted on the host at w = 0, where every row is active; the hot ranks' adds go to LDS first)
  sync_step  us per sync_step_f64 call for 3 x 100 and 3 x whole split, on doubles and on floats

    python tools/fp64_values_probe.py [--rows 804414] [--reps 50]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dsgd_amd
from dsgd_amd import host

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=804414)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()

LAM, LR = 1e-5, 0.5
data = dsgd_amd.synth.generate(a.rows, seed=0)
n_train = int(a.rows * 0.8)
split = host.split_vanilla(n_train, 3)
rng = np.random.default_rng(0)
val64 = data.val.astype(np.float64) * (1.0 + (rng.random(data.nnz) * 2.0 - 1.0) * 2.0 ** -24)
val32 = val64.astype(np.float32)
vexp = math.frexp(float(np.abs(val64).max()))[1]


def engine(values):
    eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64")
    eng.load_csr(data.row_ptr, data.col, values, data.label)
    eng.build_dim_sparsity(n_train)
    return eng


def median_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1)


def second_word_atomics(idx):
    """entries of the listed rows (all active at w = 0) with a non-zero low word at this list's shift"""
    shift = 62 - math.ceil(math.log2(len(idx))) if len(idx) > 1 else 62
    scale = 2.0 ** (shift - vexp)
    n = 0
    for r in idx.tolist():
        v = val64[data.row_ptr[r]:data.row_ptr[r + 1]] * scale
        n += int(np.count_nonzero((v != np.floor(v)) & (np.abs(v) > 0)))
    return n


out = {"rows": a.rows, "n_train": n_train, "reps": a.reps, "gradient": {}, "sync_step": {}}
e64v, e32v = engine(val64), engine(val32)
with e64v, e32v:
    assert (e64v.value_bits(), e32v.value_bits()) == (64, 32)
    whole = np.asarray(split[0], dtype=np.int32)
    for n in (100, 4096, 65536):
        idx = np.ascontiguousarray(rng.permutation(whole)[:n], dtype=np.int32)
        for e in (e64v, e32v):
            e.set_weights(np.zeros(data.dim + 1))
        d_us = median_us(lambda: e64v.gradient_f64(idx), a.reps)
        f_us = median_us(lambda: e32v.gradient_f64(idx), a.reps)
        entries = int(sum(data.row_ptr[r + 1] - data.row_ptr[r] for r in idx.tolist()))
        out["gradient"][str(n)] = {"double_us": d_us, "float_us": f_us, "ratio": round(d_us / f_us, 3), "entries": entries,
                                   "second_word_atomics": second_word_atomics(idx)}
    for name, rows in (("3x100", 100), ("3xwhole_split", None)):
        lists = [np.ascontiguousarray(rng.permutation(np.asarray(r))[:rows], dtype=np.int32) for r in split]
        reps = a.reps if rows is not None else max(5, a.reps // 5)
        rec = {}
        for key, e in (("double_us", e64v), ("float_us", e32v)):
            e.set_weights(np.zeros(data.dim + 1))
            rec[key] = median_us(lambda: e.sync_step_f64(lists, LR), reps)
        rec["ratio"] = round(rec["double_us"] / rec["float_us"], 3)
        out["sync_step"][name] = rec
print(json.dumps(out))
