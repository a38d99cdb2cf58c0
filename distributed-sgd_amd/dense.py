"""DenseLogistic: the dense mini-batch variant of BASELINE.json configs[4] (K8) as a Python object -- a thin face
over the dsgd_dense_* entry points of include/dsgd.h.  No reference counterpart (the reference's only model is the
sparse hinge SVM, core/ml/SparseSVM.scala:11); all arithmetic happens in the HIP library."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f32, ptr


def _idx(a):
    """An index list as the library takes it: 1-D int32.  Values that do not fit 32 bits would wrap onto valid rows in
    the conversion, so they are refused here, as the library refuses any other row that does not exist."""
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError("an index list is a 1-D integer array, got %s of shape %r" % (a.dtype, a.shape))
    if a.size and (int(a.max()) > np.iinfo(np.int32).max or int(a.min()) < np.iinfo(np.int32).min):
        raise IndexError("index list entry outside 32 bits")
    return np.ascontiguousarray(a, dtype=np.int32)


class DensePlan:
    """An epoch's index lists resident on the device (dsgd_dense_plan_create); owned by its DenseLogistic, which
    releases what is left of its plans when it closes."""

    def __init__(self, engine, handle, n_steps):
        self.engine, self.handle, self.n_steps = engine, handle, n_steps

    def destroy(self):
        if self.handle and self.engine._h:
            check(self.engine._lib.dsgd_dense_plan_destroy(self.engine._h, self.handle))
        self.handle = None


class DenseLogistic:
    def __init__(self, n_features, device=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.dim = int(n_features)
        check(self._lib.dsgd_dense_create(C.c_int32(self.dim), C.c_int32(device), C.byref(self._h)))
        self.n_rows = 0

    def close(self):
        if self._h:
            self._lib.dsgd_dense_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def generate(self, n_rows, seed=0):
        check(self._lib.dsgd_dense_generate(self._h, C.c_int64(n_rows), C.c_uint64(seed)))
        self.n_rows = int(n_rows)

    def load(self, X, y):
        X = np.ascontiguousarray(X, dtype=np.float32)
        y = f32(y)
        if X.ndim != 2 or X.shape[1] != self.dim or len(y) != X.shape[0]:
            raise ValueError("X must be n_rows x %d and y n_rows" % self.dim)
        check(self._lib.dsgd_dense_load(self._h, C.c_int64(X.shape[0]), ptr(X), ptr(y)))
        self.n_rows = X.shape[0]

    def set_weights(self, w):
        check(self._lib.dsgd_dense_set_weights(self._h, ptr(f32(w, self.dim))))

    def get_weights(self):
        out = np.zeros(self.dim, dtype=np.float32)
        check(self._lib.dsgd_dense_get_weights(self._h, ptr(out)))
        return out

    def step(self, row_begin, row_end, lr):
        check(self._lib.dsgd_dense_step(self._h, C.c_int64(row_begin), C.c_int64(row_end), C.c_float(lr)))

    def synchronize(self):
        check(self._lib.dsgd_dense_synchronize(self._h))

    def loss(self, row_begin, row_end):
        l, a = C.c_double(0), C.c_double(0)
        check(self._lib.dsgd_dense_loss(self._h, C.c_int64(row_begin), C.c_int64(row_end), C.byref(l), C.byref(a)))
        return l.value, a.value

    # -- mini-batches as index lists (include/dsgd.h "INDEX LISTS") ------------------------------------------------
    def step_list(self, idx, lr):
        """One step over the rows `idx` names (a row named twice counts twice); enqueued like step()."""
        idx = _idx(idx)
        check(self._lib.dsgd_dense_step_list(self._h, ptr(idx), C.c_int64(len(idx)), C.c_float(lr)))

    def loss_list(self, idx):
        idx = _idx(idx)
        l, a = C.c_double(0), C.c_double(0)
        check(self._lib.dsgd_dense_loss_list(self._h, ptr(idx), C.c_int64(len(idx)), C.byref(l), C.byref(a)))
        return l.value, a.value

    def predict_proba(self, row_begin=None, row_end=None, idx=None):
        """sigmoid(x . w) under the resident weights: of the rows [row_begin, row_end) (default: every row), or of the
        rows `idx` names, in list order."""
        if idx is not None:
            if row_begin is not None or row_end is not None:
                raise ValueError("give a row range or idx, not both")
            idx = _idx(idx)
            out = np.zeros(len(idx), dtype=np.float32)
            check(self._lib.dsgd_dense_predict_list(self._h, ptr(idx), C.c_int64(len(idx)), ptr(out)))
            return out
        rb = 0 if row_begin is None else int(row_begin)
        re = self.n_rows if row_end is None else int(row_end)
        out = np.zeros(max(re - rb, 1), dtype=np.float32)   # (an empty or reversed range is the library's to refuse)
        check(self._lib.dsgd_dense_predict(self._h, C.c_int64(rb), C.c_int64(re), ptr(out)))
        return out

    def plan(self, lists):
        """An epoch's mini-batches resident on the device: `lists` is a sequence of int arrays, one per step."""
        lists = [_idx(a) for a in lists]
        idx = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        offsets = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum([len(a) for a in lists], out=offsets[1:])
        return self.plan_flat(idx, offsets)

    def plan_flat(self, idx, offsets):
        """plan() from the flat form: every list concatenated, and n_steps + 1 prefix offsets."""
        idx = _idx(idx)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("offsets must be n_steps + 1 integers")
        h = C.c_void_p()
        check(self._lib.dsgd_dense_plan_create(self._h, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(len(offsets) - 1),
                                               C.byref(h)))
        return DensePlan(self, h, len(offsets) - 1)

    def plan_run(self, plan, step_begin, step_end, lr):
        """Steps [step_begin, step_end) of a plan, enqueued: no upload, no host synchronisation in between."""
        if plan.engine is not self:
            raise ValueError("the plan belongs to another DenseLogistic")
        check(self._lib.dsgd_dense_plan_run(self._h, plan.handle, C.c_int64(step_begin), C.c_int64(step_end), C.c_float(lr)))

    def comm_init(self, unique_id, world_size, rank):
        check(self._lib.dsgd_dense_comm_init(self._h, C.c_char_p(unique_id), C.c_int32(world_size), C.c_int32(rank)))

    def prof(self, enable=True):
        ms, n = C.c_double(0), C.c_int64(0)
        check(self._lib.dsgd_dense_prof(self._h, C.c_int32(1 if enable else 0), C.byref(ms), C.byref(n)))
        return ms.value, n.value
