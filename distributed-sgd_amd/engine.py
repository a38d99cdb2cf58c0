"""Engine: one libdsgd_hip context (one MI355X) as a Python object.

Thin, typed face over the C ABI of include/dsgd.h; all arithmetic happens in the HIP library.
Dense vectors are numpy float32 arrays of D+1 slots indexed by key (see include/dsgd.h).
"""

from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import _lib
from ._lib import BatchStats, Config, check, f32, f64, i32, ptr


class Plan:
    """Resident schedule of index lists (steps x workers); see dsgd_plan_create."""

    def __init__(self, engine, handle, n_steps, n_workers, n_samples):
        self.engine, self.handle, self.n_steps, self.n_workers, self.n_samples = engine, handle, n_steps, n_workers, n_samples

    def destroy(self):
        if self.handle:
            check(_lib.load().dsgd_plan_destroy(self.engine._ctx, self.handle))
            self.handle = None

    def info(self):
        """How the plan will run: kind ('column_slices', 'one_workgroup', 'virtual_tiles', 'row_parallel', 'not_laid_out')
        and, for column slices, the layout's shape ('row_parallel_fp64': a plan made with rp64=True); see dsgd_plan_info."""
        v = (C.c_int32 * 9)()
        check(_lib.load().dsgd_plan_info(self.engine._ctx, self.handle, v, C.c_int32(9)))
        kinds = {0: "not_laid_out", 1: "column_slices", 2: "one_workgroup", 3: "virtual_tiles", 4: "row_parallel", 5: "column_slices_fp64",
                 6: "row_parallel_fp64", 7: "logistic", 8: "logistic_column_slices"}
        return {"kind": kinds.get(int(v[0]), "?"), "slices": int(v[1]), "slot_stride": int(v[2]), "row_stride": int(v[3]),
                "col_list_stride": int(v[4]), "slots_per_lane": int(v[5]), "device_built": bool(v[6]), "record_words": int(v[7]), "threads": int(v[8])}

    def record(self, on=True):
        """Keep the gate decision of every row and the regulariser scalar of every step this plan runs (column slices and
        row-parallel fp64 plans)."""
        check(_lib.load().dsgd_plan_record(self.engine._ctx, self.handle, C.c_int32(1 if on else 0)))

    def read_record(self, step_begin=0, step_end=None):
        """(mask, s): mask bool [steps, words * 32] -- bit r of a step = row r of the step (workers in order, each list in
        order) was active; s float32 [steps] -- the regulariser scalar the step used."""
        step_end = self.n_steps if step_end is None else step_end
        lib = _lib.load()
        mw = C.c_int32(0)
        check(lib.dsgd_plan_read_record(self.engine._ctx, self.handle, C.c_int64(step_begin), C.c_int64(step_end), None, None, C.byref(mw)))
        n, m = step_end - step_begin, mw.value
        mask = np.zeros((n, max(m, 1)), dtype=np.uint32)
        s = np.zeros(n, dtype=np.float32)
        check(lib.dsgd_plan_read_record(self.engine._ctx, self.handle, C.c_int64(step_begin), C.c_int64(step_end), ptr(mask), ptr(s), None))
        bits = ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).astype(bool).reshape(n, 32 * max(m, 1))
        return bits, s


class TuningInfo(dict):
    """Engine.tuning_info(): a plain dict by name (what bench.py records); an int key reads the slot of that number."""

    SLOTS = ("stream_mode", "hsplit", "fix_shift", "cold_packed", "plan_kernel", "fix_bound", "fstep_rebalances", "eval_group")

    def __getitem__(self, key):
        return dict.__getitem__(self, self.SLOTS[key] if isinstance(key, int) else key)


class Engine:
    def __init__(self, n_features, lam, device=0, flags=0, precision="fp32"):
        """precision: "fp32" (default) or "fp64" -- the fp64 mode (DSGD_F_FP64, include/dsgd.h "THE FP64 MODE"): fp64
        weights and dimSparsity, plans of the reference's batch sizes (<= 4 workers, <= 1,024 rows per step) on the fp64
        column-slice kernel; get_weights / build_dim_sparsity return float64 there."""
        if precision not in ("fp32", "fp64"):
            raise ValueError("precision must be 'fp32' or 'fp64', not %r" % (precision,))
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        self.dim = int(n_features)
        self.dp = self.dim + 1
        self.lam = float(lam)
        self.precision = precision
        if precision == "fp64":
            flags = int(flags) | _lib.F_FP64
        cfg = Config(self.dim, int(device), self.lam, int(flags), 0)
        check(self._lib.dsgd_create(C.byref(cfg), C.byref(self._ctx)))
        self.n_rows = 0
        self.nnz = 0

    # -- lifecycle -----------------------------------------------------------------------------
    def close(self):
        if self._ctx:
            self._lib.dsgd_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data ------------------------------------------------------------------------------------
    def load_csr(self, row_ptr, col, val, label):
        """The data as CSR.  An fp64 engine keeps a float64 `val` as it is (dsgd_load_csr_f64: the reference's Double
        feature values); every other dtype, and every fp32 engine, loads float32 values."""
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = i32(col)
        as_f64 = self.precision == "fp64" and np.asarray(val).dtype == np.float64
        val = f64(val) if as_f64 else f32(val)
        label = np.ascontiguousarray(label, dtype=np.int8)
        n_rows = len(row_ptr) - 1
        if len(label) != n_rows:
            raise ValueError("label has %d entries for %d rows" % (len(label), n_rows))
        if n_rows >= 1 and (len(col) < row_ptr[-1] or len(val) < row_ptr[-1]):
            raise ValueError("col/val shorter than row_ptr[-1]")
        load = self._lib.dsgd_load_csr_f64 if as_f64 else self._lib.dsgd_load_csr
        check(load(self._ctx, C.c_int64(n_rows), ptr(row_ptr), ptr(col), ptr(val), ptr(label)))
        self.n_rows, self.nnz = n_rows, int(row_ptr[-1])

    @property
    def fp64(self):
        return self.precision == "fp64"

    def set_dim_sparsity(self, ds):
        if self.fp64 and np.asarray(ds).dtype == np.float64:   # (kept as it is)
            check(self._lib.dsgd_set_dim_sparsity_f64(self._ctx, ptr(f64(ds, self.dp))))
            return
        check(self._lib.dsgd_set_dim_sparsity(self._ctx, ptr(f32(ds, self.dp))))

    def build_dim_sparsity(self, n_train):
        if self.fp64:   # (the fp64 values, bit for bit the oracle's)
            check(self._lib.dsgd_build_dim_sparsity(self._ctx, C.c_int64(n_train), None))
            return self.get_dim_sparsity()
        out = np.zeros(self.dp, dtype=np.float32)
        check(self._lib.dsgd_build_dim_sparsity(self._ctx, C.c_int64(n_train), ptr(out)))
        return out

    def get_dim_sparsity(self):
        """dimSparsity as the fp64 context holds it (float64; fp64 engines only)."""
        out = np.zeros(self.dp, dtype=np.float64)
        check(self._lib.dsgd_get_dim_sparsity_f64(self._ctx, ptr(out)))
        return out

    def set_weights(self, w):
        if self.fp64 and np.asarray(w).dtype == np.float64:   # (kept as it is)
            check(self._lib.dsgd_set_weights_f64(self._ctx, ptr(f64(w, self.dp))))
            return
        check(self._lib.dsgd_set_weights(self._ctx, ptr(f32(w, self.dp))))

    def get_weights(self):
        if self.fp64:
            out = np.zeros(self.dp, dtype=np.float64)
            check(self._lib.dsgd_get_weights_f64(self._ctx, ptr(out)))
            return out
        out = np.zeros(self.dp, dtype=np.float32)
        check(self._lib.dsgd_get_weights(self._ctx, ptr(out)))
        return out

    def get_weights_f32(self):
        """The weights through the float entry point (an fp64 context rounds its fp64 weights)."""
        out = np.zeros(self.dp, dtype=np.float32)
        check(self._lib.dsgd_get_weights(self._ctx, ptr(out)))
        return out

    def value_bits(self):
        """64 while Double feature values are loaded (load_csr with a float64 array on an fp64 engine), 32 otherwise."""
        v = C.c_int32(0)
        check(self._lib.dsgd_value_bits(self._ctx, C.byref(v)))
        return v.value

    def precision_bits(self):
        v = C.c_int32(0)
        check(self._lib.dsgd_precision(self._ctx, C.byref(v)))
        return v.value

    # -- synchronous path ------------------------------------------------------------------------
    def gradient(self, idx, w=None):
        idx = i32(idx)
        g = np.zeros(self.dp, dtype=np.float32)
        st = BatchStats()
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_gradient(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), ptr(g), C.byref(st)))
        return g, {"n_samples": st.n_samples, "n_active": st.n_active}

    def gradient_f64(self, idx, w=None):
        """SlaveImpl.gradient in Double (dsgd_gradient_f64; fp64 engines): a float64 g of any list length, from the resident
        fp64 weights or from w (float64, which then replaces them)."""
        idx = i32(idx)
        g = np.zeros(self.dp, dtype=np.float64)
        st = BatchStats()
        wv = None if w is None else f64(w, self.dp)
        check(self._lib.dsgd_gradient_f64(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), ptr(g), C.byref(st)))
        return g, {"n_samples": st.n_samples, "n_active": st.n_active}

    def sync_step_f64(self, idx_per_worker, lr):
        """Master.fit's batch closure in Double (dsgd_sync_step_f64; fp64 engines): any number of workers and rows."""
        lists = [i32(a) for a in idx_per_worker]
        k = len(lists)
        ptrs = (C.c_void_p * max(k, 1))(*[ptr(a) for a in lists])
        ns = (C.c_int64 * max(k, 1))(*[len(a) for a in lists])
        st = BatchStats()
        check(self._lib.dsgd_sync_step_f64(self._ctx, ptrs, ns, C.c_int32(k), C.c_double(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def sync_steps_f64(self, idx, offsets, n_steps, n_workers, lr, per_step=False):
        """n_steps steps of sync_step_f64 in ONE call (dsgd_sync_steps_f64; fp64 engines, no communicator): the flat form
        plan_flat takes -- idx = all lists concatenated (step-major, worker-minor), offsets = n_steps * n_workers + 1 prefix
        offsets.  The weights get the bits of the loop of sync_step_f64 calls; returns its totals, with per_step=True also
        `active_per_step` (int64, one per step)."""
        idx = i32(idx)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if n_steps >= 1 and n_workers >= 1 and len(offsets) != n_steps * n_workers + 1:
            raise ValueError("offsets do not describe %d x %d lists" % (n_steps, n_workers))
        act = np.zeros(max(int(n_steps), 1), dtype=np.int64) if per_step else None
        st = BatchStats()
        check(self._lib.dsgd_sync_steps_f64(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(n_steps), C.c_int32(n_workers),
                                            C.c_double(lr), ptr(act), C.byref(st)))
        out = {"n_samples": st.n_samples, "n_active": st.n_active}
        if per_step:
            out["active_per_step"] = act[:n_steps]
        return out

    def forward_f64(self, idx, w=None):
        """SlaveImpl.forward with Double weights (dsgd_forward_f64; fp64 engines): float64 predictions in {-1, 0, +1}."""
        idx = i32(idx)
        pred = np.zeros(len(idx), dtype=np.float64)
        wv = None if w is None else f64(w, self.dp)
        check(self._lib.dsgd_forward_f64(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), ptr(pred)))
        return pred

    def apply(self, g_mean, lr):
        check(self._lib.dsgd_apply(self._ctx, ptr(f32(g_mean, self.dp)), C.c_float(lr)))

    def sync_step(self, idx_per_worker, lr):
        lists = [i32(a) for a in idx_per_worker]
        k = len(lists)
        ptrs = (C.c_void_p * max(k, 1))(*[ptr(a) for a in lists])
        ns = (C.c_int64 * max(k, 1))(*[len(a) for a in lists])
        st = BatchStats()
        check(self._lib.dsgd_sync_step(self._ctx, ptrs, ns, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def sync_step_ranges(self, ranges, lr, asynchronous=False):
        k = len(ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in ranges])
        if asynchronous:
            check(self._lib.dsgd_sync_step_ranges_async(self._ctx, rb, re_, C.c_int32(k), C.c_float(lr)))
            return None
        st = BatchStats()
        check(self._lib.dsgd_sync_step_ranges(self._ctx, rb, re_, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def synchronize(self):
        st = BatchStats()
        check(self._lib.dsgd_synchronize(self._ctx, C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def plan(self, steps, rp64=False):
        """steps: list (per step) of lists (per worker) of index arrays.  rp64=True (fp64 engines): a row-parallel plan
        (dsgd_plan_create_rp64_n) -- any number of workers, any list length, any D, float or Double data."""
        n_steps = len(steps)
        n_workers = len(steps[0]) if n_steps else 0
        flat, offs = [], [0]
        for s in steps:
            if len(s) != n_workers:
                raise ValueError("every step needs the same number of workers")
            for a in s:
                a = i32(a)
                flat.append(a)
                offs.append(offs[-1] + len(a))
        idx = np.concatenate(flat) if flat else np.zeros(0, np.int32)
        offsets = np.asarray(offs, dtype=np.int64)
        h = C.c_void_p()
        create = self._lib.dsgd_plan_create_rp64_n if rp64 else self._lib.dsgd_plan_create_n
        check(create(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(n_steps), C.c_int32(n_workers), C.byref(h)))
        return Plan(self, h, n_steps, n_workers, int(offsets[-1]))

    def plan_flat(self, idx, offsets, n_steps, n_workers, rp64=False):
        """A plan from the flat form: idx = all lists concatenated (step-major, worker-minor), offsets = n_steps * n_workers
        + 1 prefix offsets (what host.epoch_lists returns: one epoch of Master.fit)."""
        idx = i32(idx)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if len(offsets) != n_steps * n_workers + 1 or (n_steps and int(offsets[-1]) != len(idx)):
            raise ValueError("offsets do not describe %d x %d lists over %d entries" % (n_steps, n_workers, len(idx)))
        h = C.c_void_p()
        create = self._lib.dsgd_plan_create_rp64_n if rp64 else self._lib.dsgd_plan_create_n
        check(create(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(n_steps), C.c_int32(n_workers), C.byref(h)))
        return Plan(self, h, n_steps, n_workers, int(offsets[-1]))

    def plan_from_seed(self, jstate, split, max_samples, batch_size, rp64=False):
        """One epoch of Master.fit as a plan whose lists the DEVICE draws, draw for draw the reference's stream
        (dsgd_plan_create_from_seed).  jstate: java.util.Random's internal 48-bit state in front of the epoch; split: the
        workers' row ranges (SplitStrategy.vanilla).  Returns (plan or None, n_steps, new jstate, draws); raises
        DsgdError with code EUNSUPPORTED when the device form does not apply (draw the lists on the host then).
        rp64=True (fp64 engines): the same lists as a row-parallel plan (dsgd_plan_create_from_seed_rp64)."""
        sb = np.asarray([r.start if isinstance(r, range) else r[0] for r in split], dtype=np.int64)
        se = np.asarray([r.stop if isinstance(r, range) else r[1] for r in split], dtype=np.int64)
        st = C.c_uint64(int(jstate))
        h = C.c_void_p()
        n_steps, draws = C.c_int64(0), C.c_int64(0)
        create = self._lib.dsgd_plan_create_from_seed_rp64 if rp64 else self._lib.dsgd_plan_create_from_seed
        check(create(self._ctx, C.byref(st), ptr(sb), ptr(se), C.c_int32(len(sb)), C.c_int64(max_samples),
                     C.c_int32(batch_size), C.byref(h), C.byref(n_steps), C.byref(draws)))
        if not h.value:
            return None, 0, int(st.value), 0
        total = int(sum(min(batch_size, int(e - b) - s_ * batch_size) for s_ in range(n_steps.value) for b, e in zip(sb, se)))
        return Plan(self, h, n_steps.value, len(sb), total), n_steps.value, int(st.value), draws.value

    def plan_from_seed_job(self, jstate, job_lens, first, split_begins, max_samples, batch_size, rp64=False):
        """The epoch of a JOB of len(job_lens) workers drawn by the device, the lists of the workers hosted here
        (dsgd_plan_create_from_seed_job): job workers first .. first + len(split_begins) - 1, hosted worker i over the rows
        split_begins[i] .. + job_lens[first + i] of this engine.  Any batch size, splits up to 2^20 rows; usable with a
        communicator attached (every rank passes the same jstate, job_lens, max_samples, batch_size and number of hosted
        workers).  Returns (plan or None, n_steps, new jstate, draws) -- the state and the draws are the JOB's, the same
        on every rank; DsgdError with code EUNSUPPORTED where the device form does not apply.
        rp64=True (fp64 engines): a row-parallel plan (dsgd_plan_create_from_seed_job_rp64)."""
        jl = np.ascontiguousarray(job_lens, dtype=np.int64)
        sb = np.ascontiguousarray(split_begins, dtype=np.int64)
        if jl.ndim != 1 or sb.ndim != 1:
            raise ValueError("job_lens and split_begins are flat lists")
        st = C.c_uint64(int(jstate))
        h = C.c_void_p()
        n_steps, draws = C.c_int64(0), C.c_int64(0)
        create = self._lib.dsgd_plan_create_from_seed_job_rp64 if rp64 else self._lib.dsgd_plan_create_from_seed_job
        check(create(self._ctx, C.byref(st), ptr(jl), len(jl), int(first), len(sb), ptr(sb), int(max_samples), int(batch_size),
                     C.byref(h), C.byref(n_steps), C.byref(draws)))
        if not h.value:
            return None, 0, int(st.value), 0
        mine = jl[int(first):int(first) + len(sb)]
        total = int(sum(min(batch_size, int(ln) - s_ * batch_size) for s_ in range(n_steps.value) for ln in mine))
        return Plan(self, h, n_steps.value, len(sb), total), n_steps.value, int(st.value), draws.value

    def plan_lists(self, plan):
        """(idx, offsets) of a plan as the device holds them (tests)."""
        n_lists = plan.n_steps * plan.n_workers
        offsets = np.zeros(n_lists + 1, dtype=np.int64)
        check(self._lib.dsgd_plan_read_lists(self._ctx, plan.handle, None, C.c_int64(0), ptr(offsets), C.c_int64(n_lists + 1)))
        idx = np.zeros(int(offsets[-1]), dtype=np.int32)
        check(self._lib.dsgd_plan_read_lists(self._ctx, plan.handle, ptr(idx), C.c_int64(len(idx)), None, C.c_int64(0)))
        return idx, offsets

    def cache_trim(self, keep_bytes=0):
        """Give the device blocks of destroyed plans back (all but keep_bytes); returns the bytes still held."""
        held = C.c_int64(0)
        check(self._lib.dsgd_cache_trim(self._ctx, C.c_int64(keep_bytes), C.byref(held)))
        return held.value

    def plan_run(self, plan, step_begin, step_end, lr):
        """Enqueue the steps [step_begin, step_end) of a plan (of any kind: a logistic plan too -- Engine.lg_plan)."""
        if self.fp64:   # (the reference's learning rate is a Double)
            check(self._lib.dsgd_plan_run_f64(self._ctx, plan.handle, C.c_int64(step_begin), C.c_int64(step_end), C.c_double(lr)))
            return
        check(self._lib.dsgd_plan_run(self._ctx, plan.handle, C.c_int64(step_begin), C.c_int64(step_end), C.c_float(lr)))

    # -- evaluation --------------------------------------------------------------------------------
    def forward(self, idx, w=None):
        idx = i32(idx)
        pred = np.zeros(len(idx), dtype=np.float32)
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_forward(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), ptr(pred)))
        return pred

    def loss_acc(self, row_begin, row_end, w=None):
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_loss_acc(self._ctx, ptr(wv), C.c_int64(row_begin), C.c_int64(row_end), C.byref(loss), C.byref(acc), counts))
        return loss.value, acc.value, list(counts)

    # -- the logistic model (include/dsgd.h "THE LOGISTIC MODEL") ---------------------------------
    # P(y = +1 | x) = sigma(x . w), class = signum(x . w): the TEXTBOOK sign, not the SVM's -signum.  fp32 engines only.
    def lg_gradient(self, idx, w=None):
        """One worker's regularised sum over the listed rows (dsgd_lg_gradient): (g float32 in key order, stats).  w: None
        (the resident weights) or a vector that replaces them."""
        idx = i32(idx)
        g = np.zeros(self.dp, dtype=np.float32)
        st = BatchStats()
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_gradient(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), ptr(g), C.byref(st)))
        return g, {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_sync_step(self, idx_per_worker, lr):
        """One synchronous step over the workers' lists (dsgd_lg_sync_step): sum per worker, mean over the workers."""
        lists = [i32(a) for a in idx_per_worker]
        k = len(lists)
        ptrs = (C.c_void_p * max(k, 1))(*[ptr(a) for a in lists])
        ns = (C.c_int64 * max(k, 1))(*[len(a) for a in lists])
        st = BatchStats()
        check(self._lib.dsgd_lg_sync_step(self._ctx, ptrs, ns, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_sync_step_ranges(self, ranges, lr):
        """lg_sync_step over (begin, end) row ranges: the bits of the step over the same rows as lists."""
        k = len(ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in ranges])
        st = BatchStats()
        check(self._lib.dsgd_lg_sync_step_ranges(self._ctx, rb, re_, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_sync_steps_ranges(self, ranges, n_steps, lr):
        """n_steps steps of lg_sync_step_ranges over the SAME ranges in ONE call (dsgd_lg_sync_steps_ranges): the ranges' entries
        are laid out by column once per ranges configuration, then every step is three launches with no atomic per non-zero.
        The weights and the stats (the rows of one step) get the bits of the loop of lg_sync_step_ranges calls."""
        pairs = []
        for r in ranges:
            if len(r) != 2:
                raise ValueError("a range is a (begin, end) pair, not %r" % (r,))
            pairs.append((operator.index(r[0]), operator.index(r[1])))
        if not pairs:
            raise ValueError("no ranges")
        n_steps = operator.index(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be at least 1, not %d" % n_steps)
        k = len(pairs)
        rb = (C.c_int64 * k)(*[a for a, _ in pairs])
        re_ = (C.c_int64 * k)(*[b for _, b in pairs])
        st = BatchStats()
        check(self._lib.dsgd_lg_sync_steps_ranges(self._ctx, rb, re_, C.c_int32(k), C.c_int64(n_steps), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_sync_steps(self, idx, offsets, n_steps, n_workers, lr):
        """n_steps steps of lg_sync_step in ONE call (dsgd_lg_sync_steps): idx = all lists concatenated (step-major,
        worker-minor), offsets = n_steps * n_workers + 1 prefix offsets -- the flat form of sync_steps_f64.  The weights get
        the bits of the loop of lg_sync_step calls."""
        idx = i32(idx)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if n_steps >= 1 and n_workers >= 1 and len(offsets) != n_steps * n_workers + 1:
            raise ValueError("offsets do not describe %d x %d lists" % (n_steps, n_workers))
        st = BatchStats()
        check(self._lib.dsgd_lg_sync_steps(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(n_steps), C.c_int32(n_workers),
                                           C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_loss_acc(self, row_begin, row_end, w=None):
        """(loss, acc) of rows [row_begin, row_end): lambda |w|^2 + mean log(1 + exp(-y d)), and the share of rows with
        signum(d) == y (dsgd_lg_loss_acc)."""
        loss, acc = C.c_double(0), C.c_double(0)
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_loss_acc(self._ctx, ptr(wv), C.c_int64(row_begin), C.c_int64(row_end), C.byref(loss), C.byref(acc)))
        return loss.value, acc.value

    def lg_predict_proba(self, idx, w=None):
        """P(y = +1 | x) = sigma(x . w) of every listed row, float32 (dsgd_lg_predict)."""
        idx = i32(idx)
        p = np.zeros(len(idx), dtype=np.float32)
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_predict(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), ptr(p)))
        return p

    # -- several topics: one-vs-rest label planes on the same rows (include/dsgd.h "SEVERAL TOPICS") --------------
    lg_topics_max = 8

    def lg_topics_set(self, planes):
        """T <= 8 label planes, int8 [T, n_rows] of +1 / -1 (dsgd_lg_topics_set): the topics' weights start at zero; the
        engine's own labels and weights are not touched.  None or an empty array drops the topics."""
        if planes is None or np.size(planes) == 0:
            check(self._lib.dsgd_lg_topics_set(self._ctx, C.c_int32(0), None))
            return
        planes = np.asarray(planes)
        if planes.ndim != 2 or planes.shape[1] != self.n_rows:
            raise ValueError("planes must be [T, %d], not %r" % (self.n_rows, planes.shape))
        if planes.dtype != np.int8 and not np.array_equal(planes, planes.astype(np.int8)):
            raise ValueError("plane entries must be +1 or -1")
        planes = np.ascontiguousarray(planes, dtype=np.int8)
        check(self._lib.dsgd_lg_topics_set(self._ctx, C.c_int32(planes.shape[0]), ptr(planes)))

    @property
    def n_topics(self):
        """the topics set now, as the library holds them (dsgd_lg_topics_count); 0: none"""
        t = C.c_int32(0)
        check(self._lib.dsgd_lg_topics_count(self._ctx, C.byref(t)))
        return int(t.value)

    def _lg_topics(self):
        """T from the library itself: every array below is sized by the number the call will write"""
        t = self.n_topics
        if t < 1:
            raise _lib.DsgdError(_lib.ESTATE, "no topics set (Engine.lg_topics_set; a load drops them)")
        return t

    def lg_topics_set_weights(self, W):
        """The topics' weights, float32 [T, D + 1] in key order (dsgd_lg_topics_set_weights)."""
        t = self._lg_topics()
        W = np.ascontiguousarray(W, dtype=np.float32)
        if W.shape != (t, self.dp):
            raise ValueError("expected weights of shape (%d, %d), got %r" % (t, self.dp, W.shape))
        check(self._lib.dsgd_lg_topics_set_weights(self._ctx, ptr(W)))

    def lg_topics_get_weights(self):
        t = self._lg_topics()
        W = np.zeros((t, self.dp), dtype=np.float32)
        check(self._lib.dsgd_lg_topics_get_weights(self._ctx, ptr(W)))
        return W

    def lg_topics_sync_step(self, idx_per_worker, lr):
        """One synchronous step of EVERY topic over the workers' lists in two launches (dsgd_lg_topics_sync_step): topic t's
        weights get the bits of lg_sync_step on an engine whose labels are plane t."""
        lists = [i32(a) for a in idx_per_worker]
        k = len(lists)
        ptrs = (C.c_void_p * max(k, 1))(*[ptr(a) for a in lists])
        ns = (C.c_int64 * max(k, 1))(*[len(a) for a in lists])
        st = BatchStats()
        check(self._lib.dsgd_lg_topics_sync_step(self._ctx, ptrs, ns, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_topics_sync_steps(self, idx, offsets, n_steps, n_workers, lr):
        """n_steps steps of lg_topics_sync_step in ONE call (dsgd_lg_topics_sync_steps; lg_sync_steps' flat form)."""
        idx = i32(idx)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if n_steps >= 1 and n_workers >= 1 and len(offsets) != n_steps * n_workers + 1:
            raise ValueError("offsets do not describe %d x %d lists" % (n_steps, n_workers))
        st = BatchStats()
        check(self._lib.dsgd_lg_topics_sync_steps(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(n_steps), C.c_int32(n_workers),
                                                  C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_topics_loss_acc(self, row_begin, row_end):
        """(loss float64 [T], acc float64 [T]) of rows [row_begin, row_end) in ONE launch (dsgd_lg_topics_loss_acc)."""
        t = self._lg_topics()
        loss, acc = np.zeros(t, dtype=np.float64), np.zeros(t, dtype=np.float64)
        check(self._lib.dsgd_lg_topics_loss_acc(self._ctx, C.c_int64(row_begin), C.c_int64(row_end), ptr(loss), ptr(acc)))
        return loss, acc

    def lg_topics_predict(self, idx):
        """P(topic t | x) = sigma(x . w_t) of every listed row: float32 [T, n] (dsgd_lg_topics_predict)."""
        t = self._lg_topics()
        idx = i32(idx)
        p = np.zeros((t, len(idx)), dtype=np.float32)
        check(self._lib.dsgd_lg_topics_predict(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(p)))
        return p

    lg_max_ranges = 16   # ranges of one dsgd_lg_loss_acc_ranges call

    def lg_loss_acc_ranges(self, ranges, w=None):
        """lg_loss_acc over up to 16 (begin, end) row ranges in ONE launch and one synchronisation (dsgd_lg_loss_acc_ranges):
        a list of (loss, acc), each the bits of lg_loss_acc on that range alone.  Ranges may overlap or repeat."""
        k = len(ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in ranges])
        loss = np.zeros(max(k, 1), dtype=np.float64)
        acc = np.zeros(max(k, 1), dtype=np.float64)
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_loss_acc_ranges(self._ctx, ptr(wv), rb, re_, C.c_int32(k), ptr(loss), ptr(acc)))
        return [(float(loss[i]), float(acc[i])) for i in range(k)]

    lg_predict_max_ranges = 256   # ranges of one dsgd_lg_predict_ranges call

    def lg_predict_ranges(self, ranges, w=None, want_proba=False):
        """Master.predict / distributedLoss / distributedAccuracy for the logistic model over the workers' splits in ONE launch
        (dsgd_lg_predict_ranges): `ranges` = up to 256 disjoint (begin, end) row ranges.  Returns (classes, proba, counts,
        range_losses, loss, acc): classes int8 signum(x . w) in {-1, 0, +1}, one per row, range after range; proba (want_proba,
        else None) float32 sigma(x . w), the bits of lg_predict_proba over the same rows; counts int64 [K, 3], every range's
        exact tallies {#class == y, #class == 0, #class == -y}; range_losses float64 [K], each the bits of lg_loss_acc on
        that range alone (0.0 for an empty one); loss and accuracy over all the rows.  w as in lg_loss_acc."""
        k = len(ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in ranges])
        total = sum(max(0, int(r[1]) - int(r[0])) for r in ranges)
        cls = np.zeros(max(total, 1), dtype=np.int8)   # (never a null pointer: the library decides what is refused)
        proba = np.zeros(max(total, 1), dtype=np.float32) if want_proba else None
        counts = np.zeros((max(k, 1), 3), dtype=np.int64)
        range_loss = np.zeros(max(k, 1), dtype=np.float64)
        loss, acc = C.c_double(0), C.c_double(0)
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_predict_ranges(self._ctx, ptr(wv), rb, re_, C.c_int32(k), ptr(cls), ptr(proba), ptr(counts), ptr(range_loss),
                                               C.byref(loss), C.byref(acc)))
        return cls[:total], (proba[:total] if want_proba else None), counts[:k], range_loss[:k], loss.value, acc.value

    def lg_loss_acc_list(self, idx, w=None):
        """Loss and accuracy of the logistic model over the rows `idx` names, ONE launch (dsgd_lg_loss_acc_list; the fold of
        Master.localSampledLoss / localSampledAccuracy over a list drawn elsewhere).  A row named twice counts twice.  Returns
        (loss, acc, counts); over arange(b, e) the bits of lg_loss_acc(b, e)."""
        idx = i32(idx)
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_loss_acc_list(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), C.byref(loss), C.byref(acc), counts))
        return loss.value, acc.value, list(counts)

    def lg_loss_acc_sampled(self, jstate, row_begin, row_end, samples_count, w=None, want_idx=False):
        """loss_acc_sampled for the logistic model (dsgd_lg_loss_acc_sampled): the DEVICE draws the sample, draw for draw the
        reference's stream, and evaluates it.  The arguments, the return value -- (loss, acc, counts, new jstate, draws[, idx])
        -- and the EUNSUPPORTED refusals (nothing drawn) are loss_acc_sampled's; the figures are the bits of lg_loss_acc_list
        on idx."""
        st = C.c_uint64(int(jstate))
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        n, draws = C.c_int64(0), C.c_int64(0)
        cap = max(1, min(int(samples_count), int(row_end) - int(row_begin)))
        idx = np.zeros(cap, dtype=np.int32) if want_idx else None
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_loss_acc_sampled(self._ctx, ptr(wv), C.byref(st), C.c_int64(row_begin), C.c_int64(row_end), C.c_int64(samples_count),
                                                 C.byref(loss), C.byref(acc), counts, ptr(idx), C.byref(n), C.byref(draws)))
        out = (loss.value, acc.value, list(counts), int(st.value), draws.value)
        return out + (idx[:n.value],) if want_idx else out

    def lg_plan(self, steps, slices=False):
        """A resident LOGISTIC plan (dsgd_plan_create_lg_n) from `steps`: list (per step) of lists (per worker) of index arrays,
        as Engine.plan takes them.  It runs through plan_run / synchronize; the weights get the bits of lg_sync_steps.
        slices: see lg_plan_flat."""
        n_steps = len(steps)
        n_workers = len(steps[0]) if n_steps else 0
        flat, offs = [], [0]
        for s in steps:
            if len(s) != n_workers:
                raise ValueError("every step needs the same number of workers")
            for a in s:
                a = i32(a)
                flat.append(a)
                offs.append(offs[-1] + len(a))
        idx = np.concatenate(flat) if flat else np.zeros(0, np.int32)
        return self.lg_plan_flat(idx, np.asarray(offs, dtype=np.int64), n_steps, n_workers, slices=slices)

    def lg_plan_flat(self, idx, offsets, n_steps, n_workers, slices=False):
        """lg_plan from the flat form (what host.epoch_lists returns, what lg_sync_steps takes).
        slices=True (dsgd_plan_create_lg_cs_n): the plan additionally has its column slices laid out, and plan_run on it is ONE
        persistent launch (plan_info code 8) -- deterministic and within tests/logistic_cs_bound.py of the fp64 model, but not
        the bits of lg_sync_steps; where the slices do not apply (include/dsgd.h) it is the plan slices=False makes, code 7."""
        idx = i32(idx)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if n_steps >= 1 and n_workers >= 1 and len(offsets) != n_steps * n_workers + 1:
            raise ValueError("offsets do not describe %d x %d lists" % (n_steps, n_workers))
        h = C.c_void_p()
        create = self._lib.dsgd_plan_create_lg_cs_n if slices else self._lib.dsgd_plan_create_lg_n
        check(create(self._ctx, ptr(idx), C.c_int64(len(idx)), ptr(offsets), C.c_int64(n_steps), C.c_int32(n_workers), C.byref(h)))
        return Plan(self, h, n_steps, n_workers, int(offsets[-1]))

    def lg_plan_from_seed(self, jstate, split, max_samples, batch_size, slices=False):
        """One epoch of Master.fit as a LOGISTIC plan whose lists the device draws (dsgd_plan_create_from_seed_lg): the
        arguments, the return value -- (plan or None, n_steps, new jstate, draws) -- and the EUNSUPPORTED refusals of
        plan_from_seed.  slices=True (dsgd_plan_create_from_seed_lg_cs): as in lg_plan_flat; the lists and the state are the same."""
        sb = np.asarray([r.start if isinstance(r, range) else r[0] for r in split], dtype=np.int64)
        se = np.asarray([r.stop if isinstance(r, range) else r[1] for r in split], dtype=np.int64)
        st = C.c_uint64(int(jstate))
        h = C.c_void_p()
        n_steps, draws = C.c_int64(0), C.c_int64(0)
        create = self._lib.dsgd_plan_create_from_seed_lg_cs if slices else self._lib.dsgd_plan_create_from_seed_lg
        check(create(self._ctx, C.byref(st), ptr(sb), ptr(se), C.c_int32(len(sb)), C.c_int64(max_samples),
                     C.c_int32(batch_size), C.byref(h), C.byref(n_steps), C.byref(draws)))
        if not h.value:
            return None, 0, int(st.value), 0
        total = int(sum(min(batch_size, int(e - b) - s_ * batch_size) for s_ in range(n_steps.value) for b, e in zip(sb, se)))
        return Plan(self, h, n_steps.value, len(sb), total), n_steps.value, int(st.value), draws.value

    def lg_plan_from_seed_job(self, jstate, job_lens, first, split_begins, max_samples, batch_size):
        """A rank's window of the JOB's epoch as a LOGISTIC plan whose lists the device draws (dsgd_plan_create_from_seed_job_lg):
        the arguments, the return value -- (plan or None, n_steps, new jstate, draws), the state and the draws the JOB's, the same
        on every rank -- and the EUNSUPPORTED refusals of plan_from_seed_job.  A local call, accepted without a communicator and
        under comm_init_lg's; plan_run on the plan is then the collective run of an lg_plan_flat plan.  With first = 0 and every
        worker hosted here the plan is lg_plan_from_seed's."""
        jl = np.ascontiguousarray(job_lens, dtype=np.int64)
        sb = np.ascontiguousarray(split_begins, dtype=np.int64)
        if jl.ndim != 1 or sb.ndim != 1:
            raise ValueError("job_lens and split_begins are flat lists")
        st = C.c_uint64(int(jstate))
        h = C.c_void_p()
        n_steps, draws = C.c_int64(0), C.c_int64(0)
        check(self._lib.dsgd_plan_create_from_seed_job_lg(self._ctx, C.byref(st), ptr(jl), len(jl), int(first), len(sb), ptr(sb), int(max_samples),
                                                          int(batch_size), C.byref(h), C.byref(n_steps), C.byref(draws)))
        if not h.value:
            return None, 0, int(st.value), 0
        mine = jl[int(first):int(first) + len(sb)]
        total = int(sum(min(batch_size, int(ln) - s_ * batch_size) for s_ in range(n_steps.value) for ln in mine))
        return Plan(self, h, n_steps.value, len(sb), total), n_steps.value, int(st.value), draws.value

    def lg_eval_job(self, ranges, w=None):
        """The JOB's distributedLoss / distributedAccuracy on every rank (dsgd_lg_eval_job; COLLECTIVE under comm_init_lg): this
        rank's len(ranges) (begin, end) row ranges take the positions rank * len(ranges) + j of a job of K = len(ranges) * world
        ranges.  Returns (counts int64 [K, 3], range_losses float64 [K], loss, acc), on every rank the bits lg_predict_ranges
        returns on ONE engine holding the ranks' rows in rank order.  Without a communicator world = 1.  w as in lg_loss_acc."""
        k = len(ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in ranges])
        counts = np.zeros((self.lg_predict_max_ranges, 3), dtype=np.int64)   # (K = k * world is the library's to say)
        range_loss = np.zeros(self.lg_predict_max_ranges, dtype=np.float64)
        loss, acc = C.c_double(0), C.c_double(0)
        K = C.c_int32(0)
        wv = None if w is None else f32(w, self.dp)
        check(self._lib.dsgd_lg_eval_job(self._ctx, ptr(wv), rb, re_, C.c_int32(k), ptr(counts), ptr(range_loss), C.byref(loss), C.byref(acc),
                                         C.byref(K)))
        return counts[:K.value].copy(), range_loss[:K.value].copy(), loss.value, acc.value

    # -- the logistic model's asynchronous iteration (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS) --
    def lg_async_step(self, idx, lr, want_delta=False):
        """One iteration of Slave.asyncTask for the logistic model (dsgd_lg_async_step): the MEAN gradient over the listed rows,
        regularised once, w <- (float)(w - lr r).  Returns (delta float64 in key order, or None; stats); a peer applies the
        delta with lg_update_grad and gets the same bits."""
        idx = i32(idx)
        delta = np.zeros(self.dp, dtype=np.float64) if want_delta else None
        st = BatchStats()
        check(self._lib.dsgd_lg_async_step(self._ctx, ptr(idx), C.c_int64(len(idx)), C.c_double(lr), ptr(delta), C.byref(st)))
        return delta, {"n_samples": st.n_samples, "n_active": st.n_active}

    def lg_update_grad(self, keys, values):
        """A peer's update (dsgd_lg_update_grad): w[k] = float32(float64(w[k]) - v) for every (unique) key."""
        keys = i32(keys)
        values = f64(values)
        if keys.ndim != 1 or keys.shape != values.shape:
            raise ValueError("keys / values length mismatch")
        check(self._lib.dsgd_lg_update_grad(self._ctx, ptr(keys), ptr(values), C.c_int64(len(keys))))

    def lg_async_plan(self, assigned_ranges, batch, seed=0, positional_bug=True, first_update=0, n_updates=1, slices=False):
        """Updates [first_update, first_update + n_updates) of the zero-lag asynchronous schedule as a one-worker LOGISTIC plan
        whose lists the device draws (dsgd_async_plan_create_lg; async_plan's arguments and lists).  slices=True
        (dsgd_async_plan_create_lg_cs): additionally with its column slices, so that plan_run_async_lg is ONE persistent launch;
        a batch beyond 1,024 rows or a model the slices cannot hold is refused (DSGD_EUNSUPPORTED)."""
        k = len(assigned_ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in assigned_ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in assigned_ranges])
        h = C.c_void_p()
        create = self._lib.dsgd_async_plan_create_lg_cs if slices else self._lib.dsgd_async_plan_create_lg
        check(create(self._ctx, rb, re_, C.c_int32(k), C.c_int32(batch), C.c_uint64(seed), C.c_int32(1 if positional_bug else 0),
                     C.c_int64(first_update), C.c_int64(n_updates), C.byref(h)))
        return Plan(self, h, int(n_updates), 1, int(n_updates) * int(batch))

    def plan_run_async_lg(self, plan, step_begin, step_end, lr):
        """Enqueue the asynchronous iterations [step_begin, step_end) of a one-worker logistic plan (lg_async_plan, or lg_plan_flat
        with n_workers = 1): the bits of lg_async_step on the same lists, or on column slices one persistent launch."""
        check(self._lib.dsgd_plan_run_async_lg(self._ctx, plan.handle, C.c_int64(step_begin), C.c_int64(step_end), C.c_double(lr)))

    predict_max_ranges = 256   # K of one dsgd_predict_ranges call (host.MasterSync asks forward per split beyond it)

    def predict_ranges(self, ranges, w=None):
        """Master.predict over the workers' splits in ONE launch (dsgd_predict_ranges; core/Master.scala:61-98): `ranges` =
        the splits as (begin, end) row ranges.  Returns (pred, counts, loss, acc): pred int8 in {-1, 0, +1}, one per row,
        range after range; counts int64 [K, 3], the exact tallies {#p==y, #p==0, #p==-y} of every range; loss and accuracy
        over all the rows, loss_acc's expression.  w: None (the resident weights) or a vector that replaces them -- float64
        through dsgd_predict_ranges_f64 on an fp64 engine, float32 otherwise."""
        k = len(ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in ranges])
        total = sum(max(0, int(r[1]) - int(r[0])) for r in ranges)
        pred = np.zeros(max(total, 1), dtype=np.int8)   # (never a null pointer: the library decides what is refused)
        counts = np.zeros((max(k, 1), 3), dtype=np.int64)
        loss, acc = C.c_double(0), C.c_double(0)
        if self.fp64 and w is not None:
            check(self._lib.dsgd_predict_ranges_f64(self._ctx, ptr(f64(w, self.dp)), rb, re_, C.c_int32(k), ptr(pred), ptr(counts),
                                                    C.byref(loss), C.byref(acc)))
        else:
            wv = None if w is None else f32(w, self.dp)
            check(self._lib.dsgd_predict_ranges(self._ctx, ptr(wv), rb, re_, C.c_int32(k), ptr(pred), ptr(counts), C.byref(loss),
                                                C.byref(acc)))
        return pred[:total], counts[:k], loss.value, acc.value

    def loss_acc_list(self, idx, w=None):
        """Loss and accuracy over the rows `idx` names, tallied in ONE launch (dsgd_loss_acc_list; the fold of
        Master.localSampledLoss / localSampledAccuracy, core/Master.scala:109-118, over a list drawn elsewhere).  A row
        named twice counts twice.  Returns (loss, acc, counts) as loss_acc does; w as in predict_ranges."""
        idx = i32(idx)
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        if self.fp64 and w is not None:
            check(self._lib.dsgd_loss_acc_list_f64(self._ctx, ptr(f64(w, self.dp)), ptr(idx), C.c_int64(len(idx)), C.byref(loss),
                                                   C.byref(acc), counts))
        else:
            wv = None if w is None else f32(w, self.dp)
            check(self._lib.dsgd_loss_acc_list(self._ctx, ptr(wv), ptr(idx), C.c_int64(len(idx)), C.byref(loss), C.byref(acc), counts))
        return loss.value, acc.value, list(counts)

    def loss_acc_sampled(self, jstate, row_begin, row_end, samples_count, w=None, want_idx=False):
        """Master.localSampledLoss / localSampledAccuracy (core/Master.scala:109-118) over a sample the DEVICE draws, draw
        for draw the reference's stream (dsgd_loss_acc_sampled): the first min(samples_count, row_end - row_begin) entries of
        Random.shuffle over the window, from java.util.Random's 48-bit state `jstate`.  Returns (loss, acc, counts, new
        jstate, draws[, idx]) -- idx (want_idx) the rows evaluated, in the shuffle's order.  Raises DsgdError with code
        EUNSUPPORTED where the device form does not apply (windows beyond 2^20 rows, more than 512 rejections): nothing was
        drawn -- draw the list on the host (csrc/jrand.c) and call loss_acc_list."""
        st = C.c_uint64(int(jstate))
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        n, draws = C.c_int64(0), C.c_int64(0)
        cap = max(1, min(int(samples_count), int(row_end) - int(row_begin)))
        idx = np.zeros(cap, dtype=np.int32) if want_idx else None
        if self.fp64 and w is not None:
            check(self._lib.dsgd_loss_acc_sampled_f64(self._ctx, ptr(f64(w, self.dp)), C.byref(st), C.c_int64(row_begin), C.c_int64(row_end),
                                                      C.c_int64(samples_count), C.byref(loss), C.byref(acc), counts, ptr(idx),
                                                      C.byref(n), C.byref(draws)))
        else:
            wv = None if w is None else f32(w, self.dp)
            check(self._lib.dsgd_loss_acc_sampled(self._ctx, ptr(wv), C.byref(st), C.c_int64(row_begin), C.c_int64(row_end),
                                                  C.c_int64(samples_count), C.byref(loss), C.byref(acc), counts, ptr(idx), C.byref(n),
                                                  C.byref(draws)))
        out = (loss.value, acc.value, list(counts), int(st.value), draws.value)
        return out + (idx[:n.value],) if want_idx else out

    # -- asynchronous path -------------------------------------------------------------------------
    def async_step(self, idx, lr, want_delta=False):
        idx = i32(idx)
        if self.fp64:   # (dsgd_async_step_f64: a float64 delta, the reference's Double learning rate)
            delta = np.zeros(self.dp, dtype=np.float64) if want_delta else None
            st = BatchStats()
            check(self._lib.dsgd_async_step_f64(self._ctx, ptr(idx), C.c_int64(len(idx)), C.c_double(lr), ptr(delta), C.byref(st)))
            return delta, {"n_samples": st.n_samples, "n_active": st.n_active}
        delta = np.zeros(self.dp, dtype=np.float32) if want_delta else None
        st = BatchStats()
        check(self._lib.dsgd_async_step(self._ctx, ptr(idx), C.c_int64(len(idx)), C.c_float(lr), ptr(delta), C.byref(st)))
        return delta, {"n_samples": st.n_samples, "n_active": st.n_active}

    def update_grad(self, keys, values):
        keys = i32(keys)
        values = f64(values) if self.fp64 else f32(values)   # (fp64: the Double values as they are, no float cast)
        if len(keys) != len(values):
            raise ValueError("keys / values length mismatch")
        if self.fp64:
            check(self._lib.dsgd_update_grad_f64(self._ctx, ptr(keys), ptr(values), C.c_int64(len(keys))))
            return
        check(self._lib.dsgd_update_grad(self._ctx, ptr(keys), ptr(values), C.c_int64(len(keys))))

    # -- Sparse values at the boundary (include/dsgd.h "SPARSE VALUES") ------------------------------
    # The reference's Sparse{map, size} as parallel arrays: int32 keys (ascending on the way out) and values of the
    # engine's precision.  Results, statistics, state rules and errors are the dense twins'; the engine's precision picks
    # the ABI form, as update_grad does.
    def _sparse_out(self):
        if getattr(self, "_sp_keys", None) is None:   # D + 1 slots of scratch, once per engine: always enough room
            self._sp_keys = np.zeros(self.dp, dtype=np.int32)
            self._sp_vals = np.zeros(self.dp, dtype=np.float64 if self.fp64 else np.float32)
        return self._sp_keys, self._sp_vals

    def _sparse_in(self, pairs):
        keys, vals = pairs
        keys = i32(keys)
        vals = f64(vals) if self.fp64 else f32(vals)
        if keys.ndim != 1 or keys.shape != vals.shape:
            raise ValueError("keys / values length mismatch")
        return keys, vals

    def set_weights_sparse(self, keys, vals):
        keys, vals = self._sparse_in((keys, vals))
        fn = self._lib.dsgd_set_weights_sparse_f64 if self.fp64 else self._lib.dsgd_set_weights_sparse
        check(fn(self._ctx, ptr(keys), ptr(vals), C.c_int64(len(keys))))

    def get_weights_sparse(self):
        """The resident weights as (keys ascending, values): the entries with abs(v) > 1e-20."""
        k, v = self._sparse_out()
        nnz = C.c_int64(0)
        fn = self._lib.dsgd_get_weights_sparse_f64 if self.fp64 else self._lib.dsgd_get_weights_sparse
        check(fn(self._ctx, ptr(k), ptr(v), C.c_int64(self.dp), C.byref(nnz)))
        return k[:nnz.value].copy(), v[:nnz.value].copy()

    def gradient_sparse(self, idx, w=None):
        """SlaveImpl.gradient with Sparse in and out: (keys, vals, stats).  w: None (the resident weights) or a
        (keys, vals) pair, which then replaces them."""
        idx = i32(idx)
        wk, wv, wn = (None, None, -1) if w is None else (*self._sparse_in(w), len(w[0]))
        k, v = self._sparse_out()
        nnz = C.c_int64(0)
        st = BatchStats()
        fn = self._lib.dsgd_gradient_sparse_f64 if self.fp64 else self._lib.dsgd_gradient_sparse
        check(fn(self._ctx, ptr(wk), ptr(wv), C.c_int64(wn), ptr(idx), C.c_int64(len(idx)), ptr(k), ptr(v), C.c_int64(self.dp),
                 C.byref(nnz), C.byref(st)))
        return k[:nnz.value].copy(), v[:nnz.value].copy(), {"n_samples": st.n_samples, "n_active": st.n_active}

    def async_step_sparse(self, idx, lr):
        """One iteration of Slave.asyncTask; the delta it gossips as (keys, vals, stats)."""
        idx = i32(idx)
        k, v = self._sparse_out()
        nnz = C.c_int64(0)
        st = BatchStats()
        if self.fp64:
            check(self._lib.dsgd_async_step_sparse_f64(self._ctx, ptr(idx), C.c_int64(len(idx)), C.c_double(lr), ptr(k), ptr(v),
                                                       C.c_int64(self.dp), C.byref(nnz), C.byref(st)))
        else:
            check(self._lib.dsgd_async_step_sparse(self._ctx, ptr(idx), C.c_int64(len(idx)), C.c_float(lr), ptr(k), ptr(v),
                                                   C.c_int64(self.dp), C.byref(nnz), C.byref(st)))
        return k[:nnz.value].copy(), v[:nnz.value].copy(), {"n_samples": st.n_samples, "n_active": st.n_active}

    def async_plan(self, assigned_ranges, batch, seed=0, positional_bug=True, first_update=0, n_updates=1, rp64=False):
        """fp64 engines: updates [first_update, first_update + n_updates) of the zero-lag asynchronous schedule as a
        one-worker plan whose lists the device draws (dsgd_async_plan_create): update u is worker u mod K at its
        iteration u div K, with the rows the lock-free engine's worker draws there (oracle/hogwild_replay.hog_rows).
        rp64=True: the same lists as a row-parallel plan (dsgd_async_plan_create_rp64: Double data, any batch, any D)."""
        k = len(assigned_ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in assigned_ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in assigned_ranges])
        h = C.c_void_p()
        create = self._lib.dsgd_async_plan_create_rp64 if rp64 else self._lib.dsgd_async_plan_create
        check(create(self._ctx, rb, re_, C.c_int32(k), C.c_int32(batch), C.c_uint64(seed), C.c_int32(1 if positional_bug else 0),
                     C.c_int64(first_update), C.c_int64(n_updates), C.byref(h)))
        return Plan(self, h, int(n_updates), 1, int(n_updates) * int(batch))

    def plan_run_async(self, plan, step_begin, step_end, lr):
        """The asynchronous iterations [step_begin, step_end) of a one-worker plan on the fp64 weights."""
        check(self._lib.dsgd_plan_run_async_f64(self._ctx, plan.handle, C.c_int64(step_begin), C.c_int64(step_end), C.c_double(lr)))

    def async_start(self, assigned_ranges, batch, lr, max_updates, seed=0, positional_bug=True):
        k = len(assigned_ranges)
        rb = (C.c_int64 * max(k, 1))(*[int(r[0]) for r in assigned_ranges])
        re_ = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in assigned_ranges])
        check(self._lib.dsgd_async_start(self._ctx, rb, re_, C.c_int32(k), C.c_int32(batch), C.c_float(lr),
                                         C.c_int64(max_updates), C.c_uint64(seed), C.c_int32(1 if positional_bug else 0)))

    def async_set_exchange(self, every_updates):
        """Cross-GPU asynchronous mode: exchange the summed updates every `every_updates` local updates (0 = off)."""
        check(self._lib.dsgd_async_set_exchange(self._ctx, C.c_int64(every_updates)))

    def async_updates(self):
        n, running = C.c_int64(0), C.c_int32(0)
        check(self._lib.dsgd_async_updates(self._ctx, C.byref(n), C.byref(running)))
        return n.value, bool(running.value)

    def async_stop(self):
        check(self._lib.dsgd_async_stop(self._ctx))

    def async_wait(self):
        check(self._lib.dsgd_async_wait(self._ctx))

    def async_stats(self):
        """Counters of the lock-free engine (updates, samples, active rows, lane-level weight atomics) and its regulariser
        scalar s = 2 lambda (w . ds): as kept incrementally on the device / recomputed from the weights as they are now."""
        cnt = (C.c_int64 * 4)()
        a, b = C.c_double(0), C.c_double(0)
        check(self._lib.dsgd_async_stats(self._ctx, cnt, C.byref(a), C.byref(b)))
        return {"updates": cnt[0], "samples": cnt[1], "active": cnt[2], "atomics": cnt[3], "s_engine": a.value, "s_exact": b.value}

    def async_check(self, row_begin, row_end):
        """MasterAsync's loss check on ONE snapshot of the weights (dsgd_async_check; fp32 engines, running or not):
        (loss, acc, counts, (updates_lo, updates_hi)) of a copy taken now.  Every update with a commit number <= updates_lo
        is in the copy whole; later ones may be in it in part.  async_check_keep / async_check_weights hand the copy on."""
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        win = (C.c_int64 * 2)()
        check(self._lib.dsgd_async_check(self._ctx, C.c_int64(row_begin), C.c_int64(row_end), C.byref(loss), C.byref(acc), counts, win))
        return loss.value, acc.value, list(counts), (win[0], win[1])

    def async_check_keep(self):
        """The last async_check's snapshot becomes the best one (two device handles change places)."""
        check(self._lib.dsgd_async_check_keep(self._ctx))

    def async_check_weights(self, which=0):
        """The snapshot of the last async_check (which = 0) or the kept one (1), key order; the live weights are not touched."""
        out = np.zeros(self.dp, dtype=np.float32)
        check(self._lib.dsgd_async_check_weights(self._ctx, C.c_int32(which), ptr(out)))
        return out

    def async_set_trace(self, capacity):
        """Attach a trace of `capacity` update records to the following lock-free runs (0 detaches it)."""
        check(self._lib.dsgd_async_set_trace(self._ctx, C.c_int64(capacity)))

    def async_read_trace(self):
        """The recorded updates of the last run in commit order (record i = update number i + 1) as a dict of arrays:
        worker, it (the worker's iteration = the sampler's key), read_at (update count its weights were read at), s (the
        regulariser scalar it used), n_active, mask (bool [n, batch]: the gate decision of every sampled row);
        see dsgd_async_set_trace."""
        n, mw = C.c_int64(0), C.c_int32(0)
        check(self._lib.dsgd_async_read_trace(self._ctx, None, None, None, None, None, None, C.c_int64(0), C.byref(n), C.byref(mw)))
        k, m = n.value, mw.value
        worker = np.zeros(k, dtype=np.int32)
        it = np.zeros(k, dtype=np.uint32)
        read_at = np.zeros(k, dtype=np.int64)
        s = np.zeros(k, dtype=np.float32)
        n_active = np.zeros(k, dtype=np.int32)
        mask = np.zeros((k, m), dtype=np.uint32)
        if k:
            check(self._lib.dsgd_async_read_trace(self._ctx, ptr(worker), ptr(it), ptr(read_at), ptr(s), ptr(n_active), ptr(mask),
                                                  C.c_int64(k), None, None))
        bits = ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).astype(bool).reshape(k, 32 * m)
        # what every decision was taken on: the x . w of each sampled row, and the update count known to be in the weights
        bo = C.c_int32(0)
        check(self._lib.dsgd_async_read_trace_dots(self._ctx, None, None, C.c_int64(0), C.byref(bo)))
        seen_from = np.zeros(k, dtype=np.int64)
        dots = np.zeros((k, max(1, bo.value)), dtype=np.float32)
        if k:
            check(self._lib.dsgd_async_read_trace_dots(self._ctx, ptr(seen_from), ptr(dots), C.c_int64(k), None))
        return {"worker": worker, "it": it, "read_at": read_at, "s": s, "n_active": n_active, "mask": bits,
                "seen_from": seen_from, "dot": dots}

    # -- multi-GPU ---------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        check(_lib.load().dsgd_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, world_size, rank):
        if len(unique_id) != _lib.UNIQUE_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % _lib.UNIQUE_ID_BYTES)
        check(self._lib.dsgd_comm_init(self._ctx, C.c_char_p(unique_id), C.c_int32(world_size), C.c_int32(rank)))

    def comm_init_f64(self, unique_id, world_size, rank):
        """Attach this fp64 engine to a communicator (dsgd_comm_init_f64): one column ranking and one vexp on every rank
        from here on, sync_step_f64 / sync_step / loss_acc span the ranks; row-parallel plans (plan(..., rp64=True),
        plan_flat(rp64=True)) are accepted and their plan_run is a collective call with one agreement per call; every other
        plan is refused until comm_destroy."""
        if len(unique_id) != _lib.UNIQUE_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % _lib.UNIQUE_ID_BYTES)
        check(self._lib.dsgd_comm_init_f64(self._ctx, C.c_char_p(unique_id), C.c_int32(world_size), C.c_int32(rank)))

    def comm_init_f64v(self, unique_id, world_size, rank):
        """comm_init_f64 for Double feature values (dsgd_comm_init_f64v): the same communicator, accepted with doubles loaded
        (load_csr of a float64 array) and accepting that load while attached; sync_step_f64 on Double data gathers both words
        of every column sum, so the replicas hold the bits of ONE context over all the rows as doubles.  Float data: exactly
        comm_init_f64."""
        if len(unique_id) != _lib.UNIQUE_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % _lib.UNIQUE_ID_BYTES)
        check(self._lib.dsgd_comm_init_f64v(self._ctx, C.c_char_p(unique_id), C.c_int32(world_size), C.c_int32(rank)))

    def comm_init_lg(self, unique_id, world_size, rank):
        """Attach this fp32 engine to the communicator the LOGISTIC model's steps span (dsgd_comm_init_lg): lg_sync_step,
        lg_sync_step_ranges, lg_sync_steps_ranges, lg_sync_steps and plan_run on an lg_plan become collective -- every rank
        with the same number of hosted workers and steps, on its own shard -- and leave on every rank the bits of one engine
        over all the rows.  lg_gradient, lg_predict_proba, lg_loss_acc and lg_loss_acc_ranges stay local to the shard.  The
        SVM's calls behave as under comm_init."""
        check(self._lib.dsgd_comm_init_lg(self._ctx, C.c_char_p(unique_id), C.c_int32(world_size), C.c_int32(rank)))

    def comm_destroy(self):
        check(self._lib.dsgd_comm_destroy(self._ctx))

    # -- profiling ---------------------------------------------------------------------------------
    def prof_enable(self, on=True):
        """0 / False: off; 1 / True: bracket every profiled kernel; 2: the dominant gradient kernel only."""
        check(self._lib.dsgd_prof_enable(self._ctx, C.c_int32(int(on))))

    def prof_read(self, reset=True):
        ms, n = C.c_double(0), C.c_int64(0)
        check(self._lib.dsgd_prof_read(self._ctx, C.byref(ms), C.byref(n), C.c_int32(1 if reset else 0)))
        return ms.value, n.value

    def prof_read_kinds(self):
        """{kind: (avg ms, launches)} of the main / cold x.w / cold gradient kernels of the split layout."""
        ms = (C.c_double * 3)()
        n = (C.c_int64 * 3)()
        check(self._lib.dsgd_prof_read_kinds(self._ctx, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(("main", "cdot", "cgrad"))}

    def range_nnz(self, row_begin, row_end):
        """(non-zeros, of which in the cold stream) of rows [row_begin, row_end) as held internally."""
        a, b = C.c_int64(), C.c_int64()
        check(self._lib.dsgd_range_nnz(self._ctx, C.c_int64(row_begin), C.c_int64(row_end), C.byref(a), C.byref(b)))
        return a.value, b.value

    def tuning_info(self):
        """dsgd_tuning_info's slots by name; a slot number reads the same value (tuning_info()[7] is "eval_group": the lanes
        per row of the fp32 row-wise evaluation kernels for the loaded data)."""
        v = (C.c_int32 * 8)()
        n = 8
        while n > 6 and self._lib.dsgd_tuning_info(self._ctx, v, C.c_int32(n)) != 0:   # (an older build in an A/B run: seven or six slots)
            n -= 1
        if n == 6:
            check(self._lib.dsgd_tuning_info(self._ctx, v, C.c_int32(6)))
        info = TuningInfo(zip(TuningInfo.SLOTS[:max(n, 7)], [int(x) for x in v]))
        # slot [0]: 4 = the split layout; 5 = ... whose last row-chunk launch read the packed copies of the streams (DSGD_FSTEP_PACKED)
        info["fstep_packed"] = int(info["stream_mode"] == 5)
        return info

    def column_ranks(self):
        """Internal frequency rank of every key (D + 1 entries); identical on all ranks of a communicator."""
        v = np.zeros(self.dp, dtype=np.int32)
        check(self._lib.dsgd_column_ranks(self._ctx, ptr(v)))
        return v

    def debug_cycles(self, reset=True):
        v = (C.c_uint64 * 16)()
        check(self._lib.dsgd_debug_cycles(self._ctx, v, C.c_int32(1 if reset else 0)))
        return [int(x) for x in v]

    def grad_kernel_name(self):
        return self._lib.dsgd_grad_kernel_name(self._ctx).decode()


class EngineGroup:
    """Several contexts (one per device, each with its own rows) driven by ONE host thread: the dsgd_*_devices entry
    points of include/dsgd.h (the reference's dev role runs the master and every slave in one JVM, Main.scala:144-158).
    Arrays over workers are context-major."""

    def __init__(self, engines):
        self.engines = list(engines)
        self._lib = _lib.load()
        self._ctxs = (C.c_void_p * len(self.engines))(*[e._ctx for e in self.engines])
        self.n = len(self.engines)

    def comm_init_all(self):
        check(self._lib.dsgd_comm_init_all(self._ctxs, C.c_int32(self.n)))

    def build_dim_sparsity(self, n_train_per_engine):
        nt = (C.c_int64 * self.n)(*[int(v) for v in n_train_per_engine])
        check(self._lib.dsgd_build_dim_sparsity_devices(self._ctxs, C.c_int32(self.n), nt))

    def sync_step(self, lists_per_engine, lr):
        """lists_per_engine: per engine, the index lists of its hosted workers (the same number for every engine)."""
        k = len(lists_per_engine[0])
        flat = [i32(a) for ls in lists_per_engine for a in ls]
        if len(lists_per_engine) != self.n or any(len(ls) != k for ls in lists_per_engine):
            raise ValueError("every engine needs the same number of workers")
        ptrs = (C.c_void_p * len(flat))(*[ptr(a) for a in flat])
        ns = (C.c_int64 * len(flat))(*[len(a) for a in flat])
        st = BatchStats()
        check(self._lib.dsgd_sync_step_devices(self._ctxs, C.c_int32(self.n), ptrs, ns, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def sync_step_ranges(self, ranges_per_engine, lr):
        k = len(ranges_per_engine[0])
        if len(ranges_per_engine) != self.n or any(len(r) != k for r in ranges_per_engine):
            raise ValueError("every engine needs the same number of workers")
        flat = [r for rs in ranges_per_engine for r in rs]
        rb = (C.c_int64 * len(flat))(*[int(r[0]) for r in flat])
        re_ = (C.c_int64 * len(flat))(*[int(r[1]) for r in flat])
        st = BatchStats()
        check(self._lib.dsgd_sync_step_ranges_devices(self._ctxs, C.c_int32(self.n), rb, re_, C.c_int32(k), C.c_float(lr), C.byref(st)))
        return {"n_samples": st.n_samples, "n_active": st.n_active}

    def loss_acc(self, range_per_engine):
        rb = (C.c_int64 * self.n)(*[int(r[0]) for r in range_per_engine])
        re_ = (C.c_int64 * self.n)(*[int(r[1]) for r in range_per_engine])
        loss, acc = C.c_double(0), C.c_double(0)
        counts = (C.c_int64 * 3)()
        check(self._lib.dsgd_loss_acc_devices(self._ctxs, C.c_int32(self.n), rb, re_, C.byref(loss), C.byref(acc), counts))
        return loss.value, acc.value, list(counts)


def device_count():
    return _lib.load().dsgd_device_count()
