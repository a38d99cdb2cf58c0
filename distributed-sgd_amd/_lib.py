"""ctypes binding of include/dsgd.h -- the same symbols the JNI shim binds.

There is deliberately NO CPU fallback here: if libdsgd_hip.so is missing or no gfx950 device is
visible, calls fail loudly (DsgdError / OSError).
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.environ.get("DSGD_LIB_PATH") or os.path.join(HERE, "lib", "libdsgd_hip.so")  # (override: A/B runs of two builds)

OK, EINVAL, ERANGE, ESTATE, EHIP, ERCCL, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7
UNIQUE_ID_BYTES = 128

# every symbol include/dsgd.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    "dsgd_abi_version", "dsgd_last_error", "dsgd_device_count", "dsgd_create", "dsgd_destroy", "dsgd_load_csr",
    "dsgd_n_rows", "dsgd_set_dim_sparsity", "dsgd_build_dim_sparsity", "dsgd_set_weights", "dsgd_get_weights",
    "dsgd_gradient", "dsgd_apply", "dsgd_sync_step", "dsgd_sync_step_ranges", "dsgd_plan_create", "dsgd_plan_create_n", "dsgd_plan_create_from_seed", "dsgd_plan_read_lists", "dsgd_cache_trim",
    "dsgd_plan_destroy", "dsgd_plan_run", "dsgd_plan_info", "dsgd_plan_record", "dsgd_plan_read_record", "dsgd_sync_step_ranges_async", "dsgd_synchronize", "dsgd_forward",
    "dsgd_loss_acc", "dsgd_async_step", "dsgd_update_grad", "dsgd_async_start", "dsgd_async_updates",
    "dsgd_async_stop", "dsgd_async_wait", "dsgd_comm_unique_id", "dsgd_comm_init", "dsgd_comm_destroy",
    "dsgd_prof_enable", "dsgd_prof_read", "dsgd_prof_read_kinds", "dsgd_range_nnz", "dsgd_grad_kernel_name",
    "dsgd_device_ptrs", "dsgd_async_set_exchange", "dsgd_async_stats", "dsgd_async_set_trace", "dsgd_async_read_trace", "dsgd_async_read_trace_dots", "dsgd_tuning_info", "dsgd_column_ranks", "dsgd_debug_cycles",
    "dsgd_comm_init_all", "dsgd_build_dim_sparsity_devices", "dsgd_sync_step_devices", "dsgd_sync_step_ranges_devices",
    "dsgd_loss_acc_devices",
    "dsgd_dense_create", "dsgd_dense_destroy", "dsgd_dense_generate", "dsgd_dense_load", "dsgd_dense_set_weights",
    "dsgd_dense_get_weights", "dsgd_dense_step", "dsgd_dense_synchronize", "dsgd_dense_loss", "dsgd_dense_comm_init",
    "dsgd_dense_prof",
    "dsgd_dense_step_list", "dsgd_dense_loss_list", "dsgd_dense_predict", "dsgd_dense_predict_list",
    "dsgd_dense_plan_create", "dsgd_dense_plan_run", "dsgd_dense_plan_destroy",
    "dsgd_set_weights_f64", "dsgd_get_weights_f64", "dsgd_set_dim_sparsity_f64", "dsgd_get_dim_sparsity_f64",
    "dsgd_plan_run_f64", "dsgd_precision",
    "dsgd_async_step_f64", "dsgd_update_grad_f64", "dsgd_async_plan_create", "dsgd_plan_run_async_f64",
    "dsgd_gradient_f64", "dsgd_sync_step_f64", "dsgd_forward_f64",
    "dsgd_comm_init_f64",
    "dsgd_set_weights_sparse", "dsgd_set_weights_sparse_f64", "dsgd_get_weights_sparse", "dsgd_get_weights_sparse_f64",
    "dsgd_gradient_sparse", "dsgd_gradient_sparse_f64", "dsgd_async_step_sparse", "dsgd_async_step_sparse_f64",
    "dsgd_load_csr_f64", "dsgd_value_bits",
    "dsgd_sync_steps_f64",
    "dsgd_comm_init_f64v",
    "dsgd_plan_create_rp64_n", "dsgd_plan_create_from_seed_rp64", "dsgd_async_plan_create_rp64",
    "dsgd_predict_ranges", "dsgd_predict_ranges_f64",
    "dsgd_plan_create_from_seed_job", "dsgd_plan_create_from_seed_job_rp64",
    "dsgd_loss_acc_list", "dsgd_loss_acc_list_f64", "dsgd_loss_acc_sampled", "dsgd_loss_acc_sampled_f64",
    "dsgd_async_check", "dsgd_async_check_keep", "dsgd_async_check_weights",
    "dsgd_lg_gradient", "dsgd_lg_sync_step", "dsgd_lg_sync_step_ranges", "dsgd_lg_sync_steps", "dsgd_lg_loss_acc", "dsgd_lg_predict",
    "dsgd_plan_create_lg_n", "dsgd_plan_create_from_seed_lg", "dsgd_lg_loss_acc_ranges",
    "dsgd_lg_sync_steps_ranges",
    "dsgd_plan_create_lg_cs_n", "dsgd_plan_create_from_seed_lg_cs",
    "dsgd_comm_init_lg",
    "dsgd_lg_predict_ranges", "dsgd_lg_loss_acc_list", "dsgd_lg_loss_acc_sampled",
    "dsgd_lg_async_step", "dsgd_lg_update_grad", "dsgd_async_plan_create_lg", "dsgd_async_plan_create_lg_cs", "dsgd_plan_run_async_lg",
    "dsgd_plan_create_from_seed_job_lg", "dsgd_lg_eval_job",
    "dsgd_lg_topics_set", "dsgd_lg_topics_set_weights", "dsgd_lg_topics_get_weights", "dsgd_lg_topics_sync_step", "dsgd_lg_topics_sync_steps",
    "dsgd_lg_topics_loss_acc", "dsgd_lg_topics_predict", "dsgd_lg_topics_count",
]

F_FP64 = 0x1  # dsgd_config.flags: the fp64 mode (include/dsgd.h "THE FP64 MODE")


class Config(C.Structure):
    _fields_ = [
        ("n_features", C.c_int32),
        ("device", C.c_int32),
        ("lambda_", C.c_double),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class BatchStats(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("n_active", C.c_int64)]


class DsgdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("dsgd error %d: %s" % (code, msg))
        self.code = code


class DsgdInvalidArgument(DsgdError, ValueError):
    """DSGD_EINVAL -- what the reference's `require` failures surface as (IllegalArgumentException)."""


class DsgdIndexError(DsgdError, IndexError):
    """DSGD_ERANGE -- IndexOutOfBoundsException on the reference side."""


_lib = None


def load():
    """dlopen libdsgd_hip.so (building it is __graft_entry__.build()'s job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HIP_LIB):
        raise OSError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % HIP_LIB)
    lib = C.CDLL(HIP_LIB)
    lib.dsgd_last_error.restype = C.c_char_p
    lib.dsgd_grad_kernel_name.restype = C.c_char_p
    lib.dsgd_grad_kernel_name.argtypes = [C.c_void_p]
    for name in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.environ.get("DSGD_LIB_PATH"):   # an A/B run against an OLDER build: entry points added since are absent
                continue
            raise
        if name not in ("dsgd_last_error", "dsgd_grad_kernel_name"):
            fn.restype = C.c_int
    if hasattr(lib, "dsgd_comm_init_f64v"):
        lib.dsgd_comm_init_f64v.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]
    for name in ("dsgd_plan_create_from_seed_job", "dsgd_plan_create_from_seed_job_rp64", "dsgd_plan_create_from_seed_job_lg"):
        if hasattr(lib, name):   # (ctx, jstate*, job_len*, n_job, first, n_local, split_begin*, max_samples, batch_size, out*, n_steps*, draws*)
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                           C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("dsgd_loss_acc_list", "dsgd_loss_acc_list_f64"):
        if hasattr(lib, name):   # (ctx, w*, idx*, n, loss*, acc*, counts*)
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("dsgd_loss_acc_sampled", "dsgd_loss_acc_sampled_f64"):
        if hasattr(lib, name):   # (ctx, w*, jstate*, row_begin, row_end, samples_count, loss*, acc*, counts*, idx_out*, n*, draws*)
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "dsgd_async_check"):   # (ctx, row_begin, row_end, loss*, acc*, counts*, updates_window*)
        lib.dsgd_async_check.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.dsgd_async_check_keep.argtypes = [C.c_void_p]
        lib.dsgd_async_check_weights.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(lib, "dsgd_lg_gradient"):   # the logistic model (include/dsgd.h "THE LOGISTIC MODEL")
        lib.dsgd_lg_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.dsgd_lg_sync_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]
        lib.dsgd_lg_sync_step_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]
        lib.dsgd_lg_sync_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p]
        lib.dsgd_lg_loss_acc.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.dsgd_lg_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    if hasattr(lib, "dsgd_plan_create_lg_n"):   # logistic plans and the several-ranges evaluation
        # (ctx, idx*, n_idx, offsets*, n_steps, n_workers, out*)
        lib.dsgd_plan_create_lg_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        # (ctx, jstate*, split_begin*, split_end*, n_splits, max_samples, batch_size, out*, n_steps*, draws*)
        lib.dsgd_plan_create_from_seed_lg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]
        # (ctx, w*, row_begin*, row_end*, n_ranges, loss_out*, acc_out*)
        lib.dsgd_lg_loss_acc_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "dsgd_plan_create_lg_cs_n"):   # logistic plans on column slices: the prototypes of the two above
        lib.dsgd_plan_create_lg_cs_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        lib.dsgd_plan_create_from_seed_lg_cs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
    if hasattr(lib, "dsgd_lg_sync_steps_ranges"):   # (ctx, row_begin*, row_end*, n_workers, n_steps, lr, stats*)
        lib.dsgd_lg_sync_steps_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p]
    if hasattr(lib, "dsgd_comm_init_lg"):
        lib.dsgd_comm_init_lg.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]
    if hasattr(lib, "dsgd_lg_predict_ranges"):   # the logistic model's distributed and sampled evaluation
        # (ctx, w*, row_begin*, row_end*, n_ranges, class_out*, proba_out*, counts_out*, range_loss_out*, loss*, acc*)
        lib.dsgd_lg_predict_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        # (the prototypes of dsgd_loss_acc_list and dsgd_loss_acc_sampled)
        lib.dsgd_lg_loss_acc_list.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.dsgd_lg_loss_acc_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "dsgd_lg_async_step"):   # the logistic model's asynchronous iteration
        # (ctx, idx*, n, lr, delta_out*, stats*)
        lib.dsgd_lg_async_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
        lib.dsgd_lg_update_grad.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]   # (ctx, key*, dv*, nnz)
        for name in ("dsgd_async_plan_create_lg", "dsgd_async_plan_create_lg_cs"):
            # (ctx, assigned_begin*, assigned_end*, n_workers, batch, seed, positional_bug, first_update, n_updates, out*)
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int64, C.c_int64,
                                           C.c_void_p]
        lib.dsgd_plan_run_async_lg.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double]   # (ctx, plan, begin, end, lr)
    if hasattr(lib, "dsgd_lg_eval_job"):   # (ctx, w*, row_begin*, row_end*, n_local, counts_out*, range_loss_out*, loss*, acc*, K_out*)
        lib.dsgd_lg_eval_job.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    if hasattr(lib, "dsgd_lg_topics_set"):   # several topics (include/dsgd.h "SEVERAL TOPICS")
        lib.dsgd_lg_topics_set.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]   # (ctx, T, planes*)
        lib.dsgd_lg_topics_count.argtypes = [C.c_void_p, C.c_void_p]               # (ctx, T_out*)
        lib.dsgd_lg_topics_set_weights.argtypes = [C.c_void_p, C.c_void_p]
        lib.dsgd_lg_topics_get_weights.argtypes = [C.c_void_p, C.c_void_p]
        lib.dsgd_lg_topics_sync_step.argtypes = lib.dsgd_lg_sync_step.argtypes     # (the single model's prototypes)
        lib.dsgd_lg_topics_sync_steps.argtypes = lib.dsgd_lg_sync_steps.argtypes
        lib.dsgd_lg_topics_loss_acc.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]   # (ctx, begin, end, loss*, acc*)
        lib.dsgd_lg_topics_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]               # (ctx, idx*, n, p_out*)
    if hasattr(lib, "dsgd_dense_plan_create"):   # (handles are 64-bit: without argtypes ctypes would pass them as C ints)
        lib.dsgd_dense_step_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float]
        lib.dsgd_dense_loss_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.dsgd_dense_predict.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        lib.dsgd_dense_predict_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.dsgd_dense_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        lib.dsgd_dense_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float]
        lib.dsgd_dense_plan_destroy.argtypes = [C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def check(rc):
    if rc == OK:
        return
    msg = load().dsgd_last_error().decode("utf-8", "replace")
    if rc == EINVAL:
        raise DsgdInvalidArgument(rc, msg)
    if rc == ERANGE:
        raise DsgdIndexError(rc, msg)
    raise DsgdError(rc, msg)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def f32(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if n is not None and a.shape != (n,):
        raise ValueError("expected %d floats, got shape %r" % (n, a.shape))
    return a


def f64(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None and a.shape != (n,):
        raise ValueError("expected %d doubles, got shape %r" % (n, a.shape))
    return a


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)
