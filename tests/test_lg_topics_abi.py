"""No GPU needed: the boundary of the logistic model over several topics -- the exports, the header's words, the binding, the
refusals that need no device, and the new kernels in the gfx950 code object without scratch."""

import ctypes as C
import inspect
import os

import numpy as np

import dsgd_amd
from dsgd_amd import _lib, host
from conftest import ROOT
from test_abi import _kernel_notes

HEADER = open(os.path.join(ROOT, "include", "dsgd.h")).read()
NAMES = ["dsgd_lg_topics_set", "dsgd_lg_topics_set_weights", "dsgd_lg_topics_get_weights", "dsgd_lg_topics_sync_step",
         "dsgd_lg_topics_sync_steps", "dsgd_lg_topics_loss_acc", "dsgd_lg_topics_predict", "dsgd_lg_topics_count"]


def test_exports_header_and_binding():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and name + "(dsgd_ctx* ctx" in HEADER, name
    assert lib.dsgd_abi_version() == 1
    assert lib.dsgd_lg_topics_set.argtypes[1] is C.c_int32
    assert lib.dsgd_lg_topics_sync_step.argtypes == lib.dsgd_lg_sync_step.argtypes
    assert lib.dsgd_lg_topics_sync_steps.argtypes == lib.dsgd_lg_sync_steps.argtypes
    lg = HEADER[HEADER.index("THE LOGISTIC MODEL on the resident CSR rows"):]
    sec = lg[lg.index(" * SEVERAL TOPICS ("):lg.index(" * LIMITS (out of scope")]
    for words in ("THE CONTRACT", "BITS", "label = plane t", "TWO launches whatever T", "LG_TOPICS_MAX", "T = 0 drops the topics", "start at zero",
                  "DSGD_EINVAL", "DSGD_ERANGE", "DSGD_EUNSUPPORTED", "DSGD_ESTATE", "ANY", "dsgd_load_csr", "touch neither"):
        assert words in sec, words
    limits = lg[lg.index(" * LIMITS (out of scope"):lg.index(" * dsgd_lg_gradient: one worker's")]
    for out in ("no plans", "row ranges or column lists", "no column slices", "no ranks", "no asynchronous iteration", "one lambda and one lr", "no JNI"):
        assert out in limits, out
    for fn in ("lg_topics_set", "lg_topics_set_weights", "lg_topics_get_weights", "lg_topics_sync_step", "lg_topics_sync_steps", "lg_topics_loss_acc",
               "lg_topics_predict"):
        assert callable(getattr(dsgd_amd.Engine, fn)), fn
    assert list(inspect.signature(host.LogisticTopics.fit).parameters)[1:] == list(inspect.signature(host.LogisticSync.fit).parameters)[1:]
    assert dsgd_amd.Engine.lg_topics_max == 8


def test_refusals_that_need_no_device():
    lib = _lib.load()
    p = np.ones(4, dtype=np.int8)
    w = np.zeros(4, dtype=np.float32)
    one = (C.c_void_p * 1)(None)
    n1 = (C.c_int64 * 1)(0)
    assert lib.dsgd_lg_topics_set(None, 1, _lib.ptr(p)) == _lib.EINVAL and b"null context" in lib.dsgd_last_error()
    assert lib.dsgd_lg_topics_set_weights(None, _lib.ptr(w)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_count(None, C.byref(C.c_int32(0))) == _lib.EINVAL
    assert lib.dsgd_lg_topics_get_weights(None, _lib.ptr(w)) == _lib.EINVAL
    assert lib.dsgd_lg_topics_sync_step(None, one, n1, 1, C.c_float(0.5), None) == _lib.EINVAL
    assert lib.dsgd_lg_topics_sync_steps(None, None, 0, None, 0, 0, C.c_float(0.5), None) == _lib.EINVAL
    assert lib.dsgd_lg_topics_loss_acc(None, 0, 1, None, None) == _lib.EINVAL
    assert lib.dsgd_lg_topics_predict(None, None, 0, None) == _lib.EINVAL


def test_the_new_kernels_are_in_the_code_object_without_scratch(tmp_path):
    notes = _kernel_notes(tmp_path)
    for name in ("dsgd_lg_topics_grad_kernel", "dsgd_lg_topics_finish_kernel", "dsgd_lg_nsq_kernel", "dsgd_lg_topics_eval_kernel",
                 "dsgd_lg_topics_predict_kernel"):
        kn = {k: v for k, v in notes.items() if name in k}
        assert len(kn) == 1, (name, sorted(kn))
        v = next(iter(kn.values()))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
    grad = next(v for k, v in notes.items() if "dsgd_lg_topics_grad_kernel" in k)
    single = next(v for k, v in notes.items() if "dsgd_lg_grad_kernel" in k)
    assert grad["group_segment_fixed_size"] == single["group_segment_fixed_size"] == 16384     # the LDS head does not grow with T
    assert -(-grad["vgpr_count"] // 8) * 8 <= 80                                               # six waves per SIMD, as the single model's
    ev = next(v for k, v in notes.items() if "dsgd_lg_topics_eval_kernel" in k)
    assert ev["vgpr_count"] <= 128                                                             # a 1024-lane workgroup: four waves per SIMD
