"""No GPU needed: dsgd_lg_topics_sync_steps_cols and dsgd_lg_softmax_sync_steps_cols (include/dsgd.h "INDEX LISTS BY COLUMN LISTS")
are declared, exported and bound, refuse a null context without a device, and every kernel of csrc/dsgd_lg_lists_cols.hpp in the
shipped code object runs without scratch."""

import ctypes
import os
import re

import pytest

from dsgd_amd import _lib
from test_abi import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("model", ["topics", "softmax"])
def test_declared_exported_bound_and_null_refused(model):
    name = "dsgd_lg_%s_sync_steps_cols" % model
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert re.search(r"^int %s\(dsgd_ctx\* ctx, const int32_t\* idx, int64_t n_idx, const int64_t\* offsets[^;]*float lr, dsgd_batch_stats\* stats\);" % name,
                     header, re.M)
    assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert getattr(lib, name).argtypes == lib.dsgd_lg_sync_steps.argtypes
    idx, offsets = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int64 * 2)(0, 2)
    assert getattr(lib, name)(None, idx, 2, offsets, 1, 1, 0.5, None) == getattr(lib, name[:-5])(None, idx, 2, offsets, 1, 1, 0.5, None) != _lib.OK


def test_every_instantiation_without_scratch_or_spills(tmp_path):
    kn = {k: v for k, v in _kernel_notes(tmp_path).items() if "dsgd_lgl_" in k}
    want = (["dsgd_lgl_mark_kernel", "dsgd_lgl_clear_kernel"] + ["dsgd_lgl_%s_kernelILi%dE" % (f, gw) for f in ("cgrad", "topics_coef", "smax_coef") for gw in (16, 32, 64)]
            + ["dsgd_lgl_smax_few_coef_kernelILi%dE" % nq for nq in (1, 2, 4, 8)])
    for w in want:
        assert any(w in k for k in kn), (w, sorted(kn))
    for k, v in kn.items():
        assert len(kn) == len(want) and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
