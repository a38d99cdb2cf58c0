"""No GPU needed: dsgd_lg_softmax_set_il (include/dsgd.h "SOFTMAX, FEW CLASSES") is declared, exported and bound, refuses a null
context without a device, and every kernel of csrc/dsgd_lg_softmax_il.hpp in the shipped code object runs without scratch."""

import ctypes
import os
import re

from dsgd_amd import _lib
from test_abi import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_bound_and_null_refused():
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert re.search(r"^int dsgd_lg_softmax_set_il\(dsgd_ctx\* ctx, int32_t C[^;]*, const uint8_t\* cls[^;]*\);", header, re.M)
    assert "dsgd_lg_softmax_set_il" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.dsgd_lg_softmax_set_il.argtypes == lib.dsgd_lg_softmax_set.argtypes
    cls = (ctypes.c_uint8 * 4)(0, 1, 0, 1)
    assert lib.dsgd_lg_softmax_set_il(None, 2, cls) == lib.dsgd_lg_softmax_set(None, 2, cls) != _lib.OK


def test_every_instantiation_without_scratch_or_spills(tmp_path):
    kn = {k: v for k, v in _kernel_notes(tmp_path).items() if "dsgd_lg_softmax_il_" in k}
    for family in ("grad", "coef", "eval", "predict"):
        for nq in (1, 2, 4, 8):
            assert any("dsgd_lg_softmax_il_%s_kernelILi%dE" % (family, nq) in k for k in kn), (family, nq, sorted(kn))
    for k, v in kn.items():
        assert len(kn) == 16 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
