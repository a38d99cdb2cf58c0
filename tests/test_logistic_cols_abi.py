"""No GPU needed: dsgd_lg_sync_steps_ranges at the C ABI (include/dsgd.h "WHOLE-SPLIT STEPS BY COLUMN LISTS") -- declared,
exported, bound, version 1 -- failing cleanly without a context, and Engine.lg_sync_steps_ranges turning bad arguments down
in Python before any call into the library."""

import ctypes as C
import os
import re
import types

import pytest

import dsgd_amd
from dsgd_amd import _lib
from conftest import ROOT

NAME = "dsgd_lg_sync_steps_ranges"


def test_symbol_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsgd.h")).read()
    assert NAME in _lib.SYMBOLS and hasattr(lib, NAME)
    assert re.search(r"\bint %s\(dsgd_ctx\* ctx, const int64_t\* row_begin, const int64_t\* row_end, int32_t n_workers, int64_t n_steps, "
                     r"float lr,\s+dsgd_batch_stats\* stats\);" % NAME, header)
    assert getattr(lib, NAME).argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p]
    assert getattr(lib, NAME).restype is C.c_int
    assert lib.dsgd_abi_version() == 1 and "#define DSGD_ABI_VERSION 1" in header
    assert "WHOLE-SPLIT STEPS BY COLUMN LISTS" in header and "dsgd_lg_cgrad_kernel" in header
    assert "no fused or persistent one-launch step" in header
    assert callable(dsgd_amd.Engine.lg_sync_steps_ranges)


def test_a_null_context_is_refused():
    lib = _lib.load()
    z = C.c_int64
    assert lib.dsgd_lg_sync_steps_ranges(None, (z * 1)(0), (z * 1)(4), 1, z(3), 0.5, None) == _lib.EINVAL
    assert b"null context" in lib.dsgd_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


@pytest.mark.parametrize("ranges, n_steps, error", [
    ([], 1, ValueError),                       # no ranges
    ([(0, 4, 8)], 1, ValueError),              # not a pair
    ([(0,)], 1, ValueError),
    ([(0, 4), 7], 1, TypeError),               # not a pair at all
    ([(0.5, 4)], 1, TypeError),                # not a row number
    ([(0, 4)], 0, ValueError),                 # no steps
    ([(0, 4)], -3, ValueError),
    ([(0, 4)], 1.5, TypeError),                # not a count
])
def test_the_engine_rejects_bad_arguments_before_any_call(ranges, n_steps, error):
    stand_in = types.SimpleNamespace(_lib=_NoLibrary(), _ctx=None)
    with pytest.raises(error):
        dsgd_amd.Engine.lg_sync_steps_ranges(stand_in, ranges, n_steps, 0.5)
