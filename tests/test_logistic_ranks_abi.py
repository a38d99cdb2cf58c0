"""CPU-side checks of the logistic model across ranks (include/dsgd.h "THE LOGISTIC MODEL", ACROSS RANKS;
csrc/dsgd_lg_gather.hpp): dsgd_comm_init_lg is declared, exported, listed and bound and refuses a null context without a
device; the header says what spans the ranks and what does not; the new kernel instantiations are in the code object
without spills or scratch beside the single-context ones; and the layout helpers and the agreement's judgement hold in a
stand-alone host program (tests/cpp/lg_gather_test.cpp) under the address and undefined-behaviour sanitizers."""

import ctypes as C
import os
import re
import subprocess

import dsgd_amd
from dsgd_amd import _lib
from test_abi import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "dsgd.h")).read()


def test_comm_init_lg_declared_exported_and_bound():
    assert re.search(r"\bint\s+dsgd_comm_init_lg\s*\(\s*dsgd_ctx\*\s*\w+,\s*const char\*\s*\w+,\s*int32_t\s+\w+,\s*int32_t\s+\w+\)\s*;", HEADER)
    lib = _lib.load()
    assert "dsgd_comm_init_lg" in _lib.SYMBOLS and hasattr(lib, "dsgd_comm_init_lg")
    assert callable(getattr(dsgd_amd.Engine, "comm_init_lg"))
    uid = b"\0" * _lib.UNIQUE_ID_BYTES
    assert lib.dsgd_comm_init_lg(None, C.c_char_p(uid), C.c_int32(1), C.c_int32(0)) == _lib.EINVAL   # null context
    assert b"null" in lib.dsgd_last_error()
    assert lib.dsgd_comm_init_lg(None, None, C.c_int32(0), C.c_int32(-1)) == _lib.EINVAL             # ... whatever else is wrong


def test_the_header_says_what_spans_the_ranks_and_what_does_not():
    lg = HEADER[HEADER.index("THE LOGISTIC MODEL on the resident CSR rows"):]
    across = lg[lg.index(" * ACROSS RANKS (dsgd_comm_init_lg"):lg.index(" * LIMITS (out of scope")]
    for name in ("dsgd_lg_sync_step,", "dsgd_lg_sync_step_ranges", "dsgd_lg_sync_steps_ranges", "dsgd_lg_sync_steps ", "dsgd_plan_create_lg_n"):
        assert name in across, name
    local = across[across.index("   local "):across.index("   refused ")]
    for name in ("dsgd_lg_gradient", "dsgd_lg_predict", "dsgd_lg_loss_acc", "dsgd_lg_loss_acc_ranges"):
        assert name in local, name
    refused = across[across.index("   refused "):across.index("   errors ")]
    for name in ("dsgd_plan_create_from_seed_lg", "dsgd_plan_create_lg_cs_n", "dsgd_plan_create_from_seed_lg_cs", "dsgd_comm_init_all"):
        assert name in refused, name
    limits = lg[lg.index(" * LIMITS (out of scope"):lg.index(" * dsgd_lg_gradient: one worker's")]
    assert "no communicators" not in limits     # (it shrank by what is built)
    for still_out in ("no JNI", "host.LogisticSync", "no device-drawn lists", "no column slices", "no asynchronous engine"):
        assert still_out in limits, still_out


def test_gathered_finish_and_header_kernel_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    finish = {k: v for k, v in notes.items() if "dsgd_lg_finish_kernel" in k}
    assert len(finish) == 3, sorted(finish)       # gradient, step, and the step gathered over the ranks
    header = {k: v for k, v in notes.items() if "dsgd_lg_header_kernel" in k}
    assert len(header) == 1, sorted(header)
    # the gradient kernels are the single context's: the slots' base and vexp are arguments, not instantiations
    for name in ("dsgd_lg_grad_kernel", "dsgd_lg_grad_range_kernel", "dsgd_lg_coef_kernel", "dsgd_lg_cgrad_kernel"):
        assert sum(name in k for k in notes) == 1, name
    for k, v in {**finish, **header}.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    assert all(v["group_segment_fixed_size"] == 0 for v in header.values())


def test_gather_layout_and_agreement_in_a_sanitized_host_program(tmp_path):
    exe = str(tmp_path / "lg_gather_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_gather_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
