"""No GPU needed: the host arithmetic behind dsgd_lg_predict_ranges -- lg_pred_table and lg_pred_owner of
csrc/dsgd_lg_host.hpp (a single range's workgroups are lg_eval_blocks of its rows; the runs are contiguous; an empty range gets
no workgroup and no output; 256 ranges are served and 257 refused; reversed and overlapping ranges, rows outside the data and a
call without rows are refused; the bisection over first_block finds the owner of every workgroup of a few dozen tables) --
driven by tests/cpp/lg_eval_host_test.cpp, built with AddressSanitizer and UBSan and run as a program of its own.  Nothing is
loaded into Python under a sanitizer."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_lg_eval_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_eval_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_eval_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_library_uses_the_table_and_checks_first():
    calls = open(os.path.join(CSRC, "dsgd_lg_calls.hpp")).read()
    ranges = calls.split("\nint dsgd_lg_predict_ranges(")[1].split("\nstatic int lg_eval_list_run(")[0]
    for fn in ("lg_enter(", "lg_pred_table(", "lg_finish_blocks(", "dsgd_lg_predict_ranges_kernel", "lg_pred_lds_floats("):
        assert fn in ranges, fn
    # every refusal comes before the weights of the call replace the resident ones, and before anything is enqueued
    assert ranges.index("lg_enter(") < ranges.index("lg_pred_table(") < ranges.index("lg_report(") < ranges.index("set_weights_locked(")
    assert ranges.index("set_weights_locked(") < ranges.index("hipLaunchKernelGGL")
    lst = calls.split("\nint dsgd_lg_loss_acc_list(")[1].split("\nint dsgd_lg_loss_acc_sampled(")[0]
    assert lst.index("lg_enter(") < lst.index("lg_check_lists(") < lst.index("lg_report(") < lst.index("set_weights_locked(") < lst.index("send_idx(")
    smp = calls.split("\nint dsgd_lg_loss_acc_sampled(")[1]
    assert smp.index("lg_enter(") < smp.index("lg_report(") < smp.index("JR_MAX_LEN") < smp.index("sampled_draw(") < smp.index("set_weights_locked(") < smp.index("*jstate = ")
    # the draw is the SVM call's, as it stands: declared here, defined once, in dsgd_hip.hip
    hip = open(os.path.join(CSRC, "dsgd_hip.hip")).read()
    assert len(re.findall(r"\nstatic int sampled_draw\([^)]*\) \{", hip)) == 1 and not re.search(r"\nstatic int sampled_draw\([^)]*\) \{", calls)
    kernels = open(os.path.join(CSRC, "dsgd_lg_eval.hpp")).read()
    # both kernels are the single model's ONE evaluation body, which holds the dot, the tree and the pragma
    for name in ("dsgd_lg_predict_ranges_kernel", "dsgd_lg_eval_list_kernel"):
        body = kernels.split("%s(" % name)[-1].split("\n}\n")[0]
        assert "lg_eval_walk(m, w, hw, " in body, name
    walk = open(os.path.join(CSRC, "dsgd_logistic.hpp")).read().split("void lg_eval_walk(")[1].split("\n}\n")[0]
    assert "row_dot<LG_GROUP, LG_UNR, true>" in walk and "lg_block_sum(" in walk and "#pragma clang fp contract(off)" in walk
    assert "lg_pred_owner(l_tab" in kernels
    assert hip.index('#include "dsgd_logistic.hpp"') < hip.index('#include "dsgd_lg_eval.hpp"')
