"""No GPU needed: the host arithmetic of the logistic column lists (csrc/dsgd_lg_cols_host.hpp) -- the share size rule on both
sides of its clamps, the padding to whole shares, the workers' position bases for K = 1, K = 16 and one row, and the decision
to decline at 2^31 positions or entries -- driven by tests/cpp/lg_cols_host_test.cpp, built with AddressSanitizer and UBSan and
run as a program of its own.  Nothing is loaded into Python under a sanitizer."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_lg_cols_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_cols_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_cols_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_header_is_host_only_and_the_library_uses_it():
    text = open(os.path.join(CSRC, "dsgd_lg_cols_host.hpp")).read()
    assert not re.search(r"\bhip[A-Z_]|__global__|#include\s+<hip", text)
    calls = open(os.path.join(CSRC, "dsgd_lg_calls.hpp")).read()
    body = calls.split("\nint dsgd_lg_sync_steps_ranges(")[1].split("\nint dsgd_lg_")[0]
    # the checks, in the single step's order, before the layout is prepared or anything is enqueued
    order = [body.index(s) for s in ("lg_enter(", "lg_check_ranges(", "lg_report(", "n_steps < 1", "prepare_layout(c)", "lg_ensure(", "lgc_layout(",
                                     "lgc_launch(", "lg_launch(c, false,", "lg_step_done(")]
    assert order == sorted(order)
    assert "lgc_plan(" in calls and "lg_launch_finish(" in calls
    kernels = open(os.path.join(CSRC, "dsgd_lg_cols.hpp")).read()
    assert '#include "dsgd_lg_cols_host.hpp"' in kernels and "LGC_MAX_SHARE" in kernels
    assert "row_dot<LG_GROUP, LG_UNR, false>" in kernels and "__double2ll_rn((double)" in kernels
    # no new knob: nothing but the entry point selects the path
    assert "lgc" not in open(os.path.join(CSRC, "dsgd_route.hpp")).read().lower()
