"""No GPU needed: the logistic model's host header (csrc/dsgd_lg_host.hpp) -- the shift for n = 1, 2, 2^k +- 1, the grids, and
every refusal of the list, range and offset validation -- driven by tests/cpp/lg_host_test.cpp, built with AddressSanitizer
and UBSan and run as a program of its own.  Nothing is loaded into Python under a sanitizer."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_lg_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_header_is_host_only_and_the_library_uses_it():
    text = open(os.path.join(CSRC, "dsgd_lg_host.hpp")).read()
    assert not re.search(r"\bhip[A-Z_]|__global__|#include\s+<hip", text)
    calls = open(os.path.join(CSRC, "dsgd_lg_calls.hpp")).read()
    for fn in ("lg_check_lists(", "lg_check_ranges(", "lg_check_flat(", "lg_blocks_per_worker(", "lg_finish_blocks(", "lg_eval_blocks("):
        assert fn in calls, fn
    # every entry point checks before the layout is prepared or anything else of the call is enqueued
    for body in re.split(r"\nint dsgd_lg_", calls)[1:]:
        assert body.index("lg_report(") < body.index("prepare_layout(c)"), body[:40]
    assert "lg_shift(" in open(os.path.join(CSRC, "dsgd_logistic.hpp")).read()
