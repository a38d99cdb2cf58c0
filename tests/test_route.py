"""No GPU needed: the switches dsgd_create reads and the choice of a kernel family for every entry point (csrc/dsgd_route.hpp).

The header alone (with csrc/dsgd_limits.hpp and csrc/dsgd_layout_types.hpp), compiled with AddressSanitizer and UBSan and run as
a program of its own (tests/cpp/route_test.cpp).  The program asserts every knob's default and clamp, both sides of every
threshold of the row ranges' route, the precedence of the plan and request routes, the slice count over its whole domain,
the column lists' back-off and the lanes per row of the evaluation kernels at their thresholds; it also holds a digest of every function's outputs over a fixed grid to constants recorded from
the lines of csrc/dsgd_hip.hip that the header replaced."""

import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_route_under_sanitizers(tmp_path):
    exe = str(tmp_path / "route_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "route_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
