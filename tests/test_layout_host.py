"""No GPU needed: the host's arithmetic behind every table the gradient kernels read (csrc/dsgd_layout_host.hpp) -- wave tiles and
lane descriptors, the split streams' offsets, tile ranges, row chunks, virtual tiles, fixed-point shifts.

The header alone (with csrc/dsgd_layout_types.hpp), compiled with AddressSanitizer and UBSan and run as a program of its own
(tests/cpp/layout_host_test.cpp).  The program decodes every table with a decoder written from the records' comments and holds
the result to the inputs, on the smallest shapes at which the builders can go wrong; its input vectors are exactly as long as
the builders may read.  It also holds a digest of every table's bytes to constants recorded from the parent of the commit that
moved this arithmetic out of csrc/dsgd_hip.hip."""

import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_layout_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "layout_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "layout_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
