"""No GPU needed: the owners of device and pinned memory (csrc/dsgd_buf.hpp).

* the helper alone, compiled against a stand-in for the HIP calls it uses (tests/cpp/buf_test.cpp) with AddressSanitizer and
  UBSan, run as a program of its own: moves, growth, failed allocations, release exactly once;
* the single choke point: each of the four HIP allocation calls occurs exactly once in the sources under csrc/ -- everything
  else allocates through the two function pairs of that header."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_buf_helper_under_sanitizers(tmp_path):
    exe = str(tmp_path / "buf_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "buf_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_every_allocation_goes_through_one_place():
    text = ""
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), errors="replace") as f:
            text += f.read()
    for call in ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"):
        n = len(re.findall(r"\b%s\(" % call, text))
        assert n == 1, "%s( occurs %d times under csrc/ (once: in dsgd_buf.hpp)" % (call, n)
