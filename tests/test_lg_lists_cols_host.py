"""No GPU needed: csrc/dsgd_lg_lists_cols_host.hpp through tests/cpp/lg_lists_cols_host_test.cpp, a program of its own under ASan and UBSan."""

import os
import subprocess

from conftest import ROOT


def test_lg_lists_cols_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_lists_cols_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "distributed-sgd_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lg_lists_cols_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stderr, r.stderr
