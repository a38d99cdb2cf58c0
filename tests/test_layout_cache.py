"""No GPU needed: the cache of device layouts per row-range configuration (csrc/dsgd_layout_cache.hpp: LayoutCache), which the row
chunks, the SVM's column lists and the logistic model's share.

The header alone, compiled behind csrc/dsgd_buf.hpp against stand-ins for the HIP allocation calls (tests/cpp/layout_cache_test.cpp)
with AddressSanitizer and UBSan, run as a program of its own.  The payload owns a DevBuf, so a lost or twice-released layout is a
sanitizer finding.  The program checks the rules by name: a hit restamps, the ninth insert evicts the least recently used entry,
entries of another generation go first, the idle hook runs once per make-room that erases anything and never otherwise, declined
entries are entries, n_wg is part of the key, the size stays within eight over 100 scripted operations, clear and destruction
release everything, and a pointer from find survives further finds."""

import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_layout_cache_under_sanitizers(tmp_path):
    exe = str(tmp_path / "layout_cache_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "layout_cache_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
