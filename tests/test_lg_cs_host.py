"""No GPU needed: the decline rule of the logistic column slices (csrc/dsgd_lg_cs_host.hpp: lg_cs_pick_G) on both sides of every
limit, and the LDS words it counts against the carve the kernel uses -- driven by tests/cpp/lg_cs_host_test.cpp, built with
AddressSanitizer and UBSan and run as a program of its own.  Nothing is loaded into Python under a sanitizer."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_lg_cs_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_cs_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_cs_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_header_is_host_only_and_the_library_uses_it():
    text = open(os.path.join(CSRC, "dsgd_lg_cs_host.hpp")).read()
    assert not re.search(r"\bhip[A-Z_]|__global__|#include\s+<hip", text)
    kernel = open(os.path.join(CSRC, "dsgd_lg_cs.hpp")).read()
    assert '#include "dsgd_lg_cs_host.hpp"' in kernel and "lg_cs_lds(a.dp, G, K)" in kernel
    hip = open(os.path.join(CSRC, "dsgd_hip.hip")).read()
    assert "p->lg ? lg_cs_pick_G(c->dp, K)" in hip                      # the builder asks the rule ...
    calls = open(os.path.join(CSRC, "dsgd_lg_calls.hpp")).read()
    assert "lg_cs_lds(c->dp, G, K).words" in calls                      # ... and the launch asks the carve for its bytes
    # opt-in, no knob: nothing in the switches' header but the plan kind and its code
    route = open(os.path.join(CSRC, "dsgd_route.hpp")).read()
    assert "case PLAN_LG_CS: return 8;" in route and "case PLAN_LG: return 7;" in route and "DSGD_LG" not in route
