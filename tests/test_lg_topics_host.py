"""No GPU needed: the host header of the logistic model over several topics (csrc/dsgd_lg_topics_host.hpp) -- hostile arguments,
plane validation, the sizing at T = 1 .. 8 and the word order of the host's sums -- driven by tests/cpp/lg_topics_host_test.cpp,
built with AddressSanitizer and UBSan and run as a program of its own.  Nothing is loaded into Python under a sanitizer."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_lg_topics_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_topics_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_topics_host_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_header_is_host_only_and_the_calls_use_it():
    text = open(os.path.join(CSRC, "dsgd_lg_topics_host.hpp")).read()
    assert not re.search(r"\bhip[A-Z_]|__global__|#include\s+<hip", text)
    calls = open(os.path.join(CSRC, "dsgd_lg_topics_calls.hpp")).read()
    for fn in ("lgt_check_set(", "lgt_check_step(", "lgt_check_steps(", "lgt_check_range(", "lgt_check_list(", "lgt_hot(", "lgt_w_stride(",
               "lgt_acc_stride(", "lgt_acc_words(", "lgt_eval_hw(", "lgt_eval_lds_floats(", "lgt_part_words(", "lgt_fold("):
        assert fn in calls, fn
    # every stepping, evaluating or predicting entry point checks before anything of the call is enqueued
    for body in re.split(r"\nint dsgd_lg_topics_", calls)[1:]:
        name = body.split("(")[0]
        if name in ("sync_step", "sync_steps", "loss_acc", "predict"):
            first_launch = min(body.index(w) for w in ("hipLaunchKernelGGL", "lgt_launch(", "hipMemcpyAsync", "hipMemsetAsync") if w in body)
            assert body.index("lg_report(") < first_launch, name
            # ... and before the topics may be dropped for a new column ranking: a call refused for its arguments changes nothing
            assert body.index("lgt_enter(") < body.index("lg_report(") < body.index("lgt_ready(") < first_launch, name
    enter = calls.split("static int lgt_enter(")[1].split("\n}\n")[0]
    assert "lgt_drop(" not in enter and "prepare_layout(" not in enter
    kernels = open(os.path.join(CSRC, "dsgd_lg_topics.hpp")).read()
    assert "static_assert(LGT_HOT_WORDS == LG_HOT" in kernels and "static_assert(LGT_LDS_FLOATS == DSGD_LDS_FLOATS" in kernels
