"""No GPU needed: the host arithmetic of dsgd_lg_eval_job (csrc/dsgd_lg_eval_job.hpp) -- the gather record's offsets (lge_words,
lge_at: K = 1, 2, 12, 13, 255, 256; disjoint blocks, padded to 64, a rank's positions exactly r k .. r k + k - 1) and the fold
(lge_fold: position order, with dsgd_lg_predict_ranges' expressions; not a rank-minor order, not a pairwise tree; a writer count
of 0 or 2 reported, nothing written) -- driven by tests/cpp/lg_eval_job_test.cpp, built with AddressSanitizer and UBSan and run
as a program of its own.  Nothing is loaded into Python under a sanitizer."""

import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_lg_eval_job_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lg_eval_job_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lg_eval_job_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_library_checks_agrees_launches_gathers_and_folds_in_that_order():
    calls = open(os.path.join(CSRC, "dsgd_lg_calls.hpp")).read()
    body = calls.split("\nint dsgd_lg_eval_job(")[1].split("\nstatic int lg_eval_list_run(")[0]
    order = ["lg_enter(", "LG_PRED_MAX_RANGES / world", "lg_pred_table(", "lg_report(", "lg_agree(", "set_weights_locked(", "dsgd_lg_predict_ranges_kernel",
             "dsgd_lg_eval_fold_kernel", "rccl::AllReduce(", "read_scalars(", "lge_fold("]
    at = [body.index(s) for s in order]
    assert at == sorted(at), list(zip(order, at))
    assert body.count("rccl::AllReduce(") == 1 and "lge_drop(c)" in body     # ONE collective behind the agreement; its failure drops the record
    assert "a.cls = nullptr" in body and "a.proba = nullptr" in body        # no classes, no probabilities
    assert "d_lg_acc" not in body                                          # the record lives in a buffer of its own
    kernel = open(os.path.join(CSRC, "dsgd_lg_eval_job.hpp")).read().split("dsgd_lg_eval_fold_kernel(LgeArgs a)")[1]
    assert "#pragma clang fp contract(off)" in kernel and "ls = ls + a.loss_part[b]" in kernel and "atomic" not in kernel
    # the job form of the device-drawn lists: dsgd_plan_create_from_seed_job's path, the scope of dsgd_plan_create_lg_n
    job = calls.split("\nint dsgd_plan_create_from_seed_job_lg(")[1].split("\n}\n")[0]
    assert "plan_from_seed_job(" in job
    seed = open(os.path.join(CSRC, "dsgd_seed_host.hpp")).read()
    assert "job ? LG_SPANS : LG_ONE_PROCESS" in seed
