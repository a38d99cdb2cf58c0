"""No GPU needed: a plan's lists against the rows loaded now (csrc/dsgd_plan_check.hpp), what dsgd_plan_run asks again
after dsgd_load_csr replaced the data under a live plan.

* the header alone (pure host C++) driven by tests/cpp/plan_check_test.cpp, built with AddressSanitizer and UBSan and run as a
  program of its own: lists inside and outside the rows, the empty and one-row edges, the staged sub-batch at, below and above
  its limit, rows that shrink, grow back and grow longer;
* the caller's flat lists of dsgd_sync_steps_f64 and dsgd_plan_create_rp64_n (flat_lists_check): every kind of fault, at the
  first and the last place it can stand;
* the library asks through that header and nowhere else: the constants it restates are tied to the kernel's by a static_assert,
  and every entry point that hands a plan's lists to a kernel re-validates first;
* every kernel of the fp64 row-parallel family, and each of the three that draw an epoch's lists, has ONE launch site in the
  host sources."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _host_sources():
    """The library's host code: dsgd_hip.hip, the fp64 mode's dsgd_fp64_host.hpp and the device-drawn lists' dsgd_seed_host.hpp,
    which it includes."""
    return _read("dsgd_hip.hip") + "\n" + _read("dsgd_fp64_host.hpp") + "\n" + _read("dsgd_seed_host.hpp")


def test_plan_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_check_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "plan_check_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


def test_the_header_is_host_only():
    text = _read("dsgd_plan_check.hpp")
    assert not re.search(r"\bhip[A-Z_]|__global__|__device__|#include\s+<hip", text)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["cstddef", "cstdint"]


def test_the_library_revalidates_where_a_plans_lists_reach_a_kernel():
    hip = _host_sources()
    assert "static_assert(PLAN_STAGE_CAP == PLAN_CAP && PLAN_STAGE_CH == BT_CH" in hip
    # the three run entry points go through plan_run64 or dsgd_plan_run's own body; dsgd_plan_info asks too
    for fn in ("static int plan_run64(", "int dsgd_plan_run(", "int dsgd_plan_info("):
        body = hip[hip.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "plan_revalidate(c, p)" in body, fn
        if fn != "int dsgd_plan_info(":   # ... before the layout is prepared or anything else is enqueued
            assert body.index("plan_revalidate(c, p)") < body.index("prepare_layout(c)"), fn
    for fn in ("int dsgd_plan_run_f64(", "int dsgd_plan_run_async_f64("):
        body = hip[hip.index(fn):]
        assert "plan_run64(c, p" in body[:body.index("\n}\n")], fn
    # every successful load bumps the counter the plans are compared with
    load = hip[hip.index("static int load_csr_impl("):]
    load = load[:load.index("\n}\n")]
    assert "++c->load_gen;" in load and "++c->layout_gen;" in load


def test_every_kernel_of_the_fp64_row_parallel_family_has_one_launch_site():
    names = set(re.findall(r"__global__[^;{]*?\b(dsgd_rp64\w*)\s*\(", _read("dsgd_rp64.hpp")))
    assert len(names) >= 16 and {"dsgd_rp64_grad_kernel", "dsgd_rp64v_finish_kernel", "dsgd_rp64_header_plan_kernel",
                                 "dsgd_rp64v_s_sliced_kernel", "dsgd_rp64v_step_kernel"} <= names
    launched = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)", _host_sources())
    for name in sorted(names):
        assert launched.count(name) == 1, (name, launched.count(name))


def test_every_kernel_of_the_device_drawn_lists_has_one_launch_site():
    names = set(re.findall(r"__global__[^;{]*?\b(dsgd_jr_\w*)\s*\(", _read("dsgd_shuffle.hpp")))
    assert names == {"dsgd_jr_scan_kernel", "dsgd_jr_slice_kernel", "dsgd_jr_slice_job_kernel"}
    launched = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)", _host_sources())
    for name in sorted(names):
        assert launched.count(name) == 1, (name, launched.count(name))
    assert _read("dsgd_hip.hip").count('#include "dsgd_seed_host.hpp"') == 1
