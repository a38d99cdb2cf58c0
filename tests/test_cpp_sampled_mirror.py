"""The sampled evaluation of include/dsgd.hpp (Master::localSampledLoss / localSampledAccuracy, SparseSVM::lossAccList /
lossAccSampled; core/Master.scala:109-118) compiled with g++ and driven by tests/cpp/sampled_mirror_test.cpp, the way
tests/test_cpp_host_mirror.py drives its program: CPU checks here, the runs through the device under -m gpu."""

import os
import subprocess

import pytest

from dsgd_amd import _lib
from conftest import ROOT, has_gpu


def build(tmp_path):
    exe = str(tmp_path / "sampled_mirror_test")
    libdir = os.path.dirname(_lib.HIP_LIB)
    _lib.load()  # make sure the library is built
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "sampled_mirror_test.cpp"), "-o", exe, "-L", libdir, "-ldsgd_hip", "-ldsgd_host",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True)
    return exe


def test_cpp_sampled_mirror_compiles_and_passes_its_cpu_checks(tmp_path):
    r = subprocess.run([build(tmp_path), "cpu"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")
def test_cpp_sampled_mirror_equals_the_list_form_on_jrand_lists(tmp_path):
    r = subprocess.run([build(tmp_path), "gpu"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
