"""Master::predict / distributedLoss / distributedAccuracy of include/dsgd.hpp (core/Master.scala:61-98 over
dsgd_predict_ranges), compiled with g++ and driven by tests/cpp/predict_mirror_test.cpp: the argument checks here, the
comparison with dsgd_loss_acc at w = 0 and after a few steps through the device under -m gpu."""

import os
import subprocess

import pytest

from dsgd_amd import _lib
from conftest import ROOT, has_gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("predict_cpp") / "predict_mirror_test")
    libdir = os.path.dirname(_lib.HIP_LIB)
    _lib.load()  # make sure the library is built
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "predict_mirror_test.cpp"), "-o", out, "-L", libdir, "-ldsgd_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    return out


def test_cpp_predict_mirror_compiles_and_passes_its_cpu_checks(exe):
    r = subprocess.run([exe, "cpu"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")
def test_cpp_distributed_loss_and_accuracy_equal_loss_acc(exe):
    r = subprocess.run([exe, "gpu"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stderr
