"""A context gives back what it took (-m gpu).  The tests' seam build of the library counts, inside the two allocation pairs
of csrc/dsgd_buf.hpp, the device and pinned bytes it holds (dsgd_test_live_bytes; the product build has neither the counter
nor the export); tests/ctx_lifetime_worker.py records them before dsgd_create and after dsgd_destroy.  The difference is a
condition, not a measurement: 0 bytes.  (Counted inside the library: the card's free memory moves with other people's
work.)

One context per cycle -- fp32, fp64 on float values, fp64 on Double values -- on 3,000 synthetic rows of 2,000 features, the
hot / cold split at rank 512 and the families' thresholds lowered so that the row-wise kernel, the column lists and the row
chunks each take one of the range steps.  Between create and destroy every owner is exercised once: the data loaded twice,
dimSparsity, dense and Sparse weights, gradients, an index-list step of 2 workers, range steps, plans from lists (column
slices, virtual tiles) and from a seed, forward and loss, an asynchronous step, a peer's update, a traced Hogwild run and a
start / stop; on fp64 the row-parallel family (gradient, a step, an epoch's steps on the two-launch queue).  The last plan is
never destroyed: it is alive at dsgd_destroy, which gives its blocks back through the context's cache and deletes it; on fp32
it keeps a record (dsgd_plan_record on, a step, off, on again) and holds the record's blocks then.  A context whose plans'
column slices the host lays out (DSGD_CS_HOST_LAYOUT=1: blocks outside the cache; built, run, rebuilt over the freed ones
after a second load, alive at dsgd_destroy), a context that only loads data and has one call refused, and the dense engine
(4,096 x 512: the narrowest it accepts), are cycles of their own."""

import json
import os
import subprocess
import sys

import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

HERE = os.path.dirname(os.path.abspath(__file__))
CYCLES = ("fp32", "host_layout", "fp64_float", "fp64_double", "failure_path", "dense")


@pytest.fixture(scope="module")
def cycles():
    from test_rccl_stub import seam_env

    env = seam_env()
    env.update(DSGD_HSPLIT="512", DSGD_TCOL="1", DSGD_TCOL_MIN="512", DSGD_TCOL_MAX="2000", DSGD_FSTEP_MIN="2048")
    for k in ("DSGD_RP64_FUSED", "DSGD_STREAM_MIN", "DSGD_FSTEP", "DSGD_FSTEP_MAX", "DSGD_FSTEP_ROWS", "DSGD_TCOL_MAX_NNZ"):
        env.pop(k, None)
    proc = subprocess.run([sys.executable, os.path.join(HERE, "ctx_lifetime_worker.py")], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300)
    print(proc.stdout)
    assert proc.returncode == 0 and "CTX_LIFETIME_DONE" in proc.stdout, proc.stdout
    out = {}
    for line in proc.stdout.splitlines():
        if line.startswith("CYCLE "):
            c = json.loads(line[6:])
            out[c["name"]] = c
    assert sorted(out) == sorted(CYCLES)
    return out


@pytest.mark.parametrize("name", CYCLES)
def test_every_byte_comes_back(cycles, name):
    c = cycles[name]
    dev0, pin0 = c["before"]
    assert c["during"][0] > dev0, "the counter saw no device allocation: %r" % (c,)
    assert c["during"][1] > pin0, "the counter saw no pinned allocation: %r" % (c,)
    assert c["after"] == c["before"], "%s: %d device and %d pinned bytes did not come back" % (
        name, c["after"][0] - dev0, c["after"][1] - pin0)


def test_the_cycles_took_the_paths_they_are_meant_to(cycles):
    k = cycles["fp32"]["kernels"]
    assert k["column_lists"] == "dsgd_tc_grad_kernel" and k["row_chunks"] == "dsgd_fstep_kernel", k
    assert k["row_wise"] not in (k["column_lists"], k["row_chunks"]), k
    assert k["plan"] == "column_slices" and k["big_plan"] == "virtual_tiles", k
    assert k["alive_plan"] == "column_slices" and k["alive_record_words"] > 0, k
    h = cycles["host_layout"]
    assert h["kinds"] == ["column_slices", "column_slices"] and h["device_built"] == [False, False], h
    assert cycles["fp64_float"]["kernels"]["plan"] == "column_slices_fp64"
    assert cycles["failure_path"]["refused"]
