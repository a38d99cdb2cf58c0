"""The packed form of the row-chunk kernel on the window edges of its register arithmetic (-m gpu; csrc/dsgd_kernels.hpp
w_tile_q<..., true>: the flag squeeze, the end mark in lane n >> 3, the DPP prefix sum and its wave total, the drop of up to seven
starts in front of a tile's first row).  The matrices are built by construction (tests/packed_edge_data.py), and
tests/test_packed_edges.py shows on the CPU -- with the project's own cut, at the DSGD_FSTEP_ROWS values and row ranges used
here -- that they produce every edge: end marks on an 8-slot boundary, the largest tile (511 slots: the end mark in lane 63, bit
7), every count 1..7 of dropped starts, tiles of fewer than 8 slots, more than 64 rows and the 254-row cap, the stream's last
tile with and without a whole last word, chunks with fewer tiles than waves and with none (also as a launch's first chunk), rows
that start in a lane's slot 7 or span more than eight lanes, long rows, empty rows and cold-only rows between tiled ones.

For every matrix and DSGD_FSTEP_ROWS value: the device's hot set is the one the witness cut by; the packed form equals the
plain form bit for bit over three steps from non-zero weights (tests/test_gpu_fstep_packed.py: packed_equals_plain); the packed
form holds the fp64 oracle's derived per-coordinate bound (oracle/bounds.py through ranged_step).  The same two comparisons with
all labels -1, all +1 and alternating; and one warm context that changes the gradient family at every step -- packed chunks,
the three streaming launches, the row-wise kernel, column lists -- against fresh contexts, bit for bit: coef8 (0 / 1 in the
packed form, 0 / +-1 elsewhere) and dcold (label-folded in the packed form) are buffers of the context that every family
writes in its own convention."""

import numpy as np
import pytest

import dsgd_amd
import packed_edge_data as pe
from conftest import has_gpu
from test_gpu_fstep import FSTEP, some_weights
from test_gpu_fstep_packed import LAM, _row_chunks_from_4096_rows, packed_equals_plain, steps  # noqa: F401  (the fixture: autouse here too)
from test_gpu_parity import make_pair, ranged_step

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

MATRICES = ("phases", "ragged")


@pytest.fixture(autouse=True)
def _chunks_from_256_rows_on_the_witness_split(monkeypatch, _row_chunks_from_4096_rows):
    monkeypatch.setenv("DSGD_FSTEP_MIN", "256")            # (the smallest step here: three ranges of `ragged`)
    monkeypatch.setenv("DSGD_HSPLIT", str(pe.HOT_N))


def weights_for(seed):
    return some_weights(pe.DIM, seed, n=pe.DIM // 2, scale=0.5)


def assert_split(eng, data):
    """the hot stream holds exactly the keys the witness took for hot -- a mismatch is a failure of the test's premise"""
    hot = pe.hot_mask(data)
    assert eng.tuning_info()["hsplit"] == pe.HOT_N
    ranks = eng.column_ranks()
    assert (ranks[hot] < pe.HOT_N).all() and (ranks[~hot] >= pe.HOT_N).all()


def three_steps(name):
    rg = pe.ranges_of(name)
    return [rg["one"], rg["three"], rg.get("from_long", rg["one"])]


def against_the_oracle(data, name, seed):
    o, eng = make_pair(data, LAM, data.n_rows)
    with eng:
        assert_split(eng, data)
        eng.set_weights(weights_for(seed))
        for ranges in three_steps(name) + [pe.ranges_of(name)["one"]]:
            rows = sum(b - a for a, b in ranges)
            ranged_step(o, eng, ranges, 0.5 * 100 / rows * len(ranges))
            assert eng.grad_kernel_name() == FSTEP and eng.tuning_info()["stream_mode"] == 5


@pytest.mark.parametrize("name", MATRICES)
def test_split_as_the_witness_assumed(name):
    data = pe.matrix(name)
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(data.n_rows)
        assert_split(eng, data)
        assert eng.tuning_info()["cold_packed"] == 1   # (16-bit cold ids: what the chunked launch needs)


@pytest.mark.parametrize("rows_per_chunk", pe.FSTEP_ROWS)
@pytest.mark.parametrize("name", MATRICES)
def test_packed_equals_plain_on_the_edges(monkeypatch, name, rows_per_chunk):
    monkeypatch.setenv("DSGD_FSTEP_ROWS", rows_per_chunk)
    data = pe.matrix(name)
    packed_equals_plain(monkeypatch, data, data.n_rows, weights_for(71), three_steps(name))


@pytest.mark.parametrize("rows_per_chunk", pe.FSTEP_ROWS)
@pytest.mark.parametrize("name", MATRICES)
def test_packed_against_the_oracle_on_the_edges(monkeypatch, name, rows_per_chunk):
    monkeypatch.setenv("DSGD_FSTEP_ROWS", rows_per_chunk)
    monkeypatch.setenv("DSGD_FSTEP_PACKED", "1")
    against_the_oracle(pe.matrix(name), name, 72)


@pytest.mark.parametrize("labels", ["neg", "pos", "alt"])
@pytest.mark.parametrize("name", MATRICES)
def test_one_sided_and_alternating_labels(monkeypatch, name, labels):
    """all labels -1 / all +1: every coef8 byte the packed form writes lies on one side of the plain convention, and the gate
    is taken on the folded row sum alone"""
    monkeypatch.setenv("DSGD_FSTEP_ROWS", "64")
    data = pe.matrix(name, labels)
    assert set(data.label) == {"neg": {-1}, "pos": {1}, "alt": {-1, 1}}[labels]
    packed_equals_plain(monkeypatch, data, data.n_rows, weights_for(73), three_steps(name))
    monkeypatch.setenv("DSGD_FSTEP_PACKED", "1")
    against_the_oracle(data, name, 74)


def test_families_alternate_in_one_warm_context(monkeypatch):
    """packed chunks -> three streaming launches -> packed chunks -> row-wise -> column lists -> packed chunks in ONE context,
    each step bit-equal to the same step in a fresh context started from the weights the warm one had"""
    for k, v in (("DSGD_FSTEP_PACKED", "1"), ("DSGD_FSTEP_ROWS", "64"), ("DSGD_FSTEP_MIN", "1000"), ("DSGD_FSTEP_MAX", "6000"),
                 ("DSGD_STREAM_MIN", "6001"), ("DSGD_TCOL", "1"), ("DSGD_TCOL_MIN", "600"), ("DSGD_TCOL_MAX", "900")):
        monkeypatch.setenv(k, v)
    data = pe.matrix("phases")
    n = data.n_rows
    plan = [([(0, 5000)], FSTEP),
            ([(0, n)], "dsgd_wseg_kernel<true>"),                        # above DSGD_FSTEP_MAX
            ([(100, 1500), (1500, 4100), (4100, 5900)], FSTEP),
            ([(37, 500)], "dsgd_mb_grad_kernel"),                        # below every window
            ([(200, 1000)], "dsgd_tc_grad_kernel"),                      # inside the column lists' window
            ([(0, 5000)], FSTEP)]

    def one(eng, ranges, kernel):
        rows = sum(b - a for a, b in ranges)
        st = eng.sync_step_ranges(ranges, 0.5 * 100 / rows * len(ranges))
        assert eng.grad_kernel_name() == kernel, (ranges, eng.grad_kernel_name())
        info = eng.tuning_info()
        if kernel == FSTEP:
            assert info["stream_mode"] == 5
        return st["n_samples"], st["n_active"], info["fix_shift"], eng.get_weights()

    def context():
        eng = dsgd_amd.Engine(data.dim, LAM)
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n)
        return eng

    with context() as warm:
        assert_split(warm, data)
        w = weights_for(75)
        warm.set_weights(w)
        gated = False
        for i, (ranges, kernel) in enumerate(plan):
            got = one(warm, ranges, kernel)
            with context() as fresh:
                fresh.set_weights(w)
                want = one(fresh, ranges, kernel)
            assert got[:3] == want[:3], (i, kernel, got[:3], want[:3])
            assert got[3].tobytes() == want[3].tobytes(), "step %d (%s): %d weights differ" % (i, kernel, int((got[3] != want[3]).sum()))
            gated = gated or 0 < got[1] < got[0]
            w = got[3]
        assert gated
