"""Row chunks on the packed copies of the split streams (-m gpu; csrc/dsgd_fstep.hpp: dsgd_fstep_kernel<true>,
DSGD_FSTEP_PACKED=1) against the plain form (=0): row starts ride in bit 15 of the hot rank words, the values of both streams
carry their row's label, the hot lane tables are not read.  Every sum of the packed form is the plain form's times the label --
negation commutes with the products, the additions, their rounding and the 1e-20 filter -- so the two end on the SAME bits:
weights and active-row counts are compared bit for bit over three steps from non-zero weights, in fresh contexts, on

  * ~20,000 RCV1-like rows, one worker and three unequal ranges (one worker also against the fp64 oracle under the derived
    bound of oracle/bounds.py, as tests/test_gpu_fstep.py holds the plain form);
  * rows of ~4 non-zeros (several row starts per lane: the general path of the tile body; chunks of 64 rows cut most tiles
    short, so windows open on the starts of earlier rows);
  * rows longer than a wave tile (the long-row list) among empty rows and rows of one entry;
  * the hostile values of tests/hard_data.py -- both signs, products that vanish under the 1e-20 filter, rows on the gate --
    and -0.0 entries;
  * a second matrix loaded into a warm context (the copies are rebuilt with the split they copy).

tuning_info()["stream_mode"] says which form the last chunked launch ran (5: packed, 4: plain); every leg asserts it.
The window edges of the packed reader, on matrices built to produce them, live in tests/test_gpu_packed_edges.py."""

import numpy as np
import pytest

import dsgd_amd
import hard_data as hd
from conftest import has_gpu
from test_gpu_fstep import FSTEP, some_weights, with_long_rows
from test_gpu_parity import make_pair, ragged_data, ranged_step
from test_gpu_reload import reload_vs_fresh, run_ranges, RANGES as RELOAD_RANGES

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
_DATA = {}


@pytest.fixture(autouse=True)
def _row_chunks_from_4096_rows(monkeypatch):
    for k in ("DSGD_FSTEP", "DSGD_FSTEP_MAX", "DSGD_FSTEP_ROWS", "DSGD_STREAM_MIN", "DSGD_HSPLIT", "DSGD_FIX_SHIFT", "DSGD_FSTEP_REBALANCE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DSGD_TCOL", "0")
    monkeypatch.setenv("DSGD_FSTEP_MIN", "4096")


def data_of(name):
    if name not in _DATA:
        if name == "plain":
            _DATA[name] = dsgd_amd.synth.generate(20000, seed=61)
        elif name == "short":
            _DATA[name] = dsgd_amd.synth.generate(20000, seed=62, nnz_mean=4.0)
        elif name == "long":
            _DATA[name] = with_long_rows(ragged_data(29, n_rows=12000), 29)
        elif name == "neg_zero":   # every seventh entry of the signed trait becomes -0.0, every eleventh +0.0
            base = hd.build("signed").data
            val = base.val.copy()
            val[::7] = -0.0
            val[::11] = 0.0
            _DATA[name] = dsgd_amd.synth.Csr(base.dim, base.row_ptr.copy(), base.col.copy(), val, base.label.copy())
        else:
            _DATA[name] = hd.build(name).data
    return _DATA[name]


def steps(monkeypatch, packed, data, n_train, w0, ranges_per_step):
    monkeypatch.setenv("DSGD_FSTEP_PACKED", packed)
    out = []
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(n_train)
        eng.set_weights(w0)
        for ranges in ranges_per_step:
            rows = sum(b - a for a, b in ranges)
            st = eng.sync_step_ranges(ranges, 0.5 * 100 / rows * len(ranges))
            assert eng.grad_kernel_name() == FSTEP
            info = eng.tuning_info()
            assert info["stream_mode"] == (5 if packed == "1" else 4) and info["fstep_packed"] == int(packed)
            out.append((st["n_samples"], st["n_active"], info["fix_shift"], eng.get_weights()))
    return out


def packed_equals_plain(monkeypatch, data, n_train, w0, ranges_per_step):
    p = steps(monkeypatch, "1", data, n_train, w0, ranges_per_step)
    q = steps(monkeypatch, "0", data, n_train, w0, ranges_per_step)
    for i, (a, b) in enumerate(zip(p, q)):
        assert a[:3] == b[:3], (i, a[:3], b[:3])
        assert a[3].tobytes() == b[3].tobytes(), "step %d: %d weights differ" % (i, int((a[3] != b[3]).sum()))
    assert any(0 < a[1] < a[0] for a in p), [a[:2] for a in p]   # (some rows gated off, some not: the gate is exercised)
    return p


@pytest.mark.parametrize("workers", ["one", "three"])
def test_packed_equals_plain_on_rcv1_like_rows(monkeypatch, workers):
    data, n_train = data_of("plain"), 16000
    ranges = [(0, n_train)] if workers == "one" else [(0, 3001), (3001, 11007), (11007, n_train)]
    packed_equals_plain(monkeypatch, data, n_train, some_weights(data.dim, 61), [ranges] * 3)


@pytest.mark.parametrize("rows_per_chunk", ["64", "512"])
def test_packed_equals_plain_on_short_rows(monkeypatch, rows_per_chunk):
    """~4 non-zeros per row: lanes hold several row starts (the general path), tiles hold more than 64 rows and reach the
    254-row cap; chunks of 64 rows end tiles at any slot, so the next window opens on earlier rows' starts"""
    monkeypatch.setenv("DSGD_FSTEP_ROWS", rows_per_chunk)
    data, n_train = data_of("short"), 16000
    packed_equals_plain(monkeypatch, data, n_train, some_weights(data.dim, 62, scale=0.5),
                        [[(0, n_train)], [(7, 5000), (5000, 15991)], [(0, n_train)]])


def test_packed_equals_plain_with_long_rows(monkeypatch):
    """rows of 3,000 entries (the long-row list, served from the ranked CSR with real labels) between empty rows, one-entry rows
    and 1e-25 entries; chunks of 50 rows"""
    monkeypatch.setenv("DSGD_FSTEP_ROWS", "50")
    data, n_train = data_of("long"), 10000
    packed_equals_plain(monkeypatch, data, n_train, some_weights(data.dim, 29), [[(0, n_train)], [(0, 5000), (5000, n_train)], [(100, 2500), (2500, 4900)]])


@pytest.mark.parametrize("trait", ["signed", "wide", "zero_margin", "scaled_m30", "ragged64", "neg_zero"])
def test_packed_equals_plain_on_hostile_values(monkeypatch, trait):
    data = data_of(trait)
    w0 = hd.build("signed" if trait == "neg_zero" else trait).w.astype(np.float32)
    packed_equals_plain(monkeypatch, data, hd.N_TRAIN, w0, [hd.RANGES["whole"], hd.RANGES["halves"], hd.RANGES["whole"]])


def test_packed_against_the_oracle(monkeypatch):
    """the packed form under the derived per-coordinate bound, from non-zero weights, one worker and three"""
    monkeypatch.setenv("DSGD_FSTEP_PACKED", "1")
    data, n_train = data_of("plain"), 16000
    o, eng = make_pair(data, LAM, n_train)
    with eng:
        eng.set_weights(some_weights(data.dim, 61))
        for ranges in ([(0, n_train)], [(0, 3001), (3001, 11007), (11007, n_train)], [(0, n_train)]):
            ranged_step(o, eng, ranges, 0.5 * 100 / n_train * len(ranges))
            assert eng.grad_kernel_name() == FSTEP and eng.tuning_info()["stream_mode"] == 5


def test_packed_after_a_reload(monkeypatch):
    """a second matrix into a warm context: the packed copies go with the split they copy and are rebuilt for the new one --
    every observation bit-equal to a fresh context's on that matrix"""
    monkeypatch.setenv("DSGD_FSTEP_PACKED", "1")
    monkeypatch.setenv("DSGD_FSTEP_MIN", "1000")
    inner = run_ranges(RELOAD_RANGES, FSTEP)

    def run_checked(eng, o, name):
        out = inner(eng, o, name)
        # (the last range of RELOAD_RANGES is the row-wise kernel's; the form of the last CHUNKED launch is what is reported)
        assert eng.tuning_info()["stream_mode"] == 5
        return out

    reload_vs_fresh(run_checked, ("A", "B"))
    reload_vs_fresh(run_checked, ("A", "B", "A"))
