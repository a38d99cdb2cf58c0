"""-m gpu: the sparse compaction (dsgd_sparse_compact_kernel, csrc/dsgd_sparse.hpp) beyond one polling pass.

A workgroup sums the counts of the tiles in front of it 64 granules per pass (`for (t0 = 0; t0 < tile; t0 += 64)`), tiles are
handed out by a ticket, and the granule state is reused from launch to launch without a memset.
tests/test_gpu_sparse_boundary.py stops at dim = 47,236: 12 tiles of 4,096 keys, one pass, a handful of launches per context.
Here, against the same host compaction (flatnonzero(|v| > 1e-20) ascending, values bit for bit):
  64 and 65 tiles (the last workgroup sums 63 / 64 granules: up to one pass exactly), 66 tiles (65 granules: a second pass
  with one live lane), 129 tiles (three passes), 1,024 tiles (more workgroups than are resident at once: the ticket order
  is what keeps the chain live);
  prefix sums that are all zero or all in one term (every non-zero in the last tile / in tile 0);
  keys on either side of the pass boundaries;
  300 launches on one context, every one with other counts than the one before it;
  the regularising variant (fp32 gradient requests) and the fp64 requests at 74 tiles."""

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from test_gpu_sparse_boundary import EPS, LAM, _check_pairs, _compact, _dt, _patterns, _random_w, _same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

TILE = 4096      # SP_TILE
PASS = 64        # granules a pass polls
# dp = dim + 1 keys: 64 tiles | 64 tiles and one key; 65 full tiles | 65 tiles and one key; 129 tiles; 1,024 tiles.  Tile t sums t
# granules: the second pass begins with tile 65, the third with tile 129
DIMS = [262143, 262144, 266239, 266240, 528383, 4194303]


def _tiles(dim):
    return (dim + 1 + TILE - 1) // TILE


def test_the_sizes_are_the_edges_they_are_meant_to_be():
    assert [_tiles(d) for d in DIMS] == [64, 65, 65, 66, 129, 1024]
    assert (262143 + 1) % TILE == 0 and (262144 + 1) % TILE == 1 and (266239 + 1) % TILE == 0 and (266240 + 1) % TILE == 1


def _one_tile_only(dim, dtype, tile):
    """about half of the keys of one tile non-zero (its last key always), nothing anywhere else"""
    dp = dim + 1
    lo, hi = tile * TILE, min(dp, (tile + 1) * TILE)
    rng = np.random.default_rng(dim + tile)
    w = np.zeros(dp, dtype=dtype)
    at = lo + np.flatnonzero(rng.random(hi - lo) < 0.5)
    w[at] = rng.normal(size=len(at)).astype(dtype)
    w[hi - 1] = 0.75
    return w


def _wide_patterns(dim, dtype):
    p = _patterns(dim, dtype)
    p["last tile"] = _one_tile_only(dim, dtype, _tiles(dim) - 1)   # every prefix sum zero, the total in its last term
    p["tile 0"] = _one_tile_only(dim, dtype, 0)                    # every prefix sum the same one term
    return p


# ---- 1. the tile counts at which the summing loop takes another pass ----
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("dim", DIMS)
def test_compaction_and_scatter_past_one_polling_pass(dim, precision):
    dt = _dt(precision)
    order_rng = np.random.default_rng(3)
    with dsgd_amd.Engine(dim, LAM, precision=precision) as eng:
        for name, w in _wide_patterns(dim, dt).items():
            eng.set_weights(w)
            keys, vals = eng.get_weights_sparse()
            assert vals.dtype == dt
            _check_pairs(keys, vals, w)
            assert len(keys) == {"zero": 0, "full": dim + 1}.get(name, len(keys)), name
            if name == "ends":
                assert keys.tolist() == [0, dim]
            if name == "last tile":
                assert len(keys) > 0 and keys[0] >= (_tiles(dim) - 1) * TILE and keys[-1] == dim
            if name == "tile 0":
                assert len(keys) > 1000 and keys[-1] == TILE - 1
            # ... and back in: the pairs in a shuffled order over weights that are not zero
            eng.set_weights(np.full(dim + 1, 7, dtype=dt))
            order = order_rng.permutation(len(keys))
            eng.set_weights_sparse(keys[order], vals[order])
            host_scatter = np.zeros(dim + 1, dtype=dt)
            host_scatter[keys] = vals
            assert _same_bits(eng.get_weights(), host_scatter), name


# ---- 2. keys on either side of the pass boundaries ----
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_keys_straddling_the_pass_boundaries(precision):
    dim = 528383
    dt = _dt(precision)
    at = [0, TILE * PASS - 1, TILE * PASS, TILE * 2 * PASS - 1, TILE * 2 * PASS, dim]
    with dsgd_amd.Engine(dim, LAM, precision=precision) as eng:
        for shift in range(3):   # (other values, then other counts in front of each boundary: one key of the six left out)
            w = np.zeros(dim + 1, dtype=dt)
            w[at] = np.arange(1 + shift, len(at) + 1 + shift, dtype=dt) * (-1) ** shift
            want = list(at)
            if shift == 2:
                w[at[1]] = 0
                want.remove(at[1])
            eng.set_weights(w)
            keys, vals = eng.get_weights_sparse()
            assert keys.dtype == np.int32 and keys.tolist() == want and len(keys) == len(want)
            assert _same_bits(vals, w[want])


# ---- 3. the granule state, launch after launch ----
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_three_hundred_launches_on_one_context(precision):
    """full, zero, 5 %, last tile only, and round again: the granule a launch left behind in a slot always carries another
    count than the one this launch publishes there (the tag, not the count, is what must tell them apart)."""
    dim = 300000
    dt = _dt(precision)
    p = _wide_patterns(dim, dt)
    cycle = [p[name] for name in ("full", "zero", "5%", "last tile")]
    per_tile = [np.add.reduceat((np.abs(w.astype(np.float64)) > EPS).astype(np.int64), np.arange(0, dim + 1, TILE)) for w in cycle]
    for a, b in zip(per_tile, per_tile[1:] + per_tile[:1]):
        assert (a != b).all()
    want = [_compact(w) for w in cycle]
    with dsgd_amd.Engine(dim, LAM, precision=precision) as eng:
        for call in range(300):
            w, (k, v) = cycle[call % 4], want[call % 4]
            if call % 3 == 2:
                eng.set_weights_sparse(k, v)
            else:
                eng.set_weights(w)
            keys, vals = eng.get_weights_sparse()
            assert np.array_equal(keys, k) and _same_bits(vals, v), call
        assert _same_bits(eng.get_weights(), cycle[299 % 4])


# ---- 4. the gradient requests at 74 tiles ----
N_ROWS, N_TRAIN = 4000, 3200
_DATA = {}


def _data():
    if "d" not in _DATA:
        _DATA["d"] = dsgd_amd.synth.generate(N_ROWS, dim=300000)
    return _DATA["d"]


def _engine(precision):
    d = _data()
    eng = dsgd_amd.Engine(d.dim, LAM, precision=precision)
    eng.load_csr(d.row_ptr, d.col, d.val, d.label)
    eng.build_dim_sparsity(N_TRAIN)
    return eng


def _lists():
    rng = np.random.default_rng(5)
    dup = rng.integers(0, N_TRAIN, size=100).astype(np.int32)
    dup[50:] = dup[:50]
    return [np.asarray([123], dtype=np.int32), dup, rng.permutation(N_TRAIN)[:2000].astype(np.int32)]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_gradient_sparse_against_the_dense_twin_past_64_tiles(precision):
    """fp32: the compaction regularises the accumulator on the way and clears it behind the read (REG) -- the request that
    follows on the same context would see what was left.  fp64: the first two lists."""
    dt = _dt(precision)
    d = _data()
    assert _tiles(d.dim) == 74
    w = _random_w(d.dim, dt, nnz=20000)
    wk, wv = _compact(w)
    lists = _lists() if precision == "fp32" else _lists()[:2]
    beyond = 0
    with _engine(precision) as a, _engine(precision) as b:
        dense = b.gradient_f64 if precision == "fp64" else b.gradient
        for idx in lists:
            a.set_weights(w)
            b.set_weights(w)
            for given in (False, True):   # the resident weights; then the same weights as pairs / dense: a second request
                keys, vals, st = a.gradient_sparse(idx, (wk, wv) if given else None)
                g, st_b = dense(idx, w if given else None)
                assert g.dtype == dt
                _check_pairs(keys, vals, g)
                assert st == st_b and st["n_samples"] == len(idx)
                assert _same_bits(a.get_weights(), b.get_weights())
            beyond = max(beyond, int((keys >= PASS * TILE).sum()))
        # (the requests did reach into the tiles of the second pass)
        assert beyond > 0
        # the accumulator was cleared behind the last read: a one-row request gives that row's gradient again
        keys, vals, st = a.gradient_sparse(lists[0])
        g, st_b = dense(lists[0])
        _check_pairs(keys, vals, g)
        assert st == st_b
        assert _same_bits(a.get_weights(), b.get_weights()) and _same_bits(a.get_weights(), w)
