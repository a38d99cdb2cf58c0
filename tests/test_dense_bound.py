"""CPU: the bounds of tests/dense_bound.py are neither too tight nor vacuous.  At every shape that
tests/test_gpu_dense_edges.py steps (with a 4-CU stand-in where the row count follows the device), an honest fp32
candidate with the kernels' block / partial structure stays inside dz and dw, and each seeded fault -- last row
dropped, row `row_end` included, a workgroup's second block skipped, the two column halves swapped, 1/world
forgotten -- leaves the bound in at least one weight."""

import numpy as np
import pytest

import dense_bound as db

SMALL_CU = 4      # group a's row count is a multiple of the CU count: 229 / 88 rows here, ~14,000 / 4,120 on 256 CUs
REAL_CU = 256     # group b's 4,099-row range needs the real grid cap to reach a second block


def shapes():
    out = []
    for variant in (0, 1):
        out += [pytest.param("a", D, variant, id="a-D%d-v%d" % (D, variant)) for D in (512, 4096)]
        out += [pytest.param("b", r, variant, id="b-%d-%d-v%d" % (r[0], r[1], variant)) for r in db.B_RANGES]
        out += [pytest.param("d", D, variant, id="d-D%d-v%d" % (D, variant)) for D in db.D_WIDTHS[variant]]
    return out


def build(group, arg, variant):
    if group == "a":
        X, y, w, lr, ranges = db.case_a(arg, SMALL_CU)
        return X, y, w, lr, ranges[0], SMALL_CU
    if group == "b":
        X, y, w, lr, _, _ = db.case_b(arg[0], arg[1], variant, REAL_CU)
        return X, y, w, lr, arg, REAL_CU
    X, y, w, lr = db.case_d(arg)
    return X, y, w, lr, db.D_RANGES[0], REAL_CU


def outside(w, bd):
    return bool((np.abs(w.astype(np.float64) - bd.w_ref) > bd.dw).any())


@pytest.mark.parametrize("group,arg,variant", shapes())
def test_honest_candidate_inside_and_faults_outside(group, arg, variant):
    X, y, w, lr, (rb, re), n_cu = build(group, arg, variant)
    grid = db.launch_grid(variant, n_cu, re - rb)
    bd = db.Bound(X, y, w, lr, rb, re, variant, grid)
    for world in (1, 2):
        w1, z = db.emulate(X, y, w, lr, rb, re, variant, grid, world=world)
        err = np.abs(w1.astype(np.float64) - bd.w_ref)
        assert (err <= bd.dw).all(), (world, (err / bd.dw).max())
        assert (np.abs(z.astype(np.float64) - bd.z) <= bd.dz).all()
    assert np.abs(bd.w_ref - w).max() > 1e3 * bd.dw.max() or re - rb == 1   # the step moves w far beyond the bound
    for fault in db.FAULTS:
        if fault == "last_row_dropped" and re - rb == 1:
            continue      # would be the empty range, which the entry point refuses
        if fault == "row_end_included" and re == len(y):
            continue      # no such row
        if fault == "second_block_skipped" and -(-(re - rb) // db.rows_per_block(variant)) <= grid:
            continue      # one block per workgroup at this shape (asserted reachable below)
        w1, _ = db.emulate(X, y, w, lr, rb, re, variant, grid, world=2 if fault == "world_forgotten" else 1, fault=fault)
        assert outside(w1, bd), fault


def test_second_blocks_exist_where_claimed():
    for variant in (0, 1):
        rpb = db.rows_per_block(variant)
        for D in (512, 4096):
            rb, re = db.case_a(D, SMALL_CU)[4][0]
            assert -(-(re - rb) // rpb) > db.launch_grid(variant, SMALL_CU, re - rb)
        assert -(-4099 // rpb) == db.launch_grid(variant, REAL_CU, 4099) + 1
    # group a at D = 512: 3 or 4 blocks per workgroup, unequal, in both variants, whatever the CU count
    for n_cu in (SMALL_CU, 64, REAL_CU, 304):
        n = 3 * 16 * n_cu + 8 * n_cu + 5
        for variant in (0, 1):
            grid = db.launch_grid(variant, n_cu, n)
            counts = {len(range(wg, -(-n // db.rows_per_block(variant)), grid)) for wg in range(grid)}
            assert counts == {3, 4}, (n_cu, variant, counts)


def test_rounding_counts():
    assert db.n_z(0, 512) == 15 and db.n_z(0, 8192) == 30 and db.n_z(1, 4096) == 272
    assert db.n_g(0, 4096, 512) == 8 + 32 + 16 and db.n_g(1, 65536, 256) == 16 * 16 + 16 + 16


def test_case_d_keeps_every_row_certain():
    for D in db.D_WIDTHS[0]:
        X, y, w, lr = db.case_d(D)
        z = X.astype(np.float64) @ w.astype(np.float64)
        assert np.abs(z).min() > 0.9 and 5.0 < z.std() < 20.0, (D, np.abs(z).min(), z.std())
