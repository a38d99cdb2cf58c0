"""No GPU needed: the traits of tests/reload_data.py that make a stale cache VISIBLE in tests/test_gpu_reload.py -- a second
matrix that shares none of what a context derives from the first (row count, column ranking, vexp, lane group, row lengths),
index lists that survive or do not survive the load, and the one-workgroup kernel's limit restated from the header."""

import numpy as np

import reload_data as rl
from hard_data import vexp_of
from oracle import oracle as orc
from oracle import ref_dict as rd


def test_b_shares_nothing_a_context_derives_from_a():
    a, b = rl.matrix_a(), rl.matrix_b()
    assert (a.n_rows, b.n_rows, a.dim, b.dim) == (rl.ROWS_A, rl.ROWS_B, rl.DIM, rl.DIM)
    assert b.n_rows < a.n_rows
    # another ranking: fewer than 10 % of A's hottest columns (the hot stream's) are among B's
    shared = len(np.intersect1d(rl.hottest(a), rl.hottest(b)))
    assert shared < 0.1 * rl.HOT, shared
    # another fixed-point scale: every value times 8
    assert float(np.abs(a.val).max()) <= 1.0
    assert vexp_of(b.val) - vexp_of(a.val) == 3
    # another lane group of the evaluation kernels
    mean_a, mean_b = rl.internal_row_len(a).mean(), rl.internal_row_len(b).mean()
    assert mean_a < rl.LANE_GROUP_MEAN < mean_b, (mean_a, mean_b)
    assert (rl.lane_group(a), rl.lane_group(b)) == (16, 32)
    # ragged: every 50th row empty, two rows for the long-row list, every row ascending without repeats
    lens = np.diff(b.row_ptr)
    assert (lens[::50][np.isin(np.arange(0, b.n_rows, 50), rl.B_LONG_ROWS, invert=True)] == 0).all()
    assert (lens[list(rl.B_LONG_ROWS)] == rl.LONG_LEN).all()
    row_id = np.repeat(np.arange(b.n_rows), lens)
    same_row = row_id[1:] == row_id[:-1]
    assert (np.diff(b.col)[same_row] > 0).all() and b.col.min() >= 1 and b.col.max() <= b.dim
    assert (np.diff(a.row_ptr) > 0).all()   # (A has no empty row: B's are new to the context)


def test_the_mirror_and_the_scale_are_exact():
    from dsgd_amd import synth

    base, b = synth.generate(rl.ROWS_B, seed=8, nnz_mean=150), rl.matrix_b()
    for r in (1, 49, 51, 8999):
        s0, e0, s1, e1 = int(base.row_ptr[r]), int(base.row_ptr[r + 1]), int(b.row_ptr[r]), int(b.row_ptr[r + 1])
        to = rl.mirror_of_b(base.col[s0:e0])
        at = np.argsort(to)
        assert len(set(to.tolist())) == e0 - s0 and to.min() >= 1 and to.max() <= base.dim   # (a bijection of the keys)
        np.testing.assert_array_equal(b.col[s1:e1], to[at])
        np.testing.assert_array_equal(b.val[s1:e1].astype(np.float64), 8.0 * base.val[s0:e0][at].astype(np.float64))
    # A's hottest key is the one B's base ranked last, and the other way round
    ka, kb = rl._keys_by_rank(rl.matrix_a()), rl._keys_by_rank(base)
    assert rl.mirror_of_b([kb[0]])[0] == ka[-1] and rl.mirror_of_b([kb[-1]])[0] == ka[0]


def test_the_lists_that_survive_and_those_that_do_not():
    lo = min(rl.N_TRAIN_A, rl.N_TRAIN_B, rl.ROWS_B)
    for k, b in ((3, 100), (4, 200), (1, 100), (1, 700), (1, 4096)):
        for lst in rl.lists_inside(k, b, seed=1):
            assert len(lst) == b and len(set(lst.tolist())) == b and lst.min() >= 0 and lst.max() < lo
    assert rl.LONG_LIST.min() >= 0 and rl.LONG_LIST.max() < lo and len(set(rl.LONG_LIST.tolist())) == 100
    beyond = rl.lists_beyond_b(3, 100, seed=2)
    assert all(l.max() < rl.ROWS_B for l in beyond[:-1])
    assert beyond[-1].max() >= rl.ROWS_B and beyond[-1].min() < rl.ROWS_B   # (starts inside: the check must read on)
    assert max(l.max() for l in beyond) < rl.ROWS_A and all(len(l) == 100 for l in beyond)


def test_a_long_breaks_the_staged_sub_batch_at_the_same_row_count():
    a, al = rl.matrix_a(), rl.matrix_a_long()
    cap, ch = rl.stage_constants()
    assert (cap, ch) == (192, 128)
    assert al.n_rows == a.n_rows
    assert rl.list_fits_staged(a, rl.LONG_LIST)              # the plan made on A is the one-workgroup kernel's
    items = int(((rl.internal_row_len(al)[rl.LONG_LIST] + ch - 1) // ch).sum())
    assert items == 100 * ((rl.LONG_LEN + ch - 1) // ch) > cap
    assert not rl.list_fits_staged(al, rl.LONG_LIST)
    assert rl.list_fits_staged(rl.matrix_b(), rl.LONG_LIST) in (True, False)   # (in range: a verdict either way, no refusal)
    untouched = np.setdiff1d(np.arange(a.n_rows), rl.LONG_LIST)[:500]
    np.testing.assert_array_equal(np.diff(a.row_ptr)[untouched], np.diff(al.row_ptr)[untouched])
    assert vexp_of(al.val) == vexp_of(a.val)
    # one sign in every replaced row: no column of the list's step can cancel below the launch's grid (reload_data's docstring)
    assert (al.label[rl.LONG_LIST] == 1).all() and (a.label[rl.LONG_LIST] == -1).any()
    for r in rl.LONG_LIST[:5]:
        v = al.val[al.row_ptr[r]:al.row_ptr[r + 1]]
        assert v.min() * 2.0 ** 21 > 1000.0   # (every entry a thousand units of the coarsest grid a plan's launch uses)


def test_the_narrow_pair_has_no_cold_stream():
    n1, n2 = rl.narrow_pair()
    assert n1.dim == n2.dim == 3000 and n1.dim + 1 < rl.HOT
    assert (n1.n_rows, n2.n_rows) == (6000, 4000)


def test_perturbed_doubles_are_not_floats():
    b = rl.matrix_b()
    d = rl.perturbed_doubles(b)
    nz = d.val64 != 0.0
    assert (d.val64[nz] != d.val64[nz].astype(np.float32).astype(np.float64)).all()
    np.testing.assert_allclose(d.val64, b.val.astype(np.float64), rtol=2.0 ** -30, atol=0)


def test_both_oracles_agree_on_one_step_over_b():
    b = rl.matrix_b()
    lam, lr = 1e-5, 0.5
    o = orc.Oracle(b.dim, b.row_ptr, b.col, b.val, b.label, lam)
    o.set_dim_sparsity(o.dim_sparsity(rl.N_TRAIN_B))
    lists = rl.lists_inside(3, 100, seed=1)
    lists[0][0] = 0   # an emptied row among them
    w0 = rl.nonzero_weights(5).astype(np.float64)
    w_c = w0.copy()
    o.sync_step(w_c, lists, lr)
    # the dict reference on the listed rows alone (its data indexed by position: the lists renumbered)
    rows = np.concatenate(lists)
    data_d = []
    for r in rows:
        s, e = int(b.row_ptr[r]), int(b.row_ptr[r + 1])
        data_d.append((rd.Sparse({int(c): float(v) for c, v in zip(b.col[s:e], b.val[s:e])}, b.dim), int(b.label[r])))
    model = rd.SparseSVM(lam, rd.Sparse({int(k): float(o.ds[k]) for k in np.nonzero(o.ds)[0]}, b.dim))
    w_d = rd.master_sync_step(model, data_d, rd.Sparse({int(k): float(w0[k]) for k in np.nonzero(w0)[0]}, b.dim),
                              [list(range(100 * i, 100 * (i + 1))) for i in range(3)], lr)
    dense = np.zeros(b.dim + 1)
    for k, v in w_d.map.items():
        dense[k] = v
    np.testing.assert_allclose(w_c, dense, rtol=0, atol=1e-12)
    assert not np.array_equal(w_c, w0)
