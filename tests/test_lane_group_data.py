"""CPU: the data, the emulator and the bound of tests/lane_group_data.py are neither too tight nor vacuous.

  (a) the float32 emulator of row_dot<G, 4> + group_sum<G> stays within the derived per-row bound of the fp64 oracle's dot on
      every row of every matrix, at all four widths;
  (b) on the committed seed the oracle alone excludes at most 0.1 % of the rows of a matrix (the counts are in the module's
      docstring, and held to it here);
  (c) each seeded fault of the emulator -- the tail loop one stride late, the last butterfly stage missing, the stage of 32
      lanes taken at 16, the product filter dropped, the last lane skipped -- fails the comparison the GPU test makes;
  (d) every matrix reports its intended width through eval_group, the two on the threshold included.
"""

import re
import time

import numpy as np
import pytest

import lane_group_data as lg


@pytest.mark.parametrize("name", sorted(lg.MATRICES))
def test_emulator_within_the_bound_at_every_width(name):
    m = lg.matrix(name)
    for G in lg.WIDTHS:
        d = lg.emulate(m, G).astype(np.float64)
        err, bound = np.abs(d - m.dot), m.bound(G)
        assert (err <= bound).all(), (G, float((err / np.maximum(bound, 1e-300)).max()))
        # the bound is no blanket: the worst row uses a visible share of it, and it is far below the dots it protects
        used = float((err[bound > 0] / bound[bound > 0]).max())
        print("%s at %2d lanes: worst error / bound %.3f, median bound %.2e" % (name, G, used, float(np.median(bound))))
        assert used > 0.01 and np.median(bound) < (1e-5 if G == m.want_group else 1e-4)
        # within the bound, a compared row cannot change sign: the emulator passes the GPU test's comparison
        assert lg.agrees_with_oracle(m, G, lg.predictions(d))
        # exact zeros: the empty rows, the rows of nothing but 1e-25 and the row on the zero weight -- on both sides
        zero = np.flatnonzero(m.zero())
        want = sorted([lg.core_row(0, k) for k in range(lg.PER_LENGTH)] + list(lg.TINY_ROWS) + [lg.ZERO_W_ROW])
        assert zero.tolist() == want and not d[zero].any()


@pytest.mark.parametrize("name", sorted(lg.MATRICES))
def test_excluded_rows_within_the_cap_and_as_documented(name):
    m = lg.matrix(name)
    want = m.want_group
    doc = re.search(r"^  %s\s+(\d+)\s+([\d,]+)\s+([\d,]+)\s+([\d,]+)\s+[\d,]+ x \d+\s+\S+(?: \+ \S+)?\s+(\d+)\s+(\d+)" % name, lg.__doc__, flags=re.M)
    assert doc, "no line for %s in the module docstring" % name
    lanes, rows, nnz, held, excluded, zero = (int(g.replace(",", "")) for g in doc.groups())
    print(m.line())
    assert (lanes, rows, nnz, held, zero) == (want, m.n, m.nnz, m.held_nnz, int(m.zero().sum()))
    assert int(m.excluded(want).sum()) == excluded
    for G in lg.WIDTHS:     # (the cross-width comparison of the GPU test excludes at every width)
        assert m.excluded(G).sum() <= lg.CAP * m.n, (G, int(m.excluded(G).sum()))
    assert m.n < 4096       # quiet calls stay with the row-wise kernels


def test_shape_of_the_data():
    ptr, col, val, label, w = lg.core()
    lengths = np.diff(ptr)
    assert len(lengths) == lg.N_CORE == 138 and int(ptr[-1]) == 19968
    for length in lg.CORE_LENGTHS:
        rows = np.flatnonzero(lengths == length)
        assert len(rows) == 6 and sorted(label[rows].tolist()) == [-1, -1, -1, 1, 1, 1]
    assert val.dtype == np.float32 and w.dtype == np.float32 and w[lg.ZERO_W_COL] == 0.0
    special = set(lg.TINY_ROWS) | set(lg.MIXED_ROWS)
    row_id = np.repeat(np.arange(lg.N_CORE), lengths)
    norm = np.sqrt(np.bincount(row_id, weights=val.astype(np.float64) ** 2, minlength=lg.N_CORE))
    for r in range(lg.N_CORE):
        c = col[ptr[r]:ptr[r + 1]]
        assert (np.diff(c) > 0).all() and (len(c) == 0 or (1 <= c[0] and c[-1] <= lg.D))
        if lengths[r] and r not in special:
            assert abs(norm[r] - 1.0) < 1e-6
    assert col[ptr[lg.ZERO_W_ROW]] == lg.ZERO_W_COL and lengths[lg.ZERO_W_ROW] == 1
    for r in lg.TINY_ROWS:
        assert (val[ptr[r]:ptr[r + 1]] == np.float32(1e-25)).all()
    for r in lg.MIXED_ROWS:
        assert (val[ptr[r]:ptr[r] + 3] == np.float32(1e-25)).all() and abs(val[ptr[r] + 3]) > 1e-6
    # columns on both sides of the 1,024-weight tile whatever the ranking: more distinct columns than the tile holds
    for name in lg.MATRICES:
        m = lg.matrix(name)
        assert len(np.unique(m.col)) > 1024 + 256
        assert np.array_equal(m.row_ptr[:lg.N_CORE + 1], ptr) and np.array_equal(m.col[:ptr[-1]], col)      # ONE set of CORE rows
        assert np.array_equal(m.val[:ptr[-1]], val) and np.array_equal(m.label[:lg.N_CORE], label) and np.array_equal(m.w, w)


def test_reported_width_of_each_matrix():
    for name, (want, _, _, _) in lg.MATRICES.items():
        m = lg.matrix(name)
        assert lg.eval_group(m.held_nnz, m.n) == want == m.want_group and m.held_nnz == m.nnz + 6, name
    # the count the context holds (an explicit zero per empty row) sits on the threshold, and one above it
    assert lg.matrix("thr16").held_nnz == 96 * lg.matrix("thr16").n and lg.matrix("thr32").held_nnz == 96 * lg.matrix("thr32").n + 1
    assert sorted({v[0] for v in lg.MATRICES.values()}) == list(lg.WIDTHS)
    assert (lg.eval_group(12, 1), lg.eval_group(13, 1), lg.eval_group(192, 1), lg.eval_group(193, 1)) == (8, 16, 32, 64)


@pytest.mark.parametrize("mutant", lg.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """On every matrix where the fault exists at all (the stage of 32 lanes taken at 16 is a fault of 16 lanes only), at the
    matrix's own width: the comparison of the GPU test fails."""
    seen = 0
    for name in sorted(lg.MATRICES):
        m = lg.matrix(name)
        G = m.want_group
        if mutant == "stage_of_32_taken_at_16" and G != 16:
            assert np.array_equal(lg.emulate(m, G, mutant), lg.emulate(m, G))
            continue
        pred = lg.predictions(lg.emulate(m, G, mutant))
        keep = m.compared(G)
        changed = int((pred[keep] != m.pred[keep]).sum())
        print("%s on %s (%d lanes): %d compared predictions differ from the oracle's: caught" % (mutant, name, G, changed))
        assert changed >= 1 and not lg.agrees_with_oracle(m, G, pred), (mutant, name)
        seen += 1
    assert seen == (2 if mutant == "stage_of_32_taken_at_16" else len(lg.MATRICES))


def test_the_emulators_stages_pair_lanes_as_the_kernel_comments_say():
    # every stage is an involution, and after the stages of G lanes every lane holds the sum of all G: integers, exactly
    for G in lg.WIDTHS:
        n_stages = 3 + (G >= 16) + (G >= 32) + (G >= 64)
        v = (2.0 ** np.arange(G) % 8191).astype(np.float64)[None, :]
        for s in range(n_stages):
            p = lg._partner(G, s)
            assert np.array_equal(p[p], np.arange(G)) and (p != np.arange(G)).all() and p.max() < G
            v = v + v[:, p]
        assert (v == v[0, 0]).all() and v[0, 0] == (2.0 ** np.arange(G) % 8191).sum()
    assert lg._partner(16, 2).tolist() == [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8]
    assert lg._partner(16, 3).tolist() == list(range(15, -1, -1))


@pytest.mark.parametrize("name", sorted(lg.BIG))
def test_big_matrices_are_quick_valid_and_of_their_width(name):
    t0 = time.perf_counter()
    row_ptr, col, val, label, w = lg.big(name)
    dt = time.perf_counter() - t0
    want, n, lo, hi = lg.BIG[name]
    lengths = np.diff(row_ptr)
    assert len(lengths) == n and lengths.min() == lo and lengths.max() == hi and lg.eval_group(int(row_ptr[-1]) + int((lengths == 0).sum()), n) == want
    assert col.min() >= 1 and col.max() <= lg.D
    inner = np.ones(len(col), dtype=bool)
    inner[row_ptr[:-1][lengths > 0]] = False                       # a row's first entry has no predecessor in its row
    assert (np.diff(col.astype(np.int64))[inner[1:]] > 0).all()     # ascending and distinct within every row
    assert set(np.unique(label).tolist()) == {-1, 1} and val.dtype == np.float32 and w.dtype == np.float32
    # more rows than lane groups of 256 CUs in the 1,024-lane shape, and the ranges separate a group's successive ordinals
    n_groups = 256 * 1024 // want
    ranges = lg.big_ranges(n)
    assert n > n_groups and sorted(r for b, e in ranges for r in range(b, e)) == list(range(n))
    for t in (0, (n - n_groups) // 2, n - n_groups - 1):
        assert lg.range_of_ordinal(ranges, t) != lg.range_of_ordinal(ranges, t + n_groups)
    print("%s: %d rows, %d non-zeros, generated in %.2f s" % (name, n, int(row_ptr[-1]), dt))
