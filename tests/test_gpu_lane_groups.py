"""The fp32 row-wise evaluation kernels at every lane-group width (-m gpu): dsgd_forward_kernel<G>, dsgd_eval_kernel<G>,
dsgd_predict_kernel<G> and dsgd_eval_list_kernel<G> for G = 8, 16, 32 and 64 -- Engine.forward, loss_acc (below 4,096 rows),
predict_ranges, loss_acc_list and async_check (the 256-lane shape of dsgd_eval_kernel) on data whose mean row length selects
each width (csrc/dsgd_route.hpp: eval_group; dsgd_tuning_info slot [7] reports it, and every test asserts it first).

Data, the per-row bound and what "compared" means: tests/lane_group_data.py (CPU-checked by tests/test_lane_group_data.py,
where a float32 emulator with a seeded fault -- a late tail loop, a missing or a wrong butterfly stage, no product filter,
a skipped lane -- fails the comparison made here).  One set of CORE rows, of every length around G and G x UNR, runs at all
four widths; two more matrices sit on the threshold between 16 and 32 lanes.

  against the oracle   forward equals the fp64 oracle's prediction on every compared row (|x . w| beyond the derived bound;
                       rows of dot 0 exactly: 0 == 0), the excluded share within 0.1 %; loss_acc, predict_ranges and
                       loss_acc_list over ranges that hold no excluded row give the oracle's three tallies, exactly;
  against each other   predict_ranges == forward entry for entry, its counts == loss_acc's == the host's recount; a list of
                       a range == loss_acc of it; lists with duplicates and in reverse == the recount from forward;
                       async_check on the quiet context == loss_acc and get_weights, bit for bit;
  across widths        the CORE rows' predictions of the four contexts agree wherever a row is compared at all four widths
                       (the summation order differs: no bit-for-bit claim on the dots);
  the persistent loop  one larger matrix per width 8, 32 and 64 with more rows than lane groups on 256 CUs (16 lanes:
                       `big` in tests/test_gpu_predict.py): ranges that separate a group's successive ordinals, a list of all
                       rows, async_check -- each equal to forward and the host's recount;
  refusals             an empty range and a row outside the data leave weights and tallies as they were, at every width.
"""

import ctypes as C
import os

import numpy as np
import pytest

import dsgd_amd
import lane_group_data as lg
import waivers
from conftest import has_gpu
from dsgd_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

NAMES = ("g8", "g16", "g32", "g64", "thr16", "thr32")
CUT = 100          # a range boundary inside the CORE rows (row 100: one of length 127)


def splits(n):
    """tests/test_gpu_predict.py's cut: length 1, one that ends inside the CORE rows, an empty one, the rest"""
    return [(0, 1), (1, CUT), (CUT, CUT), (CUT, n)]


def rows_of(ranges):
    return np.concatenate([np.arange(b, e, dtype=np.int32) for b, e in ranges])


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def engine_of(m):
    eng = dsgd_amd.Engine(lg.D, lg.LAM)
    eng.load_csr(m.row_ptr, m.col, m.val, m.label)
    eng.build_dim_sparsity(m.n)
    eng.set_weights(m.w)
    return eng


def assert_width(eng, m):
    info = eng.tuning_info()
    assert info[7] == m.want_group == info["eval_group"] == lg.eval_group(m.held_nnz, m.n), (m.name, info)


@pytest.fixture(scope="module")
def contexts():
    """One fp32 context per matrix: data loaded, dimSparsity built, the weights set."""
    old = os.environ.get("DSGD_HSPLIT")
    os.environ["DSGD_HSPLIT"] = "512"   # (read when a context is created: the streams' split below D, as in test_gpu_predict.py)
    out = {}
    try:
        for name in NAMES:
            out[name] = engine_of(lg.matrix(name))
    finally:
        if old is None:
            del os.environ["DSGD_HSPLIT"]
        else:
            os.environ["DSGD_HSPLIT"] = old
    yield out
    for eng in out.values():
        eng.close()


@pytest.fixture(scope="module")
def forward_all(contexts):
    """Per matrix the forward kernel's predictions of every row, in row order -- computed once, never changed."""
    return {name: np.asarray(eng.forward(np.arange(lg.matrix(name).n, dtype=np.int32)), dtype=np.int64) for name, eng in contexts.items()}


# ---- against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_the_oracle(contexts, forward_all, name):
    eng, m = contexts[name], lg.matrix(name)
    assert_width(eng, m)
    G = m.want_group
    # the slot through the C ABI: eight are served, a ninth is refused
    v = (C.c_int32 * 9)()
    assert eng._lib.dsgd_tuning_info(eng._ctx, v, C.c_int32(8)) == _lib.OK and v[7] == G
    assert eng._lib.dsgd_tuning_info(eng._ctx, v, C.c_int32(9)) == _lib.EINVAL
    fwd = forward_all[name]
    keep, zero = m.compared(G), m.zero()
    print(m.line() + "  [7] = %d: forward, loss_acc, predict_ranges, loss_acc_list, async_check" % eng.tuning_info()[7])
    assert m.excluded(G).sum() <= lg.CAP * m.n
    assert set(np.unique(fwd).tolist()) <= {-1, 0, 1}
    assert not fwd[zero].any() and not m.pred[zero].any()          # empty rows, rows of filtered products, the zero weight
    assert np.array_equal(fwd[keep], m.pred[keep]), np.flatnonzero(keep & (fwd != m.pred))[:10]
    waivers.strict("lane groups %-5s [7] = %2d: forward == oracle on %d of %d rows" % (name, G, int(keep.sum()), m.n))


@pytest.mark.parametrize("name", NAMES)
def test_tallies_against_the_oracle(contexts, name):
    eng, m = contexts[name], lg.matrix(name)
    assert_width(eng, m)
    tight = m.tight_ranges(m.want_group)
    assert tight and sum(e - b for b, e in tight) >= (1.0 - lg.CAP) * m.n - 1
    want = [m.oracle_counts(b, e) for b, e in tight]
    pred, counts, _, _ = eng.predict_ranges(tight)
    assert np.array_equal(pred.astype(np.int64), m.pred[rows_of(tight)])     # (no excluded row in these ranges)
    wrong = [("predict_ranges", counts.tolist(), want)] if counts.tolist() != want else []
    for (b, e), c in zip(tight, want):
        wrong += [(what, (b, e), got, c) for what, got in (("loss_acc", eng.loss_acc(b, e)[2]),
                                                           ("loss_acc_list", eng.loss_acc_list(np.arange(b, e, dtype=np.int32))[2])) if got != c]
    # the tight statement and nothing else: these ranges hold no row that could excuse a difference (exposed = False)
    waivers.tight("lane groups %-5s [7] = %2d: loss_acc, predict_ranges, loss_acc_list == oracle tallies" % (name, m.want_group),
                  not wrong, False, why=str(wrong[:3]))
    if tight == [(0, m.n)]:
        # the tallies are exact; |w|^2 is a sum of D + 1 squares in float: (D + 1) roundings at the most
        o_loss, o_acc, _, _ = m.oracle.loss_acc(m.w.astype(np.float64), 0, m.n)
        nsq = float((m.w.astype(np.float64) ** 2).sum())
        for loss, acc in (eng.loss_acc(0, m.n)[:2], eng.predict_ranges(tight)[2:], eng.loss_acc_list(np.arange(m.n, dtype=np.int32))[:2]):
            assert acc == o_acc and abs(loss - o_loss) <= lg.LAM * nsq * (lg.D + 1) * 2.0 ** -24


# ---- against each other: exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["four_ranges", "single_range"])
@pytest.mark.parametrize("name", NAMES)
def test_predictions_and_tallies_come_from_one_dot(contexts, forward_all, name, single):
    eng, m = contexts[name], lg.matrix(name)
    assert_width(eng, m)
    ranges = [(0, m.n)] if single else splits(m.n)
    rows = rows_of(ranges)
    pred, counts, loss, acc = eng.predict_ranges(ranges)
    assert pred.dtype == np.int8 and len(pred) == len(rows) == m.n and counts.shape == (len(ranges), 3)
    assert np.array_equal(pred.astype(np.int64), forward_all[name][rows])
    off = 0
    for k, (b, e) in enumerate(ranges):
        if e == b:
            assert counts[k].tolist() == [0, 0, 0]
            continue
        ref = eng.loss_acc(b, e)
        assert counts[k].tolist() == ref[2] == lg.host_counts(pred[off:off + e - b], m.label[b:e]), (k, b, e)
        assert eng.loss_acc_list(np.arange(b, e, dtype=np.int32)) == ref, (k, b, e)
        off += e - b
    l_ref, a_ref, c_ref = eng.loss_acc(0, m.n)
    assert counts.sum(axis=0).tolist() == c_ref and loss == l_ref and acc == a_ref


@pytest.mark.parametrize("name", NAMES)
def test_lists_with_duplicates_and_in_reverse(contexts, forward_all, name):
    eng, m = contexts[name], lg.matrix(name)
    assert_width(eng, m)
    fwd = forward_all[name]
    rng = np.random.default_rng(5)
    core = np.arange(lg.N_CORE, dtype=np.int32)
    lists = {"reversed": np.arange(m.n - 1, -1, -1, dtype=np.int32),
             "core_twice_and_reversed": np.concatenate([core, core[::-1]]),
             "repeats": np.asarray([lg.ZERO_W_ROW] * 3 + [lg.core_row(1000, 2)] * 2 + list(lg.TINY_ROWS) * 2 + [lg.core_row(0, 0), m.n - 1, m.n - 1], dtype=np.int32),
             "drawn_with_replacement": rng.integers(0, m.n, size=m.n + 65).astype(np.int32)}
    for what, idx in lists.items():
        loss, acc, counts = eng.loss_acc_list(idx)
        assert counts == lg.host_counts(fwd[idx], m.label[idx]) and sum(counts) == len(idx), what
        assert acc == counts[0] / float(len(idx)), what
        assert np.array_equal(np.asarray(eng.forward(idx), dtype=np.int64), fwd[idx]), what


@pytest.mark.parametrize("name", NAMES)
def test_async_check_on_the_quiet_context(contexts, forward_all, name):
    eng, m = contexts[name], lg.matrix(name)
    assert_width(eng, m)
    for b, e in ((0, m.n), (1, CUT), (CUT, m.n), (lg.core_row(1000, 0), lg.core_row(1000, 0) + 1)):
        ref = eng.loss_acc(b, e)
        loss, acc, counts, window = eng.async_check(b, e)
        assert (loss, acc, counts) == ref and counts == lg.host_counts(forward_all[name][b:e], m.label[b:e]), (b, e)
        assert np.array_equal(bits(eng.async_check_weights(0)), bits(eng.get_weights())) and np.array_equal(bits(eng.get_weights()), bits(m.w))
        assert eng.loss_acc(b, e) == ref


# ---- across widths ---------------------------------------------------------------------------------------------------------------
def test_core_rows_agree_across_widths(contexts, forward_all):
    names = ("g8", "g16", "g32", "g64")
    for name in names:
        assert_width(contexts[name], lg.matrix(name))
    assert sorted(lg.matrix(name).want_group for name in names) == list(lg.WIDTHS)
    core = slice(0, lg.N_CORE)
    keep = np.ones(lg.N_CORE, dtype=bool)
    for name in names:       # (the CORE rows and the weights are the same arrays in the four matrices: so are dot and bound)
        keep &= lg.matrix(name).compared(lg.matrix(name).want_group)[core]
    print("CORE rows compared at all four widths: %d of %d" % (int(keep.sum()), lg.N_CORE))
    assert keep.sum() >= lg.N_CORE - 1
    for name in names + ("thr16", "thr32"):
        assert np.array_equal(forward_all[name][core][keep], forward_all["g8"][core][keep]), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_refusals_change_nothing(contexts, name):
    eng, m = contexts[name], lg.matrix(name)
    assert_width(eng, m)
    before_w = eng.get_weights().copy()
    before = eng.loss_acc(0, m.n)
    other = np.ones(lg.D + 1, dtype=np.float32)      # would replace the weights if a refused call got that far
    calls = [
        (ValueError, lambda: eng.predict_ranges([(5, 5), (9, 9)], w=other)),                     # no rows at all
        (ValueError, lambda: eng.predict_ranges([], w=other)),
        (IndexError, lambda: eng.predict_ranges([(0, 10), (m.n - 1, m.n + 1)], w=other)),        # a row beyond the data
        (IndexError, lambda: eng.predict_ranges([(-1, 10)], w=other)),
        (ValueError, lambda: eng.loss_acc(7, 7, w=other)),                                       # an empty range
        (IndexError, lambda: eng.loss_acc(0, m.n + 1, w=other)),
        (IndexError, lambda: eng.loss_acc(-1, 5, w=other)),
        (ValueError, lambda: eng.loss_acc_list(np.zeros(0, dtype=np.int32))),                    # an empty list
        (IndexError, lambda: eng.loss_acc_list(np.asarray([0, m.n], dtype=np.int32))),           # an index outside the rows
        (IndexError, lambda: eng.loss_acc_list(np.asarray([3, -1, 4], dtype=np.int32))),
        (IndexError, lambda: eng.forward(np.asarray([0, m.n], dtype=np.int32))),
        (ValueError, lambda: eng.async_check(CUT, CUT)),
        (IndexError, lambda: eng.async_check(0, m.n + 1)),
    ]
    for exc, call in calls:
        with pytest.raises(exc):
            call()
        assert np.array_equal(bits(eng.get_weights()), bits(before_w))
        assert eng.loss_acc(0, m.n) == before                      # the counters: the next tallies are the ones before
    pred, counts, loss, acc = eng.predict_ranges([(0, m.n)])
    assert counts[0].tolist() == before[2] and (loss, acc) == before[:2]


# ---- the persistent loop at each width -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lg.BIG))
def test_groups_that_own_several_rows(name):
    m = lg.big_matrix(name)
    G, n = m.want_group, m.n
    ranges = lg.big_ranges(n)
    rows = rows_of(ranges)
    assert len(rows) == n and len(np.unique(rows)) == n
    with engine_of(m) as eng:
        assert_width(eng, m)
        n_groups = 256 * 1024 // G                 # the 1,024-lane shape on 256 CUs; the 256-lane shape holds a quarter
        assert n > n_groups and lg.range_of_ordinal(ranges, 0) != lg.range_of_ordinal(ranges, n_groups)
        fwd = np.asarray(eng.forward(rows), dtype=np.int64)        # the reference: one group per listed row, no carry
        # forward against the oracle, as on the small matrices
        keep = m.compared(G)
        print(m.line() + "  [7] = %d: forward, predict_ranges, loss_acc_list, async_check, loss_acc on short ranges" % eng.tuning_info()[7])
        assert m.excluded(G).sum() <= lg.CAP * n
        assert np.array_equal(fwd[keep[rows]], m.pred[rows][keep[rows]])
        # the ranges: predictions entry for entry, the carried counters flushed into the right range
        pred, counts, loss, acc = eng.predict_ranges(ranges)
        assert np.array_equal(pred.astype(np.int64), fwd)
        off = 0
        for k, (b, e) in enumerate(ranges):
            assert counts[k].tolist() == lg.host_counts(fwd[off:off + e - b], m.label[b:e]), (k, b, e)
            if 0 < e - b < 4096:                   # (beyond, dsgd_loss_acc streams the split matrix in another summation order)
                assert counts[k].tolist() == eng.loss_acc(b, e)[2], (k, b, e)
            off += e - b
        total = counts.sum(axis=0).tolist()
        fwd_rows = np.empty(n, dtype=np.int64)
        fwd_rows[rows] = fwd                        # forward's predictions in row order
        assert total == lg.host_counts(fwd_rows, m.label) and sum(total) == n and acc == total[0] / n
        pred1, counts1, loss1, acc1 = eng.predict_ranges([(0, n)])
        assert np.array_equal(pred1.astype(np.int64), fwd_rows) and counts1[0].tolist() == total and (loss1, acc1) == (loss, acc)
        # a list of all rows, in order and permuted: groups own several positions
        for idx in (np.arange(n, dtype=np.int32), rows):
            l_loss, l_acc, l_counts = eng.loss_acc_list(idx)
            assert l_counts == total and (l_loss, l_acc) == (loss, acc)
        # async_check at rest: 256-lane workgroups, a quarter of the groups, several rows each
        a_loss, a_acc, a_counts, _ = eng.async_check(0, n)
        assert a_counts == total and a_acc == acc
        assert np.array_equal(bits(eng.async_check_weights(0)), bits(m.w))
        b, e = ranges[3]
        assert eng.async_check(b, e)[2] == counts[3].tolist()
        waivers.strict("lane groups %-5s [7] = %2d: predict_ranges, loss_acc_list, async_check == forward on %d rows" % (name, G, n))
