"""The topics' and softmax's list steps by the whole matrix's column lists (csrc/dsgd_lg_lists_cols.hpp;
Engine.lg_topics_sync_steps / lg_softmax_sync_steps with by_columns=True): the BITS of the list calls on the same arguments -- in
every form and at every group width, with one and with three workers, a list of one row, lists that name every row, a row named
twice (served by the list launches inside the call) and the same call twice -- and, once per family, within the bounds of
tests/logistic_bound.py and tests/softmax_bound.py of a plain fp64 step.

One matrix of 600 rows and 300 features, about 20 non-zeros a row: 47 shares of 256 entries, so columns are cut at run and share
boundaries.  Row 17 is empty; feature 300 appears in row 5 alone."""

import numpy as np
import pytest

import dsgd_amd
import logistic_bound as lb
import logistic_ref as ref
import softmax_bound as sm

pytestmark = pytest.mark.gpu

N, DIM, LAM, LR = 600, 300, 1e-5, 0.5
COLS = "dsgd_lgl_cgrad_kernel"
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

# (form, T or C, the list form's gradient kernel): the wide topics at one T per group width (lgtw_group_width: TP <= 32, <= 64, beyond)
MODELS = [("il", 5, "dsgd_lg_topics_il_grad_kernel")] + [("wide", T, "dsgd_lg_topics_wide_grad_kernel") for T in (9, 40, 103)] + \
         [("softmax", C, "dsgd_lg_softmax_grad_kernel") for C in (5, 103)] + [("softmax_il", C, "dsgd_lg_softmax_il_grad_kernel") for C in (5, 12)]
# the lists' lengths per worker; every case is 3 steps in one call
LISTS = {"K3 uneven, a list of one row": (100, 37, 1), "K1": (150,), "K3 every row": (300, 200, 100), "K3 a row twice": (100, 37, 20)}


def matrix():
    d = dsgd_amd.synth.generate(N, seed=5, dim=DIM - 1, nnz_mean=20)
    rows = [dict(zip(d.col[a:b].tolist(), d.val[a:b].tolist())) for a, b in zip(d.row_ptr[:-1], d.row_ptr[1:])]
    rows[17] = {}
    rows[5][DIM] = 0.5
    m = dsgd_amd.synth.from_rows(DIM, [(r, 1) for r in rows])
    return (m.row_ptr, m.col, m.val, m.label)


def steps(lengths, twice):
    """three steps of len(lengths) lists without a repeated row; twice: the LAST step's last list ends on the first list's first row"""
    rng, flat = np.random.default_rng(len(lengths) + sum(lengths)), []
    for _ in range(3):
        flat.append(rng.permutation(N)[:sum(lengths)].astype(np.int32))
    if twice:
        flat[2][-1] = flat[2][0]
    return np.concatenate(flat), np.concatenate([[0], np.cumsum(list(lengths) * 3)]), [np.split(f, np.cumsum(lengths)[:-1]) for f in flat]


def setup(eng, form, n, W0):
    rng = np.random.default_rng(n)
    if form in ("il", "wide"):
        labels = rng.choice(np.array([-1, 1], dtype=np.int8), size=(n, N))
        eng.lg_topics_set(labels, interleaved=form == "il", wide=form == "wide")
    else:
        labels = rng.integers(0, n, size=N).astype(np.uint8)
        eng.lg_softmax_set(labels, n, interleaved=form == "softmax_il")
    eng.lg_topics_set_weights(W0)
    return labels


@pytest.fixture(scope="module")
def pair():
    csr = matrix()
    with dsgd_amd.Engine(DIM, LAM) as a, dsgd_amd.Engine(DIM, LAM) as b:
        for eng in (a, b):
            eng.load_csr(*csr)
        yield a, b, csr


@pytest.mark.parametrize("lengths", LISTS.values(), ids=LISTS.keys())
@pytest.mark.parametrize("model", MODELS, ids=lambda m: "%s-%d" % m[:2])
def test_bits_of_the_list_form(pair, model, lengths):
    (a, b, _), (form, n, list_kernel) = pair, model
    twice = lengths == LISTS["K3 a row twice"]
    idx, offsets, _ = steps(lengths, twice)
    W0 = (np.random.default_rng(n).standard_normal((n, DIM + 1)) * 0.3).astype(np.float32)
    softmax = form.startswith("softmax")
    step = (lambda e, **kw: e.lg_softmax_sync_steps(idx, offsets, 3, len(lengths), LR, **kw)) if softmax else \
           (lambda e, **kw: e.lg_topics_sync_steps(idx, offsets, 3, len(lengths), LR, **kw))
    loss = (lambda e: e.lg_softmax_loss_acc(0, N)) if softmax else (lambda e: tuple(map(bytes, e.lg_topics_loss_acc(0, N))))
    got = []
    for eng, kw in ((a, {}), (b, {"by_columns": True}), (b, {"by_columns": True})):   # (the second time: from the same weights, the same bits)
        setup(eng, form, n, W0)
        assert step(eng, **kw) == {"n_samples": len(idx), "n_active": len(idx)}
        got.append((bits(eng.lg_topics_get_weights()), loss(eng)))
    assert b.grad_kernel_name() == (list_kernel if twice else COLS)                    # what the LAST step took
    assert not np.array_equal(got[0][0], bits(W0))
    for w, l in got[1:]:
        assert np.array_equal(w, got[0][0]) and l == got[0][1]


@pytest.mark.parametrize("form", ("wide", "softmax_il"))
def test_against_fp64(pair, form):
    """one step of three lists from set weights, by columns, against numpy fp64: the bounds of the list forms' own tests"""
    _, eng, csr = pair
    n, lengths = 9, LISTS["K3 uneven, a list of one row"]
    idx, offsets, lists = steps(lengths, False)
    W0 = (np.random.default_rng(n).standard_normal((n, DIM + 1)) * 0.3).astype(np.float32)
    labels = setup(eng, form, n, W0)
    call = eng.lg_topics_sync_steps if form == "wide" else eng.lg_softmax_sync_steps
    call(idx[:offsets[3]], offsets[:4], 1, 3, LR, by_columns=True)
    assert eng.grad_kernel_name() == COLS
    W1 = eng.lg_topics_get_weights().astype(np.float64)
    if form == "wide":
        for t in range(n):
            csr_t = csr[:3] + (labels[t],)
            assert np.all(np.abs(W1[t] - ref.sync_step(csr_t, W0[t], lists[0], LR, LAM)) <= lb.dw(csr_t, W0[t], lists[0], LR, LAM)), t
    else:
        assert np.all(np.abs(W1 - sm.sync_step(csr, W0, labels, lists[0], LR, LAM)) <= sm.dw(csr, W0, labels, lists[0], LR, LAM))


@pytest.mark.parametrize("form", ("softmax", "softmax_il"))
def test_the_topics_call_on_classes_stays_one_vs_rest(pair, form):
    """every dsgd_lg_topics_* call serves classes as one-vs-rest on their one-hot planes: by columns too, a row named twice or not"""
    a, b, _ = pair
    idx, offsets, _ = steps(LISTS["K3 a row twice"], True)
    W0 = (np.random.default_rng(12).standard_normal((12, DIM + 1)) * 0.3).astype(np.float32)
    for eng, kw in ((a, {}), (b, {"by_columns": True})):
        setup(eng, form, 12, W0)
        eng.lg_topics_sync_steps(idx, offsets, 3, 3, LR, **kw)
    Wa = bits(a.lg_topics_get_weights())
    assert np.array_equal(Wa, bits(b.lg_topics_get_weights())) and not np.array_equal(Wa, bits(W0))
    b.lg_topics_sync_steps(idx[:offsets[3]], offsets[:4], 1, 3, LR, by_columns=True)
    assert b.grad_kernel_name() == COLS


def test_the_planar_form_is_refused(pair):
    _, eng, _ = pair
    W0 = np.ones((3, DIM + 1), dtype=np.float32)
    eng.lg_topics_set(np.ones((3, N), dtype=np.int8))
    eng.lg_topics_set_weights(W0)
    with pytest.raises(dsgd_amd.DsgdError) as e:
        eng.lg_topics_sync_steps(np.arange(4, dtype=np.int32), [0, 4], 1, 1, LR, by_columns=True)
    assert e.value.code == dsgd_amd._lib.EUNSUPPORTED and np.array_equal(bits(eng.lg_topics_get_weights()), bits(W0))
