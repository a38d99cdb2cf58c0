"""-m gpu: an epoch's steps in one call (dsgd_sync_steps_f64; csrc/dsgd_rp64.hpp "an epoch's steps in one call").

The call IS the loop of dsgd_sync_step_f64 calls: every comparison with the loop, between the fused form
(DSGD_RP64_FUSED=1: one launch per step, a grid-wide arrival between the two bodies) and the two-launch queue
(DSGD_RP64_FUSED=0), and between one call and the same steps cut into several calls is on BITS.  The column sums are
integers, so nothing here depends on the order of the adds or the shape of a launch.

Data: dsgd_amd.synth.generate at 23,149 rows (18,519 train rows: one worker's whole split puts blocks_per_worker at its
cap, every workgroup flushing the hot ranks) and at 4,096 rows where a Python oracle walks the rows.  Double data: the
synthetic float values times (1 + 1e-8 * N(0, 1)) in float64 -- full 53-bit mantissas no float holds, the idea of
tests/test_gpu_fp64_values.py's own data.

Against the oracle the bound is that of tests/test_gpu_fp64_requests.py for this family: equal active counts per step and
max|w - w_o| <= 1e-12 * max(1, |w_o|_inf) (the device's sums are exact; the oracle rounds per add).

The abort path (a workgroup that gives up its wait) is not driven here: it is a few lines in the shape of the column-slice
kernels' and is reviewed by reading."""

import ctypes as C
import os

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host
from oracle import oracle as orc
from oracle import ref_dict as rd
from oracle.backend import OracleBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
LR = 0.5
NEVER = lambda losses: False
BIG, BIG_TRAIN = 23149, 18519
SMALL, SMALL_TRAIN = 4096, 3276
_CACHE = {}


def _data(n_rows):
    if n_rows not in _CACHE:
        d = dsgd_amd.synth.generate(n_rows, seed=7)
        rng = np.random.default_rng(11)
        val64 = d.val.astype(np.float64) * (1.0 + 1e-8 * rng.standard_normal(len(d.val)))
        assert not np.array_equal(val64.astype(np.float32).astype(np.float64), val64)
        _CACHE[n_rows] = (d, val64)
    return _CACHE[n_rows]


def _engine(n_rows, n_train, double, fused=None, precision="fp64"):
    """fused: DSGD_RP64_FUSED as the context finds it at its creation (None: not set)"""
    d, val64 = _data(n_rows)
    old = os.environ.pop("DSGD_RP64_FUSED", None)
    try:
        if fused is not None:
            os.environ["DSGD_RP64_FUSED"] = "1" if fused else "0"
        eng = dsgd_amd.Engine(d.dim, LAM, precision=precision)
    finally:
        os.environ.pop("DSGD_RP64_FUSED", None)
        if old is not None:
            os.environ["DSGD_RP64_FUSED"] = old
    eng.load_csr(d.row_ptr, d.col, val64 if double else d.val, d.label)
    eng.build_dim_sparsity(n_train)
    return eng


def _served(fused, double):
    """dsgd_grad_kernel_name behind a sync_steps_f64 call whose every step took the one form"""
    return "dsgd_rp64%s_%s_kernel" % ("v" if double else "", "step" if fused else "grad")


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _flat(steps):
    """steps: per step a list (per worker) of index arrays -> idx, offsets, n_steps, n_workers"""
    lists = [np.asarray(a, np.int32) for s in steps for a in s]
    offs = np.zeros(len(lists) + 1, np.int64)
    offs[1:] = np.cumsum([len(a) for a in lists])
    return np.concatenate(lists), offs, len(steps), len(steps[0])


def _loop(eng, steps, lr=LR):
    act, tot = [], 0
    for s in steps:
        st = eng.sync_step_f64(s, lr)
        act.append(st["n_active"])
        tot += st["n_samples"]
    return act, tot


def _uniform_steps(n_steps, k, n, n_train, seed):
    rng = np.random.default_rng(seed)
    split = host.split_vanilla(n_train, k)
    return [[rng.permutation(np.asarray(r))[:n].astype(np.int32) for r in split] for _ in range(n_steps)]


def _mixed_steps(k, n_train, seed):
    """8 steps; per worker and step one of: 1 row, 100 rows, 700 rows, a list with duplicates, and ONCE a worker's list of
    all the 18,519 train rows (unequal lengths within and across the steps)"""
    rng = np.random.default_rng(seed)
    steps = []
    for s in range(8):
        lists = []
        for j in range(k):
            kind = (s + 2 * j) % 4
            if s == 3 and j == 0:
                a = rng.permutation(n_train)
            elif kind == 0:
                a = rng.integers(0, n_train, size=1)
            elif kind == 1:
                a = rng.permutation(n_train)[:100]
            elif kind == 2:
                a = rng.permutation(n_train)[:700]
            else:
                a = rng.choice(rng.permutation(n_train)[:50], size=200)   # every row about four times
                assert len(np.unique(a)) < len(a)
            lists.append(a.astype(np.int32))
        steps.append(lists)
    return steps


def _check_against_the_loop(steps, double, n_rows=BIG, n_train=BIG_TRAIN):
    """cases 1 - 3: the loop, the fused form and the two-launch queue from the same start"""
    idx, offs, n_steps, k = _flat(steps)
    with _engine(n_rows, n_train, double) as ref:
        act_ref, tot_ref = _loop(ref, steps)
        w_ref = ref.get_weights()
    assert np.any(w_ref != 0.0) and sum(act_ref) > 0
    for fused in (True, False):
        with _engine(n_rows, n_train, double, fused=fused) as eng:
            st = eng.sync_steps_f64(idx, offs, n_steps, k, LR, per_step=True)
            served = eng.grad_kernel_name()
            w = eng.get_weights()
        # which form served the steps: a fused engine that quietly took the pair would compare the queue with itself
        assert served == _served(fused, double), (fused, served)
        print("fused=%s: active per step %s (loop %s)" % (fused, st["active_per_step"].tolist(), act_ref))
        assert st["active_per_step"].tolist() == act_ref, fused
        assert st["n_samples"] == tot_ref == len(idx) and st["n_active"] == sum(act_ref), fused
        assert np.array_equal(_bits(w), _bits(w_ref)), (fused, int((_bits(w) != _bits(w_ref)).sum()))


@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_twenty_steps_of_3x100_are_the_loop(double):
    """1 (and 3): 20 steps of 3 x 100 -- weights, per-step active counts and totals of 20 sync_step_f64 calls"""
    _check_against_the_loop(_uniform_steps(20, 3, 100, BIG_TRAIN, 1), double)


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_mixed_lists_are_the_loop(double, k):
    """2 (and 3): 8 steps of 1 / 100 / 700 rows, duplicates and a whole split of 18,519 rows, K = 1 and K = 6"""
    _check_against_the_loop(_mixed_steps(k, BIG_TRAIN, 20 + k), double)


@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_split_invariance(double):
    """4: steps [0, 10) then [10, 20) in two calls are one call of 20"""
    steps = _uniform_steps(20, 3, 100, BIG_TRAIN, 4)
    with _engine(BIG, BIG_TRAIN, double, fused=True) as a, _engine(BIG, BIG_TRAIN, double, fused=True) as b:
        one = a.sync_steps_f64(*_flat(steps), LR, per_step=True)
        h1 = b.sync_steps_f64(*_flat(steps[:10]), LR, per_step=True)
        h2 = b.sync_steps_f64(*_flat(steps[10:]), LR, per_step=True)
        assert one["active_per_step"].tolist() == h1["active_per_step"].tolist() + h2["active_per_step"].tolist()
        assert one["n_active"] == h1["n_active"] + h2["n_active"] and one["n_samples"] == h1["n_samples"] + h2["n_samples"]
        assert np.array_equal(_bits(a.get_weights()), _bits(b.get_weights()))


def test_slice_major_weights_on_entry():
    """5: float data, the weights left slice-major by a small plan run with lr = 0 (as tests/fp64_world2_worker.py does): the
    call gives the bits of the per-call loop entered the same way and of an engine whose weights never left rank order, and the
    next gradient_f64(w = None) reads the same weights.  (The layout itself is not visible at the boundary: the per-call
    twin keeps it too, and every later call reads whichever it finds.)"""
    warm = _uniform_steps(3, 3, 100, BIG_TRAIN, 50)
    steps = _uniform_steps(6, 3, 100, BIG_TRAIN, 51)
    probe = np.random.default_rng(52).integers(0, BIG_TRAIN, size=333).astype(np.int32)
    out = []
    for mode in ("fused", "queue", "loop", "rank_order"):
        with _engine(BIG, BIG_TRAIN, False, fused=mode != "queue") as eng:
            _loop(eng, warm)
            w0 = eng.get_weights()
            if mode != "rank_order":
                p = eng.plan(warm)
                eng.plan_run(p, 0, len(warm), 0.0)
                eng.synchronize()
                p.destroy()
            if mode == "loop":
                act, _ = _loop(eng, steps)
            else:
                act = eng.sync_steps_f64(*_flat(steps), LR, per_step=True)["active_per_step"].tolist()
            g, st = eng.gradient_f64(probe)
            out.append((act, _bits(eng.get_weights()), _bits(g), st))
            assert not np.array_equal(_bits(w0), out[-1][1])
    for other in out[1:]:
        assert out[0][0] == other[0] and out[0][3] == other[3]
        assert np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])


@pytest.mark.parametrize("k", [3, 6])
def test_float_data_against_the_oracle(k):
    """6: 20 steps of K x 100 on float data against oracle.Oracle.sync_step"""
    d, _ = _data(BIG)
    o = orc.Oracle(d.dim, d.row_ptr, d.col, d.val, d.label, LAM)
    o.set_dim_sparsity(o.dim_sparsity(BIG_TRAIN))
    steps = _uniform_steps(20, k, 100, BIG_TRAIN, 60 + k)
    w_o = np.zeros(d.dim + 1)
    act_o = []
    for s in steps:
        o.sync_step(w_o, s, LR)
        act_o.append(o.last_stats["n_active"])
    with _engine(BIG, BIG_TRAIN, False) as eng:
        st = eng.sync_steps_f64(*_flat(steps), LR, per_step=True)
        w = eng.get_weights()
    err, tol = np.abs(w - w_o).max(), 1e-12 * max(1.0, np.abs(w_o).max())
    print("K = %d: max|w - w_o| = %.3e (tol %.1e)" % (k, err, tol))
    assert st["active_per_step"].tolist() == act_o
    assert err <= tol


def _ref_dict_model(n_rows, n_train):
    key = ("rd", n_rows)
    if key not in _CACHE:
        d, val64 = _data(n_rows)
        data = [(rd.Sparse({int(c): float(v) for c, v in zip(d.col[d.row_ptr[i]:d.row_ptr[i + 1]], val64[d.row_ptr[i]:d.row_ptr[i + 1]])},
                           d.dim + 1), int(d.label[i])) for i in range(n_rows)]
        _CACHE[key] = (data, rd.SparseSVM(LAM, rd.dim_sparsity(data[:n_train])))
    return _CACHE[key]


def _dense(sp, dp):
    out = np.zeros(dp)
    for kk, v in sp.map.items():
        out[kk] = v
    return out


def _sparse(w):
    return rd.Sparse({int(kk): float(w[kk]) for kk in np.flatnonzero(w)}, len(w))


def _active(data, w, idx):
    return sum(1 for i in idx if not (data[i][1] * data[i][0].dot(w) < 0))


def test_double_data_against_ref_dict():
    """6: 20 steps of 3 x 100 on Double data against oracle/ref_dict.py on the doubles"""
    d, _ = _data(SMALL)
    data, model = _ref_dict_model(SMALL, SMALL_TRAIN)
    steps = _uniform_steps(20, 3, 100, SMALL_TRAIN, 66)
    w_ref = rd.Sparse({}, d.dim + 1)
    act_o = []
    for s in steps:
        act_o.append(sum(_active(data, w_ref, l.tolist()) for l in s))
        w_ref = rd.master_sync_step(model, data, w_ref, [l.tolist() for l in s], LR)
    w_o = _dense(w_ref, d.dim + 1)
    with _engine(SMALL, SMALL_TRAIN, True) as eng:
        st = eng.sync_steps_f64(*_flat(steps), LR, per_step=True)
        w = eng.get_weights()
    err, tol = np.abs(w - w_o).max(), 1e-12 * max(1.0, np.abs(w_o).max())
    print("ref_dict: max|w - w_o| = %.3e (tol %.1e)" % (err, tol))
    assert st["active_per_step"].tolist() == act_o
    assert err <= tol


def test_three_hundred_calls_on_one_context():
    """7: 300 calls of 2 steps on one context -- the arrival counter only grows; the bits of the 600-call loop"""
    steps = _uniform_steps(600, 3, 100, SMALL_TRAIN, 7)
    with _engine(SMALL, SMALL_TRAIN, False, fused=True) as a, _engine(SMALL, SMALL_TRAIN, False) as b:
        act = []
        for c in range(300):
            act += a.sync_steps_f64(*_flat(steps[2 * c:2 * c + 2]), LR, per_step=True)["active_per_step"].tolist()
            assert a.grad_kernel_name() == _served(True, False)
        act_ref, _ = _loop(b, steps)
        assert act == act_ref
        assert np.array_equal(_bits(a.get_weights()), _bits(b.get_weights()))


def _code(call):
    with pytest.raises(_lib.DsgdError) as e:
        call()
    return e.value.code


def test_refusals_change_nothing():
    """8: every refusal leaves the weights' bits, and the next call works"""
    steps = _uniform_steps(5, 3, 100, SMALL_TRAIN, 8)
    idx, offs, n_steps, k = _flat(steps)
    with _engine(SMALL, SMALL_TRAIN, False, precision="fp32") as e32:
        assert _code(lambda: e32.sync_steps_f64(idx, offs, n_steps, k, LR)) == _lib.ESTATE
    with _engine(SMALL, SMALL_TRAIN, False) as eng:
        _loop(eng, steps[:2])
        w0 = _bits(eng.get_weights())

        def raw(idx_, n_idx, offs_, n_steps_, k_):
            return eng._lib.dsgd_sync_steps_f64(eng._ctx, _lib.ptr(idx_), C.c_int64(n_idx), _lib.ptr(offs_), C.c_int64(n_steps_), C.c_int32(k_),
                                                C.c_double(LR), None, None)

        down = offs.copy()
        down[4] = down[3] - 1                       # offsets that decrease
        short = offs.copy()
        short[-1] -= 1                              # ... that do not end at n_idx
        empty = offs.copy()
        empty[7] = empty[6]                         # an empty list in step 2: the per-call function's answer
        bad_row = idx.copy()
        bad_row[offs[4 * k + 1]] = SMALL            # row index == n_rows in the LAST step: the per-call function's code
        per_call_empty = _code(lambda: eng.sync_step_f64([steps[0][0], steps[0][1][:0], steps[0][2]], LR))
        per_call_row = _code(lambda: eng.sync_step_f64([np.asarray([SMALL], np.int32)] + steps[0][1:], LR))
        assert (per_call_empty, per_call_row) == (_lib.EINVAL, _lib.ERANGE)
        for what, rc, want in (("offsets decrease", raw(idx, len(idx), down, n_steps, k), _lib.EINVAL),
                               ("offsets end early", raw(idx, len(idx), short, n_steps, k), _lib.EINVAL),
                               ("no steps", raw(idx, len(idx), offs, 0, k), _lib.EINVAL),
                               ("no workers", raw(idx, len(idx), offs, n_steps, 0), _lib.EINVAL),
                               ("null idx", raw(None, len(idx), offs, n_steps, k), _lib.EINVAL),
                               ("null offsets", raw(idx, len(idx), None, n_steps, k), _lib.EINVAL),
                               ("an empty list", raw(idx, len(idx), empty, n_steps, k), per_call_empty),
                               ("row == n_rows in the last step", raw(bad_row, len(idx), offs, n_steps, k), per_call_row)):
            assert rc == want, what
            assert np.array_equal(_bits(eng.get_weights()), w0), what
        # real RCCL attached at world = 1 (as tests/test_gpu_fp64_values.py attaches it): the per-step call stays the path
        eng.comm_init_f64(dsgd_amd.Engine.comm_unique_id(), 1, 0)
        try:
            assert _code(lambda: eng.sync_steps_f64(idx, offs, n_steps, k, LR)) == _lib.EUNSUPPORTED
            assert np.array_equal(_bits(eng.get_weights()), w0)
        finally:
            eng.comm_destroy()
        # the next call works, and is the loop
        st = eng.sync_steps_f64(*_flat(steps[2:]), LR, per_step=True)
        with _engine(SMALL, SMALL_TRAIN, False) as ref:
            act_ref, _ = _loop(ref, steps)
            assert st["active_per_step"].tolist() == act_ref[2:]
            assert np.array_equal(_bits(eng.get_weights()), _bits(ref.get_weights()))


class _RefDictOracle:
    """ref_dict behind the surface oracle.backend.OracleBackend drives (sync_step, loss_acc)"""

    def __init__(self, data, model, dim):
        self.data, self.model, self.dim, self.lam = data, model, dim, model.lam
        self.last_stats = {"min_abs_margin": 0.0, "n_active": 0}

    def sync_step(self, w, lists, lr):
        ws = _sparse(w)
        self.last_stats = {"min_abs_margin": 0.0, "n_active": sum(_active(self.data, ws, [int(i) for i in l]) for l in lists)}
        w[:] = _dense(rd.master_sync_step(self.model, self.data, ws, [[int(i) for i in l] for l in lists], lr), len(w))

    def loss_acc(self, w, lo, hi):
        ws = _sparse(w)
        part = self.data[lo:hi]
        c = [0, 0, 0]
        for x, y in part:
            p_ = self.model.forward(ws, x)
            c[0 if p_ == y else (1 if p_ == 0 else 2)] += 1
        n = float(hi - lo)
        return self.lam * float(np.sum(w * w)) + (c[1] + 2.0 * c[2]) / n, c[0] / n, c, 0.0


def _fit(backend, dp):
    m = host.MasterSync(backend, SMALL_TRAIN, SMALL, node_count=3, rnd=host.JavaRandom(0))
    s = m.fit(np.zeros(dp), 2, 100, 0.5, NEVER)
    return m, s


def test_master_sync_fit_on_double_data(monkeypatch):
    """9: host.MasterSync.fit, 2 epochs of 3 x 100 on Double data: one sync_steps_f64 call per epoch (DSGD_F64_STEPS=1) and the
    per-step loop (DSGD_F64_STEPS=0) leave the same bits, and the accuracies are the ref_dict oracle's"""
    d, _ = _data(SMALL)
    data, model = _ref_dict_model(SMALL, SMALL_TRAIN)
    ref, s_ref = _fit(OracleBackend(_RefDictOracle(data, model, d.dim)), d.dim + 1)
    got = {}
    for knob in ("1", "0", None):
        if knob is None:
            monkeypatch.delenv("DSGD_F64_STEPS", raising=False)
        else:
            monkeypatch.setenv("DSGD_F64_STEPS", knob)
        with _engine(SMALL, SMALL_TRAIN, True) as eng:
            calls = []
            real = eng.sync_steps_f64
            eng.sync_steps_f64 = lambda *a, **kw: (calls.append(a[2]), real(*a, **kw))[1]
            m, _ = _fit(eng, d.dim + 1)
            got[knob] = (_bits(eng.get_weights()), m.accs, m.test_accs, m.steps_run, len(calls))
            w = eng.get_weights()
    assert got["1"][4] == 2 and got["0"][4] == 0   # one call per epoch / none
    for knob in ("0", None):
        assert np.array_equal(got["1"][0], got[knob][0]) and got["1"][1:4] == got[knob][1:4]
    assert got["1"][3] == ref.steps_run
    assert got["1"][1] == ref.accs and got["1"][2] == ref.test_accs
    assert np.abs(w - s_ref.grad).max() <= 1e-12 * max(1.0, np.abs(s_ref.grad).max())
