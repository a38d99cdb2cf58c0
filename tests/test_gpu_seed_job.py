"""-m gpu: the job form of the device-drawn epoch plans (dsgd_plan_create_from_seed_job / _rp64, include/dsgd.h;
dsgd_jr_slice_job_kernel, csrc/dsgd_shuffle.hpp) against csrc/jrand.c (host.epoch_lists(native=True) over the JOB's splits,
pinned to the JVM's generator by tests/test_host_mirror.py): the lists of every window of a job entry for entry, the step
count, the generator's state and the draws identical over all windows; batches beyond 1,024 rows (chunks of 1,024); shuffles
of more than 64 rejected raw values (2^20 rows); the plans run like plans of the host's lists; refusals leave nothing
behind; accepted under a communicator where the old form stays refused.

The lists do not depend on the rows' contents.  A rank's expected lists are the job's lists of its workers with the job's
placement taken off and its own split_begin put on."""

import ctypes as C

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
N_ROWS, N_TRAIN = 23149, 18519
MAX_LEN = 1 << 20                      # JR_MAX_LEN
OLD_MAX_REJ, MAX_REJ = 64, 512         # JR_MAX_REJ, JR_JOB_MAX_REJ
STATE0 = host.JavaRandom(0).seed       # Main.scala:32 (tests/test_gpu_shuffle_large.py's)
STATE1 = host.JavaRandom(20190520).seed


def _job_split(lens):
    out, at = [], 0
    for ln in lens:
        out.append(range(at, at + ln))
        at += ln
    return out


_HOST = {}


def host_job(state, lens, max_samples, batch):
    """csrc/jrand.c over the job: ([step][worker] -> positions inside the worker's split), n_steps, the state behind the epoch,
    the raw values drawn (counted by the sequential shuffle: len - 1 + rejections each) and the rejections of every shuffle.
    Computed once per case and left unchanged."""
    key = (state, tuple(lens), max_samples, batch)
    if key not in _HOST:
        split = _job_split(lens)
        rnd = host.JavaRandom(0)
        rnd.seed = state
        idx, offs, n = host.epoch_lists(rnd, split, max_samples, batch, native=True)
        lists = [[idx[offs[s * len(lens) + j]:offs[s * len(lens) + j + 1]].astype(np.int64) - split[j].start for j in range(len(lens))]
                 for s in range(n)]
        lib = host._host_lib()
        assert lib is not None, "libdsgd_host.so is not built"
        st, draws, rej = C.c_uint64(state), 0, []
        for _ in range(n):
            for ln in lens:
                buf = np.arange(ln, dtype=np.int32)
                d = int(lib.dsgd_jrand_shuffle(C.byref(st), _lib.ptr(buf), C.c_int64(ln)))
                draws += d
                rej.append(d - (ln - 1))
        assert st.value == rnd.seed   # (the two routes of csrc/jrand.c agree: the count belongs to these lists)
        _HOST[key] = (lists, n, rnd.seed, draws, rej)
    return _HOST[key]


def expected(lists, first, begins):
    """the window's lists flat (step-major, worker-minor) with the hosted workers' own placement, and their offsets"""
    flat = [lists[s][first + i] + begins[i] for s in range(len(lists)) for i in range(len(begins))]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64)
    return (np.concatenate(flat).astype(np.int32) if flat else np.zeros(0, np.int32)), offs


def check_window(eng, state, lens, first, begins, max_samples, batch, rp64=False, keep=False):
    lists, n_h, state_h, draws_h, _ = host_job(state, lens, max_samples, batch)
    plan, n_d, state_d, draws_d = eng.plan_from_seed_job(state, lens, first, begins, max_samples, batch, rp64=rp64)
    assert plan is not None and n_d == n_h and state_d == state_h and draws_d == draws_h, (first, len(begins), n_d, n_h, draws_d, draws_h)
    idx_h, offs_h = expected(lists, first, begins)
    idx_d, offs_d = eng.plan_lists(plan)
    assert np.array_equal(offs_d, offs_h)
    assert np.array_equal(idx_d, idx_h), "window (%d, %d): first differing entry %d" % (first, len(begins), int(np.flatnonzero(idx_d != idx_h)[0]))
    if keep:
        return plan, idx_h, offs_h, n_h
    plan.destroy()
    return n_d, state_d, draws_d


def _engine(data, val=None, fp64=False):
    eng = dsgd_amd.Engine(data.dim, LAM, precision="fp64") if fp64 else dsgd_amd.Engine(data.dim, LAM)
    eng.load_csr(data.row_ptr, data.col, data.val if val is None else val, data.label)
    eng.build_dim_sparsity(N_TRAIN)
    return eng


@pytest.fixture(scope="module")
def small():
    return dsgd_amd.synth.generate(N_ROWS, seed=3)


@pytest.fixture(scope="module")
def doubles(small):
    rng = np.random.default_rng(78)
    return small.val.astype(np.float64) * (1.0 + rng.random(len(small.val)) * 2.0 ** -20)   # (not float-representable)


@pytest.fixture(scope="module")
def ctx(small):
    with _engine(small) as eng:
        yield eng


@pytest.fixture(scope="module")
def ctx64(small):
    with _engine(small, small.val.astype(np.float32), fp64=True) as eng:
        yield eng


@pytest.fixture(scope="module")
def ctx64v(small, doubles):
    with _engine(small, doubles, fp64=True) as eng:
        assert eng.value_bits() == 64
        yield eng


@pytest.fixture(scope="module")
def long_ctx():
    """2^20 + 64 rows of one to four entries, as tests/test_gpu_shuffle_large.py's"""
    data = dsgd_amd.synth.generate(MAX_LEN + 64, seed=3, dim=1000, nnz_mean=4)
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(MAX_LEN)
        yield eng


# ---- 1: every window of a job ----
JOB = (1000, 1001, 777, 1024)


def test_every_window_of_a_job_draws_the_hosts_lists(ctx):
    """8 steps of batch 100 (the third worker's last slice is 77 rows); the hosted splits lie in REVERSE order inside the loaded
    rows, 7 rows off the start: the mapping is by split_begin, not by prefix sums"""
    batch, max_samples = 100, 800
    lists, n_h, _, _, _ = host_job(STATE1, JOB, max_samples, batch)
    assert n_h == 8 and len(lists[7][2]) == 77
    seen = set()
    for first in range(len(JOB)):
        for n_local in range(1, len(JOB) - first + 1):
            lens = JOB[first:first + n_local]
            begins = [7 + sum(lens[i + 1:]) for i in range(n_local)]
            if n_local > 1:
                assert begins != sorted(begins) and begins != [sum(JOB[:first + i]) for i in range(n_local)]
            seen.add(check_window(ctx, STATE1, JOB, first, begins, max_samples, batch))
    assert len(seen) == 1   # n_steps, *jstate and *draws_out: the job's, whatever the window


# ---- 2: the whole job hosted = the old form ----
@pytest.mark.parametrize("lens", [(6173, 6173, 6173), (6173, 6150, 6173)])
def test_the_whole_job_hosted_is_the_old_form(ctx, ctx64, lens):
    """3 x 100 over splits of 6,173 rows: 62 steps, the last slice 73 rows (50 for the shorter split of the second case)"""
    split = _job_split(lens)
    begins = [r.start for r in split]
    for eng, rp64 in ((ctx, False), (ctx64, True)):
        old, n_o, state_o, draws_o = eng.plan_from_seed(STATE1, split, max(lens), 100, rp64=rp64)
        new, idx_h, offs_h, n_h = check_window(eng, STATE1, lens, 0, begins, max(lens), 100, rp64=rp64, keep=True)
        _, _, state_h, draws_h, _ = host_job(STATE1, lens, max(lens), 100)
        assert (n_o, state_o, draws_o) == (n_h, state_h, draws_h) and n_o == 62
        idx_o, offs_o = eng.plan_lists(old)
        assert np.array_equal(offs_o, offs_h) and np.array_equal(idx_o, idx_h)
        assert int(offs_h[-1] - offs_h[-2]) == 73 and int(offs_h[-2] - offs_h[-3]) == min(lens) - 6100
        assert old.info()["kind"] == new.info()["kind"]
        old.destroy()
        new.destroy()


# ---- 3: batches beyond 1,024 rows ----
@pytest.mark.parametrize("batch", [2500, 1025, 1024])
def test_batches_beyond_1024_rows(ctx, batch):
    """splits of 6,000 and 5,999 rows.  Batch 2,500: chunks of 1,024 + 1,024 + 452, the third step takes 1,000 and 999 rows;
    batch 1,025: chunks of 1,024 + 1; batch 1,024: one chunk.  FAILS WITHOUT THE FEATURE: the old form refuses batches
    beyond 1,024 rows and there is no other device draw."""
    lens = (6000, 5999)
    split = _job_split(lens)
    lists, n_h, _, _, _ = host_job(STATE1, lens, 6000, batch)
    assert n_h == -(-5999 // batch)
    if batch == 2500:
        assert [len(x) for x in lists[2]] == [1000, 999]
    check_window(ctx, STATE1, lens, 0, [r.start for r in split], 6000, batch)
    check_window(ctx, STATE1, lens, 1, [11], 6000, batch)
    if batch > 1024:
        with pytest.raises(dsgd_amd.DsgdError) as ei:
            ctx.plan_from_seed(STATE1, split, 6000, batch)
        assert ei.value.code == _lib.EUNSUPPORTED


# ---- 4: more than 64 rejections inside a shuffle ----
LONG_CASES = [(MAX_LEN,), (MAX_LEN, MAX_LEN - 5)]


def test_the_long_cases_sit_between_the_old_limit_and_the_new():
    """the CPU part: every shuffle of the cases below has more than 64 and at most 512 rejected raw values"""
    for lens in LONG_CASES:
        _, n, _, _, rej = host_job(STATE0, lens, 800, 100)
        assert n == 8 and len(rej) == 8 * len(lens)
        assert OLD_MAX_REJ < min(rej) and max(rej) <= MAX_REJ, rej
    assert min(host_job(STATE0, LONG_CASES[0], 800, 100)[4]) == 103 and max(host_job(STATE0, LONG_CASES[0], 800, 100)[4]) == 137


@pytest.mark.parametrize("lens", LONG_CASES)
def test_splits_of_2_pow_20_rows(long_ctx, lens):
    """one worker of 2^20 rows, and a job of (2^20, 2^20 - 5) rows traced one worker at a time (the context holds 2^20 + 64)"""
    seen = {check_window(long_ctx, STATE0, lens, first, [3 * first], 800, 100) for first in range(len(lens))}
    assert len(seen) == 1
    if len(lens) == 1:
        with pytest.raises(dsgd_amd.DsgdError) as ei:
            long_ctx.plan_from_seed(STATE0, _job_split(lens), 800, 100)
        assert ei.value.code == _lib.EUNSUPPORTED and "rejections inside one shuffle" in str(ei.value)


# ---- 6: the plans run ----
def _run(eng, plan, n_steps, w0):
    eng.set_weights(w0)
    eng.plan_run(plan, 0, n_steps, 0.5)
    st = eng.synchronize()
    out = (eng.get_weights(), st, plan.info()["kind"])
    plan.destroy()
    return out


def _same_bits(a, b):
    assert a[0].dtype == b[0].dtype and np.abs(a[0]).max() > 0
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8))
    assert a[1] == b[1] and a[1]["n_samples"] > 0 and a[2] == b[2]


def test_an_fp32_job_plan_runs_like_the_plan_of_its_lists(ctx, small):
    """the window first = 1, n_local = 2 of the job of test 1, against plan_flat of the same lists on a twin engine"""
    begins = [2000, 100]
    plan, idx_h, offs_h, n_h = check_window(ctx, STATE1, JOB, 1, begins, 800, 100, keep=True)
    w0 = np.zeros(small.dim + 1, dtype=np.float32)
    got = _run(ctx, plan, n_h, w0)
    with _engine(small) as twin:
        want = _run(twin, twin.plan_flat(idx_h, offs_h, n_h, 2), n_h, w0)
    _same_bits(got, want)


@pytest.mark.parametrize("double_data", [False, True])
def test_an_rp64_job_plan_runs_like_the_plan_of_its_lists(ctx64, ctx64v, small, doubles, double_data):
    eng = ctx64v if double_data else ctx64
    begins = [2000, 100]
    plan, idx_h, offs_h, n_h = check_window(eng, STATE1, JOB, 1, begins, 800, 100, rp64=True, keep=True)
    w0 = np.zeros(small.dim + 1)
    got = _run(eng, plan, n_h, w0)
    with _engine(small, doubles if double_data else small.val.astype(np.float32), fp64=True) as twin:
        want = _run(twin, twin.plan_flat(idx_h, offs_h, n_h, 2, rp64=True), n_h, w0)
    _same_bits(got, want)


# ---- 7: refusals leave nothing behind ----
def _raw(eng, lens, first, begins, max_samples=800, batch=100, rp64=False, state=STATE1):
    jl, sb = np.asarray(lens, np.int64), np.asarray(begins, np.int64)
    st, h, n_steps, draws = C.c_uint64(state), C.c_void_p(0x5A5A5A5A), C.c_int64(-1), C.c_int64(-1)
    fn = eng._lib.dsgd_plan_create_from_seed_job_rp64 if rp64 else eng._lib.dsgd_plan_create_from_seed_job
    rc = fn(eng._ctx, C.byref(st), _lib.ptr(jl), len(jl), first, len(sb), _lib.ptr(sb), max_samples, batch, C.byref(h), C.byref(n_steps),
            C.byref(draws))
    return rc, st.value, h.value, n_steps.value, draws.value, eng._lib.dsgd_last_error().decode("utf-8", "replace")


def test_refusals_leave_nothing_behind(ctx, ctx64v):
    good = lambda eng, rp64=False: check_window(eng, STATE1, JOB, 1, [2000, 100], 800, 100, rp64=rp64)   # noqa: E731
    # beyond the limits: nothing drawn, the state untouched, no plan, no steps
    rc, state, handle, n_steps, draws, msg = _raw(ctx, (MAX_LEN + 1, 1000), 1, [0])
    assert rc == _lib.EUNSUPPORTED and "splits up to %d rows" % MAX_LEN in msg, (rc, msg)
    assert state == STATE1 and handle is None and n_steps == 0 and draws == 0
    good(ctx)
    # DSGD_EINVAL: n_job < 1, n_local < 1, first < 0, first + n_local > n_job, a job_len < 1, a negative split_begin -- and null pointers
    for lens, first, begins in (((), 0, [0]), (JOB, 0, []), (JOB, -1, [0]), (JOB, 3, [0, 2000]), (JOB, 4, [0]), ((1000, 0), 0, [0]),
                                ((1000, -5), 0, [0]), (JOB, 1, [0, -1])):
        rc, state, handle, _, _, msg = _raw(ctx, lens, first, begins)
        assert rc == _lib.EINVAL, (lens, first, begins, rc, msg)
        assert state == STATE1 and handle in (None, 0x5A5A5A5A)
        good(ctx)
    jl, sb = np.asarray(JOB, np.int64), np.asarray([0], np.int64)
    st, h, n = C.c_uint64(STATE1), C.c_void_p(), C.c_int64()
    fn = ctx._lib.dsgd_plan_create_from_seed_job
    for args in ((None, _lib.ptr(jl), 4, 0, 1, _lib.ptr(sb), 800, 100, C.byref(h), C.byref(n), None),
                 (C.byref(st), None, 4, 0, 1, _lib.ptr(sb), 800, 100, C.byref(h), C.byref(n), None),
                 (C.byref(st), _lib.ptr(jl), 4, 0, 1, None, 800, 100, C.byref(h), C.byref(n), None),
                 (C.byref(st), _lib.ptr(jl), 4, 0, 1, _lib.ptr(sb), 800, 100, None, C.byref(n), None),
                 (C.byref(st), _lib.ptr(jl), 4, 0, 1, _lib.ptr(sb), 800, 100, C.byref(h), None, None),
                 (C.byref(st), _lib.ptr(jl), 4, 0, 1, _lib.ptr(sb), 800, 0, C.byref(h), C.byref(n), None)):
        assert fn(ctx._ctx, *args) == _lib.EINVAL and st.value == STATE1
    # DSGD_ERANGE: a hosted split ends beyond the rows loaded (the OTHER workers' rows are nowhere: not looked at)
    rc, state, handle, n_steps, draws, msg = _raw(ctx, JOB, 1, [0, N_ROWS - 776])
    assert rc == _lib.ERANGE and state == STATE1 and handle is None and n_steps == 0 and draws == 0, (rc, msg)
    good(ctx)
    check_window(ctx, STATE1, JOB, 2, [N_ROWS - 777], 800, 100)   # (... and up to the last row is inside)
    # the value-type and precision rules of the twins
    rc, state, handle, _, _, msg = _raw(ctx64v, JOB, 1, [2000, 100])
    assert rc == _lib.EUNSUPPORTED and "Double feature values" in msg and state == STATE1
    good(ctx64v, rp64=True)
    rc, state, handle, _, _, msg = _raw(ctx, JOB, 1, [2000, 100], rp64=True)
    assert rc == _lib.ESTATE and "fp64 context" in msg and state == STATE1
    good(ctx)


# ---- 8: under a communicator, in process ----
def test_accepted_under_a_communicator_where_the_old_form_is_refused(small):
    """real RCCL at world = 1 (tests/test_gpu_fp64_rank_plans.py::test_real_rccl_world_1_equals_no_communicator's way): the job
    form creates its row-parallel plan attached and the collective run gives the bits of the same plan with no communicator"""
    lens = (6173, 6173, 6173)
    split = _job_split(lens)
    w0 = np.zeros(small.dim + 1)
    w0[1:2001] = np.random.default_rng(79).normal(size=2000) * 0.01
    res = []
    for attach in (False, True):
        with dsgd_amd.Engine(small.dim, LAM, precision="fp64") as eng:
            eng.load_csr(small.row_ptr, small.col, small.val.astype(np.float32), small.label)
            if attach:
                eng.comm_init_f64(dsgd_amd.Engine.comm_unique_id(), 1, 0)
            eng.build_dim_sparsity(N_TRAIN)
            if attach:
                with pytest.raises(dsgd_amd.DsgdError) as ei:
                    eng.plan_from_seed(STATE1, split, 1200, 100, rp64=True)
                assert ei.value.code == _lib.EUNSUPPORTED
            plan, _, _, n_h = check_window(eng, STATE1, lens, 0, [r.start for r in split], 1200, 100, rp64=True, keep=True)
            assert n_h == 12
            res.append(_run(eng, plan, n_h, w0))
            if attach:
                eng.comm_destroy()
    assert np.array_equal(res[0][0].view(np.uint64), res[1][0].view(np.uint64)) and res[0][1] == res[1][1]
    assert res[0][1]["n_samples"] == 12 * 300 and not np.array_equal(res[0][0], w0)
