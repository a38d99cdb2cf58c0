"""Device-drawn lists (dsgd_plan_create_from_seed, csrc/dsgd_shuffle.hpp) on LONG splits.

dsgd_jr_slice_kernel keeps a bitmap of the split in dynamic LDS: len / 8 + 16,656 bytes (jr_slice_lds_bytes), beyond 64 KiB
from 391,041 rows on, up to 147,728 bytes at JR_MAX_LEN = 2^20 rows.  tests/test_gpu_shuffle.py stops at 214,510 rows (43 KB).
Here: splits of 391,041 .. 524,288 rows against csrc/jrand.c (host.epoch_lists(native=True), pinned to the JVM's generator by
tests/test_host_mirror.py) -- lists, step counts, generator state --, the refusals of the same route and what they leave
behind, and host.MasterSync falling back to the host's generator where the device form refuses.

The lists do not depend on the rows' contents: the rows are cheap (dim 1,000, ~4 non-zeros), and max_samples = 8 * batch
draws 8 steps per worker, not an epoch.

A shuffle of more than JR_MAX_REJ = 64 rejected raw values is outside the device form (expected len^2 / 2^33 per shuffle).
Counted on the CPU with csrc/jrand.c's sequential shuffle for the generator state used here (java.util.Random(0),
Main.scala:32), the largest count of any shuffle of a case (test_rejections_inside_one_shuffle_for_the_states_used_here):
    one split of 400,000 rows, 8 steps                  25
    splits of 500,000 and 391,041 rows, 8 steps         34
    one split of 524,288 rows, 8 steps                  36
    one split of 2^20 rows, 8 steps                    103 .. 137 (every shuffle beyond the limit)
so the first three MUST be served by the device (-7 there is a failure) and the last must be refused."""

import ctypes as C

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import _lib, host

gpu = pytest.mark.gpu
device = pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")

LAM = 1e-5
MAX_LEN = 1 << 20                      # JR_MAX_LEN
MAX_REJ = 64                           # JR_MAX_REJ
LDS_64K_LEN = 391041                   # the first length whose bitmap takes the slice kernel beyond 64 KiB of LDS
N_TRAIN = MAX_LEN
N_ROWS = N_TRAIN + 64
STEPS = 8
STATE0 = host.JavaRandom(0).seed       # Main.scala:32

# (lengths of the splits, batch): the success cases
CASES = [((400000,), 100), ((500000, LDS_64K_LEN), 1024), ((524288,), 100)]
LARGEST_REJ = {CASES[0]: 25, CASES[1]: 34, CASES[2]: 36}


def _split(lens):
    out, at = [], 0
    for ln in lens:
        out.append(range(at, at + ln))
        at += ln
    return out


def _lds_bytes(length):
    """jr_slice_lds_bytes: the bitmap + wanted[1024] + karr[1024] + hits[2048] + rej[64] + 4 words"""
    return 4 * (((length + 31) >> 5) + 1024 + 1024 + 2048 + 64 + 4)


# ---- the CPU part: which of these streams the device form has to serve ----
def _rejections(state, lens, n_steps):
    """rejected raw values of every shuffle of n_steps steps, in the stream's order (csrc/jrand.c, sequentially)"""
    lib = host._host_lib()
    assert lib is not None, "libdsgd_host.so is not built"
    st = C.c_uint64(state)
    out = []
    for _ in range(n_steps):
        for ln in lens:
            buf = np.arange(ln, dtype=np.int32)
            out.append(int(lib.dsgd_jrand_shuffle(C.byref(st), _lib.ptr(buf), C.c_int64(ln))) - (ln - 1))
    return out


def test_rejections_inside_one_shuffle_for_the_states_used_here():
    assert _lds_bytes(LDS_64K_LEN - 1) <= 65536 < _lds_bytes(LDS_64K_LEN) and _lds_bytes(MAX_LEN) == 147728
    for case in CASES:
        lens, _ = case
        rej = _rejections(STATE0, lens, STEPS)
        assert max(rej) == LARGEST_REJ[case] <= MAX_REJ, (lens, rej)
        # (expected len^2 / 2^33 each, spread about its square root: these are ordinary streams, not lucky ones)
        for ln, r in zip(lens * STEPS, rej):
            assert abs(r - ln * ln / 2.0 ** 33) < 6 * (ln * ln / 2.0 ** 33) ** 0.5, (ln, r)
    rej = _rejections(STATE0, (MAX_LEN,), STEPS)
    assert min(rej) == 103 and max(rej) == 137   # every one of them refuses the epoch


# ---- one context for the module: 2^20 + 64 cheap rows ----
@pytest.fixture(scope="module")
def ctx():
    data = dsgd_amd.synth.generate(N_ROWS, seed=3, dim=1000, nnz_mean=4)
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(N_TRAIN)
        yield data, eng


def _host_lists(state, split, batch):
    rnd = host.JavaRandom(0)
    rnd.seed = state
    idx, offs, n = host.epoch_lists(rnd, split, STEPS * batch, batch, native=True)
    return idx, offs, n, rnd.seed


def _device_equals_host(eng, state, split, batch):
    """the comparison of tests/test_gpu_shuffle.py's both(): offsets and lists entry for entry, step count, generator state.
    Returns the plan and the host's lists."""
    idx_h, offs_h, n_h, state_h = _host_lists(state, split, batch)
    plan, n_d, state_d, draws = eng.plan_from_seed(state, split, STEPS * batch, batch)   # (DsgdError -7: the test fails)
    assert plan is not None and n_d == n_h == STEPS
    idx_d, offs_d = eng.plan_lists(plan)
    assert np.array_equal(offs_d, offs_h)
    assert np.array_equal(idx_d, idx_h), "first differing entry %d" % int(np.flatnonzero(idx_d != idx_h)[0])
    assert state_d == state_h
    nominal = STEPS * sum(len(r) - 1 for r in split)
    assert nominal < draws <= nominal + STEPS * len(split) * MAX_REJ          # (the rejections were there to be handled)
    return plan, (idx_h, offs_h, n_h)


@gpu
@device
@pytest.mark.parametrize("lens,batch", CASES)
def test_long_splits_are_drawn_by_the_device_draw_for_draw(ctx, lens, batch):
    _, eng = ctx
    assert _lds_bytes(max(lens)) > 65536
    plan, _ = _device_equals_host(eng, STATE0, _split(lens), batch)
    plan.destroy()


@gpu
@device
def test_a_plan_drawn_on_long_splits_runs_like_the_one_from_the_hosts_lists(ctx):
    """2 workers x 1,024 rows per step over splits of 500,000 and 391,041 rows: 8 steps from zero weights, bit for bit"""
    data, eng = ctx
    lens, batch = CASES[1]
    plan, (idx_h, offs_h, n_h) = _device_equals_host(eng, STATE0, _split(lens), batch)
    out = []
    for p in (plan, eng.plan_flat(idx_h, offs_h, n_h, len(lens))):
        eng.set_weights(np.zeros(data.dim + 1, dtype=np.float32))
        eng.plan_run(p, 0, STEPS, 0.5)
        eng.synchronize()
        out.append((eng.get_weights(), p.info()["kind"]))
        p.destroy()
    assert out[0][1] == out[1][1]
    assert np.abs(out[0][0]).max() > 0
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))


def _raw_from_seed(eng, state, lens, batch):
    """dsgd_plan_create_from_seed itself, every output preset to something a refusal must overwrite or leave"""
    split = _split(lens)
    sb = np.asarray([r.start for r in split], dtype=np.int64)
    se = np.asarray([r.stop for r in split], dtype=np.int64)
    st = C.c_uint64(state)
    h = C.c_void_p(0x5A5A5A5A)
    n_steps, draws = C.c_int64(-1), C.c_int64(-1)
    rc = eng._lib.dsgd_plan_create_from_seed(eng._ctx, C.byref(st), _lib.ptr(sb), _lib.ptr(se), C.c_int32(len(sb)), C.c_int64(STEPS * batch),
                                             C.c_int32(batch), C.byref(h), C.byref(n_steps), C.byref(draws))
    return rc, st.value, h.value, n_steps.value, draws.value, eng._lib.dsgd_last_error().decode("utf-8", "replace")


@gpu
@device
def test_a_refusal_leaves_nothing_behind(ctx):
    _, eng = ctx
    # 2^20 rows: inside the length test, ~128 rejections per shuffle -- the host's check over the device's candidates refuses
    rc, state, handle, n_steps, draws, msg = _raw_from_seed(eng, STATE0, (MAX_LEN,), 100)
    assert rc == _lib.EUNSUPPORTED, (rc, msg)
    assert "rejections inside one shuffle" in msg
    assert state == STATE0 and handle is None and n_steps == 0 and draws == 0
    # ... and the context serves the next call: scratch, build stream and the plans' cache are as they were
    plan, _ = _device_equals_host(eng, STATE0, _split((400000,)), 100)
    plan.destroy()
    # 2^20 + 1 rows: refused by the length test, before the rows are looked at or anything is launched
    assert MAX_LEN + 1 <= N_ROWS
    rc, state, handle, n_steps, draws, msg = _raw_from_seed(eng, STATE0, (MAX_LEN + 1,), 100)
    assert rc == _lib.EUNSUPPORTED, (rc, msg)
    assert "splits up to %d rows" % MAX_LEN in msg
    assert state == STATE0 and handle is None and n_steps == 0 and draws == 0
    # (the same length outside the loaded rows: still the length test's answer, not DSGD_ERANGE)
    split = [range(N_ROWS, N_ROWS + MAX_LEN + 1)]
    with pytest.raises(dsgd_amd.DsgdError) as ei:
        eng.plan_from_seed(STATE0, split, STEPS * 100, 100)
    assert ei.value.code == _lib.EUNSUPPORTED
    plan, _ = _device_equals_host(eng, STATE0, _split((400000,)), 100)
    plan.destroy()


class _RefusalsSeen:
    """the engine behind the backend interface, recording the codes plan_from_seed refused with"""

    def __init__(self, eng):
        self.eng, self.refused = eng, []

    def plan_from_seed(self, *a):
        try:
            return self.eng.plan_from_seed(*a)
        except dsgd_amd.DsgdError as e:
            self.refused.append(e.code)
            raise

    def __getattr__(self, name):
        return getattr(self.eng, name)


@gpu
@device
def test_master_sync_falls_back_to_the_hosts_generator_on_a_split_of_2_pow_20_rows(ctx, monkeypatch):
    """One worker over 2^20 rows, batch 1,024 (the device form's largest: 1,024 steps, the shortest epoch it can be asked for):
    the device form is tried, refuses (more than 64 rejections per shuffle), and fit goes on with the host's lists -- the
    weights, the generator and the losses of the same fit with DSGD_DEVICE_LISTS=0."""
    data, eng = ctx
    monkeypatch.setenv("DSGD_DEVICE_LISTS_MIN_DRAWS", "1")
    out = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("DSGD_DEVICE_LISTS", "1" if mode == "device" else "0")
        backend = _RefusalsSeen(eng)
        m = host.MasterSync(backend, N_TRAIN, N_ROWS, node_count=1, rnd=host.JavaRandom(0), plans=True)
        assert m.device_lists == (mode == "device")
        s = m.fit(np.zeros(data.dim + 1), 1, 1024, 0.5, lambda losses: False)
        assert m.device_lists is False
        assert backend.refused == ([_lib.EUNSUPPORTED] if mode == "device" else [])   # (the device form WAS tried)
        out[mode] = (np.array(s.grad, dtype=np.float32), m.rnd.seed, m.steps_run, list(m.losses), list(m.test_losses))
    assert out["device"][2] == out["host"][2] == 1024 and out["device"][1] == out["host"][1] != STATE0
    assert np.abs(out["host"][0]).max() > 0
    assert np.array_equal(out["device"][0].view(np.uint32), out["host"][0].view(np.uint32))
    assert out["device"][3:] == out["host"][3:]
