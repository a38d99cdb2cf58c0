"""The consistent loss check of the asynchronous path (dsgd_async_check / _keep / _weights; csrc/dsgd_snapshot.hpp) without a
GPU: the symbols, the refusals that need no device, the snapshot kernel's residency budget beside the lock-free engine read
from the shipped code object, and host.MasterAsync.fit's call sequence with DSGD_ASYNC_SNAPSHOT on and off over a scripted
backend."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from dsgd_amd import _lib, host


def test_library_exports_the_three_entry_points():
    lib = _lib.load()
    for name in ("dsgd_async_check", "dsgd_async_check_keep", "dsgd_async_check_weights"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def test_refusals_that_need_no_device():
    lib = _lib.load()
    loss, acc = C.c_double(7.0), C.c_double(7.0)
    counts, win = (C.c_int64 * 3)(5, 5, 5), (C.c_int64 * 2)(5, 5)
    w = np.full(8, 3.0, dtype=np.float32)
    assert lib.dsgd_async_check(None, 0, 10, C.byref(loss), C.byref(acc), counts, win) == _lib.EINVAL
    assert b"null context" in lib.dsgd_last_error()
    assert lib.dsgd_async_check(None, 0, 10, None, None, None, None) == _lib.EINVAL
    assert lib.dsgd_async_check_keep(None) == _lib.EINVAL
    assert lib.dsgd_async_check_weights(None, 0, _lib.ptr(w)) == _lib.EINVAL
    assert lib.dsgd_async_check_weights(None, 1, None) == _lib.EINVAL
    assert lib.dsgd_async_check_weights(None, 2, _lib.ptr(w)) == _lib.EINVAL
    # nothing was written
    assert loss.value == acc.value == 7.0 and list(counts) == [5, 5, 5] and list(win) == [5, 5] and (w == 3.0).all()


def _kernel_notes(tmp_path):
    """{kernel name: {metadata key: int}} of the gfx950 code object inside the shipped library (as tests/test_abi.py reads it)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _lib.HIP_LIB, fat])
    subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.run([llvm + "/llvm-readelf", "--notes", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():   # (a kernel's keys are sorted: .name sits in the middle of its block, "- " opens one)
        if re.match(r"\s+- \.", line):
            cur = {}
        m = re.search(r"\.(\w+):\s+(\S+)", line)
        if m:
            if m.group(1) == "name":
                out[m.group(2)] = cur
            elif m.group(2).isdigit():
                cur[m.group(1)] = int(m.group(2))
    return out


def test_snapshot_kernel_fits_beside_two_engine_waves_per_simd(tmp_path):
    """A check must become resident beside the persistent engine (2 waves per SIMD that never leave), or it would wait for
    the engine's update budget: allocated VGPRs (granule 8) 2 x engine + snapshot <= 512, no scratch, LDS <= 16 KiB."""
    kn = _kernel_notes(tmp_path)
    hog = [v for k, v in kn.items() if "dsgd_hogwild_kernelILb0ELb0E" in k]
    snap = [v for k, v in kn.items() if "dsgd_snap_kernel" in k]
    assert len(hog) == 1 and len(snap) == 1, sorted(kn)
    alloc = lambda n: -(-n // 8) * 8
    s = snap[0]
    assert 2 * alloc(hog[0]["vgpr_count"]) + alloc(s["vgpr_count"]) <= 512, (hog[0], s)
    assert s["vgpr_spill_count"] == 0 and s.get("sgpr_spill_count", 0) == 0, s
    assert s["private_segment_fixed_size"] == 0, s
    assert s["group_segment_fixed_size"] <= 16 * 1024, s
    assert s["max_flat_workgroup_size"] == 256, s


# ---- host.MasterAsync.fit over a scripted backend ----------------------------------------------------------------------
class Scripted:
    """A backend that scripts the polls (update count, running) and the raw loss of every check, and records every call."""

    BEST = np.arange(5, dtype=np.float32) + 100.0   # what async_check_weights(1) hands out
    LIVE = np.arange(5, dtype=np.float32) - 100.0   # ... and get_weights

    def __init__(self, polls, losses):
        self.polls, self.losses, self.calls = list(polls), list(losses), []
        self.n_poll = self.n_check = 0

    def set_weights(self, w):
        self.calls.append("set_weights")

    def async_start(self, split, **kw):
        self.calls.append("async_start")

    def async_updates(self):
        p = self.polls[min(self.n_poll, len(self.polls) - 1)]
        self.n_poll += 1
        return p

    def _next_loss(self):
        l = self.losses[self.n_check]
        self.n_check += 1
        return l

    def async_check(self, a, b):
        self.calls.append("async_check")
        assert (a, b) == (80, 100)
        u = self.polls[min(self.n_poll - 1, len(self.polls) - 1)][0]
        return self._next_loss(), 0.5, [1, 1, 1], (u - 3, u + 2)

    def async_check_keep(self):
        self.calls.append("async_check_keep")

    def async_check_weights(self, which):
        self.calls.append("async_check_weights(%d)" % which)
        return self.BEST.copy()

    def loss_acc(self, a, b):
        self.calls.append("loss_acc")
        assert (a, b) == (80, 100)
        return self._next_loss(), 0.5, [1, 1, 1]

    def get_weights(self):
        self.calls.append("get_weights")
        return self.LIVE.copy()

    def async_stop(self):
        self.calls.append("async_stop")


POLLS = [(0, True), (4, True), (12, True), (13, True), (25, True), (37, True), (50, True), (61, False)]
RAW = [1.0, 0.8, 0.9, 0.7, 0.95, 0.2, 0.6]   # one per check: polls 0, 12, 25, 37, 50, 61 with check_every = 10 -- see below
LEAK = 0.5


def leaky(raw):
    out = []
    for l in raw:
        out.append(LEAK * l + (1 - LEAK) * (out[-1] if out else l))
    return out


def run_fit(monkeypatch, knob, backend):
    if knob is None:
        monkeypatch.delenv("DSGD_ASYNC_SNAPSHOT", raising=False)
    else:
        monkeypatch.setenv("DSGD_ASYNC_SNAPSHOT", knob)
    m = host.MasterAsync(backend, 80, 100, node_count=2)
    st = m.fit(np.zeros(5), max_epoch=1, batch_size=4, learning_rate=0.5, stopping_criterion=lambda losses: False,
               check_every=10, leak_loss_coef=LEAK, max_steps=60)
    return m, st


def test_fit_with_the_knob_on_checks_one_snapshot_and_reads_the_best_once(monkeypatch):
    b = Scripted(POLLS, RAW)
    m, st = run_fit(monkeypatch, "1", b)
    # with last_step = updates_lo = polled - 3: checks at polls 0 (lo -3), 12 (lo 9), 25 (lo 22), 37 (lo 34), 50 (lo 47), 61 (lo 58)
    n_checks = b.calls.count("async_check")
    assert n_checks == 6 == b.n_check
    smooth = leaky(RAW[:n_checks])
    assert m.test_losses == smooth[::-1]
    improvements = [i for i, l in enumerate(smooth) if l < min([float("inf")] + smooth[:i])]
    assert b.calls.count("async_check_keep") == len(improvements) and len(improvements) >= 2
    # a keep follows exactly the checks that improved, and nothing else
    seq = [c for c in b.calls if c in ("async_check", "async_check_keep")]
    want = []
    for i in range(n_checks):
        want.append("async_check")
        if i in improvements:
            want.append("async_check_keep")
    assert seq == want
    assert "get_weights" not in b.calls and "loss_acc" not in b.calls
    assert b.calls.count("async_check_weights(1)") == 1 and "async_check_weights(0)" not in b.calls
    assert b.calls.index("async_check_weights(1)") > b.calls.index("async_stop")   # read once, after the stop
    assert np.array_equal(st.grad, Scripted.BEST) and st.loss == min(m.test_losses)
    assert st.updates == 61


@pytest.mark.parametrize("knob", [None, "0"])
def test_fit_with_the_knob_off_is_the_sequence_it_was(monkeypatch, knob):
    b = Scripted(POLLS, RAW)
    m, st = run_fit(monkeypatch, knob, b)
    # last_step = the polled count: checks at polls 0, 12, 25, 37, 50, 61
    n_checks = b.calls.count("loss_acc")
    assert n_checks == 6
    smooth = leaky(RAW[:n_checks])
    improvements = [i for i, l in enumerate(smooth) if l < min([float("inf")] + smooth[:i])]
    seq = [c for c in b.calls if c in ("loss_acc", "get_weights")]
    want = []
    for i in range(n_checks):
        want.append("loss_acc")
        if i in improvements:
            want.append("get_weights")
    assert seq == want
    assert not any(c.startswith("async_check") for c in b.calls)
    assert b.calls == ["set_weights", "async_start"] + seq + ["async_stop"]
    assert np.array_equal(st.grad, Scripted.LIVE) and st.loss == min(m.test_losses)


def test_fit_with_the_knob_on_and_a_backend_without_the_call_is_unchanged(monkeypatch):
    class Old(Scripted):
        async_check = property()   # (hasattr is False: an older backend)

    b = Old(POLLS, RAW)
    m, st = run_fit(monkeypatch, "1", b)
    assert b.calls.count("loss_acc") == 6 and b.calls[-1] == "async_stop"
    assert np.array_equal(st.grad, Scripted.LIVE)
