"""CPU-side checks of row-parallel fp64 plans under a communicator (include/dsgd.h "ACROSS RANKS", csrc/dsgd_rp64_gather.hpp):
the call word of a plan run's agreement packs and unpacks the hosted workers, the value type and the step count up to the
largest a call takes (a stand-alone host program over the header's constexpr helpers), the plan-form kernels are in the code
object without spills or scratch beside the unchanged per-step ones, and host.MasterSync under DSGD_F64_RP_PLANS=1 runs an
epoch as ONE plan_run where the column-slice and from-seed creators are refused (a communicator) and plan_flat(rp64=True)
is not -- and does what it did without the knob."""

import os
import subprocess

import numpy as np

from dsgd_amd import _lib, host
from test_abi import _kernel_notes
from test_fp64_steps_abi import _assert_per_step, _CommBackend, _fit, _Unsupported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_the_call_word_packs_and_unpacks(tmp_path):
    src = tmp_path / "call_word.cpp"
    src.write_text(r'''
#include "dsgd_rp64_gather.hpp"
#include <cstdio>
static_assert(RP64_CALL_MAX_STEPS == 4294967295LL, "32 bits of steps");
static_assert(rp64_call_word(1, false, 0) == 1ull, "an empty run on float values: the plain k");
static_assert(rp64_call_word(2, true, 12) == (2ull | (1ull << 31) | (12ull << 32)), "the documented layout");
int main() {
  const int ks[] = {1, 2, 3, 4, 100, 65535, 65536, 0x7ffffffe, 0x7fffffff};
  const long long steps[] = {0, 1, 2, 3, 12, 231, 65535, 65536, 0x7fffffffLL, 0x80000000LL, RP64_CALL_MAX_STEPS - 1, RP64_CALL_MAX_STEPS};
  int bad = 0;
  for (int k : ks)
    for (long long s : steps)
      for (int v = 0; v < 2; ++v) {
        const unsigned long long w = rp64_call_word(k, v != 0, s);
        if (rp64_call_word_k(w) != k || rp64_call_word_v64(w) != (v != 0) || rp64_call_word_steps(w) != s) ++bad;
        // one field changed: another word
        if (w == rp64_call_word(k == 1 ? 2 : k - 1, v != 0, s) || w == rp64_call_word(k, v == 0, s) ||
            w == rp64_call_word(k, v != 0, s == 0 ? 1 : s - 1)) ++bad;
      }
  // the sum over ranks of words that are non-zero on one rank each is the word itself: what the all-reduce relies on
  if (rp64_call_word(0x7fffffff, true, RP64_CALL_MAX_STEPS) + 0ull != 0xffffffffffffffffull) ++bad;
  std::printf("%d\n", bad);
  return bad ? 1 : 0;
}
''')
    exe = tmp_path / "call_word"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["0"]


def test_plan_form_kernels_in_the_code_object_without_spills(tmp_path):
    notes = _kernel_notes(tmp_path)
    for name, lds in (("dsgd_rp64_grad_gather_plan_kernel", 8 * 1024), ("dsgd_rp64v_grad_gather_plan_kernel", 16 * 1024),
                      ("dsgd_rp64_header_plan_kernel", 16)):
        found = {k: v for k, v in notes.items() if name in k}
        assert len(found) == 1, name
        v = next(iter(found.values()))
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert lds <= v["group_segment_fixed_size"] <= lds + 64, (name, v)
    # the per-step kernels: still one instantiation each
    for name in ("dsgd_rp64_grad_gather_kernel", "dsgd_rp64v_grad_gather_kernel", "dsgd_rp64_header_kernel"):
        assert sum(name in k for k in notes) == 1, name
    # the plan form differs from the per-step gather kernel only by the rank word's store: no more registers, the same LDS
    for plan, step in (("dsgd_rp64_grad_gather_plan_kernel", "dsgd_rp64_grad_gather_kernel"), ("dsgd_rp64v_grad_gather_plan_kernel", "dsgd_rp64v_grad_gather_kernel")):
        a = next(v for k, v in notes.items() if plan in k)
        b = next(v for k, v in notes.items() if step in k)
        assert a["group_segment_fixed_size"] == b["group_segment_fixed_size"] and a["vgpr_count"] <= b["vgpr_count"]


class _RankPlansBackend(_CommBackend):
    """an fp64 backend with a communicator attached: the column-slice and from-seed creators and sync_steps_f64 raise -7,
    plan_flat(rp64=True) succeeds"""

    def __init__(self, dp):
        super().__init__(dp)
        self.refused, self.plans, self.runs = [], [], []

    def plan_flat(self, idx, offsets, n_steps, n_workers, rp64=False):
        if not rp64:
            self.refused.append("plan_flat")
            raise _Unsupported("a communicator is attached")
        plan = _Plan(np.array(idx, copy=True), np.array(offsets, copy=True), n_steps, n_workers)
        self.plans.append(plan)
        return plan

    def plan_from_seed(self, jstate, split, max_samples, batch_size, rp64=False):
        self.refused.append("plan_from_seed_rp64" if rp64 else "plan_from_seed")
        raise _Unsupported("a communicator is attached")

    def plan_run(self, plan, step_begin, step_end, lr):
        assert not plan.destroyed
        self.runs.append((plan, step_begin, step_end, lr))


class _Plan:
    def __init__(self, idx, offsets, n_steps, n_workers):
        self.idx, self.offsets, self.n_steps, self.n_workers, self.destroyed = idx, offsets, n_steps, n_workers, False
        self.n_samples = len(idx)

    def destroy(self):
        self.destroyed = True


def test_master_sync_runs_an_epoch_as_one_plan_run_under_the_knob(monkeypatch):
    monkeypatch.setenv("DSGD_F64_STEPS", "1")
    monkeypatch.setenv("DSGD_F64_RP_PLANS", "1")
    b = _RankPlansBackend(11)
    m, want = _fit(b)
    assert len(b.runs) == 2 and not b.steps and not b.batched   # ONE plan_run per epoch, no per-step call, sync_steps_f64 never asked
    for (plan, s0, s1, lr), (w_idx, w_offs, w_steps) in zip(b.runs, want):
        assert (s0, s1, lr, plan.n_workers) == (0, w_steps, 0.25, 5)
        assert np.array_equal(plan.idx, w_idx) and np.array_equal(plan.offsets, w_offs)
    assert all(p.destroyed for p in b.plans)
    # the refused creators were asked once: -7 means "try the next", not an error, and is not asked again
    assert b.refused.count("plan_flat") == 1 and b.refused.count("plan_from_seed_rp64") == 1
    assert m.steps_run == sum(w[2] for w in want)


def test_master_sync_device_lists_refused_then_one_plan_run(monkeypatch):
    """with the device-drawn lists on (the default), the first -7 comes from plan_from_seed: the chain ends at plan_flat(rp64=True) too"""
    monkeypatch.setenv("DSGD_F64_STEPS", "1")
    monkeypatch.setenv("DSGD_F64_RP_PLANS", "1")
    monkeypatch.delenv("DSGD_DEVICE_LISTS", raising=False)
    b = _RankPlansBackend(11)
    m = host.MasterSync(b, 60, 75, node_count=5, rnd=host.JavaRandom(0), plans=True)
    m.device_lists_min_draws = 0
    m.fit(np.zeros(b.dp), 2, 7, 0.25, lambda losses: False)
    rnd = host.JavaRandom(0)
    split = host.split_vanilla(60, 5)
    want = [host.epoch_lists(rnd, split, max(len(r) for r in split), 7) for _ in range(2)]
    assert m.rnd.seed == rnd.seed
    assert len(b.runs) == 2 and not b.steps and not b.batched
    for (plan, s0, s1, lr), (w_idx, w_offs, w_steps) in zip(b.runs, want):
        assert (s0, s1) == (0, w_steps) and np.array_equal(plan.idx, w_idx) and np.array_equal(plan.offsets, w_offs)
    assert "plan_from_seed" in b.refused and b.refused.count("plan_from_seed_rp64") == 1


def test_master_sync_without_the_knob_does_what_it_did(monkeypatch):
    monkeypatch.setenv("DSGD_F64_STEPS", "1")
    monkeypatch.delenv("DSGD_F64_RP_PLANS", raising=False)
    assert host.F64_RP_PLANS_DEFAULT == "0"
    b = _RankPlansBackend(11)
    _, want = _fit(b)
    assert not b.runs and not b.plans        # no row-parallel plan is asked for
    assert len(b.batched) == 2               # sync_steps_f64 tried once per epoch (-7), then the loop on the same lists
    _assert_per_step(b, want)
