// A consistent loss check beside the lock-free engine (ref: core/MasterAsync.scala:109-138): MasterAsync reads ONE
// innerGradState, computes the test loss and accuracy from its grad, and keeps that same vector as bestGrad when the leaky
// loss improves.  While dsgd_hogwild_kernel runs, the resident weights move under every kernel that reads them, so the
// check copies them first: dsgd_snap_kernel leaves a snapshot of w, the regulariser pair (w . ds, |w|^2) OF THE SNAPSHOT and
// the window of update counts the copy fell into; dsgd_eval_kernel then tallies the test rows on the snapshot (a second
// launch on the same stream -- the ordering between copy and evaluation is the stream's, nothing here waits for another
// workgroup), and the snapshot is what dsgd_async_check_keep / dsgd_async_check_weights hand on (csrc/dsgd_hip.hip).
//
// The copy: block b owns the FRA_COLS columns dsgd_wstats_cols_kernel's block b owns, one column per lane.  Every weight
// is read ONCE, with an agent-scope load as the engine reads it (csrc/dsgd_batch.hpp wload: the engine's atomics land in
// other XCDs' L2s, a plain load may be served a stale line), stored to `snap` with a plain store (the kernel boundary
// publishes it) and fed FROM THE REGISTER to wstats_cols_block: the block decomposition, the summation order and the
// finalisation of dsgd_wstats_cols_kernel, so wnorm2 of a snapshot has the bits ensure_s computes on a quiet context that
// holds those weights.
//
// The window.  The first lane of every block reads HogState::updates (agent-scope load) BEFORE the block's first weight
// load is issued and AFTER its last one has returned (an s_waitcnt vmcnt(0) and a workgroup barrier on either side), and
// folds the two with vector atomics into win[0] / win[1], which the host zeroes on the stream in front of the launch:
//   win[0] = max over the blocks of ~before   ->  updates_lo = ~win[0] = the MINIMUM of the "before" reads
//   win[1] = max over the blocks of after     ->  updates_hi           = the MAXIMUM of the "after" reads
// The engine drains an update's atomics before it draws the update's commit number (csrc/dsgd_batch.hpp, the trace's
// seen_from), hence:
//   * every update with a commit number <= updates_lo is contained in the snapshot WHOLE;
//   * an update with a commit number above updates_lo may be contained in part -- those above updates_hi included: an
//     update in flight adds to w before it has a number.  updates_hi is the count read behind the last weight, no bound on
//     what the snapshot holds; updates_hi - updates_lo is how far the engine moved while the copy ran.
// With no engine running both are the context's update count (dsgd_async_updates); st == nullptr (the engine was never
// started on this context) reads as 0.
//
// Residency: the kernel must run BESIDE the persistent engine (2 waves x 232 allocated VGPRs per SIMD, 136 KiB of LDS per
// CU), or a check would wait for the engine's update budget: 256-lane workgroups (one wave per SIMD), no dynamic LDS, the
// 36 bytes of static LDS of the finalisation, a dozen VGPRs -- tests/test_async_check_abi.py holds it to
// 2 x alloc(engine) + alloc(this) <= 512.
#pragma once

__global__ void __launch_bounds__(256) dsgd_snap_kernel(const float* w, const float* __restrict__ ds, float* __restrict__ snap,
                                                       int dp, float lambda, DevScalars* sc, float* __restrict__ redpart,
                                                       const HogState* st, unsigned long long* win) {
  __shared__ float fred[8];
  __shared__ int is_last;
  const int j = blockIdx.x * FRA_COLS + threadIdx.x;
  const bool mine = threadIdx.x < FRA_COLS && j < dp;
  unsigned long long before = 0ull;
  if (threadIdx.x == 0 && st) {
    before = __hip_atomic_load(&st->updates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the count is here before any weight is asked for)
  }
  __syncthreads();
  float wn = 0.0f;
  if (mine) wn = __hip_atomic_load(&w[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float dsj = mine ? ds[j] : 0.0f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (every weight of the wave has returned ...)
  __syncthreads();                                     // (... of the block)
  if (threadIdx.x == 0) {
    const unsigned long long after = st ? __hip_atomic_load(&st->updates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    atomicMax(&win[0], ~before);
    atomicMax(&win[1], after);
  }
  if (mine) snap[j] = wn;
  wstats_cols_block(mine, wn, dsj, lambda, sc, redpart, fred, &is_last);
}
