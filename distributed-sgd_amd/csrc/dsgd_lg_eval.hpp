// Device code of libdsgd_hip, part 15 (gfx950 only): the LOGISTIC model evaluated the way Master evaluates (include/dsgd.h
// "THE LOGISTIC MODEL", DISTRIBUTED AND SAMPLED EVALUATION).  Included by dsgd_hip.hip after dsgd_logistic.hpp:
// both kernels are lg_eval_walk with another row source, so a range's loss words are those of dsgd_lg_eval_kernel over it.
//
//   dsgd_lg_predict_ranges_kernel  Master.predict / distributedLoss / distributedAccuracy (core/Master.scala:61-98) over up to
//                             LG_PRED_MAX_RANGES disjoint row ranges in ONE launch.  Per row, decided on ONE d = x . w: the class
//                             byte signum(d), optionally sigma(d) (lg_sigma), and the row's share of its range's three tallies
//                             and of its sum of l_i -- they cannot disagree.  Range r owns the workgroups [first_block[r],
//                             first_block[r + 1]), the grid of a launch of dsgd_lg_eval_kernel over it alone.  With 256 ranges the
//                             table is a small device array (csrc/dsgd_lg_host.hpp: lg_pred_table), staged once per workgroup
//                             into LDS behind the walk's own and searched by bisection (lg_pred_owner: 8 steps at 256 ranges, on
//                             LDS, once per workgroup).  The workgroups wait for nobody: the grid may exceed what is co-resident.
//   dsgd_lg_eval_list_kernel  Master.localSampledLoss / localSampledAccuracy (:109-118): the row of position t taken from a
//                             resident int32 list.  The group of lanes g takes the positions g, g + n_groups, ... -- for a list
//                             b, b + 1, ..., e - 1 the rows dsgd_lg_eval_kernel's group g takes over [b, e).  A row named twice is
//                             counted twice.  An entry outside the rows raises DevScalars::err and is skipped, as
//                             dsgd_eval_list_kernel does (csrc/dsgd_eval_list.hpp); the host then writes nothing.
//
// What the gfx950 compile reports (hipcc -O3, tools/isa.sh; both: no scratch, no spill, dynamic LDS only):
//   dsgd_lg_predict_ranges_kernel  78 VGPRs, 73 SGPRs, 6 waves per SIMD     dsgd_lg_eval_list_kernel  70 VGPRs, 71 SGPRs, 7 waves
//
// Plain C++ and vector atomics only.
#pragma once

// dynamic LDS of dsgd_lg_predict_ranges_kernel, in floats: dsgd_lg_eval_kernel's (the hot weights, 4 tally words, the sixteen wave
// sums: an even number of floats), then the table's 3 K + 2 words of 8 bytes: first_block[K + 1], begin[K], out_off[K + 1]
__host__ __device__ constexpr int lg_pred_tab_words(int K) { return 3 * K + 2; }
__host__ __device__ constexpr int lg_pred_lds_floats(int hw, int K) { return lg_eval_lds_floats(hw) + 2 * lg_pred_tab_words(K); }

struct LgPredArgs {
  const long long* tab;        // lg_pred_table's three arrays, one behind the other
  int K;
  signed char* cls;            // [out_off[K]] signum(d), range-major; may be null
  float* proba;                // [out_off[K]] sigma(d), range-major; may be null
  unsigned long long* tally;   // [K][LG_TALLY_WORDS], zero on entry
  double* loss_part;           // [first_block[K]] one sum of l_i per workgroup
};

struct LgRowsPred {   // lg_pred_table's K ranges, the table staged into LDS
  static constexpr bool CHECKED = false;
  const long long* tab;
  int K;
  __device__ __forceinline__ void stage(float* l_tab) const {
    for (int j = threadIdx.x; j < lg_pred_tab_words(K); j += LG_EVAL_THREADS) reinterpret_cast<long long*>(l_tab)[j] = tab[j];
  }
  __device__ __forceinline__ LgSpan span(const float* lds_tab) const {
    const long long* l_tab = reinterpret_cast<const long long*>(lds_tab);
    const int range = lg_pred_owner(l_tab, K, (long long)blockIdx.x);
    const long long row_begin = l_tab[K + 1 + range], out0 = l_tab[2 * K + 1 + range];
    return {range, l_tab[range], l_tab[range + 1] - l_tab[range], row_begin, row_begin + (l_tab[2 * K + 2 + range] - out0), out0};
  }
  __device__ __forceinline__ long long row(long long t) const { return t; }
};
struct LgRowsList {   // the n positions of a list; sc: err |= 1 on an entry outside the rows
  static constexpr bool CHECKED = true;
  const int* idx;
  long long n;
  DevScalars* sc;
  __device__ __forceinline__ void stage(float*) const {}
  __device__ __forceinline__ LgSpan span(const float*) const { return {0, 0, (long long)gridDim.x, 0, n, 0}; }
  __device__ __forceinline__ long long row(long long t) const { return idx[t]; }
};
struct LgPredExtra {   // the class byte and / or sigma(d) of row t at the span's out0 + (t - begin)
  signed char* cls;
  float* proba;
  __device__ __forceinline__ void operator()(const LgSpan& s, long long t, float d) const {
    const long long o = s.out0 + (t - s.begin);
    if (cls) cls[o] = d > 0.0f ? (signed char)1 : (d < 0.0f ? (signed char)-1 : (signed char)0);
    if (proba) proba[o] = lg_sigma(d);
  }
};

// grid: first_block[K] workgroups; dynamic LDS: lg_pred_lds_floats(hw, K) floats
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_predict_ranges_kernel(CsrView m, const float* __restrict__ w, LgPredArgs a, int hw) {
  lg_eval_walk(m, w, hw, LgRowsPred{a.tab, a.K}, LgTallyRanges{a.tally}, LgPredExtra{a.cls, a.proba}, a.loss_part);
}
// grid: lg_eval_blocks(n, n_cu) workgroups; dynamic LDS as dsgd_lg_eval_kernel
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_eval_list_kernel(CsrView m, const float* __restrict__ w, const int* __restrict__ idx,
                                                                           long long n, DevScalars* sc, int hw, double* loss_part) {
  lg_eval_walk(m, w, hw, LgRowsList{idx, n, sc}, LgTallyScalars{sc}, LgNoExtra{}, loss_part);
}
