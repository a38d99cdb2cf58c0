// Device code of libdsgd_hip, part 15 (gfx950 only): the LOGISTIC model evaluated the way Master evaluates (include/dsgd.h
// "THE LOGISTIC MODEL", DISTRIBUTED AND SAMPLED EVALUATION).  Included by dsgd_hip.hip after dsgd_logistic.hpp.
//
//   dsgd_lg_predict_ranges_kernel  Master.predict / distributedLoss / distributedAccuracy (core/Master.scala:61-98) over up to
//                             LG_PRED_MAX_RANGES disjoint row ranges in ONE launch.  Per row, decided on ONE d = x . w: the class
//                             byte signum(d), optionally sigma(d) as dsgd_lg_predict_kernel rounds it, and the row's share of its
//                             range's three tallies and of its sum of l_i -- they cannot disagree.  The layout is
//                             dsgd_lg_eval_ranges_kernel's: range r owns the workgroups [first_block[r], first_block[r + 1]), the
//                             grid of a launch of dsgd_lg_eval_kernel over it alone, walks its rows with that run's stride and
//                             sums in that kernel's tree, so loss_part[blockIdx.x] holds the bits that launch would leave.  With
//                             256 ranges the table is a small device array (csrc/dsgd_lg_host.hpp: lg_pred_table), staged once per
//                             workgroup into LDS behind the weight tile and searched by bisection (lg_pred_owner: 8 steps at 256
//                             ranges, on LDS, once per workgroup).  The workgroups wait for nobody: the grid may exceed what is
//                             co-resident.
//   dsgd_lg_eval_list_kernel  Master.localSampledLoss / localSampledAccuracy (:109-118): dsgd_lg_eval_kernel with the row of
//                             position t taken from a resident int32 list.  The group of lanes g takes the positions g, g +
//                             n_groups, ... -- for a list b, b + 1, ..., e - 1 the rows dsgd_lg_eval_kernel's group g takes over
//                             [b, e) -- and the tree is the same, so the sum has the same bits.  A row named twice is counted
//                             twice.  An entry outside the rows raises DevScalars::err and is skipped, as dsgd_eval_list_kernel
//                             does (csrc/dsgd_eval_list.hpp); the host then writes nothing.
//
// The tile size hw moves no bit of either kernel (dsgd_lg_eval_ranges_kernel's argument: the same float from LDS as from
// memory, a lane's products added in the order of the row either way), so sigma(d) is the bits of dsgd_lg_predict_kernel, which
// stages no tile.
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

// grid: first_block[K] workgroups; dynamic LDS: lg_pred_lds_floats(hw, K) floats
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_predict_ranges_kernel(CsrView m, const float* __restrict__ w, LgPredArgs a, int hw) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;
  long long* l_tab = reinterpret_cast<long long*>(lds + lg_eval_lds_floats(hw));
  const int K = a.K;
  for (int j = threadIdx.x; j < hw; j += LG_EVAL_THREADS) wl[j] = w[j];
  for (int j = threadIdx.x; j < lg_pred_tab_words(K); j += LG_EVAL_THREADS) l_tab[j] = a.tab[j];
  __syncthreads();
  // this workgroup's range (the same on every lane)
  const int range = lg_pred_owner(l_tab, K, (long long)blockIdx.x);
  const long long first = l_tab[range], blocks = l_tab[range + 1] - first;
  const long long row_begin = l_tab[K + 1 + range];
  const long long out0 = l_tab[2 * K + 1 + range];
  const long long row_end = row_begin + (l_tab[2 * K + 2 + range] - out0);
  const int sub = threadIdx.x % LG_GROUP;
  const long long group = (((long long)blockIdx.x - first) * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = blocks * LG_EVAL_THREADS / LG_GROUP;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  double ls = 0.0;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], wl, w, hw, sub, r);
    if (sub == 0) {
      const long long t = out0 + (row - row_begin);
      if (a.cls) a.cls[t] = d > 0.0f ? (signed char)1 : (d < 0.0f ? (signed char)-1 : (signed char)0);
      if (a.proba) a.proba[t] = (float)(1.0 / (1.0 + exp(-(double)d)));   // (dsgd_lg_predict_kernel's expression)
      const double yd = (double)m.label[row] * (double)d;   // (exact)
      if (yd > 0.0) c0++;
      else if (yd < 0.0) c2++;
      else c1++;
      ls = ls + lg_loss(yd);
    }
  }
  lg_block_tally3(c0, c1, c2, a.tally + (long long)range * LG_TALLY_WORDS, reinterpret_cast<unsigned int*>(wl + hw));
  const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lg_eval_red_at(hw)), LG_EVAL_THREADS / 64);
  if (threadIdx.x == 0) a.loss_part[blockIdx.x] = s;
}

// grid: lg_eval_blocks(n, n_cu) workgroups; dynamic LDS as dsgd_lg_eval_kernel
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_eval_list_kernel(CsrView m, const float* __restrict__ w, const int* __restrict__ idx,
                                                                           long long n, DevScalars* sc, int hw, double* loss_part) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;
  for (int j = threadIdx.x; j < hw; j += LG_EVAL_THREADS) wl[j] = w[j];
  __syncthreads();
  const int sub = threadIdx.x % LG_GROUP;
  const long long group = ((long long)blockIdx.x * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = (long long)gridDim.x * LG_EVAL_THREADS / LG_GROUP;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  double ls = 0.0;
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {   // (uniform over the group)
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], wl, w, hw, sub, r);
    if (sub == 0) {
      const double yd = (double)m.label[row] * (double)d;   // (exact)
      if (yd > 0.0) c0++;
      else if (yd < 0.0) c2++;
      else c1++;
      ls = ls + lg_loss(yd);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&sc->counts[3], (unsigned long long)n);
  block_tally3(c0, c1, c2, sc, reinterpret_cast<unsigned int*>(wl + hw));
  const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lg_eval_red_at(hw)), LG_EVAL_THREADS / 64);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = s;
}
