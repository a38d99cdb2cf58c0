// Distributed evaluation (ref: core/Master.scala:61-98, core/Slave.scala:129-140): Master.predict hands every worker a
// ForwardRequest over its split and folds loss and accuracy over the replies.  Here ONE launch serves all K splits: per
// row one int8 prediction p = -signum(x . w), and per split the three exact tallies of dsgd_eval_kernel -- both decided
// on the SAME dot, so the predictions and the tallies of a call cannot disagree.
//
// The K row ranges arrive as a small device table: off[0..K] (prefix sums of the lengths, off[K] = all rows) followed by
// begin[0..K-1].  A group of lanes owns the rows of ordinals t, t + n_groups, ...; ordinal t belongs to the range k with
// off[k] <= t < off[k + 1] (an empty range owns no ordinal) and is row begin[k] + (t - off[k]); its byte goes to
// pred[t], which is range-major by construction.  The table is copied into LDS once per workgroup, the search is a
// bisection there (8 steps at K = 256, 2 at the reference's three workers).
//
// Tallies: a lane counts in registers while its rows stay in one range (its ordinals only grow, so it changes range at
// most K times), adds them to an LDS table [K][3] when the range changes and at the end, and the workgroup flushes every
// counter it touched with ONE global atomic (block_tally3's reasoning: the counters of a call are a handful of
// addresses).  The byte stores are plain vector stores of the group's first lane.
#pragma once

#define PRED_MAX_RANGES 256   // K of one call (include/dsgd.h: dsgd_predict_ranges)

// words of LDS behind the weight tile: off[K + 1] and begin[K] (8 bytes each), then the tallies [K][3]
__host__ __device__ constexpr int pred_lds_words(int K) { return 2 * (2 * K + 1) + 3 * K + 1; }

// the range that owns ordinal t < off[K]: the last k with off[k] <= t
__device__ __forceinline__ int pred_range_of(const long long* off, int K, long long t) {
  int lo = 0, hi = K;   // off[lo] <= t < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// A lane's three counters of the range it is in go to the LDS table when the range changes and at the end (called by a
// group's first lane only; everything by value: the counters stay in registers)
__device__ __forceinline__ void pred_tally_flush(unsigned int* tally, int k, unsigned int c0, unsigned int c1, unsigned int c2) {
  if (k < 0) return;
  if (c0) atomicAdd(&tally[3 * k + 0], c0);
  if (c1) atomicAdd(&tally[3 * k + 1], c1);
  if (c2) atomicAdd(&tally[3 * k + 2], c2);
}
// y * d < 0: correct (loss 0); d == 0 (or y == 0): loss 1; otherwise loss 2 -- the comment above dsgd_eval_kernel
#define PRED_COUNT(yd, zero)                       \
  do {                                             \
    if (k != tk) {                                 \
      pred_tally_flush(l_tally, tk, c0, c1, c2);   \
      tk = k, c0 = c1 = c2 = 0u;                   \
    }                                              \
    if ((yd) < (zero)) c0++;                       \
    else if ((yd) > (zero)) c2++;                  \
    else c1++;                                     \
  } while (0)

// LDS carve behind `base` (16-byte aligned): the table, then the zeroed tallies.  Ends with a barrier.
__device__ __forceinline__ void pred_stage_table(long long* l_tab, unsigned int* l_tally, const long long* __restrict__ tab, int K,
                                                 unsigned int threads) {
  for (int j = threadIdx.x; j < 2 * K + 1; j += threads) l_tab[j] = tab[j];
  for (int j = threadIdx.x; j < 3 * K; j += threads) l_tally[j] = 0u;
  __syncthreads();
}
// one global atomic per touched counter and workgroup
__device__ __forceinline__ void pred_flush_block(const unsigned int* l_tally, unsigned long long* counts, int K, unsigned int threads) {
  __syncthreads();
  for (int j = threadIdx.x; j < 3 * K; j += threads)
    if (l_tally[j]) atomicAdd(&counts[j], (unsigned long long)l_tally[j]);
}

// fp32: persistent 1024-lane workgroups, the hw hottest weights staged in LDS as dsgd_eval_kernel stages them, one G-lane
// group per row, row_dot<G, 4, true> -- the evaluation kernel's instantiation, so a row's sign is the one dsgd_loss_acc
// sees.  Dynamic LDS: hw4 = hw rounded up to 4 floats, then pred_lds_words(K) words.
template <int G>
__global__ void __launch_bounds__(1024) dsgd_predict_kernel(CsrView m, const float* __restrict__ w, const long long* __restrict__ tab, int K,
                                                           signed char* __restrict__ pred, unsigned long long* counts, int hw) {
  constexpr int UNR = 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;
  long long* l_off = reinterpret_cast<long long*>(lds + ((hw + 3) & ~3));
  const long long* l_begin = l_off + (K + 1);
  unsigned int* l_tally = reinterpret_cast<unsigned int*>(l_off + (2 * K + 1));
  for (int j = threadIdx.x; j < hw; j += blockDim.x) wl[j] = w[j];
  pred_stage_table(l_off, l_tally, tab, K, blockDim.x);
  const int sub = threadIdx.x % G;
  const long long group = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const long long n_groups = (long long)gridDim.x * blockDim.x / G;
  const long long total = l_off[K];
  int tk = -1;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (long long t = group; t < total; t += n_groups) {
    const int k = pred_range_of(l_off, K, t);
    const long long row = l_begin[k] + (t - l_off[k]);
    RowRegs<G, UNR> r;
    const float d = row_dot<G, UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], wl, w, hw, sub, r);
    const float yd = (float)m.label[row] * d;
    if (sub == 0) {
      pred[t] = d > 0.0f ? (signed char)-1 : (d < 0.0f ? (signed char)1 : (signed char)0);
      PRED_COUNT(yd, 0.0f);
    }
  }
  if (sub == 0) pred_tally_flush(l_tally, tk, c0, c1, c2);
  pred_flush_block(l_tally, counts, K, blockDim.x);
}

// fp64 (float or Double feature values): 256-lane workgroups, one 16-lane group per row and row_dot64<16> on the
// rank-ordered Double weights, exactly what dsgd_eval64_kernel / dsgd_eval64v_kernel compute (they stage no weights: a
// Double tile of the same reach would be twice the LDS).  Dynamic LDS: pred_lds_words(K) words.
template <typename V>
__device__ __forceinline__ void predict64_body(const CsrViewT<V>& m, const double* __restrict__ w, const long long* __restrict__ tab, int K,
                                               signed char* __restrict__ pred, unsigned long long* counts, unsigned int threads) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  long long* l_off = reinterpret_cast<long long*>(lds);
  const long long* l_begin = l_off + (K + 1);
  unsigned int* l_tally = reinterpret_cast<unsigned int*>(l_off + (2 * K + 1));
  pred_stage_table(l_off, l_tally, tab, K, threads);
  const int sub = threadIdx.x % 16;
  const long long group = ((long long)blockIdx.x * threads + threadIdx.x) / 16;
  const long long n_groups = (long long)gridDim.x * threads / 16;
  const long long total = l_off[K];
  int tk = -1;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (long long t = group; t < total; t += n_groups) {
    const int k = pred_range_of(l_off, K, t);
    const long long row = l_begin[k] + (t - l_off[k]);
    const double d = row_dot64<16>(m, row, w, 0, sub);
    const double yd = (double)m.label[row] * d;
    if (sub == 0) {
      pred[t] = d > 0.0 ? (signed char)-1 : (d < 0.0 ? (signed char)1 : (signed char)0);
      PRED_COUNT(yd, 0.0);
    }
  }
  if (sub == 0) pred_tally_flush(l_tally, tk, c0, c1, c2);
  pred_flush_block(l_tally, counts, K, threads);
}
__global__ void __launch_bounds__(256) dsgd_predict64_kernel(CsrView m, const double* __restrict__ w, const long long* __restrict__ tab, int K,
                                                            signed char* __restrict__ pred, unsigned long long* counts) {
  predict64_body(m, w, tab, K, pred, counts, blockDim.x);
}
__global__ void __launch_bounds__(256) dsgd_predict64v_kernel(CsrView64 m, const double* __restrict__ w, const long long* __restrict__ tab, int K,
                                                             signed char* __restrict__ pred, unsigned long long* counts) {
  predict64_body(m, w, tab, K, pred, counts, blockDim.x);
}
#undef PRED_COUNT
