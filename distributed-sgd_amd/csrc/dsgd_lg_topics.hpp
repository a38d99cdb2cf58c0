// Device code of libdsgd_hip, part 15 (gfx950 only): the logistic model over SEVERAL TOPICS -- one-vs-rest over T <= 8 label
// planes on the same resident rows, ONE pass over the rows and ONE launch pair per step whatever T (include/dsgd.h "THE
// LOGISTIC MODEL": SEVERAL TOPICS).  Included by dsgd_hip.hip after dsgd_logistic.hpp, whose kernels, argument
// blocks and helpers stay as they are: everything here is a sibling.
//
// The contract: topic t's weights, losses, tallies and probabilities are the BITS the single-model kernels give on a context
// whose labels are plane t.  What makes that possible:
//   the dot        lgt_row_dot is row_dot without the fetch: the same lane order, the same 1e-20 product filter, the same group
//                  sum, on W[t] -- a row's first LG_UNR * 16 non-zeros are fetched ONCE (lgt_row_load) and reused by every topic
//   the gradient   cq_t = lg_coef(d_t, plane_t[row]) 2^(S - vexp), every non-zero through lg_add's expression
//                  rn((double)x * cq_t) into acc[t][k][rank].  Integer sums do not depend on their order, so how the LDS head is
//                  shared moves no bit: topic t owns lgt_hot(T) = LG_HOT / T words of the single model's 16 KiB head (its
//                  hottest ranks; the others go to global vector atomics) -- a workgroup's LDS does not grow with T and never
//                  lowers the six waves per SIMD the registers allow.  (The whole head for a few topics per sweep would re-read
//                  the rows once per sweep: the pass over the rows is what the topics are here to share.)
//   the finish     dsgd_lg_finish_kernel<LG_STEP>'s body, one column per lane, the topic on the grid's y: the same fp64
//                  expressions with contraction off, one rounding to float per step, the accumulators left zeroed, |w_t'|^2 per
//                  workgroup by lg_block_sum into nsq_part[t][block]
//   the evaluation dsgd_lg_eval_kernel's grid, walk and fixed-order tree.  A group's lane 0 adds topic t's losses in row order
//                  into its own word of LDS (a register per topic would be an indexed array: scratch), the words then go
//                  through lg_block_tally3 and lg_block_sum topic by topic.  The hot-weight tile is smaller per topic; the
//                  tile's size moves no bit (a weight is the same float from LDS as from memory)
//   predict        sigma(d_t) = 1 / (1 + exp(-d_t)) in fp64 from the fp32 d_t, rounded to float once, p_out[t][position]
//
// What the gfx950 compile reports (hipcc -O3, tools/isa.sh; every kernel: no scratch, no spill):
//   dsgd_lg_topics_grad_kernel     79 VGPRs, 102 SGPRs, 16,384 B LDS, 6 waves per SIMD (dsgd_lg_grad_kernel: 78 VGPRs, 6 waves)
//   dsgd_lg_topics_finish_kernel   20 VGPRs,  30 SGPRs,     32 B LDS, 8 waves per SIMD
//   dsgd_lg_topics_nsq_kernel       9 VGPRs,  19 SGPRs,     32 B LDS, 8 waves per SIMD
//   dsgd_lg_topics_eval_kernel    112 VGPRs,  97 SGPRs, dynamic LDS,  4 waves per SIMD (what ONE 1024-lane workgroup per CU needs)
//   dsgd_lg_topics_predict_kernel  58 VGPRs,  70 SGPRs,      0 B LDS, 8 waves per SIMD
//
// Plain C++ and vector atomics only.
#pragma once
#include "dsgd_lg_topics_host.hpp"

static_assert(LGT_HOT_WORDS == LG_HOT, "the topics share the single model's LDS head");
static_assert(LGT_LDS_FLOATS == DSGD_LDS_FLOATS, "one LDS budget");

// the first UNR * G non-zeros of a row into registers (row_dot's fetch)
template <int G, int UNR>
__device__ __forceinline__ void lgt_row_load(const CsrView& m, long long start, long long end, int sub, RowRegs<G, UNR>& r) {
#pragma unroll
  for (int k = 0; k < UNR; ++k) {
    const long long p = start + sub + k * G;
    const bool in = p < end;
    r.c[k] = in ? m.col[p] : -1;
    r.v[k] = in ? m.val[p] : 0.0f;
  }
}
// row_dot on a row that lgt_row_load fetched: the same products in the same order, the same filter, the same group sum
template <int G, int UNR, bool LDSW>
__device__ __forceinline__ float lgt_row_dot(const CsrView& m, long long start, long long end, const float* wl, const float* __restrict__ w, int hw,
                                             int sub, const RowRegs<G, UNR>& r) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < UNR; ++k) {
    if (r.c[k] >= 0) {
      const float wv = LDSW ? w_at(wl, w, r.c[k], hw) : w[r.c[k]];
      acc += filt(r.v[k] * wv);
    }
  }
  for (long long p = start + sub + UNR * G; p < end; p += G) {
    const int c = m.col[p];
    const float wv = LDSW ? w_at(wl, w, c, hw) : w[c];
    acc += filt(m.val[p] * wv);
  }
  return group_sum<G>(acc);
}

struct LgtArgs {
  const float* w;                  // [T][w_stride] the topics' weights, rank order
  long long w_stride;
  const signed char* planes;       // [T][n_rows] +1 / -1
  int T, hot;                      // hot = lgt_hot(T): the ranks of the LDS head each topic owns
  int dp, vexp, K;
  const int* idx;                  // the lists, concatenated
  const WorkSeg* segs;             // [K] each worker's [begin, end) in idx
  long long blocks_per_worker;     // grid = K * blocks_per_worker
  unsigned long long* acc;         // [T][K][acc_stride] fixed-point column sums, rank order; zero on entry
  long long acc_stride;
  DevScalars* sc;                  // err (1: a row index outside the data)
};

// lg_add with the head's size as an argument
__device__ __forceinline__ void lgt_add(unsigned long long* hot, unsigned long long* acc, int n_hot, int c, float x, double cq) {
#pragma clang fp contract(off)
  const long long q = __double2ll_rn((double)x * cq);   // |x cq| <= 2^S <= 2^62
  if (q == 0) return;
  if (c < n_hot)
    atomicAdd(&hot[c], (unsigned long long)q);
  else
    atomicAdd(&acc[c], (unsigned long long)q);
}

// grid: K x blocks_per_worker workgroups, one 16-lane group per listed position (lg_grad_body<true>'s shape)
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_grad_kernel(CsrView m, LgtArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hot[LG_HOT];
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  const int sub = tid % LG_GROUP;
  const long long groups = a.blocks_per_worker * LG_ROWS_PER_BLOCK;
  const int n_head = a.T * a.hot;   // <= LG_HOT
  for (int j = tid; j < n_head; j += LG_THREADS) hot[j] = 0ull;
  __syncthreads();
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = (long long)a.idx[seg.begin + t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int tp = 0; tp < a.T; ++tp) {
      const float d = lgt_row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, a.w + (long long)tp * a.w_stride, 0, sub, r);
      const double cq = lg_coef(d, (double)a.planes[(long long)tp * m.n_rows + row]) * qscale;
      unsigned long long* hot_t = hot + tp * a.hot;
      unsigned long long* acc_t = a.acc + ((long long)tp * a.K + k) * a.acc_stride;
#pragma unroll
      for (int u = 0; u < LG_UNR; ++u)
        if (r.c[u] >= 0) lgt_add(hot_t, acc_t, a.hot, r.c[u], r.v[u], cq);
      for (long long p = st + sub + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) lgt_add(hot_t, acc_t, a.hot, m.col[p], m.val[p], cq);
    }
  }
  __syncthreads();
  for (int j = tid; j < n_head; j += LG_THREADS) {   // (a word is non-zero only below dp)
    const unsigned long long v = hot[j];
    if (v) {
      const int tp = j / a.hot;
      atomicAdd(&a.acc[((long long)tp * a.K + k) * a.acc_stride + (j - tp * a.hot)], v);
    }
  }
}

struct LgtFinishArgs {
  unsigned long long* acc;   // [T][K][acc_stride], zeroed here
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the lengths give each worker's shift
  int K, dp, vexp;
  float* w;                  // [T][w_stride] rank order, updated
  long long w_stride;
  double lr, lambda;
  double* nsq_part;          // [T][gridDim.x] |w_t'|^2 of each workgroup's columns
};

// grid: (lg_finish_blocks(dp), T) workgroups -- ONE column per lane, the topic on y: dsgd_lg_finish_kernel<LG_STEP>'s body
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_finish_kernel(LgtFinishArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int tp = blockIdx.y;
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  float* w = a.w + (long long)tp * a.w_stride;
  double sq = 0.0;
  if (j < a.dp) {
    const double wj = (double)w[j];
    const double reg = (2.0 * a.lambda) * wj;
    double sum = 0.0;
    for (int k = 0; k < a.K; ++k) {
      unsigned long long* at = a.acc + ((long long)tp * a.K + k) * a.acc_stride + j;
      const unsigned long long t = *at;
      if (t != 0ull) *at = 0ull;
      const long long n = a.segs[k].end - a.segs[k].begin;
      const double G = (double)(long long)t * ldexp(1.0, a.vexp - lg_shift(n));   // one rounding of the exact sum
      sum = sum + (G + reg);
    }
    const double mean = sum / (double)a.K;
    const float wn = (float)(wj - a.lr * mean);
    w[j] = wn;
    sq = (double)wn * (double)wn;
  }
  const double s = lg_block_sum(sq, red, LG_THREADS / 64);
  if (threadIdx.x == 0) a.nsq_part[(long long)tp * gridDim.x + blockIdx.x] = s;
}

// grid: as the finish -- dsgd_lg_nsq_kernel per topic (weights the finish did not write: the same grid, the same tree)
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_nsq_kernel(const float* __restrict__ w, long long w_stride, int dp, double* nsq_part) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int tp = blockIdx.y;
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  const double wj = j < dp ? (double)w[(long long)tp * w_stride + j] : 0.0;
  const double s = lg_block_sum(wj * wj, red, LG_THREADS / 64);
  if (threadIdx.x == 0) nsq_part[(long long)tp * gridDim.x + blockIdx.x] = s;
}

// grid: lg_eval_blocks(rows, n_cu) workgroups; dynamic LDS: lgt_eval_lds_floats(hw, T) floats (csrc/dsgd_lg_topics_host.hpp).
// tally: [T][LG_TALLY_WORDS], zero on entry; loss_part: [T][part_stride], topic t's word of workgroup b at [t][b]
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_topics_eval_kernel(CsrView m, const float* __restrict__ w, long long w_stride,
                                                                             const signed char* __restrict__ planes, int T, long long row_begin,
                                                                             long long row_end, unsigned long long* tally, int hw, double* loss_part,
                                                                             long long part_stride) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  double* sums = reinterpret_cast<double*>(lds + lgt_eval_sums_at(hw, T));        // [T][LGT_EVAL_GROUPS]
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + lgt_eval_cnt_at(hw, T));   // [T][3][LGT_EVAL_GROUPS]
  for (int tp = 0; tp < T; ++tp)
    for (int j = threadIdx.x; j < hw; j += LG_EVAL_THREADS) lds[tp * hw + j] = w[(long long)tp * w_stride + j];
  for (int j = threadIdx.x; j < T * LGT_EVAL_GROUPS; j += LG_EVAL_THREADS) sums[j] = 0.0;
  for (int j = threadIdx.x; j < 3 * T * LGT_EVAL_GROUPS; j += LG_EVAL_THREADS) cnt[j] = 0u;
  __syncthreads();
  const int sub = threadIdx.x % LG_GROUP;
  const int g = threadIdx.x / LG_GROUP;
  const long long group = ((long long)blockIdx.x * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = (long long)gridDim.x * LG_EVAL_THREADS / LG_GROUP;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int tp = 0; tp < T; ++tp) {
      const float d = lgt_row_dot<LG_GROUP, LG_UNR, true>(m, st, en, lds + tp * hw, w + (long long)tp * w_stride, hw, sub, r);
      if (sub == 0) {   // (this group's own words: nobody else touches them)
        const double a = (double)planes[(long long)tp * m.n_rows + row] * (double)d;   // (exact)
        const int which = a > 0.0 ? 0 : (a < 0.0 ? 2 : 1);   // signum(d) == y, == -y, d == +-0: class 0
        cnt[(tp * 3 + which) * LGT_EVAL_GROUPS + g] += 1u;
        sums[tp * LGT_EVAL_GROUPS + g] = sums[tp * LGT_EVAL_GROUPS + g] + lg_loss(a);
      }
    }
  }
  __syncthreads();
  for (int tp = 0; tp < T; ++tp) {
    const bool own = sub == 0;
    const unsigned int c0 = own ? cnt[(tp * 3 + 0) * LGT_EVAL_GROUPS + g] : 0u;
    const unsigned int c1 = own ? cnt[(tp * 3 + 1) * LGT_EVAL_GROUPS + g] : 0u;
    const unsigned int c2 = own ? cnt[(tp * 3 + 2) * LGT_EVAL_GROUPS + g] : 0u;
    const double ls = own ? sums[tp * LGT_EVAL_GROUPS + g] : 0.0;
    lg_block_tally3(c0, c1, c2, tally + tp * LG_TALLY_WORDS, reinterpret_cast<unsigned int*>(lds + T * hw));
    const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lgt_eval_red_at(hw, T)), LG_EVAL_THREADS / 64);
    if (threadIdx.x == 0) loss_part[(long long)tp * part_stride + blockIdx.x] = s;
  }
}

// p_out: [T][n], topic-major
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_predict_kernel(CsrView m, const float* __restrict__ w, long long w_stride, int T,
                                                                           const int* __restrict__ idx, long long n, float* p_out, DevScalars* sc) {
#pragma clang fp contract(off)
  const int sub = threadIdx.x % LG_GROUP;
  const long long group = ((long long)blockIdx.x * LG_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = (long long)gridDim.x * LG_ROWS_PER_BLOCK;
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the list: never taken)
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int tp = 0; tp < T; ++tp) {
      const float d = lgt_row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, w + (long long)tp * w_stride, 0, sub, r);
      if (sub == 0) p_out[(long long)tp * n + t] = (float)(1.0 / (1.0 + exp(-(double)d)));
    }
  }
}
