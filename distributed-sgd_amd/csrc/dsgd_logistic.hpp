// Device code of libdsgd_hip, part 14 (gfx950 only): the LOGISTIC model on the resident CSR rows, beside the gated hinge SVM
// (include/dsgd.h "THE LOGISTIC MODEL").  Included by dsgd_hip.hip after dsgd_kernels.hpp.
//
// The model.  y in {-1, +1}; d = x . w is the fp32 engine's own dot (row_dot: its lane order, its 1e-20 product filter).  The
// TEXTBOOK sign convention: P(y = +1 | x) = sigma(d), class = signum(d) -- the SVM beside it predicts -signum(d).
//   loss       l_i = log(1 + exp(-a)) = max(-a, 0) + log1p(exp(-|a|)),  a = y d, in fp64; reported lambda |w|^2 + mean l_i
//   gradient   c_i x_i,  c_i = sigma(d_i) - (1 + y_i) / 2 = -y_i / (1 + exp(y_i d_i))   in fp64 from the fp32 d_i: exp -> inf
//              gives -+0, exp -> 0 gives -y: no NaN for a finite d
//   regulariser  plain L2, + 2 lambda w_j on EVERY column, per worker (dimSparsity plays no part)
//   step       per worker the regularised SUM over its rows, the MEAN over the K workers, w <- w - lr mean
//
// Sibling kernels give the same bits because they are ONE body each, instantiated (the topics' kernels of
// csrc/dsgd_lg_topics.hpp and the evaluations of csrc/dsgd_lg_eval.hpp included):
//   lg_grad_body<LIST, TOPICS>  one 16-lane group per listed position (dsgd_lg_grad_kernel, dsgd_lg_topics_grad_kernel) or per row
//                             of a range (dsgd_lg_grad_range_kernel).  The first LG_UNR * 16 non-zeros of the row stay in
//                             registers for the scatter.  c_i once per row on every lane (group_sum leaves the same d on all
//                             16), then every non-zero becomes rn(c_i * x * 2^(S - vexp)), S = 62 - ceil(log2 n), added into the
//                             worker's int64 column accumulators (lg_add): ranks of the head in an LDS tile (ds_add_u64, flushed
//                             once per touched word), the others with 64-bit global vector atomics.  Grid: K x
//                             blocks_per_worker.  Integer adds do not depend on their order: a step's weights are the same bits
//                             whatever the list's order, the grid's shape, the head's size or the run.
//   lg_finish_body<M, GATHERED, TOPICS>  ONE column per lane, in fp64 with contraction off: G_k = acc_k 2^(vexp - S_k) (lg_finish_G,
//                             which leaves the accumulator zeroed), r_k = G_k + 2 lambda w_j; LG_GRADIENT: (float)r_0 to g_out in
//                             key order; LG_STEP: the r_k added in worker order, / K, w_j' = (float)(w_j - lr mean): one rounding
//                             to float per step, and |w'|^2 per workgroup (lg_block_sum: a fixed tree) in nsq_part[blockIdx.x]:
//                             the host adds the words in order, so a following evaluation needs no pass over w.  GATHERED: the
//                             finish of a step across ranks (dsgd_comm_init_lg; csrc/dsgd_lg_gather.hpp) over the K = k * world
//                             slots behind the all-reduce, in global worker order; a worker's n comes from the header words
//                             (uniform reads), vexp is the call's agreed one; the first lane also adds the job's rows of the
//                             step to the context's n_samples.  TOPICS: the topic on the grid's y.
//   dsgd_lg_async_finish_kernel  the finish of ONE worker's ASYNCHRONOUS update behind lg_grad_body with K = 1: lg_finish_G, then
//                             the mean over the list's n rows, regularised once, w_j' = (float)(w_j - lr r); optionally the
//                             double delta
//   dsgd_lg_nsq_kernel        the finish's per-workgroup sums of |w|^2 from weights it did not write (its grid, its tree); the
//                             topic, if any, on the grid's y
//   lg_eval_walk<Rows, Tally, Extra>  persistent 1024-lane workgroups, the hw hottest weights in LDS (the shape of
//                             dsgd_eval_kernel): per row lg_row_loss -- the class tally (signum(d) == y, == 0, == -y) and l_i --
//                             the tallies through lg_block_tally3, and the sum of l_i by a FIXED-ORDER TREE: a group's lane 0
//                             adds its rows in row order, the wave's lanes fold by xor butterflies, lane 0 of the workgroup adds
//                             the sixteen wave sums in order, the host adds the workgroups' words in order.  A workgroup walks
//                             ONE span of positions with the stride of the span's own run of workgroups, so a span's words do
//                             not depend on what else the launch holds; nothing is added with floating-point atomics, and the
//                             tile size hw moves no bit (a weight is the same float from LDS as from memory, row_dot adds a
//                             lane's products in the order of the row either way).  Every l_i carries at most |d_i - d_i,exact|
//                             and a few fp64 roundings of error, the tree at most (n + 64) 2^-53 of the sum
//                             (tests/logistic_bound.py: dloss).  Rows: LgRowsRange (dsgd_lg_eval_kernel), LgRowsTable (up to 16
//                             ranges from the argument table: dsgd_lg_eval_ranges_kernel), LgRowsPred and LgRowsList
//                             (csrc/dsgd_lg_eval.hpp).  Tally: LgTallyScalars (DevScalars::counts) or LgTallyRanges (the span's
//                             own LG_TALLY_WORDS words).  Extra: per row nothing, or the class byte and sigma(d).
//   lg_predict_body<TOPICS>   sigma(d) per listed position (lg_sigma: 1 / (1 + exp(-d)) in fp64 from the fp32 d, one rounding)
//   dsgd_lg_header_kernel     in front of a GATHERED step's all-reduce: the K header words -- this rank's k lengths from its
//                             WorkSegs at its own positions, zero everywhere else (so the words of the previous step are gone)
//   dsgd_lg_update_kernel     a peer's update from (key, dv) pairs: w_k = (float)((double)w_k - dv_k)
//
// What the gfx950 compile reports (hipcc -O3, tools/isa.sh; every kernel: no scratch, no spill) -- VGPRs, SGPRs, static LDS,
// waves per SIMD:
//   dsgd_lg_grad_kernel, _range_kernel   78,  74, 16,384 B, 6        dsgd_lg_async_finish_kernel  20,  30,     32 B, 8
//   dsgd_lg_finish_kernel<0, false>      10,  20,      0 B, 8        dsgd_lg_nsq_kernel            9,  18,     32 B, 8
//   dsgd_lg_finish_kernel<1, false>      22,  26,     32 B, 8        dsgd_lg_header_kernel        10,  20,      0 B, 8
//   dsgd_lg_finish_kernel<1, true>       20,  28,     32 B, 8        dsgd_lg_update_kernel        14,  30,      0 B, 8
//   dsgd_lg_eval_kernel                  70,  67,  dynamic, 7        dsgd_lg_predict_kernel       46,  52,      0 B, 8
//   dsgd_lg_eval_ranges_kernel           70,  64,  dynamic, 7
//
// Every body and helper with fp64 arithmetic opens with `#pragma clang fp contract(off)` itself: the pragma does not follow a
// call into an inlined function.  Plain C++ and vector atomics only.
#pragma once
#include "dsgd_lg_gather.hpp"
#include "dsgd_lg_host.hpp"

constexpr int LG_UNR = 4;   // non-zeros per lane kept in registers between dot and scatter: rows up to 64 non-zeros are read once
// The LDS head of the column accumulators.  A 256-lane workgroup with 2,048 words (16 KiB) lets EIGHT workgroups share a compute
// unit's 160 KiB (128 KiB used) -- the 2,048 lanes a CU holds, so LDS never lowers the occupancy the registers allow.  The
// ranking is by frequency: the head takes the columns most rows share, whose global atomics would serialise on a handful of
// addresses (csrc/dsgd_rp64.hpp measured 13x on a list of 65,536 rows without a head).  Twice the head would halve the
// workgroups per CU; the share of the non-zeros it takes on a given data set is not measured.
constexpr int LG_HOT = 2048;

struct LgArgs {
  const float* w;                  // the weights, rank order
  int dp, vexp, K;
  const int* idx;                  // LIST: the lists, concatenated
  const WorkSeg* segs;             // [K] LIST: each worker's [begin, end) in idx; ranges: its rows [begin, end)
  long long blocks_per_worker;     // grid = K * blocks_per_worker
  unsigned long long* acc;         // [K][acc_stride] fixed-point column sums, rank order; zero on entry
  long long acc_stride;
  DevScalars* sc;                  // err (1: a row index outside the data)
};

// c = -y / (1 + exp(y d)), every operation in fp64 (exp overflows to inf for y d > 709.78: c = -+0; underflows to 0: c = -y)
__device__ __forceinline__ double lg_coef(float d, double y) {
#pragma clang fp contract(off)
  return -y / (1.0 + exp(y * (double)d));
}
// l = log(1 + exp(-a)) without overflow
__device__ __forceinline__ double lg_loss(double a) {
#pragma clang fp contract(off)
  return fmax(-a, 0.0) + log1p(exp(-fabs(a)));
}
// One row of an evaluation: a = y d (exact in fp64), its tally -- which = 0: signum(d) == y, 1: d == +-0 (class 0), 2: signum(d) == -y --
// and its loss
__device__ __forceinline__ double lg_row_loss(double y, float d, int& which) {
#pragma clang fp contract(off)
  const double a = y * (double)d;
  which = a > 0.0 ? 0 : (a < 0.0 ? 2 : 1);
  return lg_loss(a);
}
// sigma(d) in fp64 from the fp32 d, rounded to float once
__device__ __forceinline__ float lg_sigma(float d) {
#pragma clang fp contract(off)
  return (float)(1.0 / (1.0 + exp(-(double)d)));
}

// hot: the n_hot hottest ranks of acc, in LDS
__device__ __forceinline__ void lg_add(unsigned long long* hot, unsigned long long* acc, int n_hot, int c, float x, double cq) {
#pragma clang fp contract(off)
  const long long q = __double2ll_rn((double)x * cq);   // |x cq| <= 2^S <= 2^62
  if (q == 0) return;                                     // (a zero adds nothing: the padding entry of an empty row, c = -+0)
  if (c < n_hot)
    atomicAdd(&hot[c], (unsigned long long)q);            // (two's complement: one add)
  else
    atomicAdd(&acc[c], (unsigned long long)q);
}

// The split form of row_dot for several weight vectors on one row: the first UNR * G non-zeros into registers (row_dot's fetch) ...
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
// ... and row_dot on the fetched row: the same products in the same order, the same filter, the same group sum
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

// a row's non-zeros (the first LG_UNR * 16 of them in r) times cq into one vector of column sums
__device__ __forceinline__ void lg_scatter(unsigned long long* hot, unsigned long long* acc, int n_hot, const CsrView& m, long long st, long long en,
                                           int sub, const RowRegs<LG_GROUP, LG_UNR>& r, double cq) {
#pragma unroll
  for (int u = 0; u < LG_UNR; ++u)
    if (r.c[u] >= 0) lg_add(hot, acc, n_hot, r.c[u], r.v[u], cq);
  for (long long p = st + sub + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) lg_add(hot, acc, n_hot, m.col[p], m.val[p], cq);
}

// A: LgArgs, or TOPICS: LgtArgs (csrc/dsgd_lg_topics.hpp) -- topic t on W[t] and label plane t, its sums in acc[t][k], its head
// the a.hot words of `hot` from t * a.hot; the row's registers are fetched once for all topics
template <bool LIST, bool TOPICS, class A>
__device__ __forceinline__ void lg_grad_body(const CsrView& m, const A& a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hot[LG_HOT];
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  unsigned long long* acc = a.acc + (long long)k * a.acc_stride;   // worker k's sums; TOPICS: topic t's are t * t_stride further
  const int sub = tid % LG_GROUP;
  const long long groups = a.blocks_per_worker * LG_ROWS_PER_BLOCK;
  int T = 1, n_hot = LG_HOT;   // (constants of the single model)
  long long t_stride = 0;
  if constexpr (TOPICS) T = a.T, n_hot = a.hot, t_stride = a.K * a.acc_stride;
  for (int j = tid; j < T * n_hot; j += LG_THREADS) hot[j] = 0ull;
  __syncthreads();
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = LIST ? (long long)a.idx[seg.begin + t] : seg.begin + t;
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists and the ranges: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    if constexpr (!TOPICS) {
      const float d = row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, a.w, 0, sub, r);
      lg_scatter(hot, acc, LG_HOT, m, st, en, sub, r, lg_coef(d, (double)m.label[row]) * qscale);
    } else {
      lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
      for (int tp = 0; tp < T; ++tp) {
        const float d = lgt_row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, a.w + (long long)tp * a.w_stride, 0, sub, r);
        const double cq = lg_coef(d, (double)a.planes[(long long)tp * m.n_rows + row]) * qscale;
        lg_scatter(hot + tp * n_hot, acc + tp * t_stride, n_hot, m, st, en, sub, r, cq);
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < T * n_hot; j += LG_THREADS) {   // (a word is non-zero only below dp)
    const unsigned long long v = hot[j];
    const int tp = TOPICS ? j / n_hot : 0;
    if (v) atomicAdd(&acc[tp * t_stride + (j - tp * n_hot)], v);
  }
}
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_grad_kernel(CsrView m, LgArgs a) { lg_grad_body<true, false>(m, a); }
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_grad_range_kernel(CsrView m, LgArgs a) { lg_grad_body<false, false>(m, a); }

// The sum of one double per lane over a workgroup of `waves` waves, on lane 0, in ONE order: xor butterflies inside a wave
// (every lane ends with the same bits), then the wave sums from 0.0 in wave order.
__device__ __forceinline__ double lg_block_sum(double v, double* red, int waves) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < waves; ++i) s = s + red[i];
  return s;
}

struct LgFinishArgs {
  unsigned long long* acc;   // [K][acc_stride], zeroed here
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the lengths give each worker's shift
  int K, dp, vexp;
  const int* perm;           // key -> rank
  float* g_out;              // LG_GRADIENT: the regularised sum of worker 0, key order
  float* w;                  // rank order; LG_STEP: updated
  double lr, lambda;
  double* nsq_part;          // LG_STEP: [gridDim.x] |w'|^2 of each workgroup's columns
  const unsigned long long* hdr;   // GATHERED: [K] each global worker's n (segs is not read)
  DevScalars* sc;                  // GATHERED: n_samples takes the step's rows (all of them active)
};
constexpr int LG_GRADIENT = 0, LG_STEP = 1;

// One worker's exact column sum over its n rows, read from its accumulator word (left zeroed) and scaled back in ONE rounding
__device__ __forceinline__ double lg_finish_G(unsigned long long* at, int vexp, long long n) {
#pragma clang fp contract(off)
  const unsigned long long t = *at;
  if (t != 0ull) *at = 0ull;
  return (double)(long long)t * ldexp(1.0, vexp - lg_shift(n));
}

// grid: lg_finish_blocks(dp) workgroups -- ONE column per lane.  A: LgFinishArgs, or TOPICS (LG_STEP only): LgtFinishArgs
// (csrc/dsgd_lg_topics.hpp), the topic's weights, accumulators and |w'|^2 words on the grid's y
template <int MODE, bool GATHERED, bool TOPICS, class A>
__device__ __forceinline__ void lg_finish_body(const A& a) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  float* w = a.w;
  unsigned long long* acc = a.acc;
  double* nsq_part = a.nsq_part;
  if constexpr (TOPICS) {
    w += (long long)blockIdx.y * a.w_stride;
    acc += (long long)blockIdx.y * a.K * a.acc_stride;
    nsq_part += (long long)blockIdx.y * gridDim.x;
  }
  double sq = 0.0;
  if (j < a.dp) {
    int r = j;
    if constexpr (MODE == LG_GRADIENT) r = a.perm[j];
    const double wj = (double)w[r];
    const double reg = (2.0 * a.lambda) * wj;
    double sum = 0.0;
    for (int k = 0; k < (MODE == LG_STEP ? a.K : 1); ++k) {
      long long n;
      if constexpr (GATHERED) n = (long long)a.hdr[k];
      else n = a.segs[k].end - a.segs[k].begin;
      const double G = lg_finish_G(acc + (long long)k * a.acc_stride + r, a.vexp, n);
      sum = sum + (G + reg);
    }
    if constexpr (MODE == LG_GRADIENT) {
      a.g_out[j] = (float)sum;
    } else {
      const double mean = sum / (double)a.K;
      const float wn = (float)(wj - a.lr * mean);
      w[r] = wn;
      sq = (double)wn * (double)wn;
    }
  }
  if (MODE == LG_STEP) {
    const double s = lg_block_sum(sq, red, LG_THREADS / 64);
    if (threadIdx.x == 0) nsq_part[blockIdx.x] = s;
  }
  if constexpr (GATHERED) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the job's rows of this step (every row contributes)
      unsigned long long rows = 0ull;
      for (int k = 0; k < a.K; ++k) rows += a.hdr[k];
      atomicAdd(&a.sc->n_samples, rows);
    }
  }
}
template <int MODE, bool GATHERED = false>
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_finish_kernel(LgFinishArgs a) {
  lg_finish_body<MODE, GATHERED, false>(a);
}

// One step's header words across ranks: hdr[first + j] = the rows of this rank's worker j, every other of the K words zero.
// grid: one workgroup
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_header_kernel(unsigned long long* hdr, int K, int first, int k, const WorkSeg* segs) {
  for (int g = threadIdx.x; g < K; g += LG_THREADS) {
    const int j = g - first;
    hdr[g] = j >= 0 && j < k ? (unsigned long long)(segs[j].end - segs[j].begin) : 0ull;
  }
}

// ---- the ASYNCHRONOUS iteration (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS; core/Slave.scala:79-111, 177-185) ----
// One worker's update over a list of n rows: behind lg_grad_body with K = 1 the finish below takes the MEAN over the list,
// regularises it once, and leaves the weights and (optionally) the delta a peer applies.  Per column, fp64, contraction off:
//   G = lg_finish_G,  gm = G / n,  r = gm + 2 lambda w_j,  delta = lr r,  w_j' = (float)(w_j - delta)
// one rounding to float; |w'|^2 per workgroup in nsq_part by LG_STEP's grid and tree.  For n = 1 these are the bits of
// lg_finish_body<LG_STEP> with K = 1 (G / 1.0 = G, 0.0 + (G + reg) = G + reg, G never -0.0).
struct LgAsyncArgs {
  unsigned long long* acc;   // [dp] the one worker's slot, zeroed here
  const WorkSeg* seg;        // the list's [begin, end): its length is n
  int dp, vexp;
  float* w;                  // rank order, updated
  double lr, lambda;
  double* nsq_part;          // [gridDim.x] |w'|^2 of each workgroup's columns
  double* delta;             // NULL, or [dp] the delta in RANK order (the host permutes it into key order)
};
// grid: lg_finish_blocks(dp) workgroups -- ONE column per lane
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_async_finish_kernel(LgAsyncArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  double sq = 0.0;
  if (j < a.dp) {
    const long long n = a.seg->end - a.seg->begin;
    const double wj = (double)a.w[j];
    const double G = lg_finish_G(a.acc + j, a.vexp, n);
    const double gm = G / (double)n;
    const double r = gm + (2.0 * a.lambda) * wj;
    const double delta = a.lr * r;
    const float wn = (float)(wj - delta);
    a.w[j] = wn;
    if (a.delta) a.delta[j] = delta;
    sq = (double)wn * (double)wn;
  }
  const double s = lg_block_sum(sq, red, LG_THREADS / 64);
  if (threadIdx.x == 0) a.nsq_part[blockIdx.x] = s;
}

// A peer's update: w_k = (float)((double)w_k - dv_k) for each (unique, host-checked) key -- the expression of the finish above,
// so replicas that apply every delta keep the bits of the replica that made it.  grid-stride over the nnz pairs.
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_update_kernel(const int* __restrict__ key, const double* __restrict__ dv, long long nnz,
                                                                   const int* __restrict__ perm, float* w, int dp) {
#pragma clang fp contract(off)
  for (long long i = (long long)blockIdx.x * LG_THREADS + threadIdx.x; i < nnz; i += (long long)gridDim.x * LG_THREADS) {
    const int k = key[i];
    if (k < 0 || k >= dp) continue;   // (the host checked the keys: never taken)
    const int r = perm[k];
    w[r] = (float)((double)w[r] - dv[i]);
  }
}

// grid: (lg_finish_blocks(dp), topics or 1), as the finish; topic t's weights at w + t * w_stride (one model: stride 0), its
// words at nsq_part[t][gridDim.x]
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_nsq_kernel(const float* __restrict__ w, long long w_stride, int dp, double* nsq_part) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  const double wj = j < dp ? (double)w[(long long)blockIdx.y * w_stride + j] : 0.0;
  const double s = lg_block_sum(wj * wj, red, LG_THREADS / 64);
  if (threadIdx.x == 0) nsq_part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// dynamic LDS, in floats: [0, hw) the hot weights, 4 tally words, then (8-byte aligned) the sixteen wave sums
__host__ __device__ constexpr int lg_eval_red_at(int hw) { return (hw + 4 + 1) & ~1; }
__host__ __device__ constexpr int lg_eval_lds_floats(int hw) { return lg_eval_red_at(hw) + 2 * (LG_EVAL_THREADS / 64); }

// a workgroup's three tallies into `counts`: block_tally3 (csrc/dsgd_kernels.hpp) with the destination as an argument
__device__ __forceinline__ void lg_block_tally3(unsigned int c0, unsigned int c1, unsigned int c2, unsigned long long* counts, unsigned int* tally) {
  __syncthreads();
  if (threadIdx.x < 3) tally[threadIdx.x] = 0u;
  __syncthreads();
  c0 = wave_sum_u32(c0);
  c1 = wave_sum_u32(c1);
  c2 = wave_sum_u32(c2);
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(&tally[0], c0);
    if (c1) atomicAdd(&tally[1], c1);
    if (c2) atomicAdd(&tally[2], c2);
  }
  __syncthreads();
  if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// What one workgroup of an evaluation walks: the positions [begin, end) of span `range`, as workgroup blockIdx.x - first of the
// span's `blocks`; out0: where the span's per-row outputs start (LgRowsPred)
struct LgSpan {
  int range;
  long long first, blocks, begin, end, out0;
};
// Row sources of lg_eval_walk.  stage(tab): before the walk's first barrier, `tab` the LDS behind lg_eval_lds_floats(hw) floats;
// span(tab): behind it, the same on every lane; row(t): the row of position t; CHECKED: row(t) may lie outside the data.
struct LgRowsRange {   // the rows [row_begin, row_end), the whole grid
  static constexpr bool CHECKED = false;
  long long row_begin, row_end;
  __device__ __forceinline__ void stage(float*) const {}
  __device__ __forceinline__ LgSpan span(const float*) const { return {0, 0, (long long)gridDim.x, row_begin, row_end, 0}; }
  __device__ __forceinline__ long long row(long long t) const { return t; }
};
struct LgRowsTable {   // up to LG_MAX_RANGES ranges (csrc/dsgd_lg_host.hpp: lg_eval_table), each its own run of workgroups
  static constexpr bool CHECKED = false;
  const LgEvalTable& tab;
  __device__ __forceinline__ void stage(float*) const {}
  __device__ __forceinline__ LgSpan span(const float*) const {   // (selects, not an indexed read of the argument)
    LgSpan s = {0, tab.r[0].first_block, tab.r[0].n_blocks, tab.r[0].row_begin, tab.r[0].row_end, 0};
#pragma unroll
    for (int i = 1; i < LG_MAX_RANGES; ++i)
      if (i < tab.n && (int)blockIdx.x >= tab.r[i].first_block) s = {i, tab.r[i].first_block, tab.r[i].n_blocks, tab.r[i].row_begin, tab.r[i].row_end, 0};
    return s;
  }
  __device__ __forceinline__ long long row(long long t) const { return t; }
};
// Tally destinations: the three words a span's tallies are added to
struct LgTallyScalars {   // DevScalars::counts, and the rows of the call in counts[3]
  DevScalars* sc;
  __device__ __forceinline__ unsigned long long* words(const LgSpan& s) const {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&sc->counts[3], (unsigned long long)(s.end - s.begin));
    return sc->counts;
  }
};
struct LgTallyRanges {   // [ranges][LG_TALLY_WORDS], zero on entry
  unsigned long long* tally;
  __device__ __forceinline__ unsigned long long* words(const LgSpan& s) const { return tally + (long long)s.range * LG_TALLY_WORDS; }
};
struct LgNoExtra {
  __device__ __forceinline__ void operator()(const LgSpan&, long long, float) const {}
};

// THE evaluation: every evaluation kernel of the single model is this body.  dynamic LDS: lg_eval_lds_floats(hw) floats, then
// what Rows stages.  loss_part[blockIdx.x]: the workgroup's sum of l_i.  The barriers are those of the staging, lg_block_tally3
// and lg_block_sum; a bad row of a CHECKED source is skipped by its whole group, in front of them.
template <class Rows, class Tally, class Extra>
__device__ __forceinline__ void lg_eval_walk(const CsrView& m, const float* w, int hw, const Rows& rows, const Tally& tally,
                                             const Extra& extra, double* loss_part) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int j = threadIdx.x; j < hw; j += LG_EVAL_THREADS) lds[j] = w[j];
  rows.stage(lds + lg_eval_lds_floats(hw));
  __syncthreads();
  const LgSpan s = rows.span(lds + lg_eval_lds_floats(hw));
  const int sub = threadIdx.x % LG_GROUP;
  const long long group = (((long long)blockIdx.x - s.first) * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = s.blocks * LG_EVAL_THREADS / LG_GROUP;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  double ls = 0.0;
  for (long long t = s.begin + group; t < s.end; t += n_groups) {
    const long long row = rows.row(t);
    if constexpr (Rows::CHECKED) {
      if (row < 0 || row >= m.n_rows) {   // (uniform over the group)
        if (sub == 0) atomicOr(&rows.sc->err, 1);
        continue;
      }
    }
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], lds, w, hw, sub, r);
    if (sub == 0) {
      extra(s, t, d);
      int which;
      const double l = lg_row_loss((double)m.label[row], d, which);
      if (which == 0) c0++;
      else if (which == 2) c2++;
      else c1++;
      ls = ls + l;
    }
  }
  lg_block_tally3(c0, c1, c2, tally.words(s), reinterpret_cast<unsigned int*>(lds + hw));
  const double sum = lg_block_sum(ls, reinterpret_cast<double*>(lds + lg_eval_red_at(hw)), LG_EVAL_THREADS / 64);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = sum;
}

// grid: lg_eval_blocks(rows, n_cu) workgroups -- a function of the range and the device alone; dynamic LDS: lg_eval_lds_floats(hw)
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_eval_kernel(CsrView m, const float* __restrict__ w, long long row_begin,
                                                                      long long row_end, DevScalars* sc, int hw, double* loss_part) {
  lg_eval_walk(m, w, hw, LgRowsRange{row_begin, row_end}, LgTallyScalars{sc}, LgNoExtra{}, loss_part);
}
// grid: t.grid workgroups; dynamic LDS as dsgd_lg_eval_kernel; tally: [t.n][LG_TALLY_WORDS], zero on entry
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_eval_ranges_kernel(CsrView m, const float* __restrict__ w, LgEvalTable t,
                                                                             unsigned long long* tally, int hw, double* loss_part) {
  lg_eval_walk(m, w, hw, LgRowsTable{t}, LgTallyRanges{tally}, LgNoExtra{}, loss_part);
}

// p_out[tp][n] (TOPICS: T weight vectors w_stride apart, the row's registers fetched once; else one)
template <bool TOPICS>
__device__ __forceinline__ void lg_predict_body(const CsrView& m, const float* __restrict__ w, long long w_stride, int T, const int* __restrict__ idx,
                                                long long n, float* p_out, DevScalars* sc) {
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
    if constexpr (!TOPICS) {
      const float d = row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, w, 0, sub, r);
      if (sub == 0) p_out[t] = lg_sigma(d);
    } else {
      lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
      for (int tp = 0; tp < T; ++tp) {
        const float d = lgt_row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, w + (long long)tp * w_stride, 0, sub, r);
        if (sub == 0) p_out[(long long)tp * n + t] = lg_sigma(d);
      }
    }
  }
}
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_predict_kernel(CsrView m, const float* __restrict__ w, const int* __restrict__ idx,
                                                                    long long n, float* p_out, DevScalars* sc) {
  lg_predict_body<false>(m, w, 0, 1, idx, n, p_out, sc);
}
