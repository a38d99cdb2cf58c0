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
// Launches:
//   lg_grad_body<LIST>        one 16-lane group per listed position (LIST: dsgd_lg_grad_kernel) or per row of a range
//                             (dsgd_lg_grad_range_kernel).  row_dot with RowRegs: the first LG_UNR * 16 non-zeros of the row stay
//                             in registers for the scatter.  c_i once per row on every lane (group_sum leaves the same d on all
//                             16), then every non-zero becomes rn(c_i * x * 2^(S - vexp)), S = 62 - ceil(log2 n), added into the
//                             worker's int64 column accumulators: ranks below LG_HOT in an LDS tile (ds_add_u64, flushed once
//                             per touched word), the others with 64-bit global vector atomics.  Grid: K x blocks_per_worker.
//                             Integer adds do not depend on their order: a step's weights are the same bits whatever the
//                             list's order, the grid's shape or the run.
//   dsgd_lg_finish_kernel<M>  ONE column per lane, in fp64 with contraction off: G_k = acc_k 2^(vexp - S_k), r_k = G_k + 2 lambda w_j;
//                             LG_GRADIENT: (float)r_0 to g_out in key order; LG_STEP: the r_k added in worker order, / K,
//                             w_j' = (float)(w_j - lr mean): one rounding to float per step.  The accumulators are left zeroed.
//                             LG_STEP also leaves |w'|^2 per workgroup (lg_block_sum: a fixed tree) in nsq_part[blockIdx.x]:
//                             the host adds the words in order, so a following evaluation needs no pass over w.
//   dsgd_lg_finish_kernel<LG_STEP, true>  the GATHERED finish of a step across ranks (dsgd_comm_init_lg; csrc/dsgd_lg_gather.hpp): the
//                             same body over the K = k * world slots behind the all-reduce, in global worker order; a worker's n
//                             comes from the header words (uniform reads), vexp is the call's agreed one.  The first lane also
//                             adds the job's rows of the step to the context's n_samples.
//   dsgd_lg_header_kernel     in front of such a step's all-reduce: the K header words -- this rank's k lengths from its WorkSegs
//                             at its own positions, zero everywhere else (so the words of the previous step are gone)
//   dsgd_lg_nsq_kernel        the same per-workgroup sums of |w|^2 from weights the finish did not write (the same grid, the
//                             same tree: the same bits)
//   dsgd_lg_eval_kernel       persistent 1024-lane workgroups, the hw hottest weights in LDS (the shape of dsgd_eval_kernel): the
//                             three class tallies (signum(d) == y, == 0, == -y) through block_tally3, and the sum of l_i by a
//                             FIXED-ORDER TREE -- a group's lane 0 adds its rows in row order, the wave's lanes fold by xor
//                             butterflies, lane 0 of the workgroup adds the sixteen wave sums in order, the host adds the
//                             workgroups' words in order.  The grid is a function of the range and the device alone, so the
//                             same call gives the same bits; nothing is added with floating-point atomics.  Every l_i carries
//                             at most |d_i - d_i,exact| and a few fp64 roundings of error, the tree at most (n + 64) 2^-53 of the sum
//                             (tests/logistic_bound.py: dloss).
//   dsgd_lg_eval_ranges_kernel  the same for up to 16 row ranges in ONE launch: every range has its own run of workgroups (the grid
//                             of a launch over it alone: the same bits), its own partial sums and its own tally words
//   dsgd_lg_predict_kernel    sigma(d) per listed position: 1 / (1 + exp(-d)) in fp64 from the fp32 d, rounded to float once.
//   dsgd_lg_async_finish_kernel  the finish of ONE worker's ASYNCHRONOUS update behind lg_grad_body with K = 1: the mean over the
//                             list's n rows, regularised once, w_j' = (float)(w_j - lr r); optionally the double delta
//   dsgd_lg_update_kernel     a peer's update from (key, dv) pairs: w_k = (float)((double)w_k - dv_k)
//
// Plain C++ and vector atomics only.
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

__device__ __forceinline__ void lg_add(unsigned long long* hot, unsigned long long* acc, int c, float x, double cq) {
#pragma clang fp contract(off)
  const long long q = __double2ll_rn((double)x * cq);   // |x cq| <= 2^S <= 2^62
  if (q == 0) return;                                     // (a zero adds nothing: the padding entry of an empty row, c = -+0)
  if (c < LG_HOT)
    atomicAdd(&hot[c], (unsigned long long)q);            // (two's complement: one add)
  else
    atomicAdd(&acc[c], (unsigned long long)q);
}

template <bool LIST>
__device__ __forceinline__ void lg_grad_body(const CsrView& m, const LgArgs& a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hot[LG_HOT];
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  unsigned long long* acc = a.acc + (long long)k * a.acc_stride;
  const int sub = tid % LG_GROUP;
  const long long groups = a.blocks_per_worker * LG_ROWS_PER_BLOCK;
  for (int j = tid; j < LG_HOT; j += LG_THREADS) hot[j] = 0ull;
  __syncthreads();
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = LIST ? (long long)a.idx[seg.begin + t] : seg.begin + t;
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists and the ranges: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, false>(m, st, en, nullptr, a.w, 0, sub, r);
    const double cq = lg_coef(d, (double)m.label[row]) * qscale;
#pragma unroll
    for (int u = 0; u < LG_UNR; ++u)
      if (r.c[u] >= 0) lg_add(hot, acc, r.c[u], r.v[u], cq);
    for (long long p = st + sub + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) lg_add(hot, acc, m.col[p], m.val[p], cq);
  }
  __syncthreads();
  for (int j = tid; j < LG_HOT; j += LG_THREADS) {   // (a word is non-zero only below dp)
    const unsigned long long v = hot[j];
    if (v) atomicAdd(&acc[j], v);
  }
}
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_grad_kernel(CsrView m, LgArgs a) { lg_grad_body<true>(m, a); }
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_grad_range_kernel(CsrView m, LgArgs a) { lg_grad_body<false>(m, a); }

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

// grid: lg_finish_blocks(dp) workgroups -- ONE column per lane
template <int MODE, bool GATHERED = false>
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_finish_kernel(LgFinishArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  double sq = 0.0;
  if (j < a.dp) {
    const int r = MODE == LG_STEP ? j : a.perm[j];
    const double wj = (double)a.w[r];
    const double reg = (2.0 * a.lambda) * wj;
    double sum = 0.0;
    for (int k = 0; k < (MODE == LG_STEP ? a.K : 1); ++k) {
      unsigned long long* at = a.acc + (long long)k * a.acc_stride + r;
      const unsigned long long t = *at;
      if (t != 0ull) *at = 0ull;
      const long long n = GATHERED ? (long long)a.hdr[k] : a.segs[k].end - a.segs[k].begin;
      const double G = (double)(long long)t * ldexp(1.0, a.vexp - lg_shift(n));   // one rounding of the exact sum
      sum = sum + (G + reg);
    }
    if (MODE == LG_GRADIENT) {
      a.g_out[j] = (float)sum;
    } else {
      const double mean = sum / (double)a.K;
      const float wn = (float)(wj - a.lr * mean);
      a.w[r] = wn;
      sq = (double)wn * (double)wn;
    }
  }
  if (MODE == LG_STEP) {
    const double s = lg_block_sum(sq, red, LG_THREADS / 64);
    if (threadIdx.x == 0) a.nsq_part[blockIdx.x] = s;
  }
  if (GATHERED && blockIdx.x == 0 && threadIdx.x == 0) {   // the job's rows of this step (every row contributes)
    unsigned long long rows = 0ull;
    for (int k = 0; k < a.K; ++k) rows += a.hdr[k];
    atomicAdd(&a.sc->n_samples, rows);
  }
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
//   G = acc 2^(vexp - S),  gm = G / n,  r = gm + 2 lambda w_j,  delta = lr r,  w_j' = (float)(w_j - delta)
// one rounding to float; the accumulators left zeroed; |w'|^2 per workgroup in nsq_part by LG_STEP's grid and tree.  For
// n = 1 these are the bits of dsgd_lg_finish_kernel<LG_STEP> with K = 1 (G / 1.0 = G, 0.0 + (G + reg) = G + reg, G never -0.0).
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
    unsigned long long* at = a.acc + j;
    const unsigned long long t = *at;
    if (t != 0ull) *at = 0ull;
    const double G = (double)(long long)t * ldexp(1.0, a.vexp - lg_shift(n));   // one rounding of the exact sum
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

// grid: lg_finish_blocks(dp), as the finish
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_nsq_kernel(const float* __restrict__ w, int dp, double* nsq_part) {
#pragma clang fp contract(off)
  __shared__ double red[LG_THREADS / 64];
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  const double wj = j < dp ? (double)w[j] : 0.0;
  const double s = lg_block_sum(wj * wj, red, LG_THREADS / 64);
  if (threadIdx.x == 0) nsq_part[blockIdx.x] = s;
}

// dynamic LDS, in floats: [0, hw) the hot weights, 4 tally words, then (8-byte aligned) the sixteen wave sums
__host__ __device__ constexpr int lg_eval_red_at(int hw) { return (hw + 4 + 1) & ~1; }
__host__ __device__ constexpr int lg_eval_lds_floats(int hw) { return lg_eval_red_at(hw) + 2 * (LG_EVAL_THREADS / 64); }

__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_eval_kernel(CsrView m, const float* __restrict__ w, long long row_begin,
                                                                      long long row_end, DevScalars* sc, int hw, double* loss_part) {
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
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], wl, w, hw, sub, r);
    if (sub == 0) {
      const double a = (double)m.label[row] * (double)d;   // (exact)
      if (a > 0.0) c0++;         // signum(d) == y
      else if (a < 0.0) c2++;    // signum(d) == -y
      else c1++;                 // d == +-0: class 0
      ls = ls + lg_loss(a);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&sc->counts[3], (unsigned long long)(row_end - row_begin));
  block_tally3(c0, c1, c2, sc, reinterpret_cast<unsigned int*>(wl + hw));
  const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lg_eval_red_at(hw)), LG_EVAL_THREADS / 64);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = s;
}

// block_tally3 into a range's own words (DevScalars::counts holds one set)
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

// Up to LG_MAX_RANGES row ranges in ONE launch (csrc/dsgd_lg_host.hpp: lg_eval_table).  A workgroup belongs to ONE range and
// walks it as dsgd_lg_eval_kernel's workgroup of the same number walks it in a launch over that range alone: the same rows in
// the same order, the same tree, its sum in loss_part[blockIdx.x] -- the host adds a range's words in order.  The tallies go
// to the range's own LG_TALLY_WORDS words of `tally` (zero on entry).  The tile size hw moves no bit: a weight is the same
// float from LDS as from memory, and row_dot adds a lane's products in the order of the row either way.
// grid: t.grid workgroups; dynamic LDS as dsgd_lg_eval_kernel
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_eval_ranges_kernel(CsrView m, const float* __restrict__ w, LgEvalTable t,
                                                                             unsigned long long* tally, int hw, double* loss_part) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;
  for (int j = threadIdx.x; j < hw; j += LG_EVAL_THREADS) wl[j] = w[j];
  __syncthreads();
  // this workgroup's range (the same on every lane; selects, not an indexed read of the argument)
  int range = 0, first = 0, blocks = t.r[0].n_blocks;
  long long row_begin = t.r[0].row_begin, row_end = t.r[0].row_end;
#pragma unroll
  for (int i = 1; i < LG_MAX_RANGES; ++i) {
    if (i < t.n && (int)blockIdx.x >= t.r[i].first_block) {
      range = i;
      first = t.r[i].first_block;
      blocks = t.r[i].n_blocks;
      row_begin = t.r[i].row_begin;
      row_end = t.r[i].row_end;
    }
  }
  const int sub = threadIdx.x % LG_GROUP;
  const long long group = ((long long)((int)blockIdx.x - first) * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = (long long)blocks * LG_EVAL_THREADS / LG_GROUP;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  double ls = 0.0;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], wl, w, hw, sub, r);
    if (sub == 0) {
      const double a = (double)m.label[row] * (double)d;   // (exact)
      if (a > 0.0) c0++;
      else if (a < 0.0) c2++;
      else c1++;
      ls = ls + lg_loss(a);
    }
  }
  lg_block_tally3(c0, c1, c2, tally + range * LG_TALLY_WORDS, reinterpret_cast<unsigned int*>(wl + hw));
  const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lg_eval_red_at(hw)), LG_EVAL_THREADS / 64);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_predict_kernel(CsrView m, const float* __restrict__ w, const int* __restrict__ idx,
                                                                    long long n, float* p_out, DevScalars* sc) {
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
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, false>(m, m.row_ptr[row], m.row_ptr[row + 1], nullptr, w, 0, sub, r);
    if (sub == 0) p_out[t] = (float)(1.0 / (1.0 + exp(-(double)d)));
  }
}
