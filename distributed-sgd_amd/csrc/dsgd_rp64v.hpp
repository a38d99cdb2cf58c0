// Device code of libdsgd_hip, part 10 (gfx950 only): the fp64 mode on DOUBLE feature values (dsgd_load_csr_f64) -- the
// reference reads `elems(1).toDouble` (utils/Dataset.scala:30) and keeps every digit of the file.  The row-parallel pair
// of dsgd_rp64.hpp again, over a value array of doubles parallel to the CSR, and the evaluation and counting kernels that
// read a value.  Included by dsgd_hip.hip after dsgd_rp64.hpp.
//
//   dsgd_rp64v_grad_kernel    one 16-lane group per listed row: x . w (filt(x * w) per entry, row_dot64's lane order and
//                             butterfly), the gate !(y * d < 0) (core/ml/SparseSVM.scala:27-28), and for an active row
//                             y * x added into the worker's TWO-WORD fixed-point column accumulators.  The last
//                             workgroup computes s = lambda * 2 * (w . ds) meanwhile.
//   dsgd_rp64v_finish_kernel  per column ONE rounding of the exact two-word sum (dsgd_round128.hpp), then
//                             orc_gradient / orc_sync_step / orc_async_step operation for operation; the accumulators
//                             are left zeroed for the next call.
//
// The grid.  A worker's list of n rows adds entries of |x| <= 2^vexp.  With S = 62 - ceil(log2 n) and v = +-x * 2^(S - vexp)
// (a power of two: exact),
//   h  = floor(v)              into a signed 64-bit word HI      (|h| <= 2^S: n of them stay inside 2^62)
//   lo = rn((v - h) * 2^32)    into an unsigned 64-bit word LO   (v - h is exact and in [0, 1): lo <= 2^32, n of them
//                                                                 stay inside 2^63 -- no carry between the words)
// and the sum is (HI * 2^32 + LO) * 2^(vexp - S - 32).  A double of exponent e (|x| in [2^e, 2^(e+1))) has its last bit at
// 2^(e - 52): it is exact on the grid when e >= vexp - (42 - ceil(log2 n)), no narrower than the float values' range of
// dsgd_rp64.hpp; below that an entry is off by at most half a grid unit.  Integer sums do not depend on the order of the
// adds: the result is bit-reproducible whatever the list's order or the launch's shape.  A value a float holds exactly
// inside the float grid's range has lo == 0 and h equal to that grid's integer: the second atomic is skipped, and the
// result has the bits of dsgd_rp64_grad_kernel.
//
// Every function opens with `#pragma clang fp contract(off)`, as in dsgd_cs64.hpp.
#pragma once
#include "dsgd_round128.hpp"

struct CsrView64 {
  long long n_rows;
  const long long* __restrict__ row_ptr;
  const int* __restrict__ col;   // frequency-ranked ids
  const double* __restrict__ val;
  const signed char* __restrict__ label;
};

struct Rp64vArgs {
  CsrView64 m;
  const double* w;                 // the weights, rank order (Sp = 0) or slice-major
  const double* ds;                // dimSparsity, rank order
  int Sp, dp, vexp, K;
  const int* idx;                  // the lists, concatenated
  const WorkSeg* segs;             // [K] each worker's [begin, end) in idx
  long long blocks_per_worker;     // grid = K * blocks_per_worker + with_s
  int with_s;                      // 1: one more workgroup, the last, computes s (0: the caller's own kernel does)
  long long* hi;                   // [K][acc_stride] the high words, rank order; zero on entry
  unsigned long long* lo;          // [K][acc_stride] the low words
  long long acc_stride;
  double lambda;
  double* s_out;                   // s = lambda * 2.0 * (w . ds)
  DevScalars* sc;                  // n_active, err (1: a row index outside the data)
};

// x . w of `row` by the 16 lanes of a group, in whichever layout the weights are (row_dot64's arithmetic and order)
__device__ __forceinline__ double rp64v_row_dot(const CsrView64& m, long long row, const double* __restrict__ w, int Sp, int sub) {
#pragma clang fp contract(off)
  const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
  double d = 0.0;
  for (long long p = st + sub; p < en; p += RP64_GROUP) d = d + filt64(m.val[p] * w[rp64_at(m.col[p], Sp)]);
#pragma unroll
  for (int off = RP64_GROUP / 2; off >= 1; off >>= 1) d = d + __shfl_xor(d, off, RP64_GROUP);
  return d;
}

__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_grad_kernel(Rp64vArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[RP64_THREADS / 64];
  __shared__ unsigned int n_act;
  __shared__ unsigned long long hot_hi[RP64_HOT];
  __shared__ unsigned long long hot_lo[RP64_HOT];
  const int tid = threadIdx.x;
  const long long last = a.with_s ? (long long)gridDim.x - 1 : -1;
  if ((long long)blockIdx.x == last) {
    // ---- s of the weights the rows see (dsgd_rp64_grad_kernel's order: the same bits) ----
    double v = 0.0;
    for (int r = tid; r < a.dp; r += RP64_THREADS) v = v + filt64(a.w[rp64_at(r, a.Sp)] * a.ds[r]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) *a.s_out = a.lambda * 2.0 * ((red[0] + red[1]) + (red[2] + red[3]));   // ref: core/ml/SparseSVM.scala:31
    return;
  }
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, rp64_shift(n) - a.vexp);   // (a power of two: x * qscale is exact)
  unsigned long long* hi = reinterpret_cast<unsigned long long*>(a.hi) + (long long)k * a.acc_stride;   // (two's complement: one add)
  unsigned long long* lo = a.lo + (long long)k * a.acc_stride;
  const int sub = tid % RP64_GROUP;
  const long long groups = a.blocks_per_worker * (RP64_THREADS / RP64_GROUP);
  if (tid == 0) n_act = 0u;
  for (int i = tid; i < RP64_HOT; i += RP64_THREADS) {
    hot_hi[i] = 0ull;
    hot_lo[i] = 0ull;
  }
  __syncthreads();
  unsigned int mine = 0u;
  for (long long t = b * (RP64_THREADS / RP64_GROUP) + tid / RP64_GROUP; t < n; t += groups) {
    const long long row = a.idx[seg.begin + t];
    if (row < 0 || row >= a.m.n_rows) {   // (the host checked the lists: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const double d = rp64v_row_dot(a.m, row, a.w, a.Sp, sub);
    const double y = (double)a.m.label[row];
    if (y * d < 0.0) continue;                                   // ref: core/ml/SparseSVM.scala:27-28 (zerosLike)
    mine += sub == 0 ? 1u : 0u;
    const double cq = y > 0.0 ? qscale : -qscale;
    const long long st = a.m.row_ptr[row], en = a.m.row_ptr[row + 1];
    for (long long p = st + sub; p < en; p += RP64_GROUP) {
      const double x = a.m.val[p];
      if (!(fabs(x) > CS64_EPS)) continue;   // filt(x * y): the Sparse constructor's filter (math/Sparse.scala:104)
      const double v = x * cq;
      const double fl = floor(v);
      const long long h = (long long)fl;                                        // |fl| <= 2^62: exact
      const unsigned long long l = (unsigned long long)__double2ll_rn((v - fl) * 4294967296.0);   // v - fl: exact, in [0, 1)
      const int c = a.m.col[p];
      if (c < RP64_HOT) {
        if (h != 0) atomicAdd(&hot_hi[c], (unsigned long long)h);
        if (l != 0ull) atomicAdd(&hot_lo[c], l);
      } else {
        if (h != 0) atomicAdd(&hi[c], (unsigned long long)h);
        if (l != 0ull) atomicAdd(&lo[c], l);
      }
    }
  }
  if (mine) atomicAdd(&n_act, mine);
  __syncthreads();
  for (int i = tid; i < RP64_HOT; i += RP64_THREADS) {   // (a word is non-zero only below dp)
    const unsigned long long vh = hot_hi[i], vl = hot_lo[i];
    if (vh) atomicAdd(&hi[i], vh);
    if (vl) atomicAdd(&lo[i], vl);
  }
  if (tid == 0 && n_act) atomicAdd(&a.sc->n_active, (unsigned long long)n_act);
}

struct Rp64vFinishArgs {
  long long* hi;             // [K][acc_stride], zeroed here
  unsigned long long* lo;
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the list lengths give each worker's shift
  int K, dp, vexp, Sp;
  const double* s;           // from dsgd_rp64v_grad_kernel
  const int* perm;           // key -> rank
  double* g_out;             // GRADIENT: the regularised sum of worker 0, key order.  ASYNC: the delta, key order (may be null)
  double* w;                 // STEP, ASYNC: the weights, updated in their layout
  double lr;
};

constexpr int RP64V_GRADIENT = 0, RP64V_STEP = 1, RP64V_ASYNC = 2;

// GRADIENT: over keys j, g[j] of the one worker (orc_gradient).  STEP: over ranks r, the fold over the workers in worker
// order, filt(acc / K), filt(mean * lr), filt(w - upd) (orc_sync_step).  ASYNC: over keys j, the one worker's
// filt(g0 / n), the support-only regulariser, filt(g * lr) written to the delta, filt(w - upd) on EVERY coordinate
// (orc_async_step: the oracle writes filt(w - 0) where nothing is listed).
template <int MODE>
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_finish_kernel(Rp64vFinishArgs a) {
#pragma clang fp contract(off)
  const double s = *a.s;
  const bool add = fabs(s) > CS64_EPS;   // (regularize_inplace: s == 0 or filtered away -> g unchanged)
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < a.dp; j += gridDim.x * blockDim.x) {
    const int r = MODE == RP64V_STEP ? j : a.perm[j];
    double gsum = 0.0;
    for (int k = 0; k < (MODE == RP64V_STEP ? a.K : 1); ++k) {
      long long* ah = a.hi + (long long)k * a.acc_stride + r;
      unsigned long long* al = a.lo + (long long)k * a.acc_stride + r;
      const long long th = *ah;
      const unsigned long long tl = *al;
      if (th != 0) *ah = 0;
      if (tl != 0ull) *al = 0ull;
      const long long n = a.segs[k].end - a.segs[k].begin;
      const double g0 = filt64(dsgd_round128(th, tl, a.vexp - rp64_shift(n) - 32));   // one rounding of the exact sum
      if (MODE == RP64V_ASYNC) {
        const double gm = filt64(g0 / (double)n);                      // Vec.mean (correctly rounded division)
        const double g = (add && gm != 0.0) ? filt64(gm + s) : gm;     // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
        const double upd = filt64(g * a.lr);                           // learningRate * regularize(grad) (ref: core/Slave.scala:99)
        if (a.g_out != nullptr) a.g_out[j] = upd;
        const long long at = rp64_at(r, a.Sp);
        a.w[at] = filt64(a.w[at] - upd);                               // ref: core/Slave.scala:101
      } else {
        const double g = (add && g0 != 0.0) ? filt64(g0 + s) : g0;     // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
        if (MODE == RP64V_GRADIENT) {
          a.g_out[j] = g;
        } else {
          gsum = filt64(gsum + g);                                     // Vec.sum over the workers
        }
      }
    }
    if (MODE == RP64V_STEP && gsum != 0.0) {
      const double mean = filt64(gsum / (double)a.K);             // Vec.mean (correctly rounded division)
      const double upd = filt64(mean * a.lr);                     // learningRate * grad (ref: core/Master.scala:194-197)
      const long long at = rp64_at(r, a.Sp);
      a.w[at] = filt64(a.w[at] - upd);
    }
  }
}

// s = lambda * 2 * (w . ds) in the summation order of dsgd_cs64_async_kernel, ONE workgroup of CS_THREADS lanes: the
// asynchronous iteration on float data runs there, and a Double-data step on values a float holds must give its bits.
// Per slice b (rank r = b + CS64_G * i at position i; the padding zero) lane t adds the pairs i2 = t, t + CS_THREADS, ...
// as cs64_wds_share does, the workgroup sums as cs64_block_sum does, and the slices' sums are added in slice order from
// 0.0 (cs64_gather).  The weights are filtered as that kernel filters them on loading.
__global__ void __launch_bounds__(CS_THREADS) dsgd_rp64v_s_sliced_kernel(const double* __restrict__ w, const double* __restrict__ ds, int Sp_w,
                                                                        int dp, double lambda, double* s_out) {
#pragma clang fp contract(off)
  __shared__ double red[CS_THREADS / 64];
  const int Sp = cs64_sp(dp);
  double tot = 0.0;
  for (int b = 0; b < CS64_G; ++b) {
    double sp = 0.0;
    for (int i2 = threadIdx.x; i2 < (Sp >> 1); i2 += CS_THREADS) {
      const long long r0 = (long long)b + (long long)CS64_G * (2 * i2), r1 = r0 + CS64_G;
      const double w0 = r0 < dp ? filt64(w[rp64_at(r0, Sp_w)]) : 0.0, d0 = r0 < dp ? ds[r0] : 0.0;
      const double w1 = r1 < dp ? filt64(w[rp64_at(r1, Sp_w)]) : 0.0, d1 = r1 < dp ? ds[r1] : 0.0;
      sp = sp + (filt64(w0 * d0) + filt64(w1 * d1));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sp = sp + __shfl_xor(sp, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sp;
    __syncthreads();
    double t[CS_THREADS / 64];
#pragma unroll
    for (int i = 0; i < CS_THREADS / 64; ++i) t[i] = red[i];
#pragma unroll
    for (int n = CS_THREADS / 64; n > 1; n >>= 1)
#pragma unroll
      for (int i = 0; i < n / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    tot = tot + t[0];
  }
  if (threadIdx.x == 0) *s_out = lambda * 2.0 * tot;
}

// prediction p = -signum(x.w) on the Double values (dsgd_forward64_kernel's twin)
__global__ void __launch_bounds__(256) dsgd_forward64v_kernel(CsrView64 m, const double* __restrict__ w, const int* __restrict__ idx,
                                                             long long n, float* pred, DevScalars* sc) {
#pragma clang fp contract(off)
  const int sub = threadIdx.x % 16;
  const long long group = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / 16;
  const long long n_groups = (long long)gridDim.x * blockDim.x / 16;
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    const double d = rp64v_row_dot(m, row, w, 0, sub);
    if (sub == 0) pred[t] = d > 0.0 ? -1.0f : (d < 0.0 ? 1.0f : 0.0f);
  }
}

// loss / accuracy tallies on the Double values (dsgd_eval64_kernel's twin)
__global__ void __launch_bounds__(256) dsgd_eval64v_kernel(CsrView64 m, const double* __restrict__ w, long long row_begin, long long row_end,
                                                          DevScalars* sc) {
#pragma clang fp contract(off)
  __shared__ unsigned int tally[4];
  const int sub = threadIdx.x % 16;
  const long long group = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / 16;
  const long long n_groups = (long long)gridDim.x * blockDim.x / 16;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    const double d = rp64v_row_dot(m, row, w, 0, sub);
    const double yd = (double)m.label[row] * d;
    if (sub == 0) {
      if (yd < 0.0) c0++;
      else if (yd > 0.0) c2++;
      else c1++;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&sc->counts[3], (unsigned long long)(row_end - row_begin));
  block_tally3(c0, c1, c2, sc, tally);
}

// dimSparsity's feature counts on the Double values (dsgd_colcount_kernel's twin: abs(v) > 1e-20 decided on the double --
// (float)v may fall on the other side)
__global__ void __launch_bounds__(1024) dsgd_colcount64v_kernel(const int* __restrict__ col, const double* __restrict__ val, long long nnz,
                                                               unsigned int* cnt, int dp, int hcnt, DevScalars* sc) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned int lcnt64v[];
  for (int j = threadIdx.x; j < hcnt; j += 1024) lcnt64v[j] = 0u;
  __syncthreads();
  for (long long p = (long long)blockIdx.x * 1024 + threadIdx.x; p < nnz; p += (long long)gridDim.x * 1024) {
    const int c = col[p];
    if (!(fabs(val[p]) > CS64_EPS)) continue;
    if (c < 0 || c >= dp) {
      atomicOr(&sc->err, 1);
      continue;
    }
    if (c < hcnt) atomicAdd(&lcnt64v[c], 1u);
    else atomicAdd(&cnt[c], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < hcnt; j += 1024) {
    const unsigned int v = lcnt64v[j];
    if (v) atomicAdd(&cnt[j], v);
  }
}
