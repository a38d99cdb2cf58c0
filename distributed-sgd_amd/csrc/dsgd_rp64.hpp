// Device code of libdsgd_hip, part 9 (gfx950 only): the fp64 mode's row-parallel gradient family -- the request /
// response gradient of one worker (SlaveImpl.gradient in Double, core/Slave.scala:142-157) and synchronous steps of ANY
// number of workers and rows (Master.fit's batch closure, core/Master.scala:184-197), where the column-slice plans of
// dsgd_cs64.hpp stop (<= 4 workers, <= 1,024 rows per step).  Included by dsgd_hip.hip after dsgd_cs64.hpp.
//
// Two launches per call:
//   dsgd_rp64_grad_kernel    one 16-lane group per listed row: x . w in fp64 (filt((double)x * w) per entry, as
//                            row_dot64), the gate !(y * d < 0) (core/ml/SparseSVM.scala:27-28), and for an active row
//                            y * x added into the worker's 64-bit fixed-point column accumulators (rank order) with integer
//                            atomics.  The last workgroup of the grid computes s = lambda * 2 * (w . ds) meanwhile.
//   dsgd_rp64_finish_kernel  per column: ONE rounding of each worker's exact sum, the support-only regulariser, and either
//                            the gradient in key order or the step's fold over the workers, mean and update
//                            (oracle/oracle.c orc_gradient / orc_sync_step, operation for operation); the accumulators are
//                            left zeroed for the next call.
//
// Under a communicator (dsgd_comm_init_f64; "across ranks" below) the sums go into this rank's slots of a gather buffer
// (dsgd_rp64_grad_gather_kernel: the same body), the buffer travels, dsgd_rp64_header_kernel turns the gathered headers
// into the finish's list ranges, and dsgd_rp64_finish_kernel<true> folds every rank's workers.
//
// The grid: a worker's list of n rows (duplicates count) adds entries of |x| <= 2^vexp scaled by 2^shift, shift = 62 -
// ceil(log2 n): no column sum leaves the 64-bit range.  Integer sums do not depend on the order of the adds -- the result
// is bit-reproducible, whatever the list's order or the grid.  An entry of exponent e is exact on the grid when
// e >= vexp - (39 - ceil(log2 n)) (include/dsgd.h "THE FP64 MODE").
//
// The weights are read (and a step's update written) in whichever layout they are: rank order (Sp = 0) or the column
// slices' slice-major [CS64_G][Sp] (dsgd_update64_kernel's rule).  Every function opens with
// `#pragma clang fp contract(off)`, as in dsgd_cs64.hpp.
#pragma once

constexpr int RP64_THREADS = 256;
constexpr int RP64_GROUP = 16;   // lanes per row (row_dot64<16>)
// the hottest column ranks (the CSR's columns are ranked by frequency: rank 0 is in most rows) are summed per workgroup
// in LDS (ds_add_u64) and flushed once per touched word: plain global atomics serialise on those few addresses (a list
// of 65,536 rows: 1.9 ms, 13x the fp32 gradient)
constexpr int RP64_HOT = 1024;

__device__ __forceinline__ long long rp64_at(long long r, int Sp) { return Sp ? (r % CS64_G) * Sp + r / CS64_G : r; }
__host__ __device__ constexpr int rp64_ceil_log2(long long n) {
  int l = 0;
  while ((1LL << l) < n) ++l;
  return l;
}
__host__ __device__ constexpr int rp64_shift(long long n) { return 62 - rp64_ceil_log2(n); }

// ---- across ranks (a communicator attached with dsgd_comm_init_f64) ----
// The gather buffer of a step of k hosted workers in a world of W ranks, K = k * W, 64-bit words, zero between calls:
//   [W (padded to 64)]   one word per rank: the k it was called with (the ranks must agree before the slots travel)
//   [K][stride]          global worker r * k + j's slot: [0, dp) its fixed-point column sums, rank order, then its header
//                        words -- the list length n (its shift is 62 - ceil(log2 n)) and its active count
// A slot is non-zero on exactly ONE rank, so ncclAllReduce(ncclInt64, ncclSum) over the buffer IS the all-gather: exact,
// whatever the order of the sum.  Behind it every rank holds every worker's integers and folds them in worker order with
// dsgd_rp64_finish_kernel<true> itself -- the bits of ONE process that hosts the K workers.
constexpr int RP64_HDR_N = 0, RP64_HDR_ACTIVE = 1, RP64_HDR_WORDS = 2;
// one message of the gather: at most 1 MiB (a slot is 378 KB at RCV1's D; wider slots are cut)
constexpr long long RP64_MSG_WORDS = (1LL << 20) / (long long)sizeof(unsigned long long);
__host__ __device__ constexpr long long rp64_gather_stride(int dp) { return ((long long)dp + RP64_HDR_WORDS + 63) & ~63LL; }

struct Rp64Args {
  CsrView m;
  const double* w;                 // the weights, rank order (Sp = 0) or slice-major
  const double* ds;                // dimSparsity, rank order
  int Sp, dp, vexp, K;
  const int* idx;                  // the lists, concatenated
  const WorkSeg* segs;             // [K] each worker's [begin, end) in idx
  long long blocks_per_worker;     // grid = K * blocks_per_worker + 1 (the last workgroup: s)
  unsigned long long* acc;         // [K][acc_stride] fixed-point column sums, rank order; zero on entry
  long long acc_stride;
  double lambda;
  double* s_out;                   // s = lambda * 2.0 * (w . ds)
  DevScalars* sc;                  // n_active, err (1: a row index outside the data)
  unsigned long long* rank_word;   // (the gather of a communicator only) this rank's word of the gather buffer: K
};

// x . w of `row` by the 16 lanes of a group, in whichever layout the weights are (row_dot64's arithmetic and order)
__device__ __forceinline__ double rp64_row_dot(const CsrView& m, long long row, const double* __restrict__ w, int Sp, int sub) {
#pragma clang fp contract(off)
  if (Sp == 0) return row_dot64<RP64_GROUP>(m, row, w, sub);
  const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
  double d = 0.0;
  for (long long p = st + sub; p < en; p += RP64_GROUP) d = d + filt64((double)m.val[p] * w[rp64_at(m.col[p], Sp)]);
#pragma unroll
  for (int off = RP64_GROUP / 2; off >= 1; off >>= 1) d = d + __shfl_xor(d, off, RP64_GROUP);
  return d;
}

// GATHER: `acc` are this rank's K slots of a communicator's gather buffer (see below) -- a slot's header words get the
// list length and the active count, the rank's word gets K, all with ordinary stores / vector atomics
template <bool GATHER>
__device__ __forceinline__ void rp64_grad_body(const Rp64Args& a) {
#pragma clang fp contract(off)
  __shared__ double red[RP64_THREADS / 64];
  __shared__ unsigned int n_act;
  __shared__ unsigned long long hot[RP64_HOT];
  const int tid = threadIdx.x;
  const long long last = (long long)gridDim.x - 1;
  if ((long long)blockIdx.x == last) {
    // ---- s of the weights the rows see: filt(w * ds) per column (orc_dense_dot), lane-strided, then the wave
    //      butterflies and the four wave sums in order: the same bits on every call ----
    double v = 0.0;
    for (int r = tid; r < a.dp; r += RP64_THREADS) v = v + filt64(a.w[rp64_at(r, a.Sp)] * a.ds[r]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) *a.s_out = a.lambda * 2.0 * ((red[0] + red[1]) + (red[2] + red[3]));   // ref: core/ml/SparseSVM.scala:31
    if (GATHER && tid == 0) *a.rank_word = (unsigned long long)a.K;
    return;
  }
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, rp64_shift(n) - a.vexp);   // (a power of two: x * qscale is exact)
  unsigned long long* acc = a.acc + (long long)k * a.acc_stride;
  const int sub = tid % RP64_GROUP;
  const long long groups = a.blocks_per_worker * (RP64_THREADS / RP64_GROUP);
  if (tid == 0) n_act = 0u;
  for (int i = tid; i < RP64_HOT; i += RP64_THREADS) hot[i] = 0ull;
  __syncthreads();
  unsigned int mine = 0u;
  for (long long t = b * (RP64_THREADS / RP64_GROUP) + tid / RP64_GROUP; t < n; t += groups) {
    const long long row = a.idx[seg.begin + t];
    if (row < 0 || row >= a.m.n_rows) {   // (the host checked the lists: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const double d = rp64_row_dot(a.m, row, a.w, a.Sp, sub);
    const double y = (double)a.m.label[row];
    if (y * d < 0.0) continue;                                   // ref: core/ml/SparseSVM.scala:27-28 (zerosLike)
    mine += sub == 0 ? 1u : 0u;
    const double cq = y > 0.0 ? qscale : -qscale;
    const long long st = a.m.row_ptr[row], en = a.m.row_ptr[row + 1];
    for (long long p = st + sub; p < en; p += RP64_GROUP) {
      const float x = a.m.val[p];
      if (!(fabs((double)x) > CS64_EPS)) continue;   // filt(x * y): the Sparse constructor's filter (math/Sparse.scala:104)
      const long long q = __double2ll_rn((double)x * cq);
      const int c = a.m.col[p];
      if (q == 0) continue;
      if (c < RP64_HOT)
        atomicAdd(&hot[c], (unsigned long long)q);
      else
        atomicAdd(&acc[c], (unsigned long long)q);
    }
  }
  if (mine) atomicAdd(&n_act, mine);
  __syncthreads();
  for (int i = tid; i < RP64_HOT; i += RP64_THREADS) {   // (a word is non-zero only below dp)
    const unsigned long long v = hot[i];
    if (v) atomicAdd(&acc[i], v);
  }
  if (GATHER) {
    if (tid == 0 && b == 0) acc[a.dp + RP64_HDR_N] = (unsigned long long)n;   // (zero until here, like every word of the slot)
    if (tid == 0 && n_act) atomicAdd(&acc[a.dp + RP64_HDR_ACTIVE], (unsigned long long)n_act);
  } else {
    if (tid == 0 && n_act) atomicAdd(&a.sc->n_active, (unsigned long long)n_act);
  }
}
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_grad_kernel(Rp64Args a) { rp64_grad_body<false>(a); }

struct Rp64FinishArgs {
  unsigned long long* acc;   // [K][acc_stride], zeroed here
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the list lengths give each worker's shift
  int K, dp, vexp, Sp;
  const double* s;           // from dsgd_rp64_grad_kernel
  const int* perm;           // key -> rank
  double* g_out;             // GRADIENT: the regularised sum of worker 0, key order
  double* w;                 // STEP: the weights, updated in their layout
  double lr;
};

// GRADIENT: over keys j, g[j] of the one worker (orc_gradient).  STEP: over ranks r, the fold over the workers in worker
// order, filt(acc / K), filt(mean * lr), filt(w - upd) (orc_sync_step; w is filtered already: a column without a
// gradient keeps its value, which is what filt(w - 0) gives)
template <bool STEP>
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_finish_kernel(Rp64FinishArgs a) {
#pragma clang fp contract(off)
  const double s = *a.s;
  const bool add = fabs(s) > CS64_EPS;   // (regularize_inplace: s == 0 or filtered away -> g unchanged)
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < a.dp; j += gridDim.x * blockDim.x) {
    const int r = STEP ? j : a.perm[j];
    double gsum = 0.0;
    for (int k = 0; k < (STEP ? a.K : 1); ++k) {
      unsigned long long* at = a.acc + (long long)k * a.acc_stride + r;
      const long long t = (long long)*at;
      if (t != 0) *at = 0ull;
      const double inv_scale = ldexp(1.0, a.vexp - rp64_shift(a.segs[k].end - a.segs[k].begin));
      const double g0 = filt64((double)t * inv_scale);           // one rounding of the exact sum (the power of two is exact)
      const double g = (add && g0 != 0.0) ? filt64(g0 + s) : g0;  // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
      if (!STEP) {
        a.g_out[j] = g;
      } else {
        gsum = filt64(gsum + g);                                  // Vec.sum over the workers
      }
    }
    if (STEP && gsum != 0.0) {
      const double mean = filt64(gsum / (double)a.K);             // Vec.mean (correctly rounded division)
      const double upd = filt64(mean * a.lr);                     // learningRate * grad (ref: core/Master.scala:194-197)
      const long long at = rp64_at(r, a.Sp);
      a.w[at] = filt64(a.w[at] - upd);
    }
  }
}

__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_grad_gather_kernel(Rp64Args a) { rp64_grad_body<true>(a); }

// Behind the gather, ONE workgroup: the K headers become the list ranges the finish takes its shifts from ({0, n}), the
// job's samples and active rows go to the context's scalars, and the header and rank words are zeroed again (the
// finish zeroes the sums: the whole buffer is zero for the next call)
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_header_kernel(unsigned long long* rank_words, int W, unsigned long long* slots,
                                                                        long long stride, int K, int dp, WorkSeg* segs, DevScalars* sc) {
  __shared__ unsigned long long tot[2];
  const int tid = threadIdx.x;
  if (tid < 2) tot[tid] = 0ull;
  __syncthreads();
  unsigned long long n_sum = 0ull, a_sum = 0ull;
  for (int k = tid; k < K; k += RP64_THREADS) {
    unsigned long long* h = slots + (long long)k * stride + dp;
    const unsigned long long n = h[RP64_HDR_N], act = h[RP64_HDR_ACTIVE];
    h[RP64_HDR_N] = 0ull;
    h[RP64_HDR_ACTIVE] = 0ull;
    WorkSeg sg;
    sg.begin = 0;
    sg.end = (long long)n;
    segs[k] = sg;
    n_sum += n;
    a_sum += act;
  }
  if (n_sum) atomicAdd(&tot[0], n_sum);
  if (a_sum) atomicAdd(&tot[1], a_sum);
  for (int r = tid; r < W; r += RP64_THREADS) rank_words[r] = 0ull;
  __syncthreads();
  if (tid == 0) {
    sc->n_samples = tot[0];
    sc->n_active = tot[1];
  }
}
