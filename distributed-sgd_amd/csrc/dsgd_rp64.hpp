// Device code of libdsgd_hip, part 9 (gfx950 only): the fp64 mode's row-parallel gradient family -- the request /
// response gradient of one worker (SlaveImpl.gradient in Double, core/Slave.scala:142-157) and synchronous steps of ANY
// number of workers and rows (Master.fit's batch closure, core/Master.scala:184-197), where the column-slice plans of
// dsgd_cs64.hpp stop (<= 4 workers, <= 1,024 rows per step) -- on float feature values and on DOUBLE ones
// (dsgd_load_csr_f64: the reference reads `elems(1).toDouble`, utils/Dataset.scala:30, and keeps every digit of the file;
// there also the asynchronous iteration, core/Slave.scala:99-101).  Included by dsgd_hip.hip after dsgd_cs64.hpp.
//
// Two launches per call, each ONE body over the value type V of the CSR view:
//   rp64_grad_body<V, GATHER>   one 16-lane group per listed row: x . w in fp64 (row_dot64: filt((double)x * w) per entry),
//                               the gate !(y * d < 0) (core/ml/SparseSVM.scala:27-28), and for an active row y * x added
//                               into the worker's fixed-point column accumulators (rank order) with integer atomics.  The
//                               last workgroup of the grid computes s = lambda * 2 * (w . ds) meanwhile (with_s).
//   rp64_finish_body<V, MODE>   per column: ONE rounding of each worker's exact sum, the support-only regulariser, and
//                               the gradient in key order (GRADIENT), the step's fold over the workers, mean and update
//                               (STEP), or one worker's asynchronous iteration and its delta (ASYNC; on float values only for
//                               row-parallel plans: float data's per-call step runs in dsgd_cs64_async_kernel) -- oracle/oracle.c orc_gradient /
//                               orc_sync_step / orc_async_step, operation for operation; the accumulators are left zeroed
//                               for the next call.
// The kernels are thin wrappers with stable names: dsgd_rp64_grad_kernel, dsgd_rp64_grad_gather_kernel,
// dsgd_rp64_finish_kernel<STEP> (float values), dsgd_rp64v_grad_kernel, dsgd_rp64v_grad_gather_kernel,
// dsgd_rp64v_finish_kernel<MODE> (Double values); for row-parallel plans (dsgd_plan_create_rp64_n and its kin) also
// dsgd_rp64_grad_rec_kernel / dsgd_rp64v_grad_rec_kernel (the gate record) and dsgd_rp64_finish_async_kernel.
//
// Under a communicator ("across ranks" below: dsgd_comm_init_f64 on float values, dsgd_comm_init_f64v on either type) the
// sums go into this rank's slots of a gather buffer (GATHER: dsgd_rp64_grad_gather_kernel, dsgd_rp64v_grad_gather_kernel),
// the buffer travels, dsgd_rp64_header_kernel turns the gathered headers into the finish's list ranges, and the SAME finish
// as without a communicator (dsgd_rp64_finish_kernel<true>, dsgd_rp64v_finish_kernel<RP64_STEP>) folds every rank's workers.
// A row-parallel PLAN's run under a communicator agrees once per call on the host (rp64_call_word) and then runs per step the
// gather kernels without the rank word (dsgd_rp64_grad_gather_plan_kernel, dsgd_rp64v_grad_gather_plan_kernel), the messages,
// dsgd_rp64_header_plan_kernel (no rank words; the job's samples and active rows run on) and the same finish.
//
// The grid.  A worker's list of n rows (duplicates count) adds entries of |x| <= 2^vexp.  With S = 62 - ceil(log2 n) and
// v = +-x * 2^(S - vexp) (a power of two: exact) an entry becomes Rp64Acc<V>::WORDS 64-bit integers, and no column sum of n
// of them leaves its word:
//   float values, ONE word    q  = rn(v)                 (|q| <= 2^S: n of them stay inside 2^62)
//   Double values, TWO words  h  = floor(v)              signed HI      (|h| <= 2^S)
//                             lo = rn((v - h) * 2^32)    unsigned LO    (v - h is exact and in [0, 1): lo <= 2^32, n of them
//                                                                        stay inside 2^63 -- no carry between the words)
// and the sum is q * 2^(vexp - S), or (HI * 2^32 + LO) * 2^(vexp - S - 32), rounded ONCE.  Integer sums do not depend on the
// order of the adds: the result is bit-reproducible whatever the list's order or the launch's shape.  An entry of exponent
// e (|x| in [2^e, 2^(e+1))) is exact on the grid when e >= vexp - (39 - ceil(log2 n)) as a float (its last bit is at
// 2^(e - 23)) and when e >= vexp - (42 - ceil(log2 n)) as a double (2^(e - 52)): the two-word range is no narrower; below
// it an entry is off by at most half a grid unit (include/dsgd.h "THE FP64 MODE").  A Double value that a float holds
// exactly inside the one-word range has lo == 0 and h == q: its second atomic is skipped and dsgd_round128 of (h, 0) is
// (double)q * 2^(vexp - S) -- the float-data call's bits.
//
// Rp64Acc<V>::quantise and Rp64Acc<V>::round are the ONLY code here that depends on the value type.
//
// The weights are read (and a step's update written) in whichever layout they are: rank order (Sp = 0) or the column
// slices' slice-major [CS64_G][Sp] (rp64_at).  Every function opens with `#pragma clang fp contract(off)`, as in
// dsgd_cs64.hpp.
#pragma once
#include "dsgd_round128.hpp"
#include "dsgd_rp64_gather.hpp"

constexpr int RP64_THREADS = 256;
constexpr int RP64_GROUP = 16;   // lanes per row (row_dot64<16>)
// the hottest column ranks (the CSR's columns are ranked by frequency: rank 0 is in most rows) are summed per workgroup
// in LDS (ds_add_u64) and flushed once per touched word: plain global atomics serialise on those few addresses (a list
// of 65,536 rows: 1.9 ms, 13x the fp32 gradient)
constexpr int RP64_HOT = 1024;

__host__ __device__ constexpr int rp64_ceil_log2(long long n) {
  int l = 0;
  while ((1LL << l) < n) ++l;
  return l;
}
__host__ __device__ constexpr int rp64_shift(long long n) { return 62 - rp64_ceil_log2(n); }

// ---- across ranks (a communicator attached with dsgd_comm_init_f64 or dsgd_comm_init_f64v) ----
// The gather buffer's layout -- the ranks' words, then per global worker a slot of one plane (float values) or two (Double
// values: HI with the header words, LO behind it) -- its message size and the rank word's encoding: dsgd_rp64_gather.hpp.

// ---- the accumulator policy: how one entry becomes integer words, and how the words' sums become ONE double ----
template <typename V>
struct Rp64Acc;
template <>
struct Rp64Acc<float> {
  static constexpr int WORDS = 1;
  __device__ __forceinline__ static void quantise(double v, unsigned long long (&q)[1]) {
#pragma clang fp contract(off)
    q[0] = (unsigned long long)__double2ll_rn(v);   // (two's complement: one add)
  }
  // the sum t[0] * 2^e2 (the power of two is exact)
  __device__ __forceinline__ static double round(const unsigned long long (&t)[1], int e2) {
#pragma clang fp contract(off)
    return (double)(long long)t[0] * ldexp(1.0, e2);
  }
};
template <>
struct Rp64Acc<double> {
  static constexpr int WORDS = 2;   // HI (signed), LO
  __device__ __forceinline__ static void quantise(double v, unsigned long long (&q)[2]) {
#pragma clang fp contract(off)
    const double fl = floor(v);
    q[0] = (unsigned long long)(long long)fl;                                  // |fl| <= 2^62: exact
    q[1] = (unsigned long long)__double2ll_rn((v - fl) * 4294967296.0);        // v - fl: exact, in [0, 1)
  }
  // the sum (t[0] * 2^32 + t[1]) * 2^(e2 - 32)
  __device__ __forceinline__ static double round(const unsigned long long (&t)[2], int e2) {
    return dsgd_round128((long long)t[0], t[1], e2 - 32);
  }
};
constexpr int RP64_MAX_WORDS = 2;

struct Rp64Args {
  const double* w;                 // the weights, rank order (Sp = 0) or slice-major
  const double* ds;                // dimSparsity, rank order
  int Sp, dp, vexp, K;
  const int* idx;                  // the lists, concatenated
  const WorkSeg* segs;             // [K] each worker's [begin, end) in idx
  long long blocks_per_worker;     // grid = K * blocks_per_worker + with_s
  int with_s;                      // 1: one more workgroup, the last, computes s (0: the caller's own kernel does)
  unsigned long long* acc[RP64_MAX_WORDS];   // per word [K][acc_stride] fixed-point column sums, rank order; zero on entry
  long long acc_stride;
  double lambda;
  double* s_out;                   // s = lambda * 2.0 * (w . ds)
  DevScalars* sc;                  // n_active, err (1: a row index outside the data)
  unsigned long long* rank_word;   // (the gather of a communicator only) this rank's word of the gather buffer: K and the value type
};

// GATHER: `acc[i]` are the planes of this rank's K slots of a communicator's gather buffer (dsgd_rp64_gather.hpp: one plane
// per word of a column sum, acc[1] = acc[0] + the plane's stride, acc_stride the slot's) -- the header words behind plane 0's
// sums get the list length and the active count, the rank's word gets K and the value type, all with ordinary stores /
// vector atomics
//
// RECORD (the steps of a row-parallel plan under dsgd_plan_record; dsgd_rp64_grad_rec_kernel, dsgd_rp64v_grad_rec_kernel): the
// gate's decision of every listed row goes into the step's mask words -- bit (seg.begin - step_base + t) for entry t of the
// worker's list, i.e. the rows of the step in worker order, each list in order -- with a 32-bit vector atomic OR by lane 0
// of the row's group (the host zeroes the words on the stream in front of the step), and the last workgroup stores
// (float)s into the step's slot.  Nothing of the dots, the gate or the integer sums changes: the weights are the bits of
// the unrecorded kernels.  RECORD = false never reads `rec`.
struct Rp64Rec {
  unsigned int* mask;      // the step's ceil(max_step_rows / 32) words, zero on entry
  float* s_used;           // the step's slot of the s record
  long long step_base;     // position in idx of the step's first entry (worker 0's seg.begin)
};
// RANK_WORD (GATHER only; its default keeps the per-step kernels as they were): false for the steps of a plan run under a
// communicator, whose ranks agreed once per call -- no rank word travels and `a.rank_word` is null.
template <typename V, bool GATHER, bool RECORD = false, bool RANK_WORD = GATHER>
__device__ __forceinline__ void rp64_grad_body(const CsrViewT<V>& m, const Rp64Args& a, const Rp64Rec& rec = Rp64Rec{}) {
#pragma clang fp contract(off)
  constexpr int WORDS = Rp64Acc<V>::WORDS;
  static_assert(WORDS <= RP64_MAX_WORDS, "a gather slot holds one plane per word of a column sum");
  __shared__ double red[RP64_THREADS / 64];
  __shared__ unsigned int n_act;
  __shared__ unsigned long long hot[WORDS][RP64_HOT];
  const int tid = threadIdx.x;
  const long long last = a.with_s ? (long long)gridDim.x - 1 : -1;
  if ((long long)blockIdx.x == last) {
    // ---- s of the weights the rows see: filt(w * ds) per column (orc_dense_dot), lane-strided, then the wave
    //      butterflies and the four wave sums in order: the same bits on every call ----
    double v = 0.0;
    for (int r = tid; r < a.dp; r += RP64_THREADS) v = v + filt64(a.w[rp64_at(r, a.Sp)] * a.ds[r]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (RECORD) {
      if (tid == 0) {
        const double s = a.lambda * 2.0 * ((red[0] + red[1]) + (red[2] + red[3]));
        *a.s_out = s;
        *rec.s_used = (float)s;
      }
      return;
    }
    if (tid == 0) *a.s_out = a.lambda * 2.0 * ((red[0] + red[1]) + (red[2] + red[3]));   // ref: core/ml/SparseSVM.scala:31
    if (GATHER && RANK_WORD && tid == 0) *a.rank_word = rp64_rank_word(a.K, WORDS == 2);
    return;
  }
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, rp64_shift(n) - a.vexp);   // (a power of two: x * qscale is exact)
  unsigned long long* acc[WORDS];
#pragma unroll
  for (int i = 0; i < WORDS; ++i) acc[i] = a.acc[i] + (long long)k * a.acc_stride;
  const int sub = tid % RP64_GROUP;
  const long long groups = a.blocks_per_worker * (RP64_THREADS / RP64_GROUP);
  if (tid == 0) n_act = 0u;
  for (int j = tid; j < RP64_HOT; j += RP64_THREADS) {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) hot[i][j] = 0ull;
  }
  __syncthreads();
  unsigned int mine = 0u;
  for (long long t = b * (RP64_THREADS / RP64_GROUP) + tid / RP64_GROUP; t < n; t += groups) {
    const long long row = a.idx[seg.begin + t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const double d = row_dot64<RP64_GROUP>(m, row, a.w, a.Sp, sub);
    const double y = (double)m.label[row];
    if (y * d < 0.0) continue;                                   // ref: core/ml/SparseSVM.scala:27-28 (zerosLike)
    mine += sub == 0 ? 1u : 0u;
    if (RECORD && sub == 0) {
      const long long bit = seg.begin - rec.step_base + t;
      atomicOr(&rec.mask[bit >> 5], 1u << (unsigned int)(bit & 31));
    }
    const double cq = y > 0.0 ? qscale : -qscale;
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    for (long long p = st + sub; p < en; p += RP64_GROUP) {
      const double x = (double)m.val[p];
      if (!(fabs(x) > CS64_EPS)) continue;   // filt(x * y): the Sparse constructor's filter (math/Sparse.scala:104)
      unsigned long long q[WORDS];
      Rp64Acc<V>::quantise(x * cq, q);
      const int c = m.col[p];
#pragma unroll
      for (int i = 0; i < WORDS; ++i) {   // (a zero word adds nothing: its atomic is skipped)
        if (q[i] == 0ull) continue;
        if (c < RP64_HOT)
          atomicAdd(&hot[i][c], q[i]);
        else
          atomicAdd(&acc[i][c], q[i]);
      }
    }
  }
  if (mine) atomicAdd(&n_act, mine);
  __syncthreads();
  for (int j = tid; j < RP64_HOT; j += RP64_THREADS) {   // (a word is non-zero only below dp)
#pragma unroll
    for (int i = 0; i < WORDS; ++i) {
      const unsigned long long v = hot[i][j];
      if (v) atomicAdd(&acc[i][j], v);
    }
  }
  if (GATHER) {
    if (tid == 0 && b == 0) acc[0][a.dp + RP64_HDR_N] = (unsigned long long)n;   // (zero until here, like every word of the slot)
    if (tid == 0 && n_act) atomicAdd(&acc[0][a.dp + RP64_HDR_ACTIVE], (unsigned long long)n_act);
  } else {
    if (tid == 0 && n_act) atomicAdd(&a.sc->n_active, (unsigned long long)n_act);
  }
}
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_grad_kernel(CsrView m, Rp64Args a) { rp64_grad_body<float, false>(m, a); }
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_grad_gather_kernel(CsrView m, Rp64Args a) { rp64_grad_body<float, true>(m, a); }
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_grad_kernel(CsrView64 m, Rp64Args a) { rp64_grad_body<double, false>(m, a); }
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_grad_gather_kernel(CsrView64 m, Rp64Args a) { rp64_grad_body<double, true>(m, a); }
// (the steps of a row-parallel plan under a communicator: the gather form without the rank word)
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_grad_gather_plan_kernel(CsrView m, Rp64Args a) { rp64_grad_body<float, true, false, false>(m, a); }
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_grad_gather_plan_kernel(CsrView64 m, Rp64Args a) { rp64_grad_body<double, true, false, false>(m, a); }
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_grad_rec_kernel(CsrView m, Rp64Args a, Rp64Rec rec) { rp64_grad_body<float, false, true>(m, a, rec); }
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_grad_rec_kernel(CsrView64 m, Rp64Args a, Rp64Rec rec) { rp64_grad_body<double, false, true>(m, a, rec); }

struct Rp64FinishArgs {
  unsigned long long* acc[RP64_MAX_WORDS];   // per word [K][acc_stride], zeroed here
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the list lengths give each worker's shift
  int K, dp, vexp, Sp;
  const double* s;           // from the grad kernel (ASYNC: from dsgd_rp64v_s_sliced_kernel)
  const int* perm;           // key -> rank
  double* g_out;             // GRADIENT: the regularised sum of worker 0, key order.  ASYNC: the delta, key order (may be null)
  double* w;                 // STEP, ASYNC: the weights, updated in their layout
  double lr;
};

constexpr int RP64_GRADIENT = 0, RP64_STEP = 1, RP64_ASYNC = 2;

// GRADIENT: over keys j, g[j] of the one worker (orc_gradient).  STEP: over ranks r, the fold over the workers in worker
// order, filt(acc / K), filt(mean * lr), filt(w - upd) (orc_sync_step; w is filtered already: a column without a
// gradient keeps its value, which is what filt(w - 0) gives).  ASYNC: over keys j, the one worker's filt(g0 / n), the
// support-only regulariser, filt(g * lr) written to the delta, filt(w - upd) on EVERY coordinate (orc_async_step: the
// oracle writes filt(w - 0) where nothing is listed).  (threads: blockDim.x, see forward64_body)
template <typename V, int MODE>
__device__ __forceinline__ void rp64_finish_body(const Rp64FinishArgs& a, unsigned int threads) {
#pragma clang fp contract(off)
  constexpr int WORDS = Rp64Acc<V>::WORDS;
  const double s = *a.s;
  const bool add = fabs(s) > CS64_EPS;   // (regularize_inplace: s == 0 or filtered away -> g unchanged)
  for (int j = blockIdx.x * threads + threadIdx.x; j < a.dp; j += gridDim.x * threads) {
    const int r = MODE == RP64_STEP ? j : a.perm[j];
    double gsum = 0.0;
    for (int k = 0; k < (MODE == RP64_STEP ? a.K : 1); ++k) {
      unsigned long long* at[WORDS];
      unsigned long long t[WORDS];
#pragma unroll
      for (int i = 0; i < WORDS; ++i) {   // (every word's load in flight before the first store)
        at[i] = a.acc[i] + (long long)k * a.acc_stride + r;
        t[i] = *at[i];
      }
#pragma unroll
      for (int i = 0; i < WORDS; ++i)
        if (t[i] != 0ull) *at[i] = 0ull;
      const long long n = a.segs[k].end - a.segs[k].begin;
      const double g0 = filt64(Rp64Acc<V>::round(t, a.vexp - rp64_shift(n)));   // one rounding of the exact sum
      if (MODE == RP64_ASYNC) {
        const double gm = filt64(g0 / (double)n);                      // Vec.mean (correctly rounded division)
        const double g = (add && gm != 0.0) ? filt64(gm + s) : gm;     // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
        const double upd = filt64(g * a.lr);                           // learningRate * regularize(grad) (ref: core/Slave.scala:99)
        if (a.g_out != nullptr) a.g_out[j] = upd;
        const long long at = rp64_at(r, a.Sp);
        a.w[at] = filt64(a.w[at] - upd);                               // ref: core/Slave.scala:101
      } else {
        const double g = (add && g0 != 0.0) ? filt64(g0 + s) : g0;     // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
        if (MODE == RP64_GRADIENT) {
          a.g_out[j] = g;
        } else {
          gsum = filt64(gsum + g);                                     // Vec.sum over the workers
        }
      }
    }
    if (MODE == RP64_STEP && gsum != 0.0) {
      const double mean = filt64(gsum / (double)a.K);             // Vec.mean (correctly rounded division)
      const double upd = filt64(mean * a.lr);                     // learningRate * grad (ref: core/Master.scala:194-197)
      const long long at = rp64_at(r, a.Sp);
      a.w[at] = filt64(a.w[at] - upd);
    }
  }
}
template <bool STEP>
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_finish_kernel(Rp64FinishArgs a) {
  rp64_finish_body<float, STEP ? RP64_STEP : RP64_GRADIENT>(a, blockDim.x);
}
template <int MODE>
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_finish_kernel(Rp64FinishArgs a) {
  rp64_finish_body<double, MODE>(a, blockDim.x);
}
// one worker's asynchronous iteration on FLOAT values: an asynchronous row-parallel plan (dsgd_async_plan_create_rp64) beyond
// what dsgd_cs64_async_kernel holds; s from dsgd_rp64v_s_sliced_kernel, as on Double values
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_finish_async_kernel(Rp64FinishArgs a) {
  rp64_finish_body<float, RP64_ASYNC>(a, blockDim.x);
}

// Behind the gather, ONE workgroup: the K headers become the list ranges the finish takes its shifts from ({0, n}), the
// job's samples and active rows go to the context's scalars, and the header and rank words are zeroed again (the
// finish zeroes the sums: the whole buffer is zero for the next call).  `stride` is the SLOT's: with two planes per slot
// (Double values) twice the plane's -- the headers are plane 0's, plane 1 has no word outside its sums.
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
// The header kernel of a plan run's step (dsgd_plan_run_f64 on a row-parallel plan under a communicator): the same ranges and
// the same zeroing of the header words, no rank words (none travel: the ranks agreed once per call), and the job's samples
// and active rows ADDED to the context's scalars -- they run on over the call's steps, and over the calls until
// dsgd_synchronize, as a local plan run's n_active does.  ONE workgroup; the stream orders the steps.
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_header_plan_kernel(unsigned long long* slots, long long stride, int K, int dp,
                                                                             WorkSeg* segs, DevScalars* sc) {
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
  __syncthreads();
  if (tid == 0) {
    sc->n_samples += tot[0];
    sc->n_active += tot[1];
  }
}

// The ASYNC finish's s = lambda * 2 * (w . ds) in the summation order of dsgd_cs64_async_kernel, ONE workgroup of CS_THREADS
// lanes: the asynchronous iteration on float data runs there, and a Double-data step on values a float holds must give its bits.
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

// ---- an epoch's steps in one call (dsgd_sync_steps_f64): ONE launch per step ----
// The fused step: phase 1 is rp64_grad_body<V, false>, phase 2 rp64_finish_body<V, RP64_STEP> over the launch's own grid,
// and between them every workgroup of the grid waits for every other one.  The host launches the fused form only for a
// grid that is resident as a whole (rp64_fused_cap: the occupancy of the kernel times the compute units); every other
// step is the two launches above, enqueued back to back.
//   arrival   every wave makes its atomics (and the last workgroup's store of s) visible with a release fence at agent
//             scope, the workgroup meets, and ONE lane adds 1 to a 64-bit counter in device memory.  The counter only
//             grows over the context's life: the host passes each launch its own target (the previous one + the grid)
//             and zeroes the counter only after an aborted call.
//   wait      that lane polls the counter (relaxed, agent scope) until it reaches the target, the workgroup meets again,
//             and every wave makes an acquire fence at agent scope in front of its own loads: the accumulators were
//             written by atomics in L2, but s and phase 2's loads go through the vector L1.
//   giving up the wait is bounded by the device's wall clock (wait_ticks: 2 s; phase 1 of a whole-split step is more
//             than a millisecond, so a count of polls would not do).  The abort word is bit 62 of the counter itself
//             (RP64_GAVE_UP), so that giving up and arriving are decided in ONE place: a workgroup out of time sets the
//             bit with a compare-and-swap against the value it last read, which is below the target -- it succeeds only
//             while the launch's arrivals are still incomplete, and from then on no poll of this launch can succeed
//             (the bit is never cleared by the device); if the counter moved, the workgroup looks again.  So either
//             every workgroup of a launch runs phase 2 or none does.  Every later launch of the call finds the bit on
//             entry and returns at once (the shape of cs64_gather's abort word).  The host finds it behind its one
//             synchronisation.
//   counting  behind the arrival one lane of workgroup 0 stores the context's running n_active into the step's word of
//             `cum` (all ones until then): the host takes the differences, and after an abort the written words name the
//             last completed step.
// (RP64_FUSED_DEFAULT: csrc/dsgd_limits.hpp)
constexpr unsigned long long RP64_GAVE_UP = 1ull << 62;
struct Rp64StepSync {
  unsigned long long* arrived;     // the arrival counter (monotonic; bit 62: a launch gave up)
  unsigned long long target;       // the counter's value once every workgroup of THIS launch has arrived
  unsigned long long wait_ticks;   // of wall_clock64
  unsigned long long* cum;         // this step's word: n_active of the call so far
};

template <typename V>
__device__ __forceinline__ void rp64_step_body(const CsrViewT<V>& m, const Rp64Args& a, const Rp64FinishArgs& f, const Rp64StepSync& y) {
#pragma clang fp contract(off)
  __shared__ int go;
  const int tid = threadIdx.x;
  if (tid == 0) go = (__hip_atomic_load(y.arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & RP64_GAVE_UP) == 0ull ? 1 : 0;
  __syncthreads();
  if (!go) return;   // (an earlier launch of the call gave up)
  rp64_grad_body<V, false>(m, a);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // every wave: its own atomics are behind it
  __syncthreads();
  if (tid == 0) {
    __hip_atomic_fetch_add(y.arrived, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int ok = 1;
    const long long t0 = wall_clock64();
    unsigned long long v = __hip_atomic_load(y.arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (unsigned int spin = 0;; ++spin) {
      if (v & RP64_GAVE_UP) {
        ok = 0;
        break;
      }
      if (v >= y.target) break;
      if ((spin & 63u) == 63u && (unsigned long long)(wall_clock64() - t0) > y.wait_ticks) {
        // (v < target here: the bit goes in only if nobody has arrived since; on failure v is the counter's new value)
        if (__hip_atomic_compare_exchange_strong(y.arrived, &v, v | RP64_GAVE_UP, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          ok = 0;
          break;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
      v = __hip_atomic_load(y.arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    go = ok;
  }
  __syncthreads();
  if (!go) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every wave, in front of its own loads of the others' sums and of s
  if (blockIdx.x == 0 && tid == 0) *y.cum = __hip_atomic_load(&a.sc->n_active, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  rp64_finish_body<V, RP64_STEP>(f, RP64_THREADS);
}
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64_step_kernel(CsrView m, Rp64Args a, Rp64FinishArgs f, Rp64StepSync y) {
  rp64_step_body<float>(m, a, f, y);
}
__global__ void __launch_bounds__(RP64_THREADS) dsgd_rp64v_step_kernel(CsrView64 m, Rp64Args a, Rp64FinishArgs f, Rp64StepSync y) {
  rp64_step_body<double>(m, a, f, y);
}
