// Device code of libdsgd_hip, part 8 (gfx950 only): the fp64 mode (DSGD_F_FP64) -- the reference's own batch sizes
// (3 x 100, application.conf:15,27; 4 x 200, kube/config-sync.yaml) with the reference's number type, Double.
// Included by dsgd_hip.hip LAST, after every fp32 kernel.
//
// ref: core/Master.scala:179-199 (the batch closure), core/Slave.scala:142-157 (a worker's regularised sum).
//
// The same column slices as dsgd_cs.hpp -- the plan layout (CsHdr, slot_meta, row_first, col / val pieces, clist) is the one
// dsgd_cs_layout_kernel builds, unchanged -- with the state of the reference: fp64 weights and dimSparsity, fp64 dot
// products, one 64-bit fixed-point accumulator per hosted worker (ds_add_u64: a worker's sum of +-x is exact), the
// fp64 regulariser / mean / update of oracle/oracle.c (orc_sync_step, orc_gradient) operation for operation, with the
// 1e-20 filter at the same points.  Always G = 16 slices: (2 + K) x Sp doubles per slice (K = 4 at RCV1's D: 142 KB of
// the 160 KiB) plus the per-slot partial dots (8 KB), the rows' gate signs (4 KB) and 32 words of reductions.
//
// The exchange: each fp64 value (a slice's partial x.w of a row, its share of w . ds) is published as TWO 8-byte granules
// {32-bit half, step tag} -- the low half at [p], the high half at [CS_XSTRIDE + p] of the slice's area -- and is taken
// only when both tags are the step's (an 8-byte store is one granule; a 16-byte one is only observed untorn).  The
// partials are added in slice order, so every workgroup takes the same gate decision.  Bounded poll, abort word: a launch
// ends with DevScalars::err = 8, never hangs (as dsgd_cs.hpp).
//
// HIP contracts a * b + c into an FMA by default; the oracle is built with -ffp-contract=off.  Every function here opens
// with `#pragma clang fp contract(off)` (scoped to its body: the fp32 kernels of the library are compiled as before).
#pragma once

constexpr int CS64_G = CS_MAX_G;   // slices
constexpr int CS64_MAX_K = 4;      // hosted workers
constexpr int CS64_XSTRIDE2 = 2 * CS_XSTRIDE;   // granules per (parity, slice): [CS_XSTRIDE] low halves, then the high halves
constexpr double CS64_EPS = 1e-20;  // ref: math/Sparse.scala:104

__device__ __forceinline__ double filt64(double v) { return fabs(v) > CS64_EPS ? v : 0.0; }

// LDS of a launch, bytes: w, ds and K accumulators per padded column; per-slot partial dots; per-row gate signs; reductions
__host__ __device__ constexpr int cs64_sp(int dp) { return (((dp + CS64_G - 1) / CS64_G) + 4) & ~3; }
__host__ __device__ constexpr long long cs64_lds_bytes(int dp, int K) {
  return 8LL * (2 + K) * cs64_sp(dp) + 8LL * CS_MAX_SLOTS + 4LL * CS_MAX_SLOTS + 8LL * 32;
}
constexpr long long CS64_LDS_MAX = 160 * 1024;

struct Cs64Args {
  const CsHdr* hdr;                 // the plan's layout, as dsgd_cs_layout_kernel built it (see CsArgs)
  const unsigned int* slot_meta;
  const unsigned short* row_first;
  const uint4* col;
  const float4* val;
  const unsigned short* clist;
  double* w;                        // the weights slice-major: [G][Sp] (dsgd_cs64_slice_kernel / dsgd_cs64_unslice_kernel)
  const double* ds;                 // dimSparsity, the same layout
  unsigned long long* xbuf;         // [2][G][2 * CS_XSTRIDE] granules {half, step tag << 32}
  unsigned int* sync;               // [2]: [1] the abort word
  DevScalars* sc;
  long long n_steps_plan, step_begin, step_end;
  int slot_stride, row_stride, cl_stride;
  unsigned int tag0;
  double lr, lambda;
  int vexp, dp, K;
  unsigned int* gate_rec;           // optional record: gate bits per step (as dsgd_cs_step_kernel), s of every step (rounded)
  float* s_rec;
  int gate_words;
};

// LDS carve of a workgroup
struct Cs64State {
  double* w_l;
  double* ds_l;
  unsigned long long* acc;   // [K][Sp], zero between steps
  double* ps;                // partial x.w per slot
  float* coef;               // per row of the step: +1 / -1 (active, the label's sign) or 0
  double* red;               // [0..15] wave sums, [16] s of the step, [17] abort flag (as an int)
  int b, Sp;
  double sp;                 // this slice's share of w . ds of the current weights
  unsigned int n_act, n_rel;
};

// the G lo/hi granule pairs of each of N exchange slots; values added in slice order.  false = given up.
template <int N>
__device__ __forceinline__ bool cs64_gather(const unsigned long long* xall, const int (&at)[N], unsigned int tag, unsigned int* abort_word,
                                            double (&sum)[N]) {
#pragma clang fp contract(off)
  unsigned int lo[N][CS64_G], hi[N][CS64_G];
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(xall), 0, CS64_G * CS64_XSTRIDE2 * 8, 0x00020000);
  bool any = false;
#pragma unroll
  for (int n = 0; n < N; ++n) any = any || at[n] >= 0;
  if (!any) return true;
  for (unsigned int spin = 0;; ++spin) {
    asm volatile("" ::: "memory");
    bool all = true;
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const unsigned int p = at[n] < 0 ? 0u : (unsigned int)at[n];
#pragma unroll
      for (int g = 0; g < CS64_G; ++g) {
        const unsigned long long x = cs_granule(rs, p, 2 * g);
        const unsigned long long y = cs_granule(rs, p + CS_XSTRIDE, 2 * g);
        lo[n][g] = (unsigned int)x;
        hi[n][g] = (unsigned int)y;
        all = all && (((unsigned int)(x >> 32) == tag && (unsigned int)(y >> 32) == tag) || at[n] < 0);
      }
    }
    if (all) break;
    if ((spin & 63u) == 63u) {
      if (spin > CS_POLL_LIMIT || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double d = 0.0;
#pragma unroll
    for (int g = 0; g < CS64_G; ++g) d = d + __hiloint2double((int)hi[n][g], (int)lo[n][g]);
    sum[n] = d;
  }
  return true;
}

// publish value v at exchange slot p of this slice: the low half, then the high half, each with the tag
__device__ __forceinline__ void cs64_publish(unsigned long long* xb, int p, double v, unsigned int tag) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  __hip_atomic_store(&xb[p], ((unsigned long long)tag << 32) | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&xb[CS_XSTRIDE + p], ((unsigned long long)tag << 32) | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum over the workgroup, the same bits on every thread (wave butterflies, then the wave sums pairwise in order)
template <int NT>
__device__ __forceinline__ double cs64_block_sum(double v, double* red16) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  cs_barrier();
  if ((threadIdx.x & 63) == 0) red16[threadIdx.x >> 6] = v;
  cs_barrier();
  double t[NT / 64];
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t[i] = red16[i];
#pragma unroll
  for (int n = NT / 64; n > 1; n >>= 1)
#pragma unroll
    for (int i = 0; i < n / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
  return t[0];
}

// this lane's part of the slice's share of w . ds: filt(w * ds) per column (orc_dense_dot), two per lane and round
template <int NT>
__device__ __forceinline__ double cs64_wds_share(const Cs64State& z) {
#pragma clang fp contract(off)
  const double2* w2 = reinterpret_cast<const double2*>(z.w_l);
  const double2* d2 = reinterpret_cast<const double2*>(z.ds_l);
  double sp = 0.0;
  for (int i2 = threadIdx.x; i2 < (z.Sp >> 1); i2 += NT) {
    const double2 wv = w2[i2], dv = d2[i2];
    sp = sp + (filt64(wv.x * dv.x) + filt64(wv.y * dv.y));
  }
  return sp;
}

// The listed columns of a step, KK hosted workers (orc_sync_step / orc_gradient per column): per worker ONE rounding of
// the exact sum, filt; the support-only regulariser filt(g + s); acc = filt(acc + g_k) over the workers in order from 0;
// filt(acc / K), filt(mean * lr), filt(w - upd).  A lane without a column works on the padding column (zero everywhere).
template <int NT, int KK, int CLT>
__device__ __forceinline__ void cs64_sweep(Cs64State& z, const unsigned short (&cl)[CLT], int n_cols, int Sp, double inv_scale, double s,
                                           bool add, double lr) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < CLT; ++i) {
    if (i * NT >= n_cols) break;   // (workgroup-uniform: the list is dense from entry 0)
    const int c = cl[i] == 0xffffu ? Sp - 1 : (int)cl[i];
    long long t[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) t[k] = (long long)z.acc[k * Sp + c];
    const double wo = z.w_l[c];
    double gsum = 0.0;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      z.acc[k * Sp + c] = 0ull;
      const double g0 = filt64((double)t[k] * inv_scale);     // one rounding of the exact sum (the power of two is exact)
      const double g1 = filt64(g0 + s);                       // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
      gsum = filt64(gsum + ((add && g0 != 0.0) ? g1 : g0));   // Vec.sum over the workers
    }
    const double mean = filt64(gsum / (double)KK);            // Vec.mean (correctly rounded division)
    const double upd = filt64(mean * lr);                     // learningRate * grad (ref: core/Master.scala:194-197)
    z.w_l[c] = gsum != 0.0 ? filt64(wo - upd) : wo;
  }
}

// The listed columns of an asynchronous iteration, one worker (orc_async_step per column, core/Slave.scala:92-101): ONE
// rounding of the exact sum, filt; the mean over the n rows of the step, inactive ones included (Vec.mean); the
// support-only regulariser filt(g + s); filt(g * lr), written to `delta` (the slice's [Sp], may be null); filt(w - upd).
template <int NT, int CLT>
__device__ __forceinline__ void cs64_async_sweep(Cs64State& z, const unsigned short (&cl)[CLT], int n_cols, int Sp, double inv_scale,
                                                 double s, bool add, double lr, double n, double* delta) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < CLT; ++i) {
    if (i * NT >= n_cols) break;   // (workgroup-uniform: the list is dense from entry 0)
    const int c = cl[i] == 0xffffu ? Sp - 1 : (int)cl[i];
    const long long t = (long long)z.acc[c];
    z.acc[c] = 0ull;
    const double g0 = filt64((double)t * inv_scale);            // one rounding of the exact sum (the power of two is exact)
    const double gm = filt64(g0 / n);                           // Vec.mean (correctly rounded division)
    const double g = (add && gm != 0.0) ? filt64(gm + s) : gm;  // ref: core/ml/SparseSVM.scala:31, math/Vec.scala:65-75
    const double upd = filt64(g * lr);                          // learningRate * regularize(grad) (ref: core/Slave.scala:99)
    if (delta != nullptr) delta[c] = upd;
    z.w_l[c] = filt64(z.w_l[c] - upd);                          // ref: core/Slave.scala:101
  }
}

// the slots of `step` into R (cs_issue over the plan's layout)
template <int NT, int SPL, int CLT>
__device__ __forceinline__ void cs64_issue(const Cs64Args& a, int b, long long step, CsSet<SPL, CLT>& R) {
  CsArgs ia;
  ia.hdr = a.hdr;
  ia.slot_meta = a.slot_meta;
  ia.row_first = a.row_first;
  ia.col = a.col;
  ia.val = a.val;
  ia.clist = a.clist;
  ia.n_steps_plan = a.n_steps_plan;
  ia.step_end = a.step_end;
  ia.slot_stride = a.slot_stride;
  ia.row_stride = a.row_stride;
  ia.cl_stride = a.cl_stride;
  cs_issue<NT, SPL, CLT>(ia, b, step, R);
}

// One step.  `cur`: the step's slots (landed); `nxt` receives the next step's.  false = the launch was aborted.
// ASYNC: one asynchronous iteration of the one worker (cs64_async_sweep), `delta` the slice's share of its update or null.
template <int NT, int SPL, int CLT, bool ASYNC = false>
__device__ __forceinline__ bool cs64_step(const Cs64Args& a, Cs64State& z, CsSet<SPL, CLT>& cur, CsSet<SPL, CLT>& nxt, long long step,
                                          double* delta = nullptr) {
#pragma clang fp contract(off)
  int tid = threadIdx.x, K = __builtin_amdgcn_readfirstlane(a.K), b = z.b, Sp = __builtin_amdgcn_readfirstlane(z.Sp);
  asm volatile("" : "+v"(tid));
  asm volatile("" : "+s"(K), "+s"(Sp));
  double* const ps = z.ps;
  float* const coef = z.coef;
  double* const red = z.red;
  const int n_slots = __builtin_amdgcn_readfirstlane((int)(cur.h.x & 0xffffu));
  const int n_rows = __builtin_amdgcn_readfirstlane((int)(cur.h.x >> 16));
  // the fp32 layout's shift is 30 - ceil(log2(largest list)); the 64-bit accumulators take 32 more bits
  const int shift = __builtin_amdgcn_readfirstlane((int)(cur.h.y & 0xffffu)) + 32;
  const int n_cols = __builtin_amdgcn_readfirstlane((int)(cur.h.y >> 16));
  const double qscale = ldexp(1.0, shift - a.vexp);
  const double inv_scale = ldexp(1.0, a.vexp - shift);
  // ---- 1: partial x.w of every slot from this slice's weights: filt((double)x * w) (oracle.c: orc_row_dot) ----
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    double p = 0.0;
#pragma unroll
    for (int j = 0; j < CS_L; ++j) p = p + filt64((double)CS_VAL(cur, i, j) * z.w_l[CS_COL(cur, i, j)]);
    const int slot = tid + NT * i;
    if (slot < n_slots) ps[slot] = p;
  }
  if (tid == 0) reinterpret_cast<int*>(red)[2 * 17] = 0;
  cs_barrier();
  // ---- 2: this slice's partial of every row (its slots in order) and its share of w . ds, published ----
  const unsigned int tag = a.tag0 + z.n_rel + 1u;
  unsigned long long* xb = a.xbuf + ((long long)(z.n_rel & 1u) * CS64_G + b) * CS64_XSTRIDE2;
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int r = tid + NT * i;
    if (r < n_rows) {
      const int f0 = (int)(cur.rf[i] & 0x7ffu), f1 = (int)((cur.rf[i] >> 16) & 0x7ffu);
      double t = 0.0;
      for (int f = f0; f < f1; ++f) t = t + ps[f];
      cs64_publish(xb, r, t, tag);
    }
  }
  if (tid == 0) cs64_publish(xb, CS_MAX_SLOTS, z.sp, tag);
  // ---- the NEXT step's slots are requested here: they land while this workgroup waits for its peers.  (Two slots per
  //      lane: behind the scatter instead, when this step's slots are dead -- both sets under the exchange and the
  //      scatter's fp64 products were 54 spilled registers) ----
  if (SPL == 1) cs64_issue<NT, SPL, CLT>(a, b, step + 1, nxt);
  // ---- 3: every slice's partials of this thread's rows, in slice order: the gate, the row's sign ----
  const unsigned long long* xall = a.xbuf + (long long)(z.n_rel & 1u) * CS64_G * CS64_XSTRIDE2;
  int at[SPL];
  double dd[SPL];
  bool act[SPL];
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int r = tid + NT * i;
    at[i] = r < n_rows ? r : (r == n_rows ? CS_MAX_SLOTS : -1);
    act[i] = false;
  }
  // (one register set of a row's 2 x G halves at a time: both sets of slots stay in registers meanwhile)
  bool got = true;
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int at1[1] = {at[i]};
    double d1[1];
    got = cs64_gather<1>(xall, at1, tag, &a.sync[1], d1) && got;
    dd[i] = d1[0];
  }
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int r = tid + NT * i;
    if (r < n_rows) {
      const bool ypos = (cur.rf[i] & 0x8000u) != 0u;
      const double yd = ypos ? dd[i] : -dd[i];
      const bool active = got && !(yd < 0.0);                   // ref: core/ml/SparseSVM.scala:27-28
      coef[r] = active ? (ypos ? 1.0f : -1.0f) : 0.0f;
      z.n_act += (active && b == 0) ? 1u : 0u;
      act[i] = active;
    } else if (r == n_rows) {
      red[16] = a.lambda * 2.0 * dd[i];                          // s = lambda * 2.0 * (w . ds), as orc regularize_inplace
    }
  }
  if (a.gate_rec != nullptr && b == 0) {   // (workgroup-uniform) the decisions on record, as dsgd_cs_step_kernel writes them
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const unsigned long long m = __ballot(act[i]);
      const int r0 = (tid & ~63) + NT * i;
      if ((tid & 63) == 0 && r0 < n_rows) {
        unsigned int* g = a.gate_rec + step * (long long)a.gate_words + (r0 >> 5);
        g[0] = (unsigned int)m;
        if (r0 + 32 < n_rows) g[1] = (unsigned int)(m >> 32);
      }
    }
  }
  if (n_rows == NT * SPL && tid == NT - 1) {
    const int at1[1] = {CS_MAX_SLOTS};
    double d1[1];
    got = cs64_gather<1>(xall, at1, tag, &a.sync[1], d1) && got;
    red[16] = a.lambda * 2.0 * d1[0];
  }
  if (!got) reinterpret_cast<int*>(red)[2 * 17] = 1;
  cs_barrier();
  if (reinterpret_cast<int*>(red)[2 * 17]) return false;
  const double s = red[16];
  const bool add = (s != 0.0) && (fabs(s) > CS64_EPS);
  if (a.s_rec != nullptr && b == 0 && tid == 0) a.s_rec[step] = (float)s;
  // ---- 4: y * x of the active rows into the accumulator of the row's worker (exact 64-bit integer sums) ----
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int slot = tid + NT * i;
    if (slot < n_slots) {
      const float cf = coef[cur.meta[i] & 0xffffu];
      if (cf != 0.0f) {
        unsigned long long* ak = z.acc + (int)((cur.meta[i] >> 16) & 15u) * Sp;
        const double cq = cf > 0.0f ? qscale : -qscale;
#pragma unroll
        for (int j = 0; j < CS_L; ++j) {
          // (unconditional: a branch per entry held an exec mask per entry -- SGPR spills; padding adds 0 to column 0)
          const long long q = __double2ll_rn((double)CS_VAL(cur, i, j) * cq);
          atomicAdd(&ak[CS_COL(cur, i, j)], (unsigned long long)q);
        }
      }
    }
  }
  if (SPL != 1) cs64_issue<NT, SPL, CLT>(a, b, step + 1, nxt);
  cs_barrier();
  // ---- 5: the listed columns: the worker sums, regulariser, fold, mean, update ----
  if constexpr (ASYNC) {
    cs64_async_sweep<NT, CLT>(z, cur.cl, n_cols, Sp, inv_scale, s, add, a.lr, (double)n_rows,
                              delta != nullptr ? delta + (long long)b * Sp : nullptr);
  } else {
    switch (K) {
      case 1: cs64_sweep<NT, 1, CLT>(z, cur.cl, n_cols, Sp, inv_scale, s, add, a.lr); break;
      case 2: cs64_sweep<NT, 2, CLT>(z, cur.cl, n_cols, Sp, inv_scale, s, add, a.lr); break;
      case 3: cs64_sweep<NT, 3, CLT>(z, cur.cl, n_cols, Sp, inv_scale, s, add, a.lr); break;
      default: cs64_sweep<NT, 4, CLT>(z, cur.cl, n_cols, Sp, inv_scale, s, add, a.lr); break;
    }
  }
  cs_barrier();
  z.sp = cs64_block_sum<NT>(cs64_wds_share<NT>(z), red);
  ++z.n_rel;
  return true;
}

template <int NT, int SPL, int CLT>
__global__ void __launch_bounds__(NT) dsgd_cs64_step_kernel(Cs64Args a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int tid = threadIdx.x;
  const int K = a.K;
  Cs64State z;
  z.b = blockIdx.x;
  z.Sp = cs64_sp(a.dp);
  z.w_l = lds64;
  z.ds_l = lds64 + z.Sp;
  z.acc = reinterpret_cast<unsigned long long*>(lds64 + 2 * z.Sp);
  z.ps = lds64 + (2 + K) * z.Sp;
  z.red = z.ps + CS_MAX_SLOTS;
  z.coef = reinterpret_cast<float*>(z.red + 32);
  z.n_act = 0u;
  z.n_rel = 0u;
  CsSet<SPL, CLT> A, B;
  cs64_issue<NT, SPL, CLT>(a, z.b, a.step_begin, A);
  {   // the slice's weights and dimSparsity (the padding holds zeros); the accumulators cleared
    const double2* ws2 = reinterpret_cast<const double2*>(a.w + (long long)z.b * z.Sp);
    const double2* ds2 = reinterpret_cast<const double2*>(a.ds + (long long)z.b * z.Sp);
    double2* wl2 = reinterpret_cast<double2*>(z.w_l);
    double2* dl2 = reinterpret_cast<double2*>(z.ds_l);
    for (int i = tid; i < (z.Sp >> 1); i += NT) {
      wl2[i] = ws2[i];
      dl2[i] = ds2[i];
    }
    for (int i = tid; i < K * z.Sp; i += NT) z.acc[i] = 0ull;
  }
  cs_barrier();
  z.sp = cs64_block_sum<NT>(cs64_wds_share<NT>(z), z.red);
  bool ok = true;
  for (long long step = a.step_begin; step < a.step_end; step += 2) {
    ok = cs64_step<NT, SPL, CLT>(a, z, A, B, step);
    if (!ok || step + 1 >= a.step_end) break;
    ok = cs64_step<NT, SPL, CLT>(a, z, B, A, step + 1);
    if (!ok) break;
  }
  if (ok) {   // (given up: no slice writes back -- see cs_launch_body)
    double2* ws2 = reinterpret_cast<double2*>(a.w + (long long)z.b * z.Sp);
    const double2* wl2 = reinterpret_cast<const double2*>(z.w_l);
    for (int i = tid; i < (z.Sp >> 1); i += NT) ws2[i] = wl2[i];
  } else if (tid == 0) {
    atomicOr(&a.sc->err, 8);
  }
  if (z.b != 0) return;
  const unsigned int n_act = wave_sum_u32(ok ? z.n_act : 0u);
  __syncthreads();
  unsigned int* r4 = reinterpret_cast<unsigned int*>(z.red);
  if ((tid & 63) == 0) r4[tid >> 6] = n_act;
  __syncthreads();
  if (tid == 0) {
    unsigned int tot = 0u;
    for (int i = 0; i < NT / 64; ++i) tot += r4[i];
    if (tot) atomicAdd(&a.sc->n_active, (unsigned long long)tot);
  }
}

// The asynchronous iterations of a ONE-worker plan (core/Slave.scala:79-111 asyncTask, oracle.c orc_async_step): the
// same layout, slices, exchange and abort word as dsgd_cs64_step_kernel (whose body this repeats: its own code stays as it
// was compiled), the finish of cs64_async_sweep.  The weights are filtered as they are loaded -- the oracle writes
// filt(w - 0) on every coordinate, listed or not.  delta: [G][Sp] slice-major updates of the listed columns, or null.
template <int NT, int SPL, int CLT>
__global__ void __launch_bounds__(NT) dsgd_cs64_async_kernel(Cs64Args a, double* delta) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const int tid = threadIdx.x;
  const int K = a.K;
  Cs64State z;
  z.b = blockIdx.x;
  z.Sp = cs64_sp(a.dp);
  z.w_l = lds64;
  z.ds_l = lds64 + z.Sp;
  z.acc = reinterpret_cast<unsigned long long*>(lds64 + 2 * z.Sp);
  z.ps = lds64 + (2 + K) * z.Sp;
  z.red = z.ps + CS_MAX_SLOTS;
  z.coef = reinterpret_cast<float*>(z.red + 32);
  z.n_act = 0u;
  z.n_rel = 0u;
  CsSet<SPL, CLT> A, B;
  cs64_issue<NT, SPL, CLT>(a, z.b, a.step_begin, A);
  {   // the slice's weights and dimSparsity (the padding holds zeros); the accumulators cleared
    const double2* ws2 = reinterpret_cast<const double2*>(a.w + (long long)z.b * z.Sp);
    const double2* ds2 = reinterpret_cast<const double2*>(a.ds + (long long)z.b * z.Sp);
    double2* wl2 = reinterpret_cast<double2*>(z.w_l);
    double2* dl2 = reinterpret_cast<double2*>(z.ds_l);
    for (int i = tid; i < (z.Sp >> 1); i += NT) {   // (filtered: see above)
      const double2 v = ws2[i];
      wl2[i] = make_double2(filt64(v.x), filt64(v.y));
      dl2[i] = ds2[i];
    }
    for (int i = tid; i < K * z.Sp; i += NT) z.acc[i] = 0ull;
  }
  cs_barrier();
  z.sp = cs64_block_sum<NT>(cs64_wds_share<NT>(z), z.red);
  bool ok = true;
  for (long long step = a.step_begin; step < a.step_end; step += 2) {
    ok = cs64_step<NT, SPL, CLT, true>(a, z, A, B, step, delta);
    if (!ok || step + 1 >= a.step_end) break;
    ok = cs64_step<NT, SPL, CLT, true>(a, z, B, A, step + 1, delta);
    if (!ok) break;
  }
  if (ok) {   // (given up: no slice writes back -- see cs_launch_body)
    double2* ws2 = reinterpret_cast<double2*>(a.w + (long long)z.b * z.Sp);
    const double2* wl2 = reinterpret_cast<const double2*>(z.w_l);
    for (int i = tid; i < (z.Sp >> 1); i += NT) ws2[i] = wl2[i];
  } else if (tid == 0) {
    atomicOr(&a.sc->err, 8);
  }
  if (z.b != 0) return;
  const unsigned int n_act = wave_sum_u32(ok ? z.n_act : 0u);
  __syncthreads();
  unsigned int* r4 = reinterpret_cast<unsigned int*>(z.red);
  if ((tid & 63) == 0) r4[tid >> 6] = n_act;
  __syncthreads();
  if (tid == 0) {
    unsigned int tot = 0u;
    for (int i = 0; i < NT / 64; ++i) tot += r4[i];
    if (tot) atomicAdd(&a.sc->n_active, (unsigned long long)tot);
  }
}

// rank-ordered fp64 vector -> slice-major [G][Sp] (the padding zero) and back
__global__ void __launch_bounds__(256) dsgd_cs64_slice_kernel(const double* __restrict__ v, double* __restrict__ out, int dp, int Sp) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < CS64_G * Sp) {
    const int b = j / Sp, i = j - b * Sp;
    const long long r = (long long)b + (long long)CS64_G * i;
    out[j] = r < dp ? v[r] : 0.0;
  }
}
__global__ void __launch_bounds__(256) dsgd_cs64_unslice_kernel(const double* __restrict__ sl, double* __restrict__ v, int dp, int Sp) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < dp) v[r] = sl[(long long)(r % CS64_G) * Sp + r / CS64_G];
}

// key order <-> rank order, fp64 (and from / to fp32: the float entry points of an fp64 context)
__global__ void dsgd_permute64_in_kernel(const double* __restrict__ in, double* out, const int* __restrict__ perm, int dp) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < dp; j += gridDim.x * blockDim.x) out[perm[j]] = filt64(in[j]);
}
__global__ void dsgd_permute64_out_kernel(const double* __restrict__ in, double* out, const int* __restrict__ perm, int dp) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < dp; j += gridDim.x * blockDim.x) out[j] = in[perm[j]];
}
__global__ void dsgd_promote64_in_kernel(const float* __restrict__ in, double* out, const int* __restrict__ perm, int dp) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < dp; j += gridDim.x * blockDim.x) out[perm[j]] = filt64((double)in[j]);
}
__global__ void dsgd_round64_out_kernel(const double* __restrict__ in, float* out, const int* __restrict__ perm, int dp) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < dp; j += gridDim.x * blockDim.x) out[j] = (float)in[perm[j]];
}

// dimSparsity in fp64 (ref: Main.scala:54-65, oracle.c orc_dim_sparsity): ds[i] = filt(1.0 / (count(feature i+1) + 1.0))
__global__ void dsgd_ds64_kernel(const unsigned int* __restrict__ cnt, const int* __restrict__ perm, double* ds, int dp) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < dp; i += gridDim.x * blockDim.x) {
    const unsigned int c = (i < dp - 1) ? cnt[perm[i + 1]] : 0u;
    ds[perm[i]] = c ? filt64(1.0 / ((double)c + 1.0)) : 0.0;
  }
}

// where rank r's weight is: rank order (Sp = 0) or the column slices' slice-major [CS64_G][Sp] (dsgd_update64_kernel's rule)
__device__ __forceinline__ long long rp64_at(long long r, int Sp) { return Sp ? (r % CS64_G) * Sp + r / CS64_G : r; }

// x . w of row `row` in fp64 by the GR lanes of a group, on float or Double values, the weights in either layout:
// filt((double)x * w) per entry, lane-strided, then a butterfly.  (The layout is decided once per row, not per entry.)
template <int GR, typename V>
__device__ __forceinline__ double row_dot64(const CsrViewT<V>& m, long long row, const double* __restrict__ w, int Sp, int sub) {
#pragma clang fp contract(off)
  const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
  double d = 0.0;
  if (Sp == 0) {
    for (long long p = st + sub; p < en; p += GR) d = d + filt64((double)m.val[p] * w[m.col[p]]);
  } else {
    for (long long p = st + sub; p < en; p += GR) d = d + filt64((double)m.val[p] * w[rp64_at(m.col[p], Sp)]);
  }
#pragma unroll
  for (int off = GR / 2; off >= 1; off >>= 1) d = d + __shfl_xor(d, off, GR);
  return d;
}

// prediction p = -signum(x.w) in fp64 (ref: core/ml/SparseSVM.scala:14, core/Slave.scala:129-140); w in rank order.
// (threads: blockDim.x, read by the kernel itself -- only there does the compiler fold it under the uniform workgroup
// assumption; read in an inlined body it costs a dependent load at the head of every launch.  So in every shared body.)
template <typename V>
__device__ __forceinline__ void forward64_body(const CsrViewT<V>& m, const double* __restrict__ w, const int* __restrict__ idx, long long n,
                                               float* pred, DevScalars* sc, unsigned int threads) {
  const int sub = threadIdx.x % 16;
  const long long group = ((long long)blockIdx.x * threads + threadIdx.x) / 16;
  const long long n_groups = (long long)gridDim.x * threads / 16;
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    const double d = row_dot64<16>(m, row, w, 0, sub);
    if (sub == 0) pred[t] = d > 0.0 ? -1.0f : (d < 0.0 ? 1.0f : 0.0f);
  }
}
__global__ void __launch_bounds__(256) dsgd_forward64_kernel(CsrView m, const double* __restrict__ w, const int* __restrict__ idx,
                                                            long long n, float* pred, DevScalars* sc) {
  forward64_body(m, w, idx, n, pred, sc, blockDim.x);
}
__global__ void __launch_bounds__(256) dsgd_forward64v_kernel(CsrView64 m, const double* __restrict__ w, const int* __restrict__ idx,
                                                             long long n, float* pred, DevScalars* sc) {
  forward64_body(m, w, idx, n, pred, sc, blockDim.x);
}

// loss / accuracy tallies in fp64 (ref: core/Master.scala:100-107, core/ml/SparseSVM.scala:16-23): exact integer counts
template <typename V>
__device__ __forceinline__ void eval64_body(const CsrViewT<V>& m, const double* __restrict__ w, long long row_begin, long long row_end,
                                            DevScalars* sc, unsigned int threads) {
#pragma clang fp contract(off)
  __shared__ unsigned int tally[4];
  const int sub = threadIdx.x % 16;
  const long long group = ((long long)blockIdx.x * threads + threadIdx.x) / 16;
  const long long n_groups = (long long)gridDim.x * threads / 16;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    const double d = row_dot64<16>(m, row, w, 0, sub);
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
__global__ void __launch_bounds__(256) dsgd_eval64_kernel(CsrView m, const double* __restrict__ w, long long row_begin, long long row_end,
                                                         DevScalars* sc) {
  eval64_body(m, w, row_begin, row_end, sc, blockDim.x);
}
__global__ void __launch_bounds__(256) dsgd_eval64v_kernel(CsrView64 m, const double* __restrict__ w, long long row_begin, long long row_end,
                                                          DevScalars* sc) {
  eval64_body(m, w, row_begin, row_end, sc, blockDim.x);
}

// dimSparsity's feature counts on Double values (colcount_body of dsgd_kernels.hpp: abs(v) > 1e-20 decided on the double)
__global__ void __launch_bounds__(1024) dsgd_colcount64v_kernel(const int* __restrict__ col, const double* __restrict__ val, long long nnz,
                                                               unsigned int* cnt, int dp, int hcnt, DevScalars* sc) {
  colcount_body(col, val, nnz, cnt, dp, hcnt, sc, CS64_EPS);
}

// |w|^2 in fp64 (ref: math/Vec.scala:55): one workgroup, lane-strided, then the wave and workgroup sums in order
__global__ void __launch_bounds__(256) dsgd_norm64_kernel(const double* __restrict__ w, int dp, double* out) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  double a = 0.0;
  for (int j = threadIdx.x; j < dp; j += 256) a = a + w[j] * w[j];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

// The lists of an asynchronous run on the zero-lag schedule: update u = first + blockIdx.x is worker k = u mod K at its own
// iteration u div K, and its rows are exactly what the lock-free engine's worker k draws there (hog_sampler / row_at of
// dsgd_hogwild_kernel; oracle/hogwild_replay.hog_rows): base + (mul * t + off) mod n_k, t = 0..batch-1.
struct AsyncListArgs {
  const long long* asg_begin;   // [K] the workers' row ranges
  const long long* asg_end;
  int K, batch, positional_bug;
  unsigned long long seed;
  long long first;
  int* idx_out;                 // [n_updates][batch]
};
__global__ void __launch_bounds__(256) dsgd_async_lists_kernel(AsyncListArgs a) {
  __shared__ unsigned long long mo[2];
  const long long u = a.first + (long long)blockIdx.x;
  const int worker = (int)(u % a.K);
  const unsigned long long it = (unsigned long long)(u / a.K);
  const long long begin = a.asg_begin[worker];
  const unsigned int n_k = (unsigned int)(a.asg_end[worker] - begin);
  if (threadIdx.x == 0) {
    const unsigned long long key = hog_mix(a.seed ^ hog_mix((unsigned long long)worker * 0x100000001B3ull + it));
    unsigned int mul = 1u + (unsigned int)(hog_mix(key) % (unsigned long long)n_k);
    while (hog_gcd32(mul, n_k) != 1u) mul = mul % n_k + 1u;
    mo[0] = mul;
    mo[1] = hog_mix(key ^ 0xABCDEF12345ull) % (unsigned long long)n_k;
  }
  __syncthreads();
  const unsigned long long mul = mo[0], off = mo[1];
  const long long base = a.positional_bug ? 0 : begin;   // ref: core/Slave.scala:87 indexes `data` by POSITION
  int* out = a.idx_out + (long long)blockIdx.x * a.batch;
  for (int t = threadIdx.x; t < a.batch; t += 256) out[t] = (int)(base + (long long)((mul * (unsigned long long)t + off) % n_k));
}

// A peer's update (core/Slave.scala:177-185, GradState.scala:8): w[k] = filt(w[k] - dv) for each (unique) key, in
// whichever layout the weights are: rank order (Sp = 0) or slice-major [G][Sp]
__global__ void __launch_bounds__(256) dsgd_update64_kernel(const int* __restrict__ key, const double* __restrict__ dv, int nnz,
                                                           const int* __restrict__ perm, double* w, int Sp) {
#pragma clang fp contract(off)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += gridDim.x * blockDim.x) {
    const int r = perm[key[i]];
    const long long at = Sp ? (long long)(r % CS64_G) * Sp + r / CS64_G : (long long)r;
    w[at] = filt64(w[at] - dv[i]);
  }
}
// ... then the whole vector filtered, as dsgd_filter_kernel does for the fp32 weights
__global__ void __launch_bounds__(256) dsgd_filter64_kernel(double* w, int n) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) w[j] = filt64(w[j]);
}
