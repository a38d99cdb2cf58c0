// Device code of libdsgd_hip, part 15 (gfx950 only): the LOGISTIC model's steps of the reference's own batch sizes (3 x 100,
// 4 x 200) as a persistent column-slice kernel -- the shape of dsgd_cs_step_kernel (csrc/dsgd_cs.hpp) with the arithmetic of
// csrc/dsgd_logistic.hpp.  Included by dsgd_hip.hip after dsgd_cs.hpp and dsgd_logistic.hpp.  DESIGN.md 3.13.
//
// What is the SVM family's, unchanged: the (step, slice) cell layout and its device builder (dsgd_cs_layout_kernel -- plain
// floats, the label in row_first bit 15, row and worker in slot_meta), cs_issue, cs_gather, the tagged granules of the
// context's exchange buffer with its tag counter, the abort word and CS_POLL_LIMIT, the slice-major weights and the two
// kernels that convert them.  LG_CS_G = 16 persistent workgroups, workgroup b owning the ranks r = b (mod 16); the weights
// stay in LDS for all steps of one dsgd_plan_run; step n + 1's slots are requested while step n waits in its exchange.
//
// Per step and slice:
//   dot      the partial x.w of every slot (<= 16 products added in sequence, the engine's 1e-20 product filter), a row's
//            slots added in order, published as ONE granule per row; the G partials of a row gathered and added in slice
//            order: every workgroup holds the same d, bit for bit.  Nothing is exchanged for w . ds: dimSparsity plays no part.
//   scatter  the lane of a slot takes d and the label of its row, cq = lg_coef(d, y) 2^(S_k - vexp) with S_k = lg_shift(n_k),
//            n_k the length of the row's worker's list (the plan's resident d_segs, requested with the step's slots), and
//            adds rn((double)x cq) -- lg_add's expression -- to the worker's int64 accumulator of the column (ds_add_u64).
//            Integer sums: whatever the order, the same bits.
//   finish   EVERY column of the slice, in fp64 with contraction off, the arithmetic of dsgd_lg_finish_kernel<LG_STEP> column
//            for column: G_k = acc_k 2^(vexp - S_k), r_k = G_k + 2 lambda w_j added in worker order, / K,
//            w_j' = (float)(w_j - lr mean); the accumulators left zeroed.  The slice's padding columns are never touched.
// The weights are NOT the row form's bits (d is a sum of slice partials, not row_dot's lane order); they are a function of the
// lists and the starting weights alone, within tests/logistic_cs_bound.py of the fp64 model.
// A launch that gives up its bounded wait ends with DevScalars::err = 8 and writes no weight back, as the SVM's.
//
// Plain C++ and vector stores only.
#pragma once
#include "dsgd_lg_cs_host.hpp"

static_assert(LG_CS_G <= CS_MAX_G && (LG_CS_G == 8 || LG_CS_G == 16), "cs_gather polls 8 or 16 slices");

struct LgCsArgs {
  CsArgs cs;              // the layout arrays, the exchange and the launch's steps (ds, clist, the mailbox and the record: unused)
  const WorkSeg* segs;    // [n_steps_plan][K]: the plan's resident list ranges -- their lengths give every worker's shift
  double lr, lambda;
};

template <int SPL>
struct LgCsSet {
  CsSet<SPL, 1> s;
  long long nk;           // lanes below K: rows of worker `lane` in the step
};

struct LgCsState {
  unsigned long long* acc;
  float* w_l;
  float* ps;
  float* d;
  unsigned int* ymask;
  double* qs;             // [CS_MAX_K] 2^(S_k - vexp)
  double* inv;            // [CS_MAX_K] 2^(vexp - S_k)
  int* red;
  int b, Sb, Sp;
  unsigned int n_rel;     // steps of this launch behind us
};

template <int SPL>
__device__ __forceinline__ void lg_cs_issue(const LgCsArgs& la, int b, long long step, LgCsSet<SPL>& R) {
  cs_issue<CS_THREADS, SPL, 1>(la.cs, b, step, R.s);
  const long long sc = step < la.cs.step_end ? step : la.cs.step_end - 1;   // (clamped, as cs_issue)
  const int k = (int)threadIdx.x < la.cs.K ? (int)threadIdx.x : la.cs.K - 1;
  const longlong2* sp = reinterpret_cast<const longlong2*>(la.segs + sc * la.cs.K + k);
  asm volatile("" : "+v"(sp));   // (a vector load, as the header's)
  const longlong2 sg = *sp;
  R.nk = sg.y - sg.x;
}

// One step.  false = the launch was aborted.
template <int SPL>
__device__ __forceinline__ bool lg_cs_step(const LgCsArgs& la, LgCsState& z, LgCsSet<SPL>& cur, LgCsSet<SPL>& nxt, long long step) {
#pragma clang fp contract(off)
  constexpr int NT = CS_THREADS;
  const CsArgs& a = la.cs;
  int tid = threadIdx.x, G = __builtin_amdgcn_readfirstlane(a.G), K = __builtin_amdgcn_readfirstlane(a.K), b = z.b,
      Sp = __builtin_amdgcn_readfirstlane(z.Sp);
  asm volatile("" : "+v"(tid));
  asm volatile("" : "+s"(G), "+s"(K), "+s"(Sp));
  const int n_slots = __builtin_amdgcn_readfirstlane((int)(cur.s.h.x & 0xffffu));
  const int n_rows = __builtin_amdgcn_readfirstlane((int)(cur.s.h.x >> 16));
  // ---- 0: the step's shifts, one per worker, from the lengths of the plan's lists (not the header's SVM shift) ----
  if (tid < K) {
    const int S = lg_shift(cur.nk);
    z.qs[tid] = ldexp(1.0, S - a.vexp);
    z.inv[tid] = ldexp(1.0, a.vexp - S);
  }
  // ---- 1: partial x.w of every slot from this slice's weights ----
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    float p = 0.0f;
#pragma unroll
    for (int j = 0; j < CS_L; ++j) p += filt(CS_VAL(cur.s, i, j) * z.w_l[CS_COL(cur.s, i, j)]);
    const int slot = tid + NT * i;
    if (slot < n_slots) z.ps[slot] = p;
  }
  if (tid == 0) z.red[17] = 0;
  cs_barrier();
  // ---- 2: this slice's partial of every row (its slots in order), one granule {value, tag} per row ----
  const unsigned int tag = a.tag0 + z.n_rel + 1u;
  unsigned long long* xb = a.xbuf + ((long long)(z.n_rel & 1u) * G + b) * CS_XSTRIDE;
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int r = tid + NT * i;
    if (r < n_rows) {
      const int f0 = (int)(cur.s.rf[i] & 0x7ffu), f1 = (int)((cur.s.rf[i] >> 16) & 0x7ffu);
      float t = 0.0f;
      for (int f = f0; f < f1; ++f) t += z.ps[f];
      __hip_atomic_store(&xb[r], ((unsigned long long)tag << 32) | __float_as_uint(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // ---- the NEXT step's slots and list lengths: they land while this workgroup waits for its peers' granules ----
  lg_cs_issue<SPL>(la, b, step + 1, nxt);
  // ---- 3: every slice's granules of this thread's rows, added in slice order: d; the labels as one bit per row ----
  const unsigned long long* xall = a.xbuf + (long long)(z.n_rel & 1u) * G * CS_XSTRIDE;
  int at[SPL];
  float dd[SPL];
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int r = tid + NT * i;
    at[i] = r < n_rows ? r : -1;
  }
  const bool got = cs_gather<SPL>(xall, G, at, tag, &a.sync[1], dd);
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int r = tid + NT * i;
    const bool in = r < n_rows;
    if (in) z.d[r] = dd[i];
    const unsigned long long m = __ballot(in && (cur.s.rf[i] & 0x8000u) != 0u);
    if ((tid & 63) == 0) {   // (rows r0 .. r0 + 63 of this wave: two words, all of them below CS_MAX_SLOTS)
      const int r0 = tid + NT * i;
      z.ymask[r0 >> 5] = (unsigned int)m;
      z.ymask[(r0 >> 5) + 1] = (unsigned int)(m >> 32);
    }
  }
  if (!got) z.red[17] = 1;
  cs_barrier();
  if (z.red[17]) return false;
  // ---- 4: rn(x cq) of every entry into the accumulator of the row's worker (exact integer sums; the non-zeros are still in
  //         registers).  |x cq| <= 2^S_k <= 2^62 ----
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int slot = tid + NT * i;
    if (slot < n_slots) {
      const int row = (int)(cur.s.meta[i] & 0xffffu), k = (int)((cur.s.meta[i] >> 16) & 15u);
      const double y = ((z.ymask[row >> 5] >> (row & 31)) & 1u) ? 1.0 : -1.0;
      const double cq = lg_coef(z.d[row], y) * z.qs[k];   // (a power of two: exact)
      unsigned long long* ak = z.acc + (long long)k * Sp;
#pragma unroll
      for (int j = 0; j < CS_L; ++j) {
        const long long q = __double2ll_rn((double)CS_VAL(cur.s, i, j) * cq);
        if (q != 0) atomicAdd(&ak[CS_COL(cur.s, i, j)], (unsigned long long)q);   // (two's complement: one add; the padding adds nothing)
      }
    }
  }
  cs_barrier();
  // ---- 5: EVERY column of the slice: dsgd_lg_finish_kernel<LG_STEP>'s arithmetic (the L2 term touches all of them) ----
  const double reg2 = 2.0 * la.lambda, kd = (double)K;
  for (int c = tid; c < z.Sb; c += NT) {
    const double wj = (double)z.w_l[c];
    const double reg = reg2 * wj;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
      unsigned long long* at_k = z.acc + (long long)k * Sp + c;
      const unsigned long long t = *at_k;
      if (t != 0ull) *at_k = 0ull;
      const double Gk = (double)(long long)t * z.inv[k];   // one rounding of the exact sum
      sum = sum + (Gk + reg);
    }
    const double mean = sum / kd;
    z.w_l[c] = (float)(wj - la.lr * mean);
  }
  cs_barrier();
  ++z.n_rel;
  return true;
}

// grid: G workgroups of CS_THREADS lanes; dynamic LDS: lg_cs_lds(dp, G, K).words words
template <int SPL>
__global__ void __launch_bounds__(CS_THREADS) dsgd_lg_cs_step_kernel(LgCsArgs la) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NT = CS_THREADS;
  const CsArgs& a = la.cs;
  const int tid = threadIdx.x;
  const int G = a.G, K = a.K;
  const LgCsLds L = lg_cs_lds(a.dp, G, K);
  LgCsState z;
  z.b = blockIdx.x;
  z.Sb = (a.dp - z.b + G - 1) / G;   // this slice's columns (ranks b, b + G, ...); beyond them: padding
  z.Sp = L.sp;
  z.acc = reinterpret_cast<unsigned long long*>(lds + L.acc);
  z.w_l = lds + L.w;
  z.ps = lds + L.ps;
  z.d = lds + L.d;
  z.ymask = reinterpret_cast<unsigned int*>(lds + L.ymask);
  z.qs = reinterpret_cast<double*>(lds + L.scale);
  z.inv = z.qs + CS_MAX_K;
  z.red = reinterpret_cast<int*>(lds + L.red);
  z.n_rel = 0u;
  // the first step's slots are requested before anything else: they land with the weights
  LgCsSet<SPL> A, B;
  lg_cs_issue<SPL>(la, z.b, a.step_begin, A);
  {   // the slice's weights: one contiguous piece (the padding holds zeros); the accumulators are cleared while it is on its way
    const float4* ws4 = reinterpret_cast<const float4*>(a.w + (long long)z.b * z.Sp);
    float4* wl4 = reinterpret_cast<float4*>(z.w_l);
    constexpr int UB = 4;
    const int n4 = z.Sp >> 2;
    for (int i0 = tid, round = 0; round == 0 || i0 < n4; i0 += NT * UB, ++round) {   // (every lane runs the first round)
      float4 wv[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int i4 = i0 + NT * u;
        wv[u] = ws4[i4 < n4 ? i4 : n4 - 1];
      }
      if (round == 0)
        for (int i = tid; i < K * z.Sp; i += NT) z.acc[i] = 0ull;
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int i4 = i0 + NT * u;
        if (i4 < n4) wl4[i4] = wv[u];
      }
    }
  }
  cs_barrier();
  bool ok = true;
  for (long long step = a.step_begin; step < a.step_end; step += 2) {   // two register sets, rotated by unrolling
    ok = lg_cs_step<SPL>(la, z, A, B, step);
    if (!ok || step + 1 >= a.step_end) break;
    ok = lg_cs_step<SPL>(la, z, B, A, step + 1);
    if (!ok) break;
  }
  if (!ok) {   // given up: NO slice has written its weights back (csrc/dsgd_cs.hpp, cs_launch_body: all or none)
    if (tid == 0) atomicOr(&a.sc->err, 8);
    return;
  }
  float4* ws4 = reinterpret_cast<float4*>(a.w + (long long)z.b * z.Sp);
  const float4* wl4 = reinterpret_cast<const float4*>(z.w_l);
  for (int i4 = tid; i4 < (z.Sp >> 2); i4 += NT) ws4[i4] = wl4[i4];
}
