// Device code of libdsgd_hip, part 16 (gfx950 only): the LOGISTIC model's ASYNCHRONOUS iterations of a ONE-worker plan as a
// persistent column-slice kernel (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS).  Included by dsgd_hip.hip
// after dsgd_lg_cs.hpp, which stays as it is: this is a SIBLING body, so that dsgd_lg_cs_step_kernel compiles to the code it
// compiled to.
//
// What is dsgd_lg_cs_step_kernel's, unchanged and shared: LgCsArgs, LgCsSet, LgCsState, lg_cs_issue, the LDS carve of
// lg_cs_lds(dp, G, 1), the (step, slice) cell layout, cs_issue / cs_gather, the tagged granules with the context's tag counter, the
// abort word and CS_POLL_LIMIT, the weights in LDS for the whole run, the next step's slots requested during the exchange, and
// the err = 8 exit that writes no weight back.  Phases 0 - 4 of a step are that kernel's, restated for K = 1 (the host refuses
// any other plan).  The finish is dsgd_lg_async_finish_kernel's arithmetic on EVERY column of the slice, fp64, contraction off:
//   G = acc 2^(vexp - S),  gm = G / n,  r = gm + 2 lambda w_j,  delta = lr r,  w_j' = (float)(w_j - delta)
// with S = lg_shift(n) and n the length of the update's list; n rides as a double (a length is below 2^40: exact) in inv[1], a
// scale word K = 1 leaves unused.
//
// Plain C++ and vector stores only.
#pragma once
#include "dsgd_lg_cs.hpp"

static_assert(CS_MAX_K >= 2, "the asynchronous step keeps n in inv[1]");

// One asynchronous update.  false = the launch was aborted.
template <int SPL>
__device__ __forceinline__ bool lg_cs_async_step(const LgCsArgs& la, LgCsState& z, LgCsSet<SPL>& cur, LgCsSet<SPL>& nxt, long long step) {
#pragma clang fp contract(off)
  constexpr int NT = CS_THREADS;
  const CsArgs& a = la.cs;
  int tid = threadIdx.x, G = __builtin_amdgcn_readfirstlane(a.G), b = z.b;
  asm volatile("" : "+v"(tid));
  asm volatile("" : "+s"(G));
  const int n_slots = __builtin_amdgcn_readfirstlane((int)(cur.s.h.x & 0xffffu));
  const int n_rows = __builtin_amdgcn_readfirstlane((int)(cur.s.h.x >> 16));
  // ---- 0: the update's shift and length, from the plan's list (lane 0 holds worker 0's n) ----
  if (tid == 0) {
    const int S = lg_shift(cur.nk);
    z.qs[0] = ldexp(1.0, S - a.vexp);
    z.inv[0] = ldexp(1.0, a.vexp - S);
    z.inv[1] = (double)cur.nk;
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
  // ---- the NEXT update's slots and list length: they land while this workgroup waits for its peers' granules ----
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
  // ---- 4: rn(x cq) of every entry into the one worker's accumulator (exact integer sums).  |x cq| <= 2^S <= 2^62 ----
  const double qs0 = z.qs[0];
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int slot = tid + NT * i;
    if (slot < n_slots) {
      const int row = (int)(cur.s.meta[i] & 0xffffu);
      const double y = ((z.ymask[row >> 5] >> (row & 31)) & 1u) ? 1.0 : -1.0;
      const double cq = lg_coef(z.d[row], y) * qs0;   // (a power of two: exact)
#pragma unroll
      for (int j = 0; j < CS_L; ++j) {
        const long long q = __double2ll_rn((double)CS_VAL(cur.s, i, j) * cq);
        if (q != 0) atomicAdd(&z.acc[CS_COL(cur.s, i, j)], (unsigned long long)q);   // (two's complement: one add; the padding adds nothing)
      }
    }
  }
  cs_barrier();
  // ---- 5: EVERY column of the slice: dsgd_lg_async_finish_kernel's arithmetic (the L2 term touches all of them) ----
  const double reg2 = 2.0 * la.lambda, inv0 = z.inv[0], nd = z.inv[1];
  for (int c = tid; c < z.Sb; c += NT) {
    const double wj = (double)z.w_l[c];
    unsigned long long* at_0 = z.acc + c;
    const unsigned long long t = *at_0;
    if (t != 0ull) *at_0 = 0ull;
    const double G0 = (double)(long long)t * inv0;   // one rounding of the exact sum
    const double gm = G0 / nd;
    const double r = gm + reg2 * wj;
    const double delta = la.lr * r;
    z.w_l[c] = (float)(wj - delta);
  }
  cs_barrier();
  ++z.n_rel;
  return true;
}

// The asynchronous iterations [step_begin, step_end) of a ONE-worker plan in one persistent launch.
// grid: G workgroups of CS_THREADS lanes; dynamic LDS: lg_cs_lds(dp, G, 1).words words
template <int SPL>
__global__ void __launch_bounds__(CS_THREADS) dsgd_lg_cs_async_kernel(LgCsArgs la) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NT = CS_THREADS;
  const CsArgs& a = la.cs;
  const int tid = threadIdx.x;
  const int G = a.G;
  const LgCsLds L = lg_cs_lds(a.dp, G, 1);
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
  // the first update's slots are requested before anything else: they land with the weights
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
        for (int i = tid; i < z.Sp; i += NT) z.acc[i] = 0ull;
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
    ok = lg_cs_async_step<SPL>(la, z, A, B, step);
    if (!ok || step + 1 >= a.step_end) break;
    ok = lg_cs_async_step<SPL>(la, z, B, A, step + 1);
    if (!ok) break;
  }
  if (!ok) {   // given up: NO slice has written its weights back (all or none, as dsgd_lg_cs_step_kernel)
    if (tid == 0) atomicOr(&a.sc->err, 8);
    return;
  }
  float4* ws4 = reinterpret_cast<float4*>(a.w + (long long)z.b * z.Sp);
  const float4* wl4 = reinterpret_cast<const float4*>(z.w_l);
  for (int i4 = tid; i4 < (z.Sp >> 2); i4 += NT) ws4[i4] = wl4[i4];
}
