// Device code of libdsgd_hip, part 15f (gfx950 only): SOFTMAX regression over 2 to 32 classes with the LANES ACROSS THE
// NON-ZEROS (include/dsgd.h "THE LOGISTIC MODEL": SOFTMAX, FEW CLASSES; DESIGN.md 3.13 "Softmax, few classes").  Included behind
// dsgd_lg_softmax.hpp, whose kernels -- and lgsm_row -- stay as they are.
//
// The layout is the interleaved topics': Wi[rank][TP], Pi[row][TP], acc[k][rank][TP].  The contract is the WIDE softmax's bits
// (csrc/dsgd_lg_softmax.hpp) for every C <= 32: weights, |w_c|^2, loss, accuracy, classes and probabilities.
//
// The split is the interleaved topics' (csrc/dsgd_lg_topics_il.hpp): one 16-lane group per row, lane `sub` takes the non-zeros
// st + sub + 16 i and carries ALL classes.  Softmax needs every logit before any coefficient, so the row is walked ONCE with
// 4 NQ fp32 accumulators per lane (NQ quads: the kernels' template argument, lgsi_quads(TP) = 1, 2, 4 or 8), one 16-byte load of
// Wi per quad and non-zero; a quad at or beyond TP is never loaded (lgsi_quad_in, uniform).  Accumulator c takes
// lgti_row_dots' sequence for class c: the registers, then the tail, d += filt(v * w), from +0.0f.
//
// From 16 partial sums per class to the wide placement "lane l holds classes 2l and 2l + 1": a reduce-scatter over the xor
// steps 1, 2, 4, 8 (lgsi_scatter).  At the step with offset 2^s a lane holds N classes, keeps the N / 2 whose bit s + 1 equals
// its own lane bit s, adds what its partner hands over for them and hands the others over.  group_sum<16> (csrc/dsgd_kernels.hpp)
// adds, per class, lane ^ 1 (pairs), lane ^ 2 (quads), the mirror within 8 (of values equal within a quad: quad + quad) and the
// mirror within 16 (half + half): the tree
//   [((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7))] + [((a8+a9)+(a10+a11)) + ((a12+a13)+(a14+a15))].
// Every step here adds the same two values that two lanes hold, in one order or the other, and IEEE addition commutes: each
// class's sum has that tree and those bits.  When two classes are left (after log2(4 NQ) - 1 steps) the remaining steps are plain
// butterflies: lane l ends with classes 2 (l mod 2 NQ) and that + 1 -- for 2l < TP its own pair, else a copy that takes no part
// (in0 = in1 = false, the wide form's `own`).  2 NQ + NQ + ... adds and exchanges per lane, not 4 * 4 NQ.
//
// Then lgtw_labels2 at the lane's pair and lgsm_row<16, GRAD>, UNCHANGED: the only floating-point order in softmax.
//
//   the gradient    dsgd_lg_softmax_il_grad_kernel<NQ> (index lists): the interleaved gradient's grid and 16 KiB head
//                   (lgti_hot(TP) ranks); quad by quad the four coefficients come back to every lane (__shfl of lane c / 2's
//                   pair) and each lane adds them for its OWN non-zeros (lgsi_add4: lgti_add<4>'s expression): 16 lanes adding
//                   in parallel.  Integer sums: no order
//   coefficients    dsgd_lg_softmax_il_coef_kernel<NQ> (row ranges): lanes with 2l < TP store their pair into cq[position][TP],
//                   exactly 0.0 for a padding class; then the EXISTING dsgd_lg_topics_cgrad_kernel<16> and interleaved finish
//   the evaluation  dsgd_lg_softmax_il_eval_kernel<NQ>: the wide softmax evaluation's 512 lanes, 32 chains (chain g = rows
//                   row_begin + 32 block + g + i n_chains, in order), grid, LDS carve and tree; the tile through lgti_w4<true>
//   predict         dsgd_lg_softmax_il_predict_kernel<NQ>: the class byte from lane 0 of the group, (float)p_c class-major
// The finish, |w_c|^2 and the weights' way across the boundary are the interleaved form's, unchanged.
//
// What the gfx950 compile reports (every instantiation: no scratch, no spill): DESIGN.md 3.13 "Softmax, few classes".
//
// Plain C++, vector loads, vector stores and vector atomics only.
#pragma once
#include "dsgd_lg_softmax_il_host.hpp"

// one non-zero (rank c, value v) into the lane's 4 NQ accumulators
template <int NQ, bool LDSW>
__device__ __forceinline__ void lgsi_nz(int c, float v, const float* wl, const float* __restrict__ wi, int tp, int hw, float (&d)[4 * NQ]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (lgsi_quad_in(NQ, q, tp)) {
      const float4 w = lgti_w4<LDSW>(wl, wi, c, tp, 4 * q, hw);
      d[4 * q + 0] += filt(v * w.x);
      d[4 * q + 1] += filt(v * w.y);
      d[4 * q + 2] += filt(v * w.z);
      d[4 * q + 3] += filt(v * w.w);
    }
  }
}

// N classes' partial sums, the step with xor offset OFF (file comment).  d[j]: bit 0 of j is the class's bit 0, the bits above
// are the class's bits not yet decided, lowest first; the decided ones are the lane's bits below OFF
template <int N, int OFF>
__device__ __forceinline__ void lgsi_scatter(const float (&d)[N], int sub, float& d0, float& d1) {
#pragma clang fp contract(off)
  if constexpr (N == 2) {
    float a = d[0], b = d[1];
#pragma unroll
    for (int off = OFF; off < LG_GROUP; off <<= 1) {
      a = a + __shfl_xor(a, off, LG_GROUP);
      b = b + __shfl_xor(b, off, LG_GROUP);
    }
    d0 = a, d1 = b;
  } else {
    static_assert(OFF < LG_GROUP, "at most 32 classes");
    const bool hi = (sub & OFF) != 0;
    float e[N / 2];
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
      const int j0 = (j & 1) | ((j >> 1) << 2), j1 = j0 | 2;
      const float keep = hi ? d[j1] : d[j0], send = hi ? d[j0] : d[j1];
      e[j] = keep + __shfl_xor(send, OFF, LG_GROUP);
    }
    lgsi_scatter<N / 2, OFF * 2>(e, sub, d0, d1);
  }
}

// THE row, written once: the row [st, en), its first chunks in r -- the logits of classes 2 (sub mod 2 NQ) and that + 1
template <int NQ, bool LDSW>
__device__ __forceinline__ void lgsi_row_logits(const CsrView& m, long long st, long long en, const float* wl, const float* __restrict__ wi, int tp,
                                                int hw, int sub, const RowRegs<LG_GROUP, LG_UNR>& r, float& d0, float& d1) {
  static_assert(NQ == 1 || NQ == 2 || NQ == 4 || NQ == 8, "a power of two of quads");
  float d[4 * NQ];
#pragma unroll
  for (int i = 0; i < 4 * NQ; ++i) d[i] = 0.0f;
#pragma unroll
  for (int k = 0; k < LG_UNR; ++k)
    if (r.c[k] >= 0) lgsi_nz<NQ, LDSW>(r.c[k], r.v[k], wl, wi, tp, hw, d);
  for (long long p = st + sub + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) lgsi_nz<NQ, LDSW>(m.col[p], m.val[p], wl, wi, tp, hw, d);
  lgsi_scatter<4 * NQ, 1>(d, sub, d0, d1);
}

// the lane's part of a row's step: the logits, the labels, the coefficient pair (exactly 0.0 where the lane owns no real class)
template <int NQ>
__device__ __forceinline__ void lgsi_row_coef(const CsrView& m, long long row, long long st, long long en, const float* __restrict__ wi,
                                              const signed char* __restrict__ pi, int C, int tp, bool own, int lo, int sub,
                                              const RowRegs<LG_GROUP, LG_UNR>& r, double qscale, double& cq0, double& cq1) {
  float d0, d1;
  lgsi_row_logits<NQ, false>(m, st, en, nullptr, wi, tp, 0, sub, r, d0, d1);
  double y0, y1;
  lgtw_labels2(pi, row, tp, lo, y0, y1);
  const bool in0 = own && lo < C, in1 = own && lo + 1 < C;
  double loss;
  int pred, ycls;
  lgsm_row<LG_GROUP, true>(d0, d1, in0, in1, in0 && y0 > 0.0, in1 && y1 > 0.0, qscale, cq0, cq1, loss, pred, ycls);
}

// lgti_add<4>'s expression for the four adjacent words of rank c from t0 on; a padding class's cq is 0: nothing is added.  A
// function of its own with lgtw_atomic_add: lgti_add names HIP's atomicAdd, which a kernel that turns a target feature off CALLS,
// and a second kernel calling that copy moved dsgd_lg_topics_il_grad_kernel's registers -- its assembly stays as it is
__device__ __forceinline__ void lgsi_add4(unsigned long long* hot, unsigned long long* acc, int n_hot, int tp, int t0, int c, float x,
                                          const double (&cq)[4]) {
#pragma clang fp contract(off)
  const double xd = (double)x;
  if (c < n_hot) {
    unsigned long long* at = hot + c * tp + t0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long q = __double2ll_rn(xd * cq[i]);   // |x cq| <= 2^S <= 2^62
      if (q != 0) lgtw_atomic_add(&at[i], (unsigned long long)q);
    }
  } else {
    unsigned long long* at = acc + (long long)c * tp + t0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long q = __double2ll_rn(xd * cq[i]);
      if (q != 0) lgtw_atomic_add(&at[i], (unsigned long long)q);
    }
  }
}

// a uniform value kept in VECTOR registers from here on (opaque to the compiler, as the wide evaluation's lane number): the
// gradient's scalar registers are all taken by the arguments, the masks and exp's constants, and what the row loop reads once per
// row or never -- the error word, the row count, the sums' base, the list, its length and stride, the labels' and the row starts' base -- costs nothing
// there.  ON: by the instantiation, no more than its scalar registers need (a vector register more can cost a wave per SIMD)
template <bool ON, typename T>
__device__ __forceinline__ T lgsi_in_vgpr(T x) {
  if constexpr (ON) asm volatile("" : "+v"(x));
  return x;
}

// (the kernels' bodies are always-inline functions, as lgtc_coef_body: what they name is inlined with them)
template <int NQ>
__device__ __forceinline__ void lgsi_grad_body(const CsrView& m, const LgtiArgs& a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hot[LGTI_HOT_WORDS];   // [a.hot][a.tp]
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const double qscale = ldexp(1.0, lg_shift(seg.end - seg.begin) - a.vexp);   // (a power of two: c * qscale is exact)
  const long long n = lgsi_in_vgpr<NQ >= 8>(seg.end - seg.begin), n_rows = lgsi_in_vgpr<NQ >= 2>(m.n_rows);
  unsigned long long* acc = lgsi_in_vgpr<NQ >= 4>(a.acc + (long long)k * a.acc_stride);
  DevScalars* sc = lgsi_in_vgpr<NQ >= 2>(a.sc);
  const signed char* pi = lgsi_in_vgpr<NQ >= 8>(a.pi);
  const int* list = lgsi_in_vgpr<NQ >= 8>(a.idx + seg.begin);
  const long long* row_ptr = lgsi_in_vgpr<NQ >= 8>(m.row_ptr);
  const int sub = tid % LG_GROUP;
  const int tp = a.tp, n_hot = a.hot;
  const bool own = 2 * sub < tp;
  const int lo = own ? 2 * sub : 0;
  const long long groups = lgsi_in_vgpr<NQ >= 8>(a.blocks_per_worker * LG_ROWS_PER_BLOCK);
  for (int j = tid; j < n_hot * tp; j += LG_THREADS) hot[j] = 0ull;
  lgtw_barrier();
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = (long long)list[t];
    if (row < 0 || row >= n_rows) {   // (the host checked the lists: never taken)
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    const long long st = row_ptr[row], en = row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    double cq0, cq1;
    lgsi_row_coef<NQ>(m, row, st, en, a.wi, pi, a.T, tp, own, lo, sub, r, qscale, cq0, cq1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (lgsi_quad_in(NQ, q, tp)) {   // (uniform: every lane of the group takes part in the exchanges)
        const double cq[4] = {__shfl(cq0, 2 * q, LG_GROUP), __shfl(cq1, 2 * q, LG_GROUP), __shfl(cq0, 2 * q + 1, LG_GROUP),
                              __shfl(cq1, 2 * q + 1, LG_GROUP)};
#pragma unroll
        for (int u = 0; u < LG_UNR; ++u)
          if (r.c[u] >= 0) lgsi_add4(hot, acc, n_hot, tp, 4 * q, r.c[u], r.v[u], cq);
        for (long long p = st + sub + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) lgsi_add4(hot, acc, n_hot, tp, 4 * q, m.col[p], m.val[p], cq);
      }
    }
  }
  lgtw_barrier();
  for (int j = tid; j < n_hot * tp; j += LG_THREADS) {   // (the head is acc's first words; a word is non-zero only below dp)
    const unsigned long long v = hot[j];
    if (v) lgtw_atomic_add(&acc[j], v);
  }
}

template <int NQ>
__device__ __forceinline__ void lgsi_coef_body(const CsrView& m, const LgtcCoefArgs& a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);
  const int sub = tid % LG_GROUP;
  const int tp = a.tp;
  const bool own = 2 * sub < tp;
  const int lo = own ? 2 * sub : 0;
  double* cq = a.cq + (long long)a.pos_base[k] * tp + lo;
  const long long groups = a.blocks_per_worker * LG_ROWS_PER_BLOCK;
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = seg.begin + t;
    if (row < 0 || row >= m.n_rows) {   // (the host checked the ranges: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    double cq0, cq1;
    lgsi_row_coef<NQ>(m, row, st, en, a.wi, a.pi, a.T, tp, own, lo, sub, r, qscale, cq0, cq1);
    if (own) *reinterpret_cast<double2*>(cq + t * tp) = make_double2(cq0, cq1);   // (an empty row's as any other's: p = 1 / C)
  }
}

template <int NQ>
__device__ __forceinline__ void lgsi_eval_body(const CsrView& m, const float* __restrict__ wi, const signed char* __restrict__ pi, int C,
                                               long long row_begin, long long row_end, unsigned long long* tally, int hw, double* loss_part) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tp = lgti_tp(C), tid = threadIdx.x;
  double* sums = reinterpret_cast<double*>(lds + lgsm_eval_sums_at(hw, C));             // [LGSM_EVAL_CHAINS]
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + lgsm_eval_cnt_at(hw, C));   // {correct, wrong}
  for (int j = tid; j < hw * tp; j += LGSM_EVAL_THREADS) lds[j] = wi[j];                // (Wi's first hw ranks ARE the tile)
  if (tid < 2) cnt[tid] = 0u;
  lgtw_barrier();
  const int sub = tid % LG_GROUP, g = tid / LG_GROUP;   // the chain: rows row_begin + (block, g) + i * n_chains, in order
  const bool own = 2 * sub < tp;
  const int lo = own ? 2 * sub : 0;
  const bool in0 = own && lo < C, in1 = own && lo + 1 < C;
  const long long n_chains = (long long)gridDim.x * LGSM_EVAL_CHAINS;
  double ls = 0.0;
  for (long long row = row_begin + (long long)blockIdx.x * LGSM_EVAL_CHAINS + g; row < row_end; row += n_chains) {
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    float d0, d1;
    lgsi_row_logits<NQ, true>(m, st, en, lds, wi, tp, hw, sub, r, d0, d1);
    double y0, y1;
    lgtw_labels2(pi, row, tp, lo, y0, y1);
    double p0, p1, l;
    int pred, ycls;
    lgsm_row<LG_GROUP, false>(d0, d1, in0, in1, in0 && y0 > 0.0, in1 && y1 > 0.0, 1.0, p0, p1, l, pred, ycls);
    ls = ls + l;
    if (sub == 0) (void)__hip_atomic_fetch_add(&cnt[pred == ycls ? 0 : 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (sub == 0) sums[g] = ls;   // (the same bits in every lane of the group)
  lgtw_barrier();
  if (tid < 2) {
    const unsigned int v = cnt[tid];
    if (v) lgtw_atomic_add(&tally[tid], (unsigned long long)v);
  }
  // one fixed tree: chain g's sum on lane sub == 0 of the 16-lane run g, 0.0 on the others
  const double mine = sub == 0 ? sums[g] : 0.0;
  const double total = lg_block_sum(mine, reinterpret_cast<double*>(lds + lgsm_eval_red_at(hw, C)), LGSM_EVAL_THREADS / 64);
  if (tid == 0) loss_part[blockIdx.x] = total;
}

template <int NQ>
__device__ __forceinline__ void lgsi_predict_body(const CsrView& m, const float* __restrict__ wi, int C, const int* __restrict__ idx, long long n,
                                                  unsigned char* cls_out, float* p_out, DevScalars* sc) {
#pragma clang fp contract(off)
  const int tp = lgti_tp(C);
  const int sub = threadIdx.x % LG_GROUP;
  const bool own = 2 * sub < tp;
  const int lo = own ? 2 * sub : 0;
  const bool in0 = own && lo < C, in1 = own && lo + 1 < C;
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
    float d0, d1;
    lgsi_row_logits<NQ, false>(m, st, en, nullptr, wi, tp, 0, sub, r, d0, d1);
    double p0, p1, l;
    int pred, ycls;
    lgsm_row<LG_GROUP, false>(d0, d1, in0, in1, false, false, 1.0, p0, p1, l, pred, ycls);
    if (sub == 0) cls_out[t] = (unsigned char)pred;
    if (p_out) {
      if (in0) p_out[(long long)lo * n + t] = (float)p0;
      if (in1) p_out[(long long)(lo + 1) * n + t] = (float)p1;
    }
  }
}

// grid: K x blocks_per_worker workgroups (lg_blocks_per_worker, the interleaved gradient's), one 16-lane group per listed
// position; a: LgtiArgs with T = C and hot = lgti_hot(tp); NQ = lgsi_quads(tp)
template <int NQ>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_softmax_il_grad_kernel(CsrView m, LgtiArgs a) {
  lgsi_grad_body<NQ>(m, a);
}

// grid: K x blocks_per_worker workgroups, one 16-lane group per row of the worker's range; a: LgtcCoefArgs with T = C
template <int NQ>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_softmax_il_coef_kernel(CsrView m, LgtcCoefArgs a) {
  lgsi_coef_body<NQ>(m, a);
}

// grid: lgsm_eval_blocks(rows, n_cu) workgroups of LGSM_EVAL_THREADS = 512 lanes; dynamic LDS: lgsm_eval_lds_floats(hw, C) floats.
// tally: {correct, wrong}, zero on entry; loss_part: one word per workgroup
template <int NQ>
LGTI_KERNEL void __launch_bounds__(LGSM_EVAL_THREADS) dsgd_lg_softmax_il_eval_kernel(CsrView m, const float* __restrict__ wi,
                                                                                   const signed char* __restrict__ pi, int C, long long row_begin,
                                                                                   long long row_end, unsigned long long* tally, int hw,
                                                                                   double* loss_part) {
  lgsi_eval_body<NQ>(m, wi, pi, C, row_begin, row_end, tally, hw, loss_part);
}

// grid-stride over the listed positions, one 16-lane group each.  cls_out: [n]; p_out: [C][n], class-major, or null
template <int NQ>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_softmax_il_predict_kernel(CsrView m, const float* __restrict__ wi, int C,
                                                                               const int* __restrict__ idx, long long n, unsigned char* cls_out,
                                                                               float* p_out, DevScalars* sc) {
  lgsi_predict_body<NQ>(m, wi, C, idx, n, cls_out, p_out, sc);
}
