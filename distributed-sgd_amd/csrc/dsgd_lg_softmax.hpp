// Device code of libdsgd_hip, part 15e (gfx950 only): SOFTMAX (multinomial logistic) regression over 2 to 128 mutually exclusive
// classes on the WIDE topic layout (include/dsgd.h "THE LOGISTIC MODEL": SOFTMAX; DESIGN.md 3.13 "Softmax over the wide layout").
// Included behind dsgd_lg_topics_wide.hpp and dsgd_lg_topics_cols.hpp, whose kernels stay as they are.
//
// The layout is the wide form's: Wi[rank][TP], Pi[row][TP] (+1 at the row's class, -1 at the other classes, +1 at the padding
// classes C <= c < TP), acc[k][rank][TP].  A row is served by a lane group of GW = 16, 32 or 64 lanes, lane l owns classes 2l and
// 2l + 1, and lgtw_row_dots leaves the group with all C logits of the row, two per lane, each the single model's bits.
//
// What is new is ONE reduction across the group between the dot and the scatter (the one-vs-rest forms have none), written
// once, in lgsm_row:
//   m    = max_c z_c over the REAL classes: the lane's own pair (-inf for a class it does not own), then an xor butterfly of
//          fmaxf over offsets 1 .. GW / 2.  The maximum of finite floats does not depend on the order.
//   e_c  = exp((double)z_c - (double)m), fp64, contraction off; exp(-inf) = 0.0 for a class the lane does not own
//   S    = sum_c e_c: the lane's own two terms, then an xor butterfly of fp64 adds over offsets 1 .. GW / 2.  Every step adds two
//          values that two lanes hold in either order, and IEEE addition commutes: every lane ends with the same bits.
//   p_c  = e_c / S; the gradient's coefficient (p_c - [c == y]) 2^(S_k - vexp) lies in [-2^S_k-vexp, 2^S_k-vexp] as lg_coef's
//   the row's class y, the predicted class (the LOWEST c with z_c == m) and the lane that holds z_y are found by wave votes
//   (a ballot's bits of the group, count-trailing-zeros: integers, no order); z_y comes from its lane by ONE __shfl, and
//   l = log(S) - ((double)z_y - (double)m) is then the same bits in every lane of the group.
// The butterflies and votes run over lanes of ONE group, and a group takes every branch of the row walk as a whole.
//
//   the gradient    dsgd_lg_softmax_grad_kernel<GW> (index lists): the wide gradient's grid, row walk, 32 KiB LDS head and
//                   scatter (lgtw_chunk_add) with the softmax coefficient in lg_coef's place
//   coefficients    dsgd_lg_softmax_coef_kernel<GW> (row ranges): the topics' coefficient kernel's walk; one 16-byte store per
//                   lane into cq[position][TP], exactly 0.0 for a padding class.  The step then runs the EXISTING
//                   dsgd_lg_topics_cgrad_kernel<GW> and the wide finish
//   the evaluation  dsgd_lg_softmax_eval_kernel<GW>: the wide evaluation's chains and LDS weight tile in workgroups of 512 lanes
//                   (32 chains; 256 registers per lane, so no scratch); ONE loss sum per chain (every lane of the group
//                   carries the same bits, lane 0 of the group stores them), the 32 chain sums
//                   folded by lg_block_sum; correct / wrong are integer atomics (LDS, then `tally`).  No floating-point atomic:
//                   the loss is a function of the weights and the range alone
//   predict         dsgd_lg_softmax_predict_kernel<GW>: per listed position the class byte and, where asked, (float)p_c into
//                   p_out[c][position]
// The finish, |w_c|^2 and the weights' way across the boundary are the wide form's, unchanged.
//
// What the gfx950 compile reports (every instantiation: no scratch, no spill): DESIGN.md 3.13 "Softmax over the wide layout".
//
// Plain C++, vector loads, vector stores and vector atomics only.
#pragma once
#include "dsgd_lg_softmax_host.hpp"

// the bits of the lane's own group in a wave-wide vote, lane 0 of the group at bit 0
template <int GW>
__device__ __forceinline__ unsigned long long lgsm_group_vote(bool v) {
  const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
  if constexpr (GW == 64) {
    return b;
  } else {
    const int base = (int)(threadIdx.x & 63u) & ~(GW - 1);
    return (b >> base) & ((1ull << GW) - 1ull);
  }
}
// the lowest class among the group's votes (v0: the lane's class 2l, v1: its class 2l + 1); LGSM_NONE where nobody votes
template <int GW>
__device__ __forceinline__ int lgsm_lowest(bool v0, bool v1) {
  const unsigned long long b0 = lgsm_group_vote<GW>(v0), b1 = lgsm_group_vote<GW>(v1);
  const int c0 = b0 ? 2 * __builtin_ctzll(b0) : LGSM_NONE;
  const int c1 = b1 ? 2 * __builtin_ctzll(b1) + 1 : LGSM_NONE;
  return c0 < c1 ? c0 : c1;
}

// THE softmax arithmetic of one row, by every lane of its group.  d0, d1: the lane's two logits; in0, in1: the lane owns a REAL
// class there (a padding class and an idle lane: false -- no part in m, S or the votes); y0, y1: that class is the row's (false
// wherever in is).  GRAD: o0, o1 = (p - [c == y]) * qscale, exactly 0.0 where in is false; nothing else is written.  Otherwise
// o0, o1 = p (0.0 where in is false), loss = log(S) - (z_y - m), pred and ycls the predicted and the row's class.
template <int GW, bool GRAD>
__device__ __forceinline__ void lgsm_row(float d0, float d1, bool in0, bool in1, bool y0, bool y1, double qscale, double& o0, double& o1,
                                         double& loss, int& pred, int& ycls) {
#pragma clang fp contract(off)
  const float ninf = -__builtin_inff();
  float m = __builtin_fmaxf(in0 ? d0 : ninf, in1 ? d1 : ninf);
#pragma unroll
  for (int off = 1; off < GW; off <<= 1) m = __builtin_fmaxf(m, __shfl_xor(m, off, GW));
  const double md = (double)m;
  // (exp(-inf) = +0.0 exactly: every lane runs the same straight-line exp -- behind a branch the compiler kept exp's constants in
  //  vector registers across the row walk; one exp at a time, as the wide evaluation)
  const double ninfd = -__builtin_inf();
  const double e0 = exp(in0 ? (double)d0 - md : ninfd);
  __builtin_amdgcn_sched_barrier(0);
  const double e1 = exp(in1 ? (double)d1 - md : ninfd);
  __builtin_amdgcn_sched_barrier(0);
  double S = e0 + e1;
#pragma unroll
  for (int off = 1; off < GW; off <<= 1) S = S + __shfl_xor(S, off, GW);
  const double p0 = e0 / S, p1 = e1 / S;   // (S >= 1: the class of the maximum adds exp(0))
  if constexpr (GRAD) {
    o0 = (p0 - (y0 ? 1.0 : 0.0)) * qscale;   // (a power of two: exact)
    o1 = (p1 - (y1 ? 1.0 : 0.0)) * qscale;
  } else {
    const double lS = log(S);
    ycls = lgsm_lowest<GW>(y0, y1);
    pred = lgsm_lowest<GW>(in0 && d0 == m, in1 && d1 == m);
    const float zy = __shfl((ycls & 1) ? d1 : d0, (ycls >> 1) & (GW - 1), GW);
    loss = lS - ((double)zy - md);
    o0 = p0;
    o1 = p1;
  }
}

// the lane's part of a row's step: the dots, the labels, the coefficient pair
template <int GW>
__device__ __forceinline__ void lgsm_row_coef(const CsrView& m, long long row, long long st, long long en, const float* __restrict__ wi,
                                              const signed char* __restrict__ pi, int C, int tp, bool own, int lo, int sub,
                                              const RowRegs<LG_GROUP, LG_UNR>& r, double qscale, double& cq0, double& cq1) {
  float d0, d1;
  lgtw_row_dots<false>(m, st, en, nullptr, wi, tp, lo, 0, sub, r, d0, d1);
  double y0, y1;
  lgtw_labels2(pi, row, tp, lo, y0, y1);
  const bool in0 = own && lo < C, in1 = own && lo + 1 < C;
  double loss;
  int pred, ycls;
  lgsm_row<GW, true>(d0, d1, in0, in1, in0 && y0 > 0.0, in1 && y1 > 0.0, qscale, cq0, cq1, loss, pred, ycls);
}

// grid: K x blocks_per_worker workgroups (lgtw_blocks_per_worker), one GW-lane group per listed position; a: LgtiArgs with
// T = C and hot = lgtw_hot(tp)
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_softmax_grad_kernel(CsrView m, LgtiArgs a) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  __shared__ unsigned long long hot[LGTW_HOT_WORDS];   // [a.hot][a.tp]
  constexpr int ROWS = LG_THREADS / GW;
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  unsigned long long* acc = a.acc + (long long)k * a.acc_stride;
  const int sub = tid % LG_GROUP;
  const int tp = a.tp, n_hot = a.hot;
  const bool own = 2 * (tid % GW) < tp;
  const int lo = own ? 2 * (tid % GW) : 0;
  const long long groups = a.blocks_per_worker * ROWS;
  for (int j = tid; j < n_hot * tp; j += LG_THREADS) hot[j] = 0ull;
  lgtw_barrier();
  for (long long t = b * ROWS + tid / GW; t < n; t += groups) {
    const long long row = (long long)a.idx[seg.begin + t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists: never taken)
      if (tid % GW == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    double cq0, cq1;
    lgsm_row_coef<GW>(m, row, st, en, a.wi, a.pi, a.T, tp, own, lo, sub, r, qscale, cq0, cq1);
#pragma unroll
    for (int u = 0; u < LG_UNR; ++u)
      if (st + u * LG_GROUP < en) lgtw_chunk_add(r.c[u], r.v[u], hot, acc, n_hot, tp, lo, cq0, cq1);
    for (long long p = st + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) {
      const bool in = p + sub < en;
      lgtw_chunk_add(in ? m.col[p + sub] : -1, in ? m.val[p + sub] : 0.0f, hot, acc, n_hot, tp, lo, cq0, cq1);
    }
  }
  lgtw_barrier();
  for (int j = tid; j < n_hot * tp; j += LG_THREADS) {   // (the head is acc's first words; a word is non-zero only below dp)
    const unsigned long long v = hot[j];
    if (v) lgtw_atomic_add(&acc[j], v);
  }
}

// grid: K x blocks_per_worker workgroups, one GW-lane group per row of the worker's range; a: LgtcCoefArgs with T = C
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_softmax_coef_kernel(CsrView m, LgtcCoefArgs a) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  constexpr int ROWS = LG_THREADS / GW;
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);
  const int sub = tid % LG_GROUP;
  const int tp = a.tp;
  const bool own = 2 * (tid % GW) < tp;
  const int lo = own ? 2 * (tid % GW) : 0;
  double* cq = a.cq + (long long)a.pos_base[k] * tp + lo;
  const long long groups = a.blocks_per_worker * ROWS;
  for (long long t = b * ROWS + tid / GW; t < n; t += groups) {
    const long long row = seg.begin + t;
    if (row < 0 || row >= m.n_rows) {   // (the host checked the ranges: never taken)
      if (tid % GW == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    double cq0, cq1;
    lgsm_row_coef<GW>(m, row, st, en, a.wi, a.pi, a.T, tp, own, lo, sub, r, qscale, cq0, cq1);
    if (own) *reinterpret_cast<double2*>(cq + t * tp) = make_double2(cq0, cq1);   // (an empty row's as any other's: p = 1 / C)
  }
}

// grid: lgsm_eval_blocks(rows, n_cu) workgroups of LGSM_EVAL_THREADS = 512 lanes (the wide evaluation's 1,024 leave a lane 128
// registers: the dots' 32 accumulators and the constants of exp and log do not fit them without scratch; 512 leave 256);
// dynamic LDS: lgsm_eval_lds_floats(hw, C) floats.  tally: {correct, wrong}, zero on entry; loss_part: one word per workgroup
template <int GW>
LGTI_KERNEL void __launch_bounds__(LGSM_EVAL_THREADS) dsgd_lg_softmax_eval_kernel(CsrView m, const float* __restrict__ wi,
                                                                                const signed char* __restrict__ pi, int C, long long row_begin,
                                                                                long long row_end, unsigned long long* tally, int hw, double* loss_part) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int CHAINS = GW / LG_GROUP;   // of the workgroup's LGSM_EVAL_CHAINS chains, per lane group
  const int tp = lgti_tp(C), tid = threadIdx.x;
  double* sums = reinterpret_cast<double*>(lds + lgsm_eval_sums_at(hw, C));             // [LGSM_EVAL_CHAINS]
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + lgsm_eval_cnt_at(hw, C));   // {correct, wrong}
  for (int j = tid; j < hw * tp; j += LGSM_EVAL_THREADS) lds[j] = wi[j];                // (Wi's first hw ranks ARE the tile)
  if (tid < 2) cnt[tid] = 0u;
  lgtw_barrier();
  const int sub = tid % LG_GROUP;
  const bool own = 2 * (tid % GW) < tp;
  const int lo = own ? 2 * (tid % GW) : 0;
  const bool in0 = own && lo < C, in1 = own && lo + 1 < C;
  const long long n_chains = (long long)gridDim.x * LGSM_EVAL_CHAINS;
  for (int s = 0; s < CHAINS; ++s) {
    const int g = (tid / GW) * CHAINS + s;   // the chain: rows row_begin + (block, g) + i * n_chains, in order
    double ls = 0.0;
    for (long long row = row_begin + (long long)blockIdx.x * LGSM_EVAL_CHAINS + g; row < row_end; row += n_chains) {
      const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
      RowRegs<LG_GROUP, LG_UNR> r;
      lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
      float d0, d1;
      lgtw_row_dots<true>(m, st, en, lds, wi, tp, lo, hw, sub, r, d0, d1);
      double y0, y1;
      lgtw_labels2(pi, row, tp, lo, y0, y1);
      double p0, p1, l;
      int pred, ycls;
      lgsm_row<GW, false>(d0, d1, in0, in1, in0 && y0 > 0.0, in1 && y1 > 0.0, 1.0, p0, p1, l, pred, ycls);
      ls = ls + l;
      if (tid % GW == 0) (void)__hip_atomic_fetch_add(&cnt[pred == ycls ? 0 : 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (tid % GW == 0) sums[g] = ls;   // (the same bits in every lane of the group)
  }
  lgtw_barrier();
  if (tid < 2) {
    const unsigned int v = cnt[tid];
    if (v) lgtw_atomic_add(&tally[tid], (unsigned long long)v);
  }
  // one fixed tree: chain g's sum on lane sub == 0 of the 16-lane run g, 0.0 on the others
  const double ls = sub == 0 ? sums[tid / LG_GROUP] : 0.0;
  const double total = lg_block_sum(ls, reinterpret_cast<double*>(lds + lgsm_eval_red_at(hw, C)), LGSM_EVAL_THREADS / 64);
  if (tid == 0) loss_part[blockIdx.x] = total;
}

// grid-stride over the listed positions, one GW-lane group each.  cls_out: [n]; p_out: [C][n], class-major, or null
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_softmax_predict_kernel(CsrView m, const float* __restrict__ wi, int C, const int* __restrict__ idx,
                                                                            long long n, unsigned char* cls_out, float* p_out, DevScalars* sc) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  const int tp = lgti_tp(C);
  const int sub = threadIdx.x % LG_GROUP;
  const bool own = 2 * (threadIdx.x % GW) < tp;
  const int lo = own ? 2 * (threadIdx.x % GW) : 0;
  const bool in0 = own && lo < C, in1 = own && lo + 1 < C;
  const long long group = ((long long)blockIdx.x * LG_THREADS + threadIdx.x) / GW;
  const long long n_groups = (long long)gridDim.x * (LG_THREADS / GW);
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the list: never taken)
      if (threadIdx.x % GW == 0) atomicOr(&sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    float d0, d1;
    lgtw_row_dots<false>(m, st, en, nullptr, wi, tp, lo, 0, sub, r, d0, d1);
    double p0, p1, l;
    int pred, ycls;
    lgsm_row<GW, false>(d0, d1, in0, in1, false, false, 1.0, p0, p1, l, pred, ycls);
    if (threadIdx.x % GW == 0) cls_out[t] = (unsigned char)pred;
    if (p_out) {
      if (in0) p_out[(long long)lo * n + t] = (float)p0;
      if (in1) p_out[(long long)(lo + 1) * n + t] = (float)p1;
    }
  }
}
