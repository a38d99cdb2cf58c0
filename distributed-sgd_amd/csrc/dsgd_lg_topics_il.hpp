// Device code of libdsgd_hip, part 15b (gfx950 only): the logistic model over several topics, INTERLEAVED -- 1 to 32 topics whose
// weights, labels and column sums lie side by side per rank, row and column (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS,
// INTERLEAVED).  Included behind dsgd_lg_topics.hpp, whose planar kernels stay as they are.
//
// The layout (TP = T rounded up to a multiple of 4; csrc/dsgd_lg_topics_il_host.hpp):
//   Wi[rank][TP]      floats: the topics' weights of one column in ONE 16-byte load per four topics (TP = 32: one 128-byte line)
//   Pi[row][TP]       bytes: a row's labels in one 4-byte load per four topics
//   acc[k][rank][TP]  64-bit words: a non-zero's adds go to adjacent words
// The contract is the planar form's: topic t's BITS are the single model's.  Every topic's dot is lgt_row_dot's sequence (the lane
// order, filt(v * w), the registers then the tail, group_sum), its coefficient lg_coef * qscale, its adds lg_add's expression, its
// finish lg_finish_body<LG_STEP>'s, its |w'|^2 lg_block_sum over the same 256 columns, its losses lg_row_loss in row order per
// group and the planar evaluation's tree.
//
//   the dots       lgti_row_dots<TB>: TB fp32 accumulators (TB = 4: one quad) over the row held in registers, then the tail
//   the gradient   dsgd_lg_topics_il_grad_kernel<TB>: per row the topics in blocks of TB (the block unrolled, no indexed registers);
//                  the LDS head holds the lgti_hot(TP) hottest ranks with ALL their topics
//   the finish     dsgd_lg_topics_il_finish_kernel<true>: lane = column, quad by quad: one 16-byte load of Wi, per worker two
//                  16-byte loads of the column's words (zeroed where set); <false>: |w_t|^2 of weights the finish did not write
//   the evaluation dsgd_lg_topics_il_eval_kernel: the planar kernel's grid, stride, LDS words and tree; the tile is lds[hw][TP]
//   predict        dsgd_lg_topics_il_predict_kernel: p_out[t][position]
//   pack / unpack  dsgd_lg_topics_il_pack_kernel<IN>: one topic's rank-order vector into / out of Wi
//
// What the gfx950 compile reports (hipcc -O3, tools/isa.sh; every kernel: no scratch, no spill): DESIGN.md 3.13 "Interleaved".
//
// Plain C++ and vector atomics only.
#pragma once
#include "dsgd_lg_topics_il_host.hpp"

static_assert(LGTI_HOT_WORDS == LG_HOT, "the interleaved head is the single model's 16 KiB");
// fp32 products and sums stay single instructions in these kernels: no packed fp32 forms (v_pk_mul_f32 and its kin), whose
// lanes the bit contract would have to trust as well
#define LGTI_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
constexpr int LGTI_TB = 4;   // topics per register block (DESIGN.md 3.13 "Interleaved": the compile report of 4 and 8)

// four topics' weights of rank c: from the tile lds[hw][TP] (ranks below hw) or from Wi -- two loads and a select of VALUES, as w_at
template <bool LDSW>
__device__ __forceinline__ float4 lgti_w4(const float* wl, const float* __restrict__ wi, int c, int tp, int t0, int hw) {
  if constexpr (!LDSW) {
    return *reinterpret_cast<const float4*>(wi + (long long)c * tp + t0);
  } else {
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const f4 lds_cf4;
    const bool hot = c < hw;
    const f4 l = *(lds_cf4*)(wl + (hot ? c : 0) * tp + t0);
    float4 a = make_float4(l.x, l.y, l.z, l.w);
    if (!hot) a = *reinterpret_cast<const float4*>(wi + (long long)c * tp + t0);
    return a;
  }
}

// lgt_row_dot for the TB topics from t0 on the fetched row: accumulator i takes exactly topic t0 + i's sequence
template <int TB, bool LDSW>
__device__ __forceinline__ void lgti_row_dots(const CsrView& m, long long start, long long end, const float* wl, const float* __restrict__ wi, int tp,
                                              int t0, int hw, int sub, const RowRegs<LG_GROUP, LG_UNR>& r, float (&d)[TB]) {
  static_assert(TB == 4 || TB == 8, "whole quads");
#pragma unroll
  for (int i = 0; i < TB; ++i) d[i] = 0.0f;
#pragma unroll
  for (int k = 0; k < LG_UNR; ++k) {
    if (r.c[k] >= 0) {
#pragma unroll
      for (int q = 0; q < TB / 4; ++q) {
        const float4 w = lgti_w4<LDSW>(wl, wi, r.c[k], tp, t0 + 4 * q, hw);
        d[4 * q + 0] += filt(r.v[k] * w.x);
        d[4 * q + 1] += filt(r.v[k] * w.y);
        d[4 * q + 2] += filt(r.v[k] * w.z);
        d[4 * q + 3] += filt(r.v[k] * w.w);
      }
    }
  }
  for (long long p = start + sub + LG_UNR * LG_GROUP; p < end; p += LG_GROUP) {
    const int c = m.col[p];
    const float v = m.val[p];
#pragma unroll
    for (int q = 0; q < TB / 4; ++q) {
      const float4 w = lgti_w4<LDSW>(wl, wi, c, tp, t0 + 4 * q, hw);
      d[4 * q + 0] += filt(v * w.x);
      d[4 * q + 1] += filt(v * w.y);
      d[4 * q + 2] += filt(v * w.z);
      d[4 * q + 3] += filt(v * w.w);
    }
  }
#pragma unroll
  for (int i = 0; i < TB; ++i) d[i] = group_sum<LG_GROUP>(d[i]);
}

// the labels of topics [t0, t0 + 4) of one row: one load of Pi
__device__ __forceinline__ void lgti_labels4(const signed char* __restrict__ pi, long long row, int tp, int t0, double (&y)[4]) {
  const int word = *reinterpret_cast<const int*>(pi + row * tp + t0);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = (double)(signed char)(word >> (8 * i));
}

struct LgtiArgs {
  const float* wi;                 // [dp][tp] the topics' weights, rank order
  const signed char* pi;           // [n_rows][tp] +1 / -1
  int T, tp, hot;                  // hot = lgti_hot(tp): the ranks of the LDS head
  int dp, vexp, K;
  const int* idx;                  // the lists, concatenated
  const WorkSeg* segs;             // [K] each worker's [begin, end) in idx
  long long blocks_per_worker;     // grid = K * blocks_per_worker
  unsigned long long* acc;         // [K][acc_stride] = [K][rank][tp] fixed-point column sums; zero on entry
  long long acc_stride;
  DevScalars* sc;                  // err (1: a row index outside the data)
};

// lg_add for TB adjacent words of rank c; a padding topic's cq is 0: nothing is added
template <int TB>
__device__ __forceinline__ void lgti_add(unsigned long long* hot, unsigned long long* acc, int n_hot, int tp, int t0, int c, float x,
                                         const double (&cq)[TB]) {
#pragma clang fp contract(off)
  const double xd = (double)x;
  if (c < n_hot) {
    unsigned long long* at = hot + c * tp + t0;
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      const long long q = __double2ll_rn(xd * cq[i]);   // |x cq| <= 2^S <= 2^62
      if (q != 0) atomicAdd(&at[i], (unsigned long long)q);
    }
  } else {
    unsigned long long* at = acc + (long long)c * tp + t0;
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      const long long q = __double2ll_rn(xd * cq[i]);
      if (q != 0) atomicAdd(&at[i], (unsigned long long)q);
    }
  }
}

// grid: K x blocks_per_worker workgroups (lg_grad_body<true>'s), one 16-lane group per listed position
template <int TB>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_il_grad_kernel(CsrView m, LgtiArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hot[LGTI_HOT_WORDS];   // [a.hot][a.tp]
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  unsigned long long* acc = a.acc + (long long)k * a.acc_stride;
  const int sub = tid % LG_GROUP;
  const long long groups = a.blocks_per_worker * LG_ROWS_PER_BLOCK;
  const int tp = a.tp, n_hot = a.hot;
  for (int j = tid; j < n_hot * tp; j += LG_THREADS) hot[j] = 0ull;
  __syncthreads();
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = (long long)a.idx[seg.begin + t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int t0 = 0; t0 < tp; t0 += TB) {
      float d[TB];
      lgti_row_dots<TB, false>(m, st, en, nullptr, a.wi, tp, t0, 0, sub, r, d);
      double cq[TB];
#pragma unroll
      for (int q = 0; q < TB / 4; ++q) {
        double y[4];
        lgti_labels4(a.pi, row, tp, t0 + 4 * q, y);
#pragma unroll
        for (int i = 0; i < 4; ++i) cq[4 * q + i] = t0 + 4 * q + i < a.T ? lg_coef(d[4 * q + i], y[i]) * qscale : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LG_UNR; ++u)
        if (r.c[u] >= 0) lgti_add<TB>(hot, acc, n_hot, tp, t0, r.c[u], r.v[u], cq);
      for (long long p = st + sub + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) lgti_add<TB>(hot, acc, n_hot, tp, t0, m.col[p], m.val[p], cq);
    }
  }
  __syncthreads();
  for (int j = tid; j < n_hot * tp; j += LG_THREADS) {   // (the head is acc's first words; a word is non-zero only below dp)
    const unsigned long long v = hot[j];
    if (v) atomicAdd(&acc[j], v);
  }
}

struct LgtiFinishArgs {
  unsigned long long* acc;   // [K][acc_stride], zeroed here
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the lengths give each worker's shift
  int K, dp, vexp, T, tp;
  float* wi;                 // [dp][tp], updated (STEP)
  double lr, lambda;
  double* nsq_part;          // [T][gridDim.x] |w_t'|^2 of each workgroup's columns
};

// grid: lg_finish_blocks(dp) workgroups -- ONE column per lane, its TP topics quad by quad.  STEP: lg_finish_body<LG_STEP>'s
// arithmetic per (column, topic); else |w_t|^2 alone (dsgd_lg_nsq_kernel's).  Topic t's tree has its own LDS words.
template <bool STEP>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_il_finish_kernel(LgtiFinishArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[LG_TOPICS_IL_MAX][LG_THREADS / 64];
  const int j = blockIdx.x * LG_THREADS + threadIdx.x;
  for (int t0 = 0; t0 < a.tp; t0 += 4) {
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < a.dp) {
      float4* wp = reinterpret_cast<float4*>(a.wi + (long long)j * a.tp + t0);
      const float4 w4 = *wp;
      const double wj[4] = {(double)w4.x, (double)w4.y, (double)w4.z, (double)w4.w};
      if constexpr (STEP) {
        double reg[4], sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) reg[i] = (2.0 * a.lambda) * wj[i], sum[i] = 0.0;
        for (int k = 0; k < a.K; ++k) {
          const double back = ldexp(1.0, a.vexp - lg_shift(a.segs[k].end - a.segs[k].begin));   // (lg_finish_G's scale)
          ulonglong2* ap = reinterpret_cast<ulonglong2*>(a.acc + (long long)k * a.acc_stride + (long long)j * a.tp + t0);
          const ulonglong2 lo = ap[0], hi = ap[1];
          if ((lo.x | lo.y) != 0ull) ap[0] = make_ulonglong2(0ull, 0ull);
          if ((hi.x | hi.y) != 0ull) ap[1] = make_ulonglong2(0ull, 0ull);
          const unsigned long long word[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double G = (double)(long long)word[i] * back;
            sum[i] = sum[i] + (G + reg[i]);
          }
        }
        float wn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double mean = sum[i] / (double)a.K;
          wn[i] = (float)(wj[i] - a.lr * mean);
          sq[i] = (double)wn[i] * (double)wn[i];
        }
        *wp = make_float4(wn[0], wn[1], wn[2], wn[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) sq[i] = wj[i] * wj[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (t0 + i < a.T) {   // (uniform: the barrier inside is reached by all lanes or none)
        const double s = lg_block_sum(sq[i], red[t0 + i], LG_THREADS / 64);
        if (threadIdx.x == 0) a.nsq_part[(long long)(t0 + i) * gridDim.x + blockIdx.x] = s;
      }
    }
  }
}

// grid: lg_eval_blocks(rows, n_cu) workgroups; dynamic LDS: lgti_eval_lds_floats(hw, T) floats.  tally: [T][LG_TALLY_WORDS], zero
// on entry; loss_part: [T][part_stride].  dsgd_lg_topics_eval_kernel with the tile lds[hw][TP] and the dots in blocks
LGTI_KERNEL void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_topics_il_eval_kernel(CsrView m, const float* __restrict__ wi, const signed char* __restrict__ pi,
                                                                                int T, long long row_begin, long long row_end, unsigned long long* tally,
                                                                                int hw, double* loss_part, long long part_stride) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tp = lgti_tp(T);
  double* sums = reinterpret_cast<double*>(lds + lgti_eval_sums_at(hw, T));               // [T][LGT_EVAL_GROUPS]
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + lgti_eval_cnt_at(hw, T));     // [T][3][LGT_EVAL_GROUPS]
  for (int j = threadIdx.x; j < hw * tp; j += LG_EVAL_THREADS) lds[j] = wi[j];            // (Wi's first hw ranks ARE the tile)
  for (int j = threadIdx.x; j < T * LGT_EVAL_GROUPS; j += LG_EVAL_THREADS) sums[j] = 0.0;
  for (int j = threadIdx.x; j < 3 * T * LGT_EVAL_GROUPS; j += LG_EVAL_THREADS) cnt[j] = 0u;
  __syncthreads();
  const int sub = threadIdx.x % LG_GROUP;
  const int g = threadIdx.x / LG_GROUP;
  const long long group = ((long long)blockIdx.x * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = (long long)gridDim.x * LG_EVAL_THREADS / LG_GROUP;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int t0 = 0; t0 < tp; t0 += 4) {
      float d[4];
      lgti_row_dots<4, true>(m, st, en, lds, wi, tp, t0, hw, sub, r, d);
      if (sub == 0) {   // (this group's own words: nobody else touches them)
        double y[4];
        lgti_labels4(pi, row, tp, t0, y);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = t0 + i;
          if (t < T) {
            int which;
            const double l = lg_row_loss(y[i], d[i], which);
            cnt[(t * 3 + which) * LGT_EVAL_GROUPS + g] += 1u;
            sums[t * LGT_EVAL_GROUPS + g] = sums[t * LGT_EVAL_GROUPS + g] + l;
          }
        }
      }
    }
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const bool own = sub == 0;
    const unsigned int c0 = own ? cnt[(t * 3 + 0) * LGT_EVAL_GROUPS + g] : 0u;
    const unsigned int c1 = own ? cnt[(t * 3 + 1) * LGT_EVAL_GROUPS + g] : 0u;
    const unsigned int c2 = own ? cnt[(t * 3 + 2) * LGT_EVAL_GROUPS + g] : 0u;
    const double ls = own ? sums[t * LGT_EVAL_GROUPS + g] : 0.0;
    lg_block_tally3(c0, c1, c2, tally + t * LG_TALLY_WORDS, reinterpret_cast<unsigned int*>(lds + tp * hw));
    const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lgti_eval_red_at(hw, T)), LG_EVAL_THREADS / 64);
    if (threadIdx.x == 0) loss_part[(long long)t * part_stride + blockIdx.x] = s;
  }
}

// lg_predict_body<true> with the dots in blocks.  p_out: [T][n], topic-major
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_il_predict_kernel(CsrView m, const float* __restrict__ wi, int T, const int* __restrict__ idx,
                                                                              long long n, float* p_out, DevScalars* sc) {
  const int tp = lgti_tp(T);
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
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int t0 = 0; t0 < tp; t0 += 4) {
      float d[4];
      lgti_row_dots<4, false>(m, st, en, nullptr, wi, tp, t0, 0, sub, r, d);
      if (sub == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (t0 + i < T) p_out[(long long)(t0 + i) * n + t] = lg_sigma(d[i]);
      }
    }
  }
}

// topic t's rank-order vector v[dp] into Wi (IN) or out of it; grid-stride over the columns
template <bool IN>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_il_pack_kernel(float* v, float* wi, int dp, int tp, int t) {
  for (int j = blockIdx.x * LG_THREADS + threadIdx.x; j < dp; j += gridDim.x * LG_THREADS) {
    if constexpr (IN) wi[(long long)j * tp + t] = v[j];
    else v[j] = wi[(long long)j * tp + t];
  }
}
