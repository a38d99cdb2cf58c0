// Device code of libdsgd_hip, part 15c (gfx950 only): the logistic model over several topics, WIDE -- 1 to 128 topics over the
// interleaved layout, the LANES ACROSS THE TOPICS (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS, WIDE; DESIGN.md 3.13
// "Several topics, wide").  Included behind dsgd_lg_topics_il.hpp, whose kernels stay as they are.
//
// The layout is the interleaved form's (csrc/dsgd_lg_topics_il_host.hpp): Wi[rank][TP], Pi[row][TP], acc[k][rank][TP].
//
// The split.  A row is served by a lane group of GW = 16, 32 or 64 lanes (the smallest with 2 GW >= TP; a wave holds 64 / GW
// rows).  Lane l of the group OWNS topics 2l and 2l + 1: per non-zero ONE 8-byte load of Wi[c] + 2l -- the group's loads are one
// run of TP * 4 contiguous bytes -- per row one 2-byte load of Pi[row] + 2l, per non-zero two adds into adjacent 64-bit words
// of acc[k][c], adjacent lanes on adjacent words.  Lanes with 2l >= TP load topic 0's words and write nothing.  No dot crosses
// a lane: there is no reduction over the group, and what is per topic (coefficient, loss sum) lives in its lane.
//
// The row's column ids and values are the same for every lane of the group.  They are fetched coalesced, sixteen at a time:
// lane j of every 16-lane run of the group loads non-zero st + 16 i + j (the runs of a wider group load the same 64 bytes: one
// request), and the sixteen are handed round inside the run by __shfl(x, j, 16).  The first LG_UNR = 4 chunks -- 64 non-zeros,
// RowRegs' number -- stay in registers between the dot and the scatter; longer rows load their tail chunks twice.
//
// The dot keeps the single model's bits.  row_dot (csrc/dsgd_kernels.hpp) gives lane `sub` of ITS 16-lane group the positions
// st + sub + 16 k in increasing order, each `acc += filt(v * w)` from 0.0f, and group_sum<16> folds the 16 lanes by four
// involutions: quad xor 1 (a0 + a1), quad xor 2 ((a0 + a1) + (a2 + a3)), the mirror within 8 (quad + quad), the mirror within
// 16 (half + half).  Every step adds two values that two lanes hold in either order, and IEEE addition commutes, so every lane
// ends with the balanced tree
//   [((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7))] + [((a8+a9)+(a10+a11)) + ((a12+a13)+(a14+a15))].
// A lane here keeps those 16 accumulators PER OWNED TOPIC in registers (the chunk loop is unrolled: static indices):
// accumulator j takes the products of the positions = j (mod 16) in order, then lgtw_fold is that tree.  A position past the
// row's end has v = 0 and rank 0: it adds filt(0 * w) = +0.0f, which changes no accumulator -- none is ever -0.0f, they start
// at +0.0f and filt gives no -0.0f -- so "adds nothing" holds in bits.  Contraction off, packed fp32 off (LGTI_KERNEL).
//
//   the gradient   dsgd_lg_topics_wide_grad_kernel<GW>: the dot, per topic lg_coef * qscale (0 for a padding topic), per
//                  non-zero lgti_add's expression into the LDS head (the lgtw_hot(TP) hottest ranks with all their topics,
//                  flushed into acc's first words) or acc
//   the finish     dsgd_lg_topics_wide_finish_kernel<STEP>: the interleaved finish's walk with red[128][4]
//   the evaluation dsgd_lg_topics_wide_eval_kernel<GW>: the planar kernel's grid and its 64 chains of rows per workgroup (chain
//                  g = the rows of the planar group g, in its order); a lane group walks its GW / 16 chains one after the
//                  other, the owning lane carries a chain's loss sum per topic in a register.  The chain sums are staged in
//                  LDS [T][64] and read by lane sub == 0 of group g into lg_block_sum: the planar tree.  The tallies are
//                  integer atomics, one per row and topic into the workgroup's 32-bit LDS words [T][3], those into `tally`
//                  (integers: no order; six more registers per lane did not fit the 128 a 1024-lane workgroup leaves)
//   predict        dsgd_lg_topics_wide_predict_kernel<GW>: lg_sigma(d) into p_out[t][position]
//   pack / unpack  dsgd_lg_topics_il_pack_kernel: it serves any TP
//
// What the gfx950 compile reports (hipcc -O3, tools/isa.sh; every kernel: no scratch, no spill): DESIGN.md 3.13 "Several topics,
// wide".
//
// Plain C++, vector loads, vector stores and vector atomics only.
#pragma once
#include "dsgd_lg_topics_wide_host.hpp"

static_assert(LG_GROUP == 16, "the chunk of the walk is the single model's lane group");
static_assert(LGTW_HOT_WORDS * 8 * LGTW_PER_CU <= DSGD_LDS_FLOATS * 4, "the heads of the workgroups a compute unit holds fit its LDS");

// A kernel that turns a target feature off (LGTI_KERNEL) inlines only what is marked always-inline: HIP's 64-bit atomicAdd and
// __syncthreads are not, and would be CALLED -- per non-zero, in the scatter.  The same operations, always inline:
__device__ __forceinline__ void lgtw_atomic_add(unsigned long long* at, unsigned long long v) {
  (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lgtw_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the lane's two weights of rank c (lo = 2l): from the tile lds[hw][TP] (ranks below hw) or from Wi -- two loads and a select
// of VALUES, as lgti_w4
template <bool LDSW>
__device__ __forceinline__ float2 lgtw_w2(const float* wl, const float* __restrict__ wi, int c, int tp, int lo, int hw) {
  if constexpr (!LDSW) {
    return *reinterpret_cast<const float2*>(wi + (long long)c * tp + lo);
  } else {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const f2 lds_cf2;
    const bool hot = c < hw;
    const f2 l = *(lds_cf2*)(wl + (hot ? c : 0) * tp + lo);
    float2 a = make_float2(l.x, l.y);
    if (!hot) a = *reinterpret_cast<const float2*>(wi + (long long)c * tp + lo);
    return a;
  }
}

// sixteen non-zeros (lane j of the run holds number j: rank cc, value vv; past the row's end -1 and 0.0f) into the lane's
// accumulators: a0[j] / a1[j] take number j's product with topic lo's / lo + 1's weight
template <bool LDSW>
__device__ __forceinline__ void lgtw_chunk_dot(int cc, float vv, const float* wl, const float* __restrict__ wi, int tp, int lo, int hw,
                                               float (&a0)[16], float (&a1)[16]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = __shfl(cc, j, 16);
    const float v = __shfl(vv, j, 16);
    const float2 w = lgtw_w2<LDSW>(wl, wi, c < 0 ? 0 : c, tp, lo, hw);   // (unconditional: the sixteen loads are in flight together)
    a0[j] += filt(v * w.x);
    a1[j] += filt(v * w.y);
    // (the evaluation has 128 registers per lane, and a weight pair in flight holds seven of them -- its LDS address and pair,
    //  its 64-bit global address and pair: four pairs in flight, not sixteen)
    if (LDSW && j % 4 == 3) __builtin_amdgcn_sched_barrier(0);
  }
}

// group_sum<16>'s tree over the lane's own sixteen accumulators
__device__ __forceinline__ float lgtw_fold(const float (&a)[16]) {
#pragma clang fp contract(off)
  const float q0 = (a[0] + a[1]) + (a[2] + a[3]), q1 = (a[4] + a[5]) + (a[6] + a[7]);
  const float q2 = (a[8] + a[9]) + (a[10] + a[11]), q3 = (a[12] + a[13]) + (a[14] + a[15]);
  return (q0 + q1) + (q2 + q3);
}

// the row [st, en), its first chunks in r (lgt_row_load with sub = lane % 16): the dots of topics lo and lo + 1
template <bool LDSW>
__device__ __forceinline__ void lgtw_row_dots(const CsrView& m, long long st, long long en, const float* wl, const float* __restrict__ wi, int tp, int lo,
                                              int hw, int sub, const RowRegs<LG_GROUP, LG_UNR>& r, float& d0, float& d1) {
  float a0[16], a1[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a0[j] = 0.0f, a1[j] = 0.0f;
#pragma unroll
  for (int u = 0; u < LG_UNR; ++u)
    if (st + u * LG_GROUP < en) lgtw_chunk_dot<LDSW>(r.c[u], r.v[u], wl, wi, tp, lo, hw, a0, a1);   // (the same for the whole group)
  for (long long p = st + LG_UNR * LG_GROUP; p < en; p += LG_GROUP) {
    const bool in = p + sub < en;
    lgtw_chunk_dot<LDSW>(in ? m.col[p + sub] : -1, in ? m.val[p + sub] : 0.0f, wl, wi, tp, lo, hw, a0, a1);
  }
  d0 = lgtw_fold(a0);
  d1 = lgtw_fold(a1);
}

// the labels of topics lo and lo + 1 of one row: one 2-byte load of Pi
__device__ __forceinline__ void lgtw_labels2(const signed char* __restrict__ pi, long long row, int tp, int lo, double& y0, double& y1) {
  const short word = *reinterpret_cast<const short*>(pi + row * tp + lo);
  y0 = (double)(signed char)word;
  y1 = (double)(signed char)(word >> 8);
}

// lgti_add's expression for sixteen non-zeros and the lane's two words; a padding topic's and an idle lane's cq is 0
__device__ __forceinline__ void lgtw_chunk_add(int cc, float vv, unsigned long long* hot, unsigned long long* acc, int n_hot, int tp, int lo, double cq0,
                                               double cq1) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = __shfl(cc, j, 16);
    const float v = __shfl(vv, j, 16);
    if (c < 0) continue;
    const double xd = (double)v;
    const long long q0 = __double2ll_rn(xd * cq0), q1 = __double2ll_rn(xd * cq1);   // |x cq| <= 2^S <= 2^62
    if (c < n_hot) {
      unsigned long long* at = hot + c * tp + lo;
      if (q0 != 0) lgtw_atomic_add(&at[0], (unsigned long long)q0);
      if (q1 != 0) lgtw_atomic_add(&at[1], (unsigned long long)q1);
    } else {
      unsigned long long* at = acc + (long long)c * tp + lo;
      if (q0 != 0) lgtw_atomic_add(&at[0], (unsigned long long)q0);
      if (q1 != 0) lgtw_atomic_add(&at[1], (unsigned long long)q1);
    }
  }
}

// grid: K x blocks_per_worker workgroups (lgtw_blocks_per_worker), one GW-lane group per listed position; a: LgtiArgs with
// hot = lgtw_hot(tp)
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_wide_grad_kernel(CsrView m, LgtiArgs a) {
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
    float d0, d1;
    lgtw_row_dots<false>(m, st, en, nullptr, a.wi, tp, lo, 0, sub, r, d0, d1);
    double y0, y1;
    lgtw_labels2(a.pi, row, tp, lo, y0, y1);
    const double cq0 = own && lo < a.T ? lg_coef(d0, y0) * qscale : 0.0;
    const double cq1 = own && lo + 1 < a.T ? lg_coef(d1, y1) * qscale : 0.0;
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

// grid: lg_finish_blocks(dp) workgroups -- dsgd_lg_topics_il_finish_kernel's walk (ONE column per lane, its TP topics quad by
// quad, lg_finish_body<LG_STEP>'s arithmetic per (column, topic), lg_block_sum over the same 256 columns) with room for 128
// topics' trees.  A kernel of its own: widening the interleaved kernel's `red` through a shared body moved that kernel's
// instructions, and its assembly stays as it is.
template <bool STEP>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_wide_finish_kernel(LgtiFinishArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[LG_TOPICS_WIDE_MAX][LG_THREADS / 64];
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

// grid: lg_eval_blocks(rows, n_cu) workgroups; dynamic LDS: lgtw_eval_lds_floats(hw, T) floats.  tally: [T][LG_TALLY_WORDS], zero
// on entry; loss_part: [T][part_stride]
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_topics_wide_eval_kernel(CsrView m, const float* __restrict__ wi,
                                                                                  const signed char* __restrict__ pi, int T, long long row_begin,
                                                                                  long long row_end, unsigned long long* tally, int hw, double* loss_part,
                                                                                  long long part_stride) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int CHAINS = GW / LG_GROUP;   // of the workgroup's LGT_EVAL_GROUPS chains, per lane group
  const int tp = lgti_tp(T);
  double* sums = reinterpret_cast<double*>(lds + lgtw_eval_sums_at(hw, T));              // [T][LGT_EVAL_GROUPS]
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + lgtw_eval_cnt_at(hw, T));    // [T][3]
  for (int j = threadIdx.x; j < hw * tp; j += LG_EVAL_THREADS) lds[j] = wi[j];           // (Wi's first hw ranks ARE the tile)
  for (int j = threadIdx.x; j < 3 * T; j += LG_EVAL_THREADS) cnt[j] = 0u;
  lgtw_barrier();
  const int sub = threadIdx.x % LG_GROUP;
  const bool own = 2 * (threadIdx.x % GW) < tp;
  const int lo = own ? 2 * (threadIdx.x % GW) : 0;
  const bool t0_in = own && lo < T, t1_in = own && lo + 1 < T;
  const long long n_groups = (long long)gridDim.x * LGT_EVAL_GROUPS;
  for (int s = 0; s < CHAINS; ++s) {
    const int g = (threadIdx.x / GW) * CHAINS + s;   // the chain: the planar kernel's group g of this workgroup
    double ls0 = 0.0, ls1 = 0.0;
    for (long long row = row_begin + (long long)blockIdx.x * LGT_EVAL_GROUPS + g; row < row_end; row += n_groups) {
      const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
      RowRegs<LG_GROUP, LG_UNR> r;
      lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
      float d0, d1;
      lgtw_row_dots<true>(m, st, en, lds, wi, tp, lo, hw, sub, r, d0, d1);
      double y0, y1;
      lgtw_labels2(pi, row, tp, lo, y0, y1);
      int w0, w1;
      const double l0 = lg_row_loss(y0, d0, w0);
      ls0 = ls0 + l0;
      __builtin_amdgcn_sched_barrier(0);   // (one exp and log1p at a time: the two interleaved do not fit the lane's 128 registers)
      const double l1 = lg_row_loss(y1, d1, w1);
      ls1 = ls1 + l1;
      if (t0_in) atomicAdd(&cnt[lo * 3 + w0], 1u);   // (integers: no order; a register per tally would not fit the 128 a lane has)
      if (t1_in) atomicAdd(&cnt[lo * 3 + 3 + w1], 1u);
    }
    // (the lane's number once more, opaque to the compiler: what the store derives from it is computed here and is not kept
    //  in registers across the walk, where every one of the lane's 128 is taken)
    int tx = threadIdx.x;
    asm volatile("" : "+v"(tx));
    const int l2 = 2 * (tx % GW), g2 = (tx / GW) * CHAINS + s;
    if (l2 < T) sums[l2 * LGT_EVAL_GROUPS + g2] = ls0;
    if (l2 + 1 < T) sums[(l2 + 1) * LGT_EVAL_GROUPS + g2] = ls1;
  }
  int tx = threadIdx.x;
  asm volatile("" : "+v"(tx));
  lgtw_barrier();
  for (int j = tx; j < 3 * T; j += LG_EVAL_THREADS) {
    const unsigned int v = cnt[j];
    if (v) lgtw_atomic_add(&tally[(j / 3) * LG_TALLY_WORDS + j % 3], (unsigned long long)v);
  }
  double* red = reinterpret_cast<double*>(lds + lgtw_eval_red_at(hw, T));
  for (int t = 0; t < T; ++t) {   // the planar tree: chain g's sum on lane sub == 0 of group g, 0.0 on the others
    const double ls = tx % LG_GROUP == 0 ? sums[t * LGT_EVAL_GROUPS + tx / LG_GROUP] : 0.0;
    const double s = lg_block_sum(ls, red, LG_EVAL_THREADS / 64);
    if (tx == 0) loss_part[(long long)t * part_stride + blockIdx.x] = s;
    lgtw_barrier();   // (lane 0 has read the wave sums before the next topic's are written)
  }
}

// grid-stride over the listed positions, one GW-lane group each.  p_out: [T][n], topic-major
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_wide_predict_kernel(CsrView m, const float* __restrict__ wi, int T, const int* __restrict__ idx,
                                                                                long long n, float* p_out, DevScalars* sc) {
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  const int tp = lgti_tp(T);
  const int sub = threadIdx.x % LG_GROUP;
  const bool own = 2 * (threadIdx.x % GW) < tp;
  const int lo = own ? 2 * (threadIdx.x % GW) : 0;
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
    if (own && lo < T) p_out[(long long)lo * n + t] = lg_sigma(d0);
    if (own && lo + 1 < T) p_out[(long long)(lo + 1) * n + t] = lg_sigma(d1);
  }
}
