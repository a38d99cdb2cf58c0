// Device code of libdsgd_hip, part 15g (gfx950 only): the topics' and softmax's steps over INDEX LISTS by COLUMN LISTS
// (include/dsgd.h dsgd_lg_topics_sync_steps_cols, dsgd_lg_softmax_sync_steps_cols; DESIGN.md 3.13 "Index lists by column
// lists").  Included behind dsgd_lg_topics_cols.hpp, dsgd_lg_softmax.hpp and dsgd_lg_softmax_il.hpp, whose kernels stay as
// they are; it serves the interleaved and the wide topics, the wide softmax and the softmax over few classes.
//
// The list gradients scatter one 64-bit atomic per non-zero and topic.  The whole-split steps avoid that by walking entries
// sorted by column, but their layout is made per ranges configuration because a range repeats its rows.  A list does not, so
// here the layout is the one of the WHOLE matrix -- one LgColsLayout over the single range [0, n_rows), made once per loaded
// matrix by the single model's builder (lgc_layout), where an entry's position IS its row -- and a step says which rows take
// part through an OWNER WORD per row (csrc/dsgd_lg_lists_cols_host.hpp: the worker and the row's position in the step's
// concatenated lists, or LGL_NONE).  A step is FIVE launches whatever T, C or K:
//
//   dsgd_lgl_mark_kernel          owner[idx[i]] = {worker, i - base} for every listed row: one lane per row, plain 4-byte stores.
//                                 The host sends a step here only if it names no row twice: no two lanes write one word.
//   dsgd_lgl_*_coef_kernel        the coefficient kernels of the ranges, over a list: the row is idx[seg.begin + t] and its pair
//                                 goes to cq[seg.begin + t - base][TP] + 2l.  The per-row bodies are the ranges' and the lists'
//                                 own (lgtw_row_dots + lg_coef, lgsm_row_coef, lgsi_row_coef) with the same weights and the same
//                                 shift lg_shift(list length): the same bits.  (A walk of its own, not a switch in
//                                 lgtc_coef_body and its kin: those take LgtcCoefArgs, which has no list, and a member more
//                                 moves the arguments of every existing coefficient kernel.)
//   dsgd_lgl_cgrad_kernel<GW>     grid (shares, K): a workgroup walks ONE share of the matrix's entries for worker blockIdx.y,
//                                 as lgtc_grad_body does -- 256 / GW lane groups on contiguous runs, sixteen entries fetched
//                                 coalesced and handed round by __shfl, the runs' flags counted first.  The lane that fetched an
//                                 entry also gathers its row's owner word (4 bytes from a table of n_rows words, which stays in
//                                 cache) and hands it round with the entry.  An entry whose row another worker or nobody owns
//                                 costs no coefficient load and adds nothing; an owned entry loads cq[position][2l .. 2l + 1]
//                                 and adds rn((double)x * cq) -- lgti_add's expression -- to the lane's TWO 64-bit register sums.
//                                 At a flag the sums go to acc[k][rank][2l .. 2l + 1] by lgtc_flush: a plain 16-byte store for a
//                                 column inside the run, 64-bit integer atomics for a column cut by the run, zero sums skipped.
//                                 (One pass with 2 K sums chosen by the owner's worker was not built: K is not known at compile
//                                 time, so the sums would be indexed registers, which go to scratch.)
//   the finish                    the form's own, unchanged, with the lists' ranges as `segs`.
//   dsgd_lgl_clear_kernel         owner[idx[i]] = LGL_NONE for the listed rows: the table is all LGL_NONE between steps.
//
// The sums are integers: the accumulators hold the bits the list forms leave, whatever the order and the store / atomic split.
// Contraction off, packed fp32 off (LGTI_KERNEL); no LDS beyond the 16 flag words, no floating-point atomic.
// What the gfx950 compile reports (every instantiation: no scratch, no spill): DESIGN.md 3.13.
//
// Plain C++, vector loads, vector stores and vector atomics only.
#pragma once
#include "dsgd_lg_lists_cols_host.hpp"

struct LglMarkArgs {
  const int* idx;                  // the call's index array
  const WorkSeg* segs;             // [K] the step's lists: [begin, end) in idx, one behind the other
  long long base;                  // segs[0].begin: position = place in idx - base
  long long n_rows;
  long long blocks_per_worker;     // grid = (blocks_per_worker, K)
  unsigned int* owner;             // [n_rows]
  DevScalars* sc;                  // err (1: a row outside the data)
};

// grid: (blocks_per_worker, K) workgroups of LGL_THREADS lanes, one lane per listed row
template <bool MARK>
__device__ __forceinline__ void lgl_mark_body(const LglMarkArgs& a) {
  const int k = (int)blockIdx.y;
  const WorkSeg seg = a.segs[k];
  const long long step = a.blocks_per_worker * LGL_THREADS;
  for (long long i = seg.begin + (long long)blockIdx.x * LGL_THREADS + threadIdx.x; i < seg.end; i += step) {
    const long long row = (long long)a.idx[i];
    if (row < 0 || row >= a.n_rows) {   // (the host checked the lists: never taken)
      atomicOr(&a.sc->err, 1);
      continue;
    }
    a.owner[row] = MARK ? lgl_pack(k, i - a.base) : LGL_NONE;
  }
}
__global__ void __launch_bounds__(LGL_THREADS) dsgd_lgl_mark_kernel(LglMarkArgs a) { lgl_mark_body<true>(a); }
__global__ void __launch_bounds__(LGL_THREADS) dsgd_lgl_clear_kernel(LglMarkArgs a) { lgl_mark_body<false>(a); }

struct LglCoefArgs {
  const float* wi;                 // [dp][tp] the weights, rank order
  const signed char* pi;           // [n_rows][tp] +1 / -1
  int T, tp, vexp, K;
  const int* idx;                  // the call's index array
  const WorkSeg* segs;             // [K] the step's lists in idx
  long long base;                  // segs[0].begin
  long long blocks_per_worker;     // grid = K * blocks_per_worker (lgtw_blocks_per_worker)
  double* cq;                      // [the step's rows][tp] c_i 2^(S_k - vexp) per topic or class
  DevScalars* sc;                  // err (1: a row outside the data)
};

enum LglModel { LGL_TOPICS = 0, LGL_SOFTMAX = 1, LGL_SOFTMAX_IL = 2 };

// MODEL LGL_TOPICS and LGL_SOFTMAX: P = GW, the lanes per row; LGL_SOFTMAX_IL: P = NQ, the quads of classes, sixteen lanes per row
template <int MODEL, int P>
__device__ __forceinline__ void lgl_coef_body(const CsrView& m, const LglCoefArgs& a) {
#pragma clang fp contract(off)
  constexpr int GW = MODEL == LGL_SOFTMAX_IL ? LG_GROUP : P;
  constexpr int ROWS = LG_THREADS / GW;
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  const int sub = tid % LG_GROUP;
  const int tp = a.tp;
  const bool own = 2 * (tid % GW) < tp;
  const int lo = own ? 2 * (tid % GW) : 0;
  const int* list = a.idx + seg.begin;
  double* cq = a.cq + (seg.begin - a.base) * tp + lo;
  const long long groups = a.blocks_per_worker * ROWS;
  for (long long t = b * ROWS + tid / GW; t < n; t += groups) {
    const long long row = (long long)list[t];
    if (row < 0 || row >= m.n_rows) {   // (the host checked the lists: never taken)
      if (tid % GW == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    double cq0, cq1;
    if constexpr (MODEL == LGL_TOPICS) {   // lgtc_coef_body's lines
      float d0, d1;
      lgtw_row_dots<false>(m, st, en, nullptr, a.wi, tp, lo, 0, sub, r, d0, d1);
      double y0, y1;
      lgtw_labels2(a.pi, row, tp, lo, y0, y1);
      cq0 = lo < a.T ? lg_coef(d0, y0) * qscale : 0.0;
      cq1 = lo + 1 < a.T ? lg_coef(d1, y1) * qscale : 0.0;
    } else if constexpr (MODEL == LGL_SOFTMAX) {
      lgsm_row_coef<P>(m, row, st, en, a.wi, a.pi, a.T, tp, own, lo, sub, r, qscale, cq0, cq1);
    } else {
      lgsi_row_coef<P>(m, row, st, en, a.wi, a.pi, a.T, tp, own, lo, sub, r, qscale, cq0, cq1);
    }
    if (own) *reinterpret_cast<double2*>(cq + t * tp) = make_double2(cq0, cq1);   // (an empty row's as any other's)
  }
}

// grid: K x blocks_per_worker workgroups, one GW-lane group per listed row
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lgl_topics_coef_kernel(CsrView m, LglCoefArgs a) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  lgl_coef_body<LGL_TOPICS, GW>(m, a);
}
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lgl_smax_coef_kernel(CsrView m, LglCoefArgs a) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  lgl_coef_body<LGL_SOFTMAX, GW>(m, a);
}
template <int NQ>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lgl_smax_few_coef_kernel(CsrView m, LglCoefArgs a) {
#pragma clang fp contract(off)
  static_assert(NQ == 1 || NQ == 2 || NQ == 4 || NQ == 8, "quads of classes");
  lgl_coef_body<LGL_SOFTMAX_IL, NQ>(m, a);
}

struct LglGradArgs {
  LgtcGradArgs g;                  // the matrix's layout (one range: its slots are ranks), cq[the step's rows][tp], acc[K][rank][tp]
  const unsigned int* owner;       // [n_rows] lgl_pack(worker, position) or LGL_NONE
};

// group_flags: lgtc_groups(GW) LDS words
template <int GW>
__device__ __forceinline__ void lgl_grad_body(const LglGradArgs& q, int* group_flags) {
#pragma clang fp contract(off)
  LgtcGradArgs a = q.g;
  const unsigned int k = blockIdx.y;
  a.acc += (long long)k * a.acc_stride;                     // (the layout has one worker: its slots name worker 0's words)
  const int tid = threadIdx.x, sub = tid % LG_GROUP, g = tid / GW;
  const int tp = a.tp;
  const bool own = 2 * (tid % GW) < tp;
  const int lo = own ? 2 * (tid % GW) : 0;
  const int run = lgtc_group_entries(a.share, GW);
  const long long e0 = (long long)blockIdx.x * a.share;
  const long long r0 = e0 + (long long)g * run, r1 = r0 + run;   // (the array is padded to whole shares: in bounds)
  const TcShare sh = a.shares[blockIdx.x];
  // the flags of the run, counted by its lanes and summed over the group
  int nf = 0;
  for (int i = tid % GW; i < run; i += GW) nf += (a.ent[r0 + i].y & LGC_FIRST) ? 1 : 0;
#pragma unroll
  for (int off = GW / 2; off >= 1; off >>= 1) nf += __shfl_xor(nf, off, GW);
  if (tid % GW == 0) group_flags[g] = nf;
  lgtw_barrier();
  // relative column = flags up to and including the entry, less one where the share's first entry is flagged
  int col = (a.ent[e0].y & LGC_FIRST) ? -1 : 0;
  for (int i = 0; i < g; ++i) col += group_flags[i];
  bool inside = false;                                      // the current column's first entry lies in this run
  long long s0 = 0, s1 = 0;
  const double* cq = a.cq + lo;
  for (long long p = r0; p < r1; p += LG_GROUP) {
    const uint2 e = a.ent[p + sub];
    // the entry's position is its row.  One gather per entry, by the lane that fetched it; the layout's padding at and beyond n_ent
    // (zero words, which would read as row 0) is nobody's: no load and no add, whatever row 0's coefficients hold
    const unsigned int ow = p + sub < a.n_ent ? q.owner[e.y & ~LGC_FIRST] : LGL_NONE;
    double2 c[LG_GROUP];
#pragma unroll
    for (int j = 0; j < LG_GROUP; ++j) {                    // (the owned entries' loads are in flight together)
      const unsigned int o = (unsigned int)__shfl((int)ow, j, LG_GROUP);
      c[j] = make_double2(0.0, 0.0);
      if ((unsigned int)lgl_worker(o) == k) c[j] = *reinterpret_cast<const double2*>(cq + lgl_pos(o) * tp);   // (the same for the whole group)
    }
#pragma unroll
    for (int j = 0; j < LG_GROUP; ++j) {
      const unsigned int y = (unsigned int)__shfl((int)e.y, j, LG_GROUP);
      const unsigned int o = (unsigned int)__shfl((int)ow, j, LG_GROUP);
      const double xd = (double)__uint_as_float((unsigned int)__shfl((int)e.x, j, LG_GROUP));
      if (y & LGC_FIRST) {                                  // (the same for the whole group)
        if (own) lgtc_flush(a, sh, col, inside, lo, s0, s1);
        ++col;
        inside = true;
        s0 = 0, s1 = 0;
      }
      if ((unsigned int)lgl_worker(o) == k) {               // an entry of another worker's row, or of nobody's, adds nothing
        s0 += __double2ll_rn(xd * c[j].x);                  // lgti_add's expression; |x cq| <= 2^S <= 2^62
        s1 += __double2ll_rn(xd * c[j].y);
      }
    }
  }
  const bool goes_on = r1 < a.n_ent && !(a.ent[r1].y & LGC_FIRST);   // the last column has entries in the next run
  if (own) lgtc_flush(a, sh, col, inside && !goes_on, lo, s0, s1);
}

// grid: (one workgroup per share of the matrix's entries, K workers)
template <int GW>
LGTI_KERNEL void __launch_bounds__(LGC_THREADS) dsgd_lgl_cgrad_kernel(LglGradArgs q) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  __shared__ int group_flags[lgtc_groups(GW)];
  lgl_grad_body<GW>(q, group_flags);
}
