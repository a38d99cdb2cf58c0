// Device code of libdsgd_hip, part 15d (gfx950 only): the logistic model over several topics, WHOLE-SPLIT STEPS BY COLUMN LISTS
// with the LANES ACROSS THE TOPICS (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS, ROW RANGES; DESIGN.md 3.13 "Several
// topics, whole-split steps by column lists").  Included behind dsgd_lg_topics_wide.hpp and dsgd_lg_cols.hpp, whose kernels stay
// as they are; it serves the interleaved and the wide form, which share one layout.
//
// A whole-split step repeats the SAME rows, so the single model lays the ranges' entries out once, sorted by (worker, column)
// (csrc/dsgd_lg_cols.hpp: an entry is {x, position | LGC_FIRST}, the entries are cut into shares, slot_of_cid names the word
// `k * lg_stride + rank` of every non-empty column).  That layout does not depend on the label: it is used here as it stands.
// A step is THREE launches whatever T:
//
//   dsgd_lg_topics_coef_kernel<GW>    the wide gradient's split over ROW RANGES: a row is served by GW lanes, lane l owns topics
//                                     2l and 2l + 1.  lgt_row_load, lgtw_row_dots<false> and lgtw_labels2 as behind the lists,
//                                     then cq = lg_coef(d, y) * 2^(S_k - vexp) (0.0 for a padding topic) in ONE 16-byte store per
//                                     lane to cq[position][TP] + 2l, adjacent lanes on adjacent words.  Every position is written
//                                     by every step: nothing to clear.  No LDS, no atomics.
//   dsgd_lg_topics_cgrad_kernel<GW>   one share per workgroup, its 256 / GW lane groups each walk a contiguous run of
//                                     share * GW / 256 entries.  The entry words are the same for the whole group: fetched
//                                     coalesced, sixteen at a time, by the lanes of every 16-lane run and handed round by
//                                     __shfl(x, j, 16), as the wide walk does.  Per entry a lane loads the 16 bytes
//                                     cq[position][2l .. 2l + 1] (the group: one run of 8 TP bytes; the chunk's sixteen loads go
//                                     out together) and adds q = rn(x * cq) -- lgti_add's expression -- per owned topic into TWO
//                                     64-bit REGISTER sums.  The entries are sorted by column and a lane owns its topics, so the
//                                     sums live in registers between two flags: no LDS table, no atomic per entry.
//                                     At a flag the sums go to acc[k][rank][2l .. 2l + 1]: a column that begins and ends inside the
//                                     group's run gets one plain 16-byte store; a column cut by the run's start (its first entry
//                                     is unflagged) or by the run's end (the next run's first entry is unflagged and lies below
//                                     n_ent) gets one 64-bit atomic per word from every run that holds a part.  Zero sums are
//                                     skipped: the finish leaves the accumulators zeroed.
//                                     The compact id of a run's first column is the share's first (TcShare::cid0) plus the flags
//                                     in front of the run: the groups count the flags of their runs first (8 bytes per entry
//                                     against the 8 TP of the coefficients) and exchange the counts through 16 LDS words.
//   the finish                        the form's own, unchanged: dsgd_lg_topics_il_finish_kernel<true> or
//                                     dsgd_lg_topics_wide_finish_kernel<true> with the ranges as `segs` (they read the lengths).
//
// The sums are integers: the accumulators hold the bits the list forms leave, whatever the order and the store / atomic split.
// Contraction off, packed fp32 off (LGTI_KERNEL); atomics and barriers through lgtw_atomic_add / lgtw_barrier (no calls).
// What the gfx950 compile reports (every instantiation: no scratch, no spill): DESIGN.md 3.13.
//
// Plain C++, vector loads, vector stores and vector atomics only.
#pragma once
#include "dsgd_lg_topics_cols_host.hpp"

struct LgtcCoefArgs {
  const float* wi;                 // [dp][tp] the topics' weights, rank order
  const signed char* pi;           // [n_rows][tp] +1 / -1
  int T, tp, vexp, K;
  const WorkSeg* segs;             // [K] the workers' rows [begin, end)
  const int* pos_base;             // [K] where each worker's rows start in cq
  long long blocks_per_worker;     // grid = K * blocks_per_worker (lgtw_blocks_per_worker)
  double* cq;                      // [rows of all workers][tp] c_i 2^(S_k - vexp) per topic
  DevScalars* sc;                  // err (1: a row outside the data)
};

// (the kernels' bodies are always-inline functions: what a kernel that turns a target feature off names itself -- __shfl,
//  __double2ll_rn, make_double2 -- would be CALLED; named from here it is inlined with the body)
template <int GW>
__device__ __forceinline__ void lgtc_coef_body(const CsrView& m, const LgtcCoefArgs& a) {
#pragma clang fp contract(off)
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
    float d0, d1;
    lgtw_row_dots<false>(m, st, en, nullptr, a.wi, tp, lo, 0, sub, r, d0, d1);
    double y0, y1;
    lgtw_labels2(a.pi, row, tp, lo, y0, y1);
    const double cq0 = lo < a.T ? lg_coef(d0, y0) * qscale : 0.0;
    const double cq1 = lo + 1 < a.T ? lg_coef(d1, y1) * qscale : 0.0;
    if (own) *reinterpret_cast<double2*>(cq + t * tp) = make_double2(cq0, cq1);   // (an empty row's as any other's)
  }
}

// grid: K x blocks_per_worker workgroups, one GW-lane group per row of the worker's range
template <int GW>
LGTI_KERNEL void __launch_bounds__(LG_THREADS) dsgd_lg_topics_coef_kernel(CsrView m, LgtcCoefArgs a) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  lgtc_coef_body<GW>(m, a);
}

struct LgtcGradArgs {
  const uint2* ent;                // [n_shares * share] {x, position | LGC_FIRST}; zero beyond n_ent
  const TcShare* shares;           // per share: the compact id of its first column, the columns it touches
  const int* slot_of_cid;          // compact id -> k * lg_stride + rank
  const double* cq;                // [positions][tp]
  unsigned long long* acc;         // [K][acc_stride] = [K][rank][tp] fixed-point column sums; zero on entry
  long long acc_stride;
  long long n_ent;
  int share;                       // a multiple of LGC_THREADS, at most LGC_MAX_SHARE
  int tp;
  unsigned int lg_stride;          // the layout's words per worker
};

// the lane's two sums of relative column `col` into the accumulator: alone (the column lies inside the run) or added
__device__ __forceinline__ void lgtc_flush(const LgtcGradArgs& a, const TcShare& sh, int col, bool alone, int lo, long long s0, long long s1) {
  if ((s0 | s1) == 0 || (unsigned int)col >= (unsigned int)sh.n_local) return;   // (a zero adds nothing: the words are zero already)
  unsigned long long* at = a.acc + lgtc_acc_word((unsigned int)a.slot_of_cid[sh.cid0 + (unsigned int)col], a.lg_stride, a.acc_stride, a.tp) + lo;
  if (alone) {
    // (a vector type of its own: through make_ulonglong2 the finish kernels, which store it too, came out with other instructions)
    typedef unsigned long long lgtc_u2 __attribute__((ext_vector_type(2)));
    lgtc_u2 v;
    v.x = (unsigned long long)s0, v.y = (unsigned long long)s1;
    *reinterpret_cast<lgtc_u2*>(at) = v;
  } else {   // the neighbouring runs add their parts: integers, any order
    if (s0 != 0) lgtw_atomic_add(&at[0], (unsigned long long)s0);
    if (s1 != 0) lgtw_atomic_add(&at[1], (unsigned long long)s1);
  }
}

// group_flags: lgtc_groups(GW) LDS words
template <int GW>
__device__ __forceinline__ void lgtc_grad_body(const LgtcGradArgs& a, int* group_flags) {
#pragma clang fp contract(off)
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
    double2 c[LG_GROUP];
#pragma unroll
    for (int j = 0; j < LG_GROUP; ++j) {                    // (unconditional: the sixteen loads are in flight together)
      const unsigned int pos = (unsigned int)__shfl((int)e.y, j, LG_GROUP) & ~LGC_FIRST;
      c[j] = *reinterpret_cast<const double2*>(cq + (long long)pos * tp);
    }
#pragma unroll
    for (int j = 0; j < LG_GROUP; ++j) {
      const unsigned int y = (unsigned int)__shfl((int)e.y, j, LG_GROUP);
      const double xd = (double)__uint_as_float((unsigned int)__shfl((int)e.x, j, LG_GROUP));
      if (y & LGC_FIRST) {                                  // (the same for the whole group)
        if (own) lgtc_flush(a, sh, col, inside, lo, s0, s1);
        ++col;
        inside = true;
        s0 = 0, s1 = 0;
      }
      s0 += __double2ll_rn(xd * c[j].x);                    // lgti_add's expression; |x cq| <= 2^S <= 2^62.  Beyond n_ent x = 0: adds 0
      s1 += __double2ll_rn(xd * c[j].y);
    }
  }
  const bool goes_on = r1 < a.n_ent && !(a.ent[r1].y & LGC_FIRST);   // the last column has entries in the next run
  if (own) lgtc_flush(a, sh, col, inside && !goes_on, lo, s0, s1);
}

// grid: one workgroup per share
template <int GW>
LGTI_KERNEL void __launch_bounds__(LGC_THREADS) dsgd_lg_topics_cgrad_kernel(LgtcGradArgs a) {
#pragma clang fp contract(off)
  static_assert(GW == 16 || GW == 32 || GW == 64, "group width");
  __shared__ int group_flags[lgtc_groups(GW)];
  lgtc_grad_body<GW>(a, group_flags);
}
