// Device code of libdsgd_hip, part 15 (gfx950 only): the LOGISTIC model's whole-split steps by COLUMN LISTS (include/dsgd.h
// dsgd_lg_sync_steps_ranges, DESIGN.md 3.13 "Whole-split steps by column lists").  Included by dsgd_hip.hip after
// dsgd_logistic.hpp and dsgd_tcol.hpp.
//
// dsgd_lg_grad_range_kernel scatters one 64-bit atomic per non-zero.  A whole-split step repeats the SAME rows every time, so
// -- as the SVM's column lists do (csrc/dsgd_tcol.hpp) -- the entries of the ranges' rows are laid out once per ranges
// configuration, sorted by (worker, column), and a step takes the gradient column by column, where a sum is local:
//
//   the layout               count -> scan -> shares -> fill: dsgd_tc_count_kernel, dsgd_tc_scan_kernel and dsgd_tc_shares_kernel
//                            as they stand, then dsgd_lgc_fill_kernel.  An entry is 8 bytes: the float x as the CSR has it, and
//                            the row's position in the step's coefficient table (31 bits) under a "first entry of its column"
//                            flag (bit 31).  The entries are cut into equal shares, one per workgroup; slot_of_cid names the
//                            accumulator word of every non-empty (worker, column).
//   dsgd_lg_coef_kernel      one 16-lane group per row of every worker's range: d by row_dot<LG_GROUP, LG_UNR, false> on the
//                            resident weights -- lg_grad_body's instantiation and arguments: its bits -- then
//                            cq = lg_coef(d, y) * 2^(S_k - vexp) as a double at the row's position.  Plain stores; every
//                            position is written by every step: nothing to clear.
//   dsgd_lg_cgrad_kernel     one share per workgroup, a wave walks a contiguous quarter of it 64 entries at a time.  The column
//                            of an entry relative to the share's first is the number of flags up to it: a ballot and a
//                            popcount per round, the waves' totals through LDS.  q = rn(x * cq[pos]) -- lg_add's expression --
//                            goes into an LDS table of 64-bit sums by relative column; a round whose 64 entries lie in one
//                            column (the hot head) adds its sum once.  A column wholly inside the share is STORED to the
//                            worker's accumulator by this share alone; a column cut by a share boundary gets one 64-bit
//                            atomic per share.  Columns without an entry are not written: the finish leaves the accumulators
//                            zeroed.  No per-workgroup partials leave the launch.
//   dsgd_lg_finish_kernel<LG_STEP>   as behind the row form: its code, grid and arguments.
//
// The sums are integers: the accumulators hold the bits the row form leaves, whatever the order.
// Plain C++ and vector atomics only.
#pragma once

#include "dsgd_lg_cols_host.hpp"
#include "dsgd_logistic.hpp"
#include "dsgd_tcol.hpp"

constexpr unsigned int LGC_FIRST = 1u << 31;   // an entry's position word: the first entry of its (worker, column)

// the entries to their places (grid as dsgd_tc_count_kernel: (x, workers), a 16-lane group per row); ptr / cursor / cid: what
// dsgd_tc_scan_kernel left.  The order inside a column is whatever the atomics produce.
__global__ void __launch_bounds__(TC_THREADS) dsgd_lgc_fill_kernel(CsrView m, const WorkSeg* __restrict__ segs, int dp,
                                                                  const unsigned int* __restrict__ ptr, unsigned int* __restrict__ cursor,
                                                                  const int* __restrict__ cid, const int* __restrict__ pos_base, long long acc_stride,
                                                                  uint2* __restrict__ ent, int* __restrict__ slot_of_cid) {
  const WorkSeg sg = segs[blockIdx.y];
  const int sub = threadIdx.x & (TC_G - 1);
  const long long group = ((long long)blockIdx.x * TC_THREADS + threadIdx.x) / TC_G;
  const long long n_groups = (long long)gridDim.x * TC_ROWS_PER_WG;
  const long long kbase = (long long)blockIdx.y * dp;
  const unsigned int pb = (unsigned int)pos_base[blockIdx.y];
  for (long long row = sg.begin + group; row < sg.end; row += n_groups) {
    const unsigned int pos = pb + (unsigned int)(row - sg.begin);
    for (long long p = m.row_ptr[row] + sub; p < m.row_ptr[row + 1]; p += TC_G) {
      const int col = m.col[p];
      const long long key = kbase + col;
      const unsigned int at = atomicAdd(&cursor[key], 1u);
      const bool first = at == ptr[key];
      ent[at] = make_uint2(__float_as_uint(m.val[p]), pos | (first ? LGC_FIRST : 0u));
      if (first) slot_of_cid[cid[key]] = (int)((long long)blockIdx.y * acc_stride + col);
    }
  }
}

struct LgcCoefArgs {
  const float* w;                  // the weights, rank order
  int vexp, K;
  const WorkSeg* segs;             // [K] the workers' rows [begin, end)
  const int* pos_base;             // [K] where each worker's rows start in cq
  long long blocks_per_worker;     // grid = K * blocks_per_worker
  double* cq;                      // [rows of all workers] c_i 2^(S_k - vexp)
  DevScalars* sc;                  // err (1: a row outside the data)
};

__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_coef_kernel(CsrView m, LgcCoefArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int k = (int)((long long)blockIdx.x / a.blocks_per_worker);
  const long long b = (long long)blockIdx.x - (long long)k * a.blocks_per_worker;
  const WorkSeg seg = a.segs[k];
  const long long n = seg.end - seg.begin;
  const double qscale = ldexp(1.0, lg_shift(n) - a.vexp);   // (a power of two: c * qscale is exact)
  double* cq = a.cq + a.pos_base[k];
  const int sub = tid % LG_GROUP;
  const long long groups = a.blocks_per_worker * LG_ROWS_PER_BLOCK;
  for (long long t = b * LG_ROWS_PER_BLOCK + tid / LG_GROUP; t < n; t += groups) {
    const long long row = seg.begin + t;
    if (row < 0 || row >= m.n_rows) {   // (the host checked the ranges: never taken)
      if (sub == 0) atomicOr(&a.sc->err, 1);
      continue;
    }
    RowRegs<LG_GROUP, LG_UNR> r;
    const float d = row_dot<LG_GROUP, LG_UNR, false>(m, m.row_ptr[row], m.row_ptr[row + 1], nullptr, a.w, 0, sub, r);
    if (sub == 0) cq[t] = lg_coef(d, (double)m.label[row]) * qscale;
  }
}

struct LgcGradArgs {
  const uint2* ent;                // [n_shares * share] {x, position | LGC_FIRST}; zero beyond n_ent
  const TcShare* shares;           // per share: the compact id of its first column, the columns it touches
  const int* slot_of_cid;          // compact id -> word of acc
  const double* cq;
  unsigned long long* acc;         // [K][acc_stride] fixed-point column sums, rank order; zero on entry
  long long n_ent;
  int share;                       // a multiple of LGC_THREADS, at most LGC_MAX_SHARE
};

// grid: one workgroup per share
__global__ void __launch_bounds__(LGC_THREADS) dsgd_lg_cgrad_kernel(LgcGradArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long tab[LGC_MAX_SHARE];
  __shared__ int wave_flags[LGC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long e0 = (long long)blockIdx.x * a.share;
  const long long e1 = e0 + a.share < a.n_ent ? e0 + a.share : a.n_ent;
  const int rounds = a.share / LGC_THREADS;               // of 64 entries per wave: 1 .. LGC_NU
  const long long wbase = e0 + (long long)wave * rounds * 64 + lane;
  // the wave's entries and their coefficients, requested at once (the array is padded to whole shares: in bounds)
  uint2 en[LGC_NU];
  double cq[LGC_NU];
#pragma unroll
  for (int u = 0; u < LGC_NU; ++u) en[u] = u < rounds ? a.ent[wbase + u * 64] : make_uint2(0u, 0u);
#pragma unroll
  for (int u = 0; u < LGC_NU; ++u) {
    const bool in = u < rounds && wbase + u * 64 < e1;
    if (!in) en[u] = make_uint2(0u, 0u);                  // (x = 0, position 0, no flag: adds nothing)
    cq[u] = in ? a.cq[en[u].y & ~LGC_FIRST] : 0.0;
  }
  const TcShare sh = a.shares[blockIdx.x];
  const int n_local = sh.n_local < LGC_MAX_SHARE ? sh.n_local : LGC_MAX_SHARE;   // (a share of s entries touches at most s columns)
  const unsigned int head = a.ent[e0].y;                  // the share's first entry: its column is relative column 0, flagged or not
  const bool next_cut = e1 < a.n_ent && !(a.ent[e1].y & LGC_FIRST);   // the last column goes on in the next share
  for (int j = tid; j < n_local; j += LGC_THREADS) tab[j] = 0ull;
  int nf = 0;
#pragma unroll
  for (int u = 0; u < LGC_NU; ++u) nf += __popcll(__ballot((en[u].y & LGC_FIRST) != 0u));
  if (lane == 0) wave_flags[wave] = nf;
  __syncthreads();
  int base = (head & LGC_FIRST) ? -1 : 0;                 // relative column = flags up to and including the entry, + base
  for (int i = 0; i < wave; ++i) base += wave_flags[i];
  const unsigned long long le = lane == 63 ? ~0ull : (2ull << lane) - 1ull;   // lanes up to and including this one
#pragma unroll
  for (int u = 0; u < LGC_NU; ++u) {
    if (u < rounds) {                                     // (workgroup-uniform)
      const unsigned long long fl = __ballot((en[u].y & LGC_FIRST) != 0u);
      const int dc = base + __popcll(fl & le);
      const long long q = __double2ll_rn((double)__uint_as_float(en[u].x) * cq[u]);   // lg_add's expression; |x cq| <= 2^62
      if ((fl & ~1ull) == 0ull) {                         // the round's 64 entries lie in ONE column: one add for the wave
        long long s = q;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0 && s != 0 && (unsigned int)dc < (unsigned int)LGC_MAX_SHARE) atomicAdd(&tab[dc], (unsigned long long)s);
      } else if (q != 0 && (unsigned int)dc < (unsigned int)LGC_MAX_SHARE) {
        atomicAdd(&tab[dc], (unsigned long long)q);       // (two's complement: one add)
      }
      base += __popcll(fl);
    }
  }
  __syncthreads();
  for (int j = tid; j < n_local; j += LGC_THREADS) {
    const unsigned long long v = tab[j];
    if (v == 0ull) continue;                              // (a zero adds nothing: the word is zero already)
    unsigned long long* at = a.acc + a.slot_of_cid[sh.cid0 + (unsigned int)j];
    const bool cut = (j == 0 && !(head & LGC_FIRST)) || (j == n_local - 1 && next_cut);
    if (cut) atomicAdd(at, v);                            // the neighbouring shares add their parts: integers, any order
    else *at = v;                                         // this share's alone
  }
}
