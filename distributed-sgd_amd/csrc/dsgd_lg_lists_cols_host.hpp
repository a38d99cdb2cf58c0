// The host arithmetic of the topics' and softmax's LIST steps by COLUMN LISTS (include/dsgd.h dsgd_lg_topics_sync_steps_cols,
// dsgd_lg_softmax_sync_steps_cols; DESIGN.md 3.13 "Index lists by column lists"; pure C++, no HIP:
// tests/cpp/lg_lists_cols_host_test.cpp compiles it alone; csrc/dsgd_lg_lists_cols.hpp and csrc/dsgd_lg_lists_cols_calls.hpp
// compile the same numbers).
//
// The column-list layout of the WHOLE matrix names a row by its number.  A step says which rows take part through one 32-bit
// OWNER WORD per row of the matrix: the worker whose list names the row and the row's position in the step's concatenated
// lists, where its coefficients cq[position][TP] stand.
//
//   lgl_pack / lgl_worker / lgl_pos   the owner word: the worker in the top LGL_WORKER_BITS, the position below.  LGL_NONE
//                                     (all ones) is no worker's word: the workers stay below LGL_MAX_WORKERS = 2^8 - 1
//   lgl_step_repeats                  whether the rows idx[begin, end) of ONE step name a row twice, in one list or in two; `seen`
//                                     is a bitmap of n_rows bits, all clear on entry and on return
//   lgl_route                         what serves a step: the column lists, or the list form (LGL_LISTS_*: why)
#pragma once

#include <cstdint>

constexpr int LGL_WORKER_BITS = 8;
constexpr int LGL_POS_BITS = 32 - LGL_WORKER_BITS;
constexpr long long LGL_MAX_POS = 1LL << LGL_POS_BITS;                // a step's rows, all lists together: positions stay BELOW it
constexpr int LGL_MAX_WORKERS = (1 << LGL_WORKER_BITS) - 1;           // at most 255 workers: worker 255's words would reach LGL_NONE
constexpr unsigned int LGL_NONE = 0xffffffffu;                        // the row takes no part in the step
constexpr int LGL_THREADS = 256;                                      // lanes of a workgroup of the mark and the clear kernel

#if defined(__HIPCC__)
#define LGL_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define LGL_HD inline
#endif

LGL_HD constexpr unsigned int lgl_pack(int worker, long long pos) { return ((unsigned int)worker << LGL_POS_BITS) | (unsigned int)pos; }
LGL_HD constexpr int lgl_worker(unsigned int word) { return (int)(word >> LGL_POS_BITS); }
LGL_HD constexpr long long lgl_pos(unsigned int word) { return (long long)(word & ((1u << LGL_POS_BITS) - 1u)); }
static_assert(lgl_worker(LGL_NONE) == LGL_MAX_WORKERS, "no worker below the limit packs a word that reads as LGL_NONE's worker");

inline long long lgl_seen_words(long long n_rows) { return (n_rows + 63) / 64; }

// the indices were checked against [0, n_rows) before (lgt_check_steps)
inline bool lgl_step_repeats(const int32_t* idx, long long begin, long long end, uint64_t* seen) {
  bool twice = false;
  long long i = begin;
  for (; i < end && !twice; ++i) {
    uint64_t& w = seen[idx[i] >> 6];
    const uint64_t bit = 1ull << (idx[i] & 63);
    twice = (w & bit) != 0;
    w |= bit;
  }
  for (long long j = begin; j < i; ++j) seen[idx[j] >> 6] = 0;   // (only the words this step touched)
  return twice;
}

enum LglRoute {
  LGL_COLS = 0,         // mark, coefficients, column gradient with owners, finish, clear
  LGL_LISTS_REPEAT,     // a row named twice: one owner word cannot hold two positions
  LGL_LISTS_POSITIONS,  // LGL_MAX_POS rows or more in the step
  LGL_LISTS_WORKERS,    // more than LGL_MAX_WORKERS workers
  LGL_LISTS_NO_LAYOUT,  // the whole matrix has no column lists (lgc_plan declined it) or no memory for them or the tables
};

// positions: the step's rows, all lists together; layout: the matrix's column lists and the step's tables are to be had
inline LglRoute lgl_route(long long positions, int n_workers, bool repeats, bool layout) {
  if (!layout) return LGL_LISTS_NO_LAYOUT;
  if (n_workers > LGL_MAX_WORKERS) return LGL_LISTS_WORKERS;
  if (positions >= LGL_MAX_POS) return LGL_LISTS_POSITIONS;
  return repeats ? LGL_LISTS_REPEAT : LGL_COLS;
}

// workgroups of the mark and the clear kernel per worker: one lane per listed row of the longest list, capped
inline long long lgl_mark_blocks(long long longest, int n_workers, int n_cu) {
  const long long want = (longest + LGL_THREADS - 1) / LGL_THREADS;
  long long cap = (long long)(n_cu > 0 ? n_cu : 1) * 8 / (n_workers > 0 ? n_workers : 1);
  if (cap < 1) cap = 1;
  const long long b = want < cap ? want : cap;
  return b < 1 ? 1 : b;
}
