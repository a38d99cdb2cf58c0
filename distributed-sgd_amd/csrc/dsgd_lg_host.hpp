// The host arithmetic of the logistic model (pure C++, no HIP: tests/cpp/lg_host_test.cpp compiles it alone; csrc/dsgd_logistic.hpp
// and csrc/dsgd_hip.hip compile the same numbers).
//
//   lg_shift            S = 62 - ceil(log2 n): the fixed-point shift of a worker's list of n rows (the rule of csrc/dsgd_rp64.hpp;
//                       |c_i| <= 1 and |x| <= 2^vexp, so n entries of |q| <= 2^S stay inside 2^62)
//   lg_blocks_per_worker  the workgroups one worker's list or range is spread over
//   lg_finish_blocks    the finish kernel's grid: ONE column per lane, so that the per-workgroup sums of |w|^2 do not depend on
//                       the device (the loss is the same number wherever it is computed)
//   lg_eval_blocks      the evaluation's persistent grid
//   lg_eval_table       the grid of an evaluation of up to LG_MAX_RANGES row ranges in ONE launch: range r gets its own run of
//                       lg_eval_blocks(rows_r) workgroups, one run behind the other (the grid each range has in a launch of its own)
//   lg_pred_table       the same for up to LG_PRED_MAX_RANGES disjoint ranges (dsgd_lg_predict_ranges): three arrays for the device,
//                       searched by lg_pred_owner; the refusals of the SVM's dsgd_predict_ranges
//   lg_check_lists      a step's per-worker lists             (what is wrong, and where: plain data, the callers word the message)
//   lg_check_ranges     a step's per-worker row ranges
//   lg_check_flat       an epoch's flat lists                 (csrc/dsgd_plan_check.hpp: flat_lists_check)
#pragma once

#include <cstddef>
#include <cstdint>

#include "dsgd_plan_check.hpp"

#ifdef __HIPCC__
#define LG_HD __host__ __device__
#else
#define LG_HD
#endif

constexpr int LG_THREADS = 256;
constexpr int LG_GROUP = 16;                          // lanes per row
constexpr int LG_ROWS_PER_BLOCK = LG_THREADS / LG_GROUP;
constexpr int LG_EVAL_THREADS = 1024;
constexpr long long LG_MAX_LIST = 1LL << 40;          // S >= 22: far beyond any list that fits a device; keeps the shift positive

LG_HD constexpr int lg_ceil_log2(long long n) {
  int l = 0;
  while ((1LL << l) < n) ++l;
  return l;
}
LG_HD constexpr int lg_shift(long long n) { return 62 - lg_ceil_log2(n); }

// one workgroup per 16 rows of the longest list, all workers together at most `per_cu` workgroups per compute unit (every
// workgroup flushes its LDS head once: more of them only add flushes)
inline long long lg_blocks_per_worker(long long max_items, int n_workers, int n_cu, int per_cu) {
  const long long want = (max_items + LG_ROWS_PER_BLOCK - 1) / LG_ROWS_PER_BLOCK;
  long long cap = (long long)n_cu * per_cu / (n_workers > 0 ? n_workers : 1);
  if (cap < 1) cap = 1;
  const long long b = want < cap ? want : cap;
  return b < 1 ? 1 : b;
}
inline long long lg_finish_blocks(int dp) { return ((long long)dp + LG_THREADS - 1) / LG_THREADS; }
inline long long lg_eval_blocks(long long rows, int n_cu) {
  const long long per = LG_EVAL_THREADS / LG_GROUP;
  long long b = (rows + per - 1) / per;
  if (b > n_cu) b = n_cu;
  return b < 1 ? 1 : b;
}

// Several ranges, one launch (dsgd_lg_eval_ranges_kernel): range r is walked by the workgroups [first_block, first_block +
// n_blocks) and by no other, n_blocks = lg_eval_blocks(rows of r) -- the stride, the per-workgroup sums and their order are
// those of a launch over that range alone, so its loss has the same bits.  Ranges may overlap or repeat: each has its own
// workgroups, its own words of partial sums (at its workgroups' numbers) and its own tallies.
constexpr int LG_MAX_RANGES = 16;
constexpr int LG_TALLY_WORDS = 4;   // per range: signum(d) == y, == 0, == -y, and a spare (32-byte rows)
struct LgEvalRange {
  long long row_begin, row_end;
  int first_block, n_blocks;
};
struct LgEvalTable {
  LgEvalRange r[LG_MAX_RANGES];
  int n, grid;
};
// false: fewer than one range or more than LG_MAX_RANGES, a null table or no compute unit (the ranges themselves:
// lg_check_ranges, which the callers ask first)
inline bool lg_eval_table(const int64_t* row_begin, const int64_t* row_end, int n_ranges, int n_cu, LgEvalTable* t) {
  if (!row_begin || !row_end || !t || n_ranges < 1 || n_ranges > LG_MAX_RANGES || n_cu < 1) return false;
  *t = LgEvalTable{};
  int at = 0;
  for (int i = 0; i < n_ranges; ++i) {
    t->r[i].row_begin = row_begin[i];
    t->r[i].row_end = row_end[i];
    t->r[i].first_block = at;
    t->r[i].n_blocks = (int)lg_eval_blocks(row_end[i] - row_begin[i], n_cu);
    at += t->r[i].n_blocks;
  }
  t->n = n_ranges;
  t->grid = at;
  return true;
}

// Up to LG_PRED_MAX_RANGES ranges, one launch (dsgd_lg_predict_ranges_kernel, csrc/dsgd_lg_eval.hpp): too many for a select
// chain over kernel arguments, so the table is three arrays the kernel stages into LDS and searches by bisection.  Range r
// is walked by the workgroups [first_block[r], first_block[r + 1]), lg_eval_blocks(rows of r) of them -- the grid of a launch
// of dsgd_lg_eval_kernel over that range alone, so its loss has the same bits -- and its row begin[r] + t writes output
// position out_off[r] + t (range-major: out_off are the prefix sums of the lengths).  An EMPTY range gets no workgroup and
// no output: first_block[r] == first_block[r + 1] and out_off[r] == out_off[r + 1].  The owner of workgroup b is the LAST r
// with first_block[r] <= b (lg_pred_owner: an empty range never is).
// The refusals are those of the SVM's dsgd_predict_ranges, in its order; n_rows < 0 skips the check against the loaded rows.
constexpr int LG_PRED_MAX_RANGES = 256;
enum LgPredFault {
  LGP_OK = 0,
  LGP_ARGS,       // a null pointer, n_ranges < 1 or no compute unit
  LGP_TOO_MANY,   // more than LG_PRED_MAX_RANGES ranges
  LGP_REVERSED,   // range `range`: begin > end
  LGP_OUTSIDE,    // range `range` (not empty) leaves the n_rows loaded rows
  LGP_OVERLAP,    // ranges `range` and `other` share a row
  LGP_NO_ROWS,    // every range is empty
};
struct LgPredTable {
  LgPredFault fault = LGP_OK;
  int range = -1, other = -1;     // of a refusal
  int n = 0;                      // ranges
  long long grid = 0;             // workgroups: first_block[n]
  long long total = 0;            // rows: out_off[n]
  long long longest = 0;          // rows of the longest range (the launch's tile rule)
};
// first_block and out_off: n_ranges + 1 words each, begin: n_ranges
inline LgPredTable lg_pred_table(const int64_t* row_begin, const int64_t* row_end, int n_ranges, int n_cu, long long n_rows, long long* first_block,
                                 long long* begin, long long* out_off) {
  LgPredTable t;
  if (!row_begin || !row_end || !first_block || !begin || !out_off || n_ranges < 1 || n_cu < 1) {
    t.fault = LGP_ARGS;
    return t;
  }
  if (n_ranges > LG_PRED_MAX_RANGES) {
    t.fault = LGP_TOO_MANY;
    return t;
  }
  for (int r = 0; r < n_ranges; ++r) {
    if (row_begin[r] > row_end[r]) {
      t.fault = LGP_REVERSED, t.range = r;
      return t;
    }
    if (row_begin[r] == row_end[r]) continue;
    if (n_rows >= 0 && (row_begin[r] < 0 || row_end[r] > n_rows)) {
      t.fault = LGP_OUTSIDE, t.range = r;
      return t;
    }
  }
  // (at most 256 ranges: every pair)
  for (int r = 0; r < n_ranges; ++r)
    for (int s = r + 1; s < n_ranges; ++s)
      if (row_begin[r] < row_end[r] && row_begin[s] < row_end[s] && row_begin[r] < row_end[s] && row_begin[s] < row_end[r]) {
        t.fault = LGP_OVERLAP, t.range = r, t.other = s;
        return t;
      }
  first_block[0] = out_off[0] = 0;
  for (int r = 0; r < n_ranges; ++r) {
    const long long rows = row_end[r] - row_begin[r];
    begin[r] = row_begin[r];
    first_block[r + 1] = first_block[r] + (rows > 0 ? lg_eval_blocks(rows, n_cu) : 0);
    out_off[r + 1] = out_off[r] + rows;
    if (rows > t.longest) t.longest = rows;
  }
  if (out_off[n_ranges] == 0) {
    t.fault = LGP_NO_ROWS;
    return t;
  }
  t.n = n_ranges;
  t.grid = first_block[n_ranges];
  t.total = out_off[n_ranges];
  return t;
}
// the range that owns workgroup b < first_block[K]: the last r with first_block[r] <= b (the bisection of pred_range_of,
// csrc/dsgd_predict.hpp)
LG_HD inline int lg_pred_owner(const long long* first_block, int K, long long b) {
  int lo = 0, hi = K;   // first_block[lo] <= b < first_block[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first_block[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

enum LgFault {
  LG_OK = 0,
  LG_NO_WORKERS,    // n_workers < 1 or a null table
  LG_EMPTY,         // worker `worker`: a null or empty list, an empty or reversed range
  LG_TOO_LONG,      // worker `worker`: more than LG_MAX_LIST rows
  LG_INDEX,         // worker `worker`, position `pos`: `value` is not a loaded row (ranges: the range leaves the rows)
  LG_FIRST_OFFSET,  // (flat lists) offsets[0] != 0
  LG_END,           // (flat lists) offsets end elsewhere than n_idx
  LG_OFFSETS,       // (flat lists) offsets decrease or leave idx
};
struct LgCheck {
  LgFault kind = LG_OK;
  long long worker = -1, pos = -1, value = 0;
  long long longest = 0, total = 0;   // of a step that is in order
};

inline LgCheck lg_fault(LgFault kind, long long worker, long long pos, long long value) {
  LgCheck v;
  v.kind = kind;
  v.worker = worker;
  v.pos = pos;
  v.value = value;
  return v;
}

inline LgCheck lg_check_lists(const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers, long long n_rows) {
  if (n_workers < 1 || !idx_per_worker || !n_per_worker) return lg_fault(LG_NO_WORKERS, -1, -1, n_workers);
  LgCheck v;
  for (int k = 0; k < n_workers; ++k) {   // (the shape first: an empty list is refused whatever the others hold)
    if (n_per_worker[k] < 1 || !idx_per_worker[k]) return lg_fault(LG_EMPTY, k, -1, n_per_worker[k]);
    if (n_per_worker[k] > LG_MAX_LIST) return lg_fault(LG_TOO_LONG, k, -1, n_per_worker[k]);
    v.total += n_per_worker[k];
    if (n_per_worker[k] > v.longest) v.longest = n_per_worker[k];
  }
  for (int k = 0; k < n_workers; ++k) {
    const long long t = plan_first_outside(idx_per_worker[k], n_per_worker[k], n_rows);
    if (t >= 0) return lg_fault(LG_INDEX, k, t, idx_per_worker[k][t]);
  }
  return v;
}

inline LgCheck lg_check_ranges(const int64_t* row_begin, const int64_t* row_end, int n_workers, long long n_rows) {
  if (n_workers < 1 || !row_begin || !row_end) return lg_fault(LG_NO_WORKERS, -1, -1, n_workers);
  LgCheck v;
  for (int k = 0; k < n_workers; ++k) {
    if (row_end[k] <= row_begin[k]) return lg_fault(LG_EMPTY, k, -1, row_end[k] - row_begin[k]);
  }
  for (int k = 0; k < n_workers; ++k) {
    if (row_begin[k] < 0) return lg_fault(LG_INDEX, k, 0, row_begin[k]);
    if (row_end[k] > n_rows) return lg_fault(LG_INDEX, k, 1, row_end[k]);
    const long long n = row_end[k] - row_begin[k];
    if (n > LG_MAX_LIST) return lg_fault(LG_TOO_LONG, k, -1, n);
    v.total += n;
    if (n > v.longest) v.longest = n;
  }
  return v;
}

// offsets: n_steps * n_workers + 1 positions into idx (the layout of dsgd_sync_steps_f64); `worker` is the LIST's number
// (step * n_workers + worker)
inline LgCheck lg_check_flat(const int32_t* idx, long long n_idx, const int64_t* offsets, long long n_steps, int n_workers, long long n_rows) {
  if (!idx || !offsets || n_steps < 1 || n_workers < 1 || n_idx < 1) return lg_fault(LG_NO_WORKERS, -1, -1, n_workers);
  if (n_steps > INT64_MAX / n_workers - 1) return lg_fault(LG_NO_WORKERS, -1, -1, n_steps);
  const FlatListsCheck f = flat_lists_check(idx, n_idx, offsets, n_steps, n_workers, n_rows);
  switch (f.kind) {
    case FLAT_LISTS_OK: break;
    case FLAT_LISTS_FIRST_OFFSET: return lg_fault(LG_FIRST_OFFSET, 0, 0, f.value);
    case FLAT_LISTS_END: return lg_fault(LG_END, f.list, f.pos, f.value);
    case FLAT_LISTS_OFFSETS: return lg_fault(LG_OFFSETS, f.list, f.pos, f.value);
    case FLAT_LISTS_EMPTY: return lg_fault(LG_EMPTY, f.list, f.pos, f.value);
    case FLAT_LISTS_INDEX: return lg_fault(LG_INDEX, -1, f.pos, f.value);
  }
  LgCheck v;
  v.total = n_idx;
  for (long long i = 0; i < n_steps * n_workers; ++i) {
    const long long n = offsets[i + 1] - offsets[i];
    if (n > LG_MAX_LIST) return lg_fault(LG_TOO_LONG, i, -1, n);
    if (n > v.longest) v.longest = n;
  }
  return v;
}
