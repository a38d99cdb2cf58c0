// The host arithmetic of the logistic model's column lists (pure C++, no HIP: tests/cpp/lg_cols_host_test.cpp compiles it
// alone; csrc/dsgd_lg_cols.hpp and csrc/dsgd_lg_calls.hpp compile the same numbers).  DESIGN.md 3.13 "Whole-split steps by
// column lists".
//
//   lgc_share     entries per workgroup of dsgd_lg_cgrad_kernel: the entries spread over eight workgroups per compute unit,
//                 in whole workgroups' worth of lanes (LGC_THREADS), between LGC_MIN_SHARE and LGC_MAX_SHARE
//   lgc_plan      whether a ranges configuration can have a layout at all, and its sizes: the share, the shares, the entries
//                 padded to whole shares (every load of the gradient kernel is in bounds without a clamp), and where each
//                 worker's rows start in the step's coefficient table (row t of worker k: pos_base[k] + t)
#pragma once

#include <cstdint>

#include "dsgd_lg_host.hpp"

constexpr int LGC_THREADS = 256;
constexpr int LGC_WAVES = LGC_THREADS / 64;
constexpr int LGC_NU = 8;                               // entries per lane: a wave walks its part of a share in up to 8 rounds of 64
constexpr int LGC_MAX_SHARE = LGC_THREADS * LGC_NU;     // 2,048 entries: 16 KiB of 64-bit sums, eight workgroups per compute unit
constexpr int LGC_MIN_SHARE = LGC_THREADS;
constexpr int LGC_PER_CU = 8;                           // workgroups per compute unit the entries are spread over
constexpr long long LGC_LIMIT = 1LL << 31;              // entries and positions stay BELOW it (31-bit positions, 32-bit cursors)

enum LgcFault {
  LGC_OK = 0,
  LGC_NO_ENTRIES,   // nothing to lay out
  LGC_ENTRIES,      // 2^31 entries or more
  LGC_POSITIONS,    // the workers' rows together reach 2^31
  LGC_KEYS,         // workers x columns (or workers x accumulator stride) reach 2^31: the scan's keys and the slots are ints
};
struct LgcPlan {
  int share = 0;              // entries per workgroup
  long long n_shares = 0;     // workgroups
  long long n_pad = 0;        // entries allocated: n_shares * share
  long long positions = 0;    // words of the coefficient table
};

inline int lgc_share(long long n_ent, int n_cu) {
  const long long slots = (long long)(n_cu > 0 ? n_cu : 1) * LGC_PER_CU;
  long long s = (n_ent + slots - 1) / slots;
  s = (s + LGC_THREADS - 1) / LGC_THREADS * LGC_THREADS;
  if (s < LGC_MIN_SHARE) s = LGC_MIN_SHARE;
  if (s > LGC_MAX_SHARE) s = LGC_MAX_SHARE;
  return (int)s;
}

// the ranges are in order (lg_check_ranges came first); n_ent: the entries of their rows; pos_base: [n_workers] out
inline LgcFault lgc_plan(const int64_t* row_begin, const int64_t* row_end, int n_workers, long long n_ent, int dp, long long acc_stride, int n_cu,
                         LgcPlan* p, long long* pos_base) {
  *p = LgcPlan{};
  long long pos = 0;
  for (int k = 0; k < n_workers; ++k) {
    pos_base[k] = pos;
    pos += row_end[k] - row_begin[k];   // (each at most LG_MAX_LIST = 2^40, checked against the limit one by one: no overflow)
    if (pos >= LGC_LIMIT) return LGC_POSITIONS;
  }
  if ((long long)n_workers * dp >= LGC_LIMIT || (long long)n_workers * acc_stride >= LGC_LIMIT) return LGC_KEYS;
  if (n_ent < 1) return LGC_NO_ENTRIES;
  if (n_ent >= LGC_LIMIT) return LGC_ENTRIES;
  p->share = lgc_share(n_ent, n_cu);
  p->n_shares = (n_ent + p->share - 1) / p->share;
  p->n_pad = p->n_shares * p->share;
  p->positions = pos;
  return LGC_OK;
}
