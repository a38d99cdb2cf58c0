// The host arithmetic of the WIDE form of the logistic model over several topics (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL
// TOPICS, WIDE; pure C++, no HIP: tests/cpp/lg_topics_wide_host_test.cpp compiles it alone; csrc/dsgd_lg_topics_wide.hpp and
// csrc/dsgd_lg_topics_wide_calls.hpp compile the same numbers).  The layout is the interleaved form's, unchanged
// (csrc/dsgd_lg_topics_il_host.hpp: lgti_tp, lgti_w_words, lgti_plane_bytes, lgti_acc_stride, lgti_interleave_planes); the lists'
// checks, the partial-sum block and the order of the host's sums are the planar form's (csrc/dsgd_lg_topics_host.hpp).
//
//   lgtw_group_width     lanes per row: the smallest of 16, 32, 64 with 2 * GW >= TP -- lane l of a group owns topics 2l and 2l + 1
//   lgtw_check_set       dsgd_lg_topics_set_wide's arguments: lgti_check_set's refusals in its order, T up to LG_TOPICS_WIDE_MAX
//   lgtw_hot             ranks of the gradient kernel's LDS head, all TP topics of each
//   lgtw_blocks_per_worker  the gradient's workgroups per worker: one per LG_THREADS / GW rows of the longest list, capped
//   lgtw_eval_*_at       the evaluation's dynamic LDS behind the tile lds[hw][TP]: 4 spare words, the sixteen wave sums, the
//                        chains' loss sums [T][LGT_EVAL_GROUPS] (doubles: where lg_block_sum's tree reads them) and the
//                        workgroup's tallies [T][3] (32-bit words, integer atomics).  No word per group and tally as in the other forms
//   lgtw_eval_hw         the ranks of the tile: lgti_eval_hw's rule over this carve
#pragma once

#include "dsgd_lg_topics_il_host.hpp"

constexpr int LG_TOPICS_WIDE_MAX = 128;
// The LDS head of the wide gradient kernel: 4,096 words (32 KiB).  The kernel's registers allow four waves per SIMD -- four
// 256-lane workgroups per compute unit -- and four heads of 32 KiB take 128 of its 160 KiB, so LDS does not lower that.  It
// holds the 4096 / TP hottest ranks with all TP topics each: 32 ranks at TP = 128, 1,024 at TP = 4.
constexpr int LGTW_HOT_WORDS = 4096;
constexpr int LGTW_PER_CU = 4;           // workgroups per compute unit the gradient's grid is capped at (the four the registers allow)

LG_HD constexpr int lgtw_group_width(int tp) { return tp <= 32 ? 16 : (tp <= 64 ? 32 : 64); }
LG_HD constexpr int lgtw_hot(int tp) { return tp >= 4 ? LGTW_HOT_WORDS / tp : 0; }

inline long long lgtw_blocks_per_worker(long long max_items, int n_workers, int n_cu, int gw) {
  const long long per = LG_THREADS / gw;
  const long long want = (max_items + per - 1) / per;
  long long cap = (long long)n_cu * LGTW_PER_CU / (n_workers > 0 ? n_workers : 1);
  if (cap < 1) cap = 1;
  const long long b = want < cap ? want : cap;
  return b < 1 ? 1 : b;
}

// lgt_check_set's refusals in its order -- T, the pointer, the rows, then every entry plane by plane -- for T up to 128: the
// planar check runs over the planes eight at a time
inline LgtCheck lgtw_check_set(int32_t T, const int8_t* planes, long long n_rows) {
  LgtCheck v;
  if (T < 0 || T > LG_TOPICS_WIDE_MAX) {
    v.kind = LGT_BAD_T, v.value = T;
    return v;
  }
  for (int t0 = 0; t0 < T; t0 += LG_TOPICS_MAX) {
    const int n = T - t0 < LG_TOPICS_MAX ? T - t0 : LG_TOPICS_MAX;
    v = lgt_check_set(n, planes && n_rows >= 1 ? planes + (size_t)t0 * (size_t)n_rows : planes, n_rows);
    if (v.kind != LGT_OK) {
      if (v.kind == LGT_ENTRY) v.topic += t0;
      return v;
    }
  }
  return v;
}

// (always inlined: left to its own cost model the compiler CALLED these from the 3,000-instruction evaluation kernel, and a call
//  spills what lives across it)
#define LGTW_HD LG_HD __attribute__((always_inline)) inline
LGTW_HD constexpr int lgtw_eval_red_at(int hw, int T) { return (lgti_tp(T) * hw + 4 + 1) & ~1; }
LGTW_HD constexpr int lgtw_eval_sums_at(int hw, int T) { return lgtw_eval_red_at(hw, T) + 2 * (LG_EVAL_THREADS / 64); }
LGTW_HD constexpr int lgtw_eval_cnt_at(int hw, int T) { return lgtw_eval_sums_at(hw, T) + 2 * T * LGT_EVAL_GROUPS; }
LGTW_HD constexpr int lgtw_eval_lds_floats(int hw, int T) { return lgtw_eval_cnt_at(hw, T) + 3 * T; }
static_assert(lgtw_eval_lds_floats(64, LG_TOPICS_WIDE_MAX) <= LGT_LDS_FLOATS, "the carve and a tile of 64 ranks fit at T = 128");
inline int lgtw_eval_hw(long long rows, int hw_eval, int T) {
  int hw = rows >= 4096 ? hw_eval : (hw_eval < 1024 ? hw_eval : 1024);
  if (hw < 0) hw = 0;
  hw &= ~63;
  while (hw > 0 && lgtw_eval_lds_floats(hw, T) > LGT_LDS_FLOATS) hw -= 64;
  return hw;
}
