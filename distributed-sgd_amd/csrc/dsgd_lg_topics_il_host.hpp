// The host arithmetic of the INTERLEAVED form of the logistic model over several topics (include/dsgd.h "THE LOGISTIC MODEL":
// SEVERAL TOPICS, INTERLEAVED; pure C++, no HIP: tests/cpp/lg_topics_il_host_test.cpp compiles it alone; csrc/dsgd_lg_topics_il.hpp
// and csrc/dsgd_lg_topics_il_calls.hpp compile the same numbers).  The checks of the lists, the partial-sum block and the order of
// the host's sums are the planar form's (csrc/dsgd_lg_topics_host.hpp: lgt_check_*, lgt_part_words, lgt_nsq_at, lgt_loss_at,
// lgt_fold), unchanged.
//
//   lgti_tp              T rounded up to a multiple of 4: the topics of one rank, one row or one column lie side by side, TP - T
//                        padding topics (weight 0, label +1, never reported) fill the last quad
//   lgti_check_set       dsgd_lg_topics_set_il's arguments: lgt_check_set's refusals in its order, T up to LG_TOPICS_IL_MAX
//   lgti_w_words         floats of Wi[rank][TP]            lgti_plane_bytes   bytes of Pi[row][TP]
//   lgti_acc_stride      words between two workers' column sums acc[k][rank][TP]; lgti_acc_words: all K of them
//   lgti_hot             ranks of the gradient kernel's LDS head, all TP topics of each
//   lgti_eval_hw         the ranks of the evaluation's hot-weight tile lds[hw][TP]: lgt_eval_hw's rule with the tile costing
//                        TP * hw floats; lgti_eval_*_at / lgti_eval_lds_floats: the regions behind it, as the planar form's
#pragma once

#include "dsgd_lg_topics_host.hpp"

constexpr int LG_TOPICS_IL_MAX = 32;
// The LDS head of the interleaved gradient kernel: the single model's 2,048 words (16 KiB), so eight 256-lane workgroups still
// share a compute unit's 160 KiB and LDS does not lower the waves per SIMD the registers allow (5: the gradient kernel has 90
// VGPRs with TB = 4).  The head holds the 2048 / TP hottest ranks with all TP topics each -- 64 ranks at TP = 32.  It was not
// grown: five workgroups of 32 KiB would take a compute unit's whole 160 KiB and leave the next register saving nothing to
// run in, and the share of the non-zeros a larger head takes is not measured.
constexpr int LGTI_HOT_WORDS = 2048;
constexpr int LGTI_PAD = 4;              // floats / bytes behind Wi and Pi: the quad a block of TB = 8 reads past TP = 4, 12, 20, 28

LG_HD constexpr int lgti_tp(int T) { return (T + 3) & ~3; }
LG_HD constexpr int lgti_hot(int tp) { return tp >= 4 ? LGTI_HOT_WORDS / tp : 0; }
inline long long lgti_w_words(int dp, int tp) { return (long long)dp * tp + LGTI_PAD; }
inline long long lgti_plane_bytes(long long n_rows, int tp) { return n_rows * tp + LGTI_PAD; }
inline long long lgti_acc_stride(int dp, int tp) { return lgt_acc_stride(dp) * tp; }
inline long long lgti_acc_words(int tp, int K, int dp) { return (long long)K * lgti_acc_stride(dp, tp); }

// lgt_check_set's refusals in its order -- T, the pointer, the rows, then every entry plane by plane -- for T up to 32: the
// planar check runs over the planes eight at a time
inline LgtCheck lgti_check_set(int32_t T, const int8_t* planes, long long n_rows) {
  LgtCheck v;
  if (T < 0 || T > LG_TOPICS_IL_MAX) {
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

// Pi[row][TP] from the caller's topic-major planes [T][n_rows] (checked); padding topics are +1
inline void lgti_interleave_planes(const int8_t* planes, int T, long long n_rows, int8_t* pi) {
  const int tp = lgti_tp(T);
  for (long long i = 0; i < n_rows; ++i)
    for (int t = 0; t < tp; ++t) pi[(size_t)i * tp + t] = t < T ? planes[(size_t)t * (size_t)n_rows + (size_t)i] : (int8_t)1;
  for (int j = 0; j < LGTI_PAD; ++j) pi[(size_t)n_rows * tp + j] = 1;
}

// dynamic LDS of the evaluation, in floats: the tile lds[hw][TP], 4 tally words, then (8-byte aligned) the sixteen wave sums, the
// groups' loss sums [T][LGT_EVAL_GROUPS] (doubles) and their tallies [T][3][LGT_EVAL_GROUPS] (32-bit words)
LG_HD constexpr int lgti_eval_red_at(int hw, int T) { return (lgti_tp(T) * hw + 4 + 1) & ~1; }
LG_HD constexpr int lgti_eval_sums_at(int hw, int T) { return lgti_eval_red_at(hw, T) + 2 * (LG_EVAL_THREADS / 64); }
LG_HD constexpr int lgti_eval_cnt_at(int hw, int T) { return lgti_eval_sums_at(hw, T) + 2 * T * LGT_EVAL_GROUPS; }
LG_HD constexpr int lgti_eval_lds_floats(int hw, int T) { return lgti_eval_cnt_at(hw, T) + 3 * T * LGT_EVAL_GROUPS; }
inline int lgti_eval_hw(long long rows, int hw_eval, int T) {
  int hw = rows >= 4096 ? hw_eval : (hw_eval < 1024 ? hw_eval : 1024);
  if (hw < 0) hw = 0;
  hw &= ~63;
  while (hw > 0 && lgti_eval_lds_floats(hw, T) > LGT_LDS_FLOATS) hw -= 64;
  return hw;
}
