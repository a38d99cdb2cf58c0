// The host arithmetic of SOFTMAX regression over the wide topic layout (include/dsgd.h "THE LOGISTIC MODEL": SOFTMAX; pure C++,
// no HIP: tests/cpp/lg_softmax_host_test.cpp compiles it alone; csrc/dsgd_lg_softmax.hpp and csrc/dsgd_lg_softmax_calls.hpp
// compile the same numbers).  The layout, the group width, the gradient's head and grid are the wide form's, unchanged
// (csrc/dsgd_lg_topics_wide_host.hpp); the ranges' limits are the topics' (csrc/dsgd_lg_topics_cols_host.hpp).
//
//   lgsm_check_set       dsgd_lg_softmax_set's arguments in order: C (0 drops; 1, negative or beyond LG_SOFTMAX_MAX refused), the
//                        pointer, the rows, then every class byte (< C)
//   lgsm_one_hot         the caller's class bytes as the wide setter's planes [C][n_rows]: +1 at the row's class, -1 elsewhere
//   lgsm_eval_blocks     the evaluation's workgroups (512 lanes, 32 chains each): one per 32 rows, at most one per compute unit
//   lgsm_eval_*_at       the evaluation's dynamic LDS behind the tile lds[hw][TP]: 4 spare words, the eight wave sums, ONE loss sum
//                        per chain [LGSM_EVAL_CHAINS] (doubles) and the workgroup's two tallies (32-bit words: correct, wrong)
//   lgsm_eval_hw         the ranks of the tile: lgtw_eval_hw's rule over this carve
//   lgsm_fold            the order of the host's sums: per class the nb |w_c|^2 words from 0.0 in workgroup order, the classes'
//                        sums from 0.0 in class order, the grid's loss words from 0.0 in workgroup order;
//                        loss = lambda sum_c |w_c|^2 + ls / n, acc = correct / n
#pragma once

#include "dsgd_lg_topics_cols_host.hpp"

constexpr int LG_SOFTMAX_MIN = 2;
constexpr int LG_SOFTMAX_MAX = LG_TOPICS_WIDE_MAX;
constexpr int LGSM_NONE = 255;           // "no class": what a vote nobody joins gives (a class is below 128)

enum LgsmFault {
  LGSM_OK = 0,
  LGSM_BAD_C,      // C negative, 1 or above LG_SOFTMAX_MAX
  LGSM_NULL,       // C >= 2 and no class bytes
  LGSM_NO_ROWS,    // C >= 2 and no rows loaded
  LGSM_ENTRY,      // row `row`: class `value` >= C
};
struct LgsmCheck {
  LgsmFault kind = LGSM_OK;
  long long row = -1;
  int value = 0;
};

// C == 0 (drop the classes) needs no bytes; nothing is read before C is in range
inline LgsmCheck lgsm_check_set(int32_t C, const uint8_t* cls, long long n_rows) {
  LgsmCheck v;
  if (C < 0 || C == 1 || C > LG_SOFTMAX_MAX) {
    v.kind = LGSM_BAD_C, v.value = C;
    return v;
  }
  if (C == 0) return v;
  if (!cls) {
    v.kind = LGSM_NULL;
    return v;
  }
  if (n_rows < 1) {
    v.kind = LGSM_NO_ROWS;
    return v;
  }
  for (long long i = 0; i < n_rows; ++i)
    if (cls[i] >= C) {
      v.kind = LGSM_ENTRY, v.row = i, v.value = cls[i];
      return v;
    }
  return v;
}

// planes: [C][n_rows], topic-major (checked bytes)
inline void lgsm_one_hot(const uint8_t* cls, int C, long long n_rows, int8_t* planes) {
  for (int c = 0; c < C; ++c)
    for (long long i = 0; i < n_rows; ++i) planes[(size_t)c * (size_t)n_rows + (size_t)i] = cls[i] == c ? (int8_t)1 : (int8_t)-1;
}

// The evaluation runs workgroups of 512 lanes, not the other forms' 1,024: a lane then has 256 registers, and the dots' 32
// accumulators, exp's and log's constants fit without scratch.  A workgroup walks 32 chains of rows.
constexpr int LGSM_EVAL_THREADS = 512;
constexpr int LGSM_EVAL_CHAINS = LGSM_EVAL_THREADS / LG_GROUP;
inline long long lgsm_eval_blocks(long long rows, int n_cu) {
  long long b = (rows + LGSM_EVAL_CHAINS - 1) / LGSM_EVAL_CHAINS;
  if (b > n_cu) b = n_cu;
  return b < 1 ? 1 : b;
}
LGTW_HD constexpr int lgsm_eval_red_at(int hw, int C) { return (lgti_tp(C) * hw + 4 + 1) & ~1; }
LGTW_HD constexpr int lgsm_eval_sums_at(int hw, int C) { return lgsm_eval_red_at(hw, C) + 2 * (LGSM_EVAL_THREADS / 64); }
LGTW_HD constexpr int lgsm_eval_cnt_at(int hw, int C) { return lgsm_eval_sums_at(hw, C) + 2 * LGSM_EVAL_CHAINS; }
LGTW_HD constexpr int lgsm_eval_lds_floats(int hw, int C) { return lgsm_eval_cnt_at(hw, C) + 2; }
static_assert(lgsm_eval_lds_floats(256, LG_SOFTMAX_MAX) <= LGT_LDS_FLOATS, "the carve and a tile of 256 ranks fit at C = 128");
inline int lgsm_eval_hw(long long rows, int hw_eval, int C) {
  int hw = rows >= 4096 ? hw_eval : (hw_eval < 1024 ? hw_eval : 1024);
  if (hw < 0) hw = 0;
  hw &= ~63;
  while (hw > 0 && lgsm_eval_lds_floats(hw, C) > LGT_LDS_FLOATS) hw -= 64;
  return hw;
}

// part: the topics' partial-sum block (lgt_part_words(C, ...)) as the device left it -- the classes' |w_c|^2 words, then the
// evaluation's loss words in the FIRST class's row; tally: {correct, wrong}; grid: the evaluation's workgroups
inline void lgsm_fold(const double* part, const unsigned long long* tally, int C, int dp, int n_cu, long long grid, long long rows, double lambda,
                      double* loss, double* acc) {
  const long long nb = lg_finish_blocks(dp);
  double nsq = 0.0, ls = 0.0;   // (in order: the same bits on every call)
  for (int c = 0; c < C; ++c) {
    double one = 0.0;
    for (long long i = 0; i < nb; ++i) one += part[lgt_nsq_at(c, dp) + i];
    nsq += one;
  }
  for (long long i = 0; i < grid; ++i) ls += part[lgt_loss_at(C, 0, dp, n_cu) + i];
  const double n = (double)rows;
  if (loss) *loss = lambda * nsq + ls / n;
  if (acc) *acc = (double)tally[0] / n;
}
