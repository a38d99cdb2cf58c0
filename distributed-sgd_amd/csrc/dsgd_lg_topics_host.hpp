// The host arithmetic of the logistic model over SEVERAL TOPICS (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS; pure C++,
// no HIP: tests/cpp/lg_topics_host_test.cpp compiles it alone; csrc/dsgd_lg_topics.hpp and csrc/dsgd_lg_topics_calls.hpp compile
// the same numbers).
//
//   lgt_check_set        dsgd_lg_topics_set's arguments: T, the planes' pointer, then every plane entry (+1 or -1)
//   lgt_check_step       a step's per-worker lists     (lg_check_lists: the refusals of dsgd_lg_sync_step, in its order)
//   lgt_check_steps      an epoch's flat lists         (lg_check_flat:  the refusals of dsgd_lg_sync_steps)
//   lgt_check_range      an evaluation's row range     (lg_check_ranges with one range)
//   lgt_check_list       a prediction's list           (lg_check_lists with one worker)
//   lgt_hot              ranks of the LDS head one topic owns in the gradient kernel: the LGT_HOT_WORDS words of the single
//                        model's head (LG_HOT) shared evenly, so a workgroup's LDS does not grow with T
//   lgt_w_stride         floats between two topics' weight vectors (rank order): D + 1 rounded up to 64 floats (256-byte rows)
//   lgt_acc_stride       words between two workers' column sums; lgt_acc_words: [T][K][stride]
//   lgt_eval_hw          the hot-weight tile ONE topic gets in the evaluation: dsgd_lg_loss_acc's rule for the range, then what
//                        T tiles and the per-group sums leave of the LDS, in steps of 64 (the tile's size moves no bit: DESIGN 3.13)
//   lgt_eval_lds_floats  the evaluation's dynamic LDS, in floats
//   lgt_part_words       doubles of the partial-sum block: [T][nb] |w_t|^2 words, then [T][n_cu] loss words
//   lgt_fold             the order in which the host adds the words: per topic the nb |w|^2 words from 0.0 in workgroup order,
//                        the grid's loss words from 0.0 in workgroup order, loss = lambda nsq + ls / n, acc = tally / n --
//                        dsgd_lg_loss_acc's expressions
#pragma once

#include <cstddef>
#include <cstdint>

#include "dsgd_lg_host.hpp"

constexpr int LG_TOPICS_MAX = 8;
constexpr int LGT_HOT_WORDS = 2048;      // (= LG_HOT, csrc/dsgd_logistic.hpp: static_assert in csrc/dsgd_lg_topics.hpp)
constexpr int LGT_LDS_FLOATS = 40960;    // (= DSGD_LDS_FLOATS, csrc/dsgd_limits.hpp: likewise)
constexpr int LGT_EVAL_GROUPS = LG_EVAL_THREADS / LG_GROUP;   // rows in flight per evaluation workgroup

enum LgtFault {
  LGT_OK = 0,
  LGT_BAD_T,       // T outside [0, LG_TOPICS_MAX]
  LGT_NULL,        // T >= 1 and no planes
  LGT_NO_ROWS,     // T >= 1 and no rows loaded
  LGT_ENTRY,       // plane `topic`, row `row`: `value` is neither +1 nor -1
};
struct LgtCheck {
  LgtFault kind = LGT_OK;
  int topic = -1;
  long long row = -1;
  int value = 0;
};

// T == 0 (drop the topics) needs no planes; nothing is read before T is in range
inline LgtCheck lgt_check_set(int32_t T, const int8_t* planes, long long n_rows) {
  LgtCheck v;
  if (T < 0 || T > LG_TOPICS_MAX) {
    v.kind = LGT_BAD_T, v.value = T;
    return v;
  }
  if (T == 0) return v;
  if (!planes) {
    v.kind = LGT_NULL;
    return v;
  }
  if (n_rows < 1) {
    v.kind = LGT_NO_ROWS;
    return v;
  }
  for (int t = 0; t < T; ++t)
    for (long long i = 0; i < n_rows; ++i) {
      const int8_t y = planes[(size_t)t * (size_t)n_rows + (size_t)i];
      if (y != 1 && y != -1) {
        v.kind = LGT_ENTRY, v.topic = t, v.row = i, v.value = y;
        return v;
      }
    }
  return v;
}

inline LgCheck lgt_check_step(const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers, long long n_rows) {
  return lg_check_lists(idx_per_worker, n_per_worker, n_workers, n_rows);
}
inline LgCheck lgt_check_steps(const int32_t* idx, long long n_idx, const int64_t* offsets, long long n_steps, int n_workers, long long n_rows) {
  return lg_check_flat(idx, n_idx, offsets, n_steps, n_workers, n_rows);
}
inline LgCheck lgt_check_range(int64_t row_begin, int64_t row_end, long long n_rows) { return lg_check_ranges(&row_begin, &row_end, 1, n_rows); }
inline LgCheck lgt_check_list(const int32_t* idx, int64_t n, long long n_rows) {
  if (n < 1 || !idx) return lg_fault(LG_NO_WORKERS, -1, -1, 1);
  return lg_check_lists(&idx, &n, 1, n_rows);
}

LG_HD constexpr int lgt_hot(int T) { return T >= 1 ? LGT_HOT_WORDS / T : 0; }
inline long long lgt_w_stride(int dp) { return ((long long)dp + 63) & ~63LL; }
inline long long lgt_acc_stride(int dp) { return ((long long)dp + 31) & ~31LL; }
inline long long lgt_acc_words(int T, int K, int dp) { return (long long)T * K * lgt_acc_stride(dp); }

// dynamic LDS of the evaluation, in floats: T tiles of hw weights, 4 tally words, then (8-byte aligned) the sixteen wave sums,
// the groups' loss sums [T][LGT_EVAL_GROUPS] (doubles) and their tallies [T][3][LGT_EVAL_GROUPS] (32-bit words)
LG_HD constexpr int lgt_eval_red_at(int hw, int T) { return (T * hw + 4 + 1) & ~1; }
LG_HD constexpr int lgt_eval_sums_at(int hw, int T) { return lgt_eval_red_at(hw, T) + 2 * (LG_EVAL_THREADS / 64); }
LG_HD constexpr int lgt_eval_cnt_at(int hw, int T) { return lgt_eval_sums_at(hw, T) + 2 * T * LGT_EVAL_GROUPS; }
LG_HD constexpr int lgt_eval_lds_floats(int hw, int T) { return lgt_eval_cnt_at(hw, T) + 3 * T * LGT_EVAL_GROUPS; }
inline int lgt_eval_hw(long long rows, int hw_eval, int T) {
  int hw = rows >= 4096 ? hw_eval : (hw_eval < 1024 ? hw_eval : 1024);
  if (hw < 0) hw = 0;
  hw &= ~63;
  while (hw > 0 && lgt_eval_lds_floats(hw, T) > LGT_LDS_FLOATS) hw -= 64;
  return hw;
}

inline long long lgt_part_words(int T, int dp, int n_cu) { return (long long)T * (lg_finish_blocks(dp) + n_cu); }
// where topic t's |w|^2 words and loss words start in the block
inline long long lgt_nsq_at(int t, int dp) { return (long long)t * lg_finish_blocks(dp); }
inline long long lgt_loss_at(int T, int t, int dp, int n_cu) { return (long long)T * lg_finish_blocks(dp) + (long long)t * n_cu; }

// part: the block above as the device left it; tally: [T][LG_TALLY_WORDS]; grid: the evaluation's workgroups
inline void lgt_fold(const double* part, const unsigned long long* tally, int T, int dp, int n_cu, long long grid, long long rows, double lambda,
                     double* loss, double* acc) {
  const long long nb = lg_finish_blocks(dp);
  for (int t = 0; t < T; ++t) {
    double nsq = 0.0, ls = 0.0;   // (in order: the same bits on every call)
    for (long long i = 0; i < nb; ++i) nsq += part[lgt_nsq_at(t, dp) + i];
    for (long long i = 0; i < grid; ++i) ls += part[lgt_loss_at(T, t, dp, n_cu) + i];
    const double n = (double)rows;
    if (loss) loss[t] = lambda * nsq + ls / n;
    if (acc) acc[t] = (double)tally[(size_t)t * LG_TALLY_WORDS] / n;
  }
}
