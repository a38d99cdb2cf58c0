// csrc/dsgd_lg_topics_host.hpp alone (pure host C++): hostile arguments, plane validation, the sizing at T = 1 and 8, and the
// order in which the host adds the loss and |w|^2 words.  Built with AddressSanitizer and UBSan by tests/test_lg_topics_host.py
// and run as a program of its own.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_lg_topics_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void test_set() {
  std::vector<int8_t> p(8 * 10, 1);
  CHECK(lgt_check_set(0, nullptr, 0).kind == LGT_OK);           // dropping the topics needs nothing
  CHECK(lgt_check_set(-1, p.data(), 10).kind == LGT_BAD_T);
  CHECK(lgt_check_set(9, p.data(), 10).kind == LGT_BAD_T);
  CHECK(lgt_check_set(INT32_MIN, nullptr, 10).kind == LGT_BAD_T);   // T first: nothing else is looked at
  CHECK(lgt_check_set(INT32_MAX, nullptr, -5).kind == LGT_BAD_T);
  CHECK(lgt_check_set(1, nullptr, 10).kind == LGT_NULL);
  CHECK(lgt_check_set(1, p.data(), 0).kind == LGT_NO_ROWS);
  CHECK(lgt_check_set(1, p.data(), -3).kind == LGT_NO_ROWS);
  for (int T = 1; T <= 8; ++T) CHECK(lgt_check_set(T, p.data(), 10).kind == LGT_OK);
  for (int bad : {0, 2, -2, 127, -128}) {                        // every entry is +1 or -1; the first offender is named
    p[7 * 10 + 9] = (int8_t)bad;
    const LgtCheck v = lgt_check_set(8, p.data(), 10);
    CHECK(v.kind == LGT_ENTRY && v.topic == 7 && v.row == 9 && v.value == bad);
    CHECK(lgt_check_set(7, p.data(), 10).kind == LGT_OK);       // (only T planes are read)
    p[7 * 10 + 9] = -1;
  }
  p[3] = 0, p[25] = 5;
  const LgtCheck v = lgt_check_set(8, p.data(), 10);
  CHECK(v.kind == LGT_ENTRY && v.topic == 0 && v.row == 3);
}

static void test_lists() {
  const int32_t a[3] = {0, 5, 9}, bad[3] = {0, 10, 2}, neg[1] = {-1};
  const int32_t* two[2] = {a, bad};
  const int64_t n2[2] = {3, 3};
  LgCheck v = lgt_check_step(two, n2, 2, 10);
  CHECK(v.kind == LG_INDEX && v.worker == 1 && v.pos == 1 && v.value == 10);
  CHECK(lgt_check_step(two, n2, 1, 10).kind == LG_OK);
  CHECK(lgt_check_step(two, n2, 0, 10).kind == LG_NO_WORKERS);
  CHECK(lgt_check_step(nullptr, n2, 2, 10).kind == LG_NO_WORKERS);
  const int64_t n0[2] = {3, 0};
  CHECK(lgt_check_step(two, n0, 2, 10).kind == LG_EMPTY);
  CHECK(lgt_check_list(a, 3, 10).kind == LG_OK && lgt_check_list(a, 3, 9).kind == LG_INDEX);
  CHECK(lgt_check_list(neg, 1, 10).kind == LG_INDEX);
  CHECK(lgt_check_list(nullptr, 3, 10).kind != LG_OK && lgt_check_list(a, 0, 10).kind != LG_OK);
  CHECK(lgt_check_range(0, 10, 10).kind == LG_OK && lgt_check_range(0, 11, 10).kind == LG_INDEX);
  CHECK(lgt_check_range(-1, 5, 10).kind == LG_INDEX && lgt_check_range(5, 5, 10).kind == LG_EMPTY && lgt_check_range(6, 5, 10).kind == LG_EMPTY);
  const int32_t flat[4] = {1, 2, 3, 10};
  const int64_t offs[3] = {0, 2, 4}, offs_bad[3] = {0, 3, 2}, offs_first[3] = {1, 2, 4};
  CHECK(lgt_check_steps(flat, 4, offs, 2, 1, 11).kind == LG_OK);
  CHECK(lgt_check_steps(flat, 4, offs, 2, 1, 10).kind == LG_INDEX);
  CHECK(lgt_check_steps(flat, 4, offs_bad, 2, 1, 11).kind != LG_OK);
  CHECK(lgt_check_steps(flat, 4, offs_first, 2, 1, 11).kind == LG_FIRST_OFFSET);
  CHECK(lgt_check_steps(nullptr, 4, offs, 2, 1, 11).kind == LG_NO_WORKERS);
  CHECK(lgt_check_steps(flat, 4, offs, 0, 1, 11).kind == LG_NO_WORKERS);
}

static void test_sizes() {
  const int dp = 47237, n_cu = 256;
  CHECK(lgt_hot(1) == 2048 && lgt_hot(2) == 1024 && lgt_hot(3) == 682 && lgt_hot(8) == 256 && lgt_hot(0) == 0);
  for (int T = 1; T <= LG_TOPICS_MAX; ++T) {
    CHECK(T * lgt_hot(T) <= LGT_HOT_WORDS);                     // the topics' shares fit the one head
    CHECK(lgt_hot(T) >= 256);
    CHECK(lgt_w_stride(dp) >= dp && lgt_w_stride(dp) % 64 == 0 && lgt_w_stride(dp) - dp < 64);
    CHECK(lgt_acc_stride(dp) >= dp && lgt_acc_stride(dp) % 32 == 0);
    CHECK(lgt_acc_words(T, 3, dp) == (long long)T * 3 * lgt_acc_stride(dp));
    CHECK(lgt_part_words(T, dp, n_cu) == (long long)T * (lg_finish_blocks(dp) + n_cu));
    CHECK(lgt_nsq_at(T - 1, dp) + lg_finish_blocks(dp) == lgt_loss_at(T, 0, dp, n_cu));          // the blocks do not overlap
    CHECK(lgt_loss_at(T, T - 1, dp, n_cu) + n_cu == lgt_part_words(T, dp, n_cu));
    for (long long rows : {1LL, 1000LL, 4095LL, 4096LL, 1LL << 20}) {
      for (int hw_eval : {0, 63, 64, 1000, 40000, LGT_LDS_FLOATS}) {
        const int hw = lgt_eval_hw(rows, hw_eval, T);
        CHECK(hw >= 0 && hw <= hw_eval && hw % 64 == 0);
        CHECK(lgt_eval_lds_floats(hw, T) <= LGT_LDS_FLOATS);
        if (rows < 4096) CHECK(hw <= 1024);
        // the regions follow one another: tiles, tally words, wave sums (8-byte aligned), group sums, group tallies
        CHECK(lgt_eval_red_at(hw, T) >= T * hw + 4 && lgt_eval_red_at(hw, T) % 2 == 0);
        CHECK(lgt_eval_sums_at(hw, T) == lgt_eval_red_at(hw, T) + 2 * (LG_EVAL_THREADS / 64));
        CHECK(lgt_eval_cnt_at(hw, T) == lgt_eval_sums_at(hw, T) + 2 * T * LGT_EVAL_GROUPS);
      }
    }
  }
  CHECK(lgt_eval_hw(1 << 20, LGT_LDS_FLOATS, 1) > 30000);       // one topic keeps nearly the whole tile
  CHECK(lgt_eval_hw(1 << 20, LGT_LDS_FLOATS, 8) >= 4096);       // eight share it
}

static void test_fold_order() {
  // words whose sum depends on the order: 1e16 + 1 + 1 - 1e16 is 0 from the left in doubles, 2 in any order that pairs the ones
  const int T = 2, dp = 600, n_cu = 4;                           // 3 finish workgroups
  const long long nb = lg_finish_blocks(dp);
  CHECK(nb == 3);
  std::vector<double> part((size_t)lgt_part_words(T, dp, n_cu), 1e300);   // (words beyond the grid must not be read: they would show)
  std::vector<unsigned long long> tally(T * LG_TALLY_WORDS, 0);
  const double w0[3] = {1e16, 1.0, -1e16}, w1[3] = {0.5, 0.25, 0.125};
  for (int i = 0; i < 3; ++i) part[(size_t)lgt_nsq_at(0, dp) + i] = w0[i], part[(size_t)lgt_nsq_at(1, dp) + i] = w1[i];
  const double l0[2] = {3.0, 1.0}, l1[2] = {1e16, 1.0};
  for (int i = 0; i < 2; ++i) part[(size_t)lgt_loss_at(T, 0, dp, n_cu) + i] = l0[i], part[(size_t)lgt_loss_at(T, 1, dp, n_cu) + i] = l1[i];
  tally[0] = 3, tally[LG_TALLY_WORDS] = 1;
  double loss[2], acc[2];
  lgt_fold(part.data(), tally.data(), T, dp, n_cu, 2, 4, 0.5, loss, acc);
  double nsq0 = 0.0;
  nsq0 += 1e16, nsq0 += 1.0, nsq0 += -1e16;                      // in workgroup order from 0.0
  CHECK(nsq0 == 0.0);
  CHECK(loss[0] == 0.5 * nsq0 + (0.0 + 3.0 + 1.0) / 4.0);
  CHECK(loss[1] == 0.5 * 0.875 + ((0.0 + 1e16) + 1.0) / 4.0);
  CHECK(acc[0] == 0.75 && acc[1] == 0.25);
  lgt_fold(part.data(), tally.data(), T, dp, n_cu, 2, 4, 0.5, nullptr, acc);   // either output may be absent
  lgt_fold(part.data(), tally.data(), T, dp, n_cu, 2, 4, 0.5, loss, nullptr);
}

int main() {
  test_set();
  test_lists();
  test_sizes();
  test_fold_order();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
