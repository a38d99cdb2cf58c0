// csrc/dsgd_lg_topics_il_host.hpp alone (pure host C++): TP, the set call's checks in order, the interleaved planes, the head and
// the evaluation's LDS budget at T = 1 .. 32.  Built with AddressSanitizer and UBSan by tests/test_lg_topics_il_host.py.
#include <cstdio>
#include <vector>

#include "dsgd_lg_topics_il_host.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static void test_set() {
  const long long n = 10;
  std::vector<int8_t> p(32 * n, 1);
  CHECK(lgti_check_set(0, nullptr, 0).kind == LGT_OK);            // dropping the topics needs nothing
  CHECK(lgti_check_set(-1, p.data(), n).kind == LGT_BAD_T && lgti_check_set(33, p.data(), n).kind == LGT_BAD_T);
  CHECK(lgti_check_set(INT32_MAX, nullptr, -5).kind == LGT_BAD_T);   // T first: nothing else is looked at
  CHECK(lgti_check_set(9, nullptr, 0).kind == LGT_NULL);          // then the pointer ...
  CHECK(lgti_check_set(9, p.data(), 0).kind == LGT_NO_ROWS && lgti_check_set(32, p.data(), -3).kind == LGT_NO_ROWS);   // ... then the rows ...
  for (int T = 1; T <= LG_TOPICS_IL_MAX; ++T) CHECK(lgti_check_set(T, p.data(), n).kind == LGT_OK);
  for (int bad : {0, 2, -128}) {                                   // ... then every entry; the first offender is named
    p[31 * n + 9] = (int8_t)bad;
    const LgtCheck v = lgti_check_set(32, p.data(), n);
    CHECK(v.kind == LGT_ENTRY && v.topic == 31 && v.row == 9 && v.value == bad);
    CHECK(lgti_check_set(31, p.data(), n).kind == LGT_OK);        // (only T planes are read)
    p[31 * n + 9] = -1;
  }
  p[8 * n + 3] = 0, p[20 * n] = 5;
  const LgtCheck v = lgti_check_set(32, p.data(), n);
  CHECK(v.kind == LGT_ENTRY && v.topic == 8 && v.row == 3);
}

static void test_planes() {
  const long long n = 7;
  for (int T : {1, 5, 32}) {
    const int tp = lgti_tp(T);
    std::vector<int8_t> p((size_t)T * n), pi((size_t)lgti_plane_bytes(n, tp), 0);
    for (size_t i = 0; i < p.size(); ++i) p[i] = (i * 7 + i / 3) % 2 ? 1 : -1;
    lgti_interleave_planes(p.data(), T, n, pi.data());
    for (size_t j = 0; j < pi.size(); ++j) {   // row j / tp, topic j % tp; padding topics and the bytes behind the rows are +1
      const int t = (int)(j % tp);
      CHECK(pi[j] == (j < (size_t)n * tp && t < T ? p[(size_t)t * n + j / tp] : 1));
    }
  }
}

static void test_sizes() {
  const int dp = 47237;
  CHECK(lgti_tp(1) == 4 && lgti_tp(4) == 4 && lgti_tp(5) == 8 && lgti_tp(9) == 12 && lgti_tp(32) == 32);
  CHECK(lgti_hot(4) == 512 && lgti_hot(8) == 256 && lgti_hot(32) == 64);
  for (int T = 1; T <= LG_TOPICS_IL_MAX; ++T) {
    const int tp = lgti_tp(T);
    CHECK(tp % 4 == 0 && tp >= T && tp - T < 4);
    CHECK(lgti_hot(tp) * tp <= LGTI_HOT_WORDS && lgti_hot(tp) >= 1);
    CHECK(lgti_w_words(dp, tp) >= (long long)dp * tp + 4 && lgti_plane_bytes(1000, tp) >= 1000LL * tp + 4);
    CHECK(lgti_acc_stride(dp, tp) >= (long long)dp * tp && lgti_acc_stride(dp, tp) % 2 == 0);
    CHECK(lgti_acc_words(tp, 3, dp) == 3 * lgti_acc_stride(dp, tp));
    for (long long rows : {1LL, 4095LL, 4096LL, 1LL << 20}) {
      for (int hw_eval : {0, 63, 64, 1000, 40000, LGT_LDS_FLOATS}) {
        const int hw = lgti_eval_hw(rows, hw_eval, T);
        CHECK(hw >= 0 && hw <= hw_eval && hw % 64 == 0 && (rows >= 4096 || hw <= 1024));
        CHECK(lgti_eval_lds_floats(hw, T) <= LGT_LDS_FLOATS);
        // the regions follow one another; doubles live at even float offsets
        CHECK(lgti_eval_red_at(hw, T) >= tp * hw + 4 && lgti_eval_red_at(hw, T) % 2 == 0 && lgti_eval_sums_at(hw, T) % 2 == 0);
        CHECK(lgti_eval_sums_at(hw, T) == lgti_eval_red_at(hw, T) + 2 * (LG_EVAL_THREADS / 64));
        CHECK(lgti_eval_cnt_at(hw, T) == lgti_eval_sums_at(hw, T) + 2 * T * LGT_EVAL_GROUPS);
      }
    }
  }
  // at T = 32 the per-group words take 40 KiB of the 160; what is left holds 958 ranks of 32 floats
  CHECK((lgti_eval_lds_floats(0, 32) - lgti_eval_sums_at(0, 32)) * 4 == 40 * 1024);
  CHECK(lgti_eval_hw(1 << 20, LGT_LDS_FLOATS, 32) == 896 && lgti_eval_hw(1 << 20, LGT_LDS_FLOATS, 1) > 8192);
  CHECK(lgti_hot(lgti_tp(9)) == 170 && lgti_hot(lgti_tp(5)) == 256);   // tests/topics_hard_cases.py: N_HOT, and EVAL_TILES below
  for (int T : {5, 9, 32}) CHECK(lgti_eval_hw(600, 63, T) == 0 && lgti_eval_hw(600, 64, T) == 64 && lgti_eval_hw(600, 127, T) == 64 && lgti_eval_hw(600, 128, T) == 128);
}

int main() {
  test_set();
  test_planes();
  test_sizes();
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::fprintf(stderr, "all checks passed\n");
  return failures ? 1 : 0;
}
