// csrc/dsgd_lg_topics_wide_host.hpp alone (pure host C++): the group width, the set call's checks in order, the head, the grid and
// the evaluation's LDS carve at TP = 4, 36, 104, 128.  Built with AddressSanitizer and UBSan by tests/test_lg_topics_wide_host.py.
#include <cstdio>
#include <vector>

#include "dsgd_lg_topics_wide_host.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static void test_set() {
  const long long n = 10;
  std::vector<int8_t> p(128 * n, 1);
  CHECK(lgtw_check_set(0, nullptr, 0).kind == LGT_OK);            // dropping the topics needs nothing
  CHECK(lgtw_check_set(-1, p.data(), n).kind == LGT_BAD_T && lgtw_check_set(129, p.data(), n).kind == LGT_BAD_T);
  CHECK(lgtw_check_set(INT32_MAX, nullptr, -5).kind == LGT_BAD_T);   // T first: nothing else is looked at
  CHECK(lgtw_check_set(100, nullptr, 0).kind == LGT_NULL);        // then the pointer ...
  CHECK(lgtw_check_set(100, p.data(), 0).kind == LGT_NO_ROWS && lgtw_check_set(128, p.data(), -3).kind == LGT_NO_ROWS);   // ... then the rows ...
  for (int T = 1; T <= LG_TOPICS_WIDE_MAX; ++T) CHECK(lgtw_check_set(T, p.data(), n).kind == LGT_OK);
  for (int bad : {0, 2, -128}) {                                   // ... then every entry; the first offender is named
    p[127 * n + 9] = (int8_t)bad;
    const LgtCheck v = lgtw_check_set(128, p.data(), n);
    CHECK(v.kind == LGT_ENTRY && v.topic == 127 && v.row == 9 && v.value == bad);
    CHECK(lgtw_check_set(127, p.data(), n).kind == LGT_OK);       // (only T planes are read)
    p[127 * n + 9] = -1;
  }
  p[40 * n + 3] = 0, p[100 * n] = 5;
  CHECK(lgtw_check_set(128, p.data(), n).topic == 40 && lgtw_check_set(128, p.data(), n).row == 3);
}

static void test_sizes() {
  CHECK(lgtw_group_width(4) == 16 && lgtw_group_width(32) == 16 && lgtw_group_width(36) == 32 && lgtw_group_width(64) == 32);
  CHECK(lgtw_group_width(68) == 64 && lgtw_group_width(104) == 64 && lgtw_group_width(128) == 64);
  CHECK(lgtw_hot(4) == 1024 && lgtw_hot(36) == 113 && lgtw_hot(104) == 39 && lgtw_hot(128) == 32);
  CHECK(lgtw_blocks_per_worker(1, 3, 256, 64) == 1 && lgtw_blocks_per_worker(100, 3, 256, 64) == 25 && lgtw_blocks_per_worker(100, 3, 256, 16) == 7);
  for (int T = 1; T <= LG_TOPICS_WIDE_MAX; ++T) {
    const int tp = lgti_tp(T), gw = lgtw_group_width(tp);
    CHECK(2 * gw >= tp && (gw == 16 || 2 * (gw / 2) < tp));       // two topics per lane, and the smallest such width
    CHECK(lgtw_hot(tp) * tp <= LGTW_HOT_WORDS && lgtw_hot(tp) >= 1);
    for (long long rows : {1LL, 4095LL, 4096LL, 1LL << 20}) {
      for (int hw_eval : {0, 63, 64, 1000, 40000, LGT_LDS_FLOATS}) {
        const int hw = lgtw_eval_hw(rows, hw_eval, T);
        CHECK(hw >= 0 && hw <= hw_eval && hw % 64 == 0 && (rows >= 4096 || hw <= 1024));
        CHECK(lgtw_eval_lds_floats(hw, T) <= LGT_LDS_FLOATS);
        CHECK(lgtw_eval_red_at(hw, T) >= tp * hw + 4 && lgtw_eval_red_at(hw, T) % 2 == 0);
        CHECK(lgtw_eval_sums_at(hw, T) == lgtw_eval_red_at(hw, T) + 2 * (LG_EVAL_THREADS / 64));
        CHECK(lgtw_eval_cnt_at(hw, T) == lgtw_eval_sums_at(hw, T) + 2 * T * LGT_EVAL_GROUPS);
      }
    }
  }
  // at T = 128 the chain sums take 64 KiB of the 160 and the interleaved carve no longer fits; what is left holds 128 ranks
  CHECK(lgti_eval_lds_floats(0, 128) > LGT_LDS_FLOATS && lgtw_eval_lds_floats(0, 128) == 4 + 32 + 16384 + 384);
  CHECK(lgtw_eval_hw(1 << 20, LGT_LDS_FLOATS, 128) == 128 && lgtw_eval_hw(1 << 20, LGT_LDS_FLOATS, 103) == 256);
  CHECK(lgtw_eval_hw(1 << 20, LGT_LDS_FLOATS, 33) == 960 && lgtw_eval_hw(1 << 20, LGT_LDS_FLOATS, 1) > 8192);
  CHECK(lgtw_hot(lgti_tp(33)) == 113 && lgtw_hot(lgti_tp(65)) == 60 && lgtw_hot(lgti_tp(103)) == 39 && lgtw_hot(lgti_tp(128)) == 32);   // tests/topics_hard_cases.py: N_HOT
  for (int T : {33, 65, 103, 128}) CHECK(lgtw_eval_hw(600, 63, T) == 0 && lgtw_eval_hw(600, 64, T) == 64 && lgtw_eval_hw(600, 127, T) == 64 && lgtw_eval_hw(600, 128, T) == 128);
}

int main() {
  test_set();
  test_sizes();
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::fprintf(stderr, "all checks passed\n");
  return failures ? 1 : 0;
}
