// csrc/dsgd_lg_softmax_host.hpp alone (pure host C++), under ASan and UBSan by tests/test_lg_softmax_host.py: set checks, planes, carve, refusals.
#include <cstdio>
#include <vector>

#include "dsgd_lg_softmax_host.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static void test_set() {
  const long long n = 10;
  std::vector<uint8_t> cls(n, 0);
  CHECK(lgsm_check_set(0, nullptr, 0).kind == LGSM_OK);                // dropping the classes needs nothing
  for (int bad : {-1, 1, 129, INT32_MAX}) CHECK(lgsm_check_set(bad, nullptr, -5).kind == LGSM_BAD_C);   // C first: nothing else is looked at
  CHECK(lgsm_check_set(5, nullptr, n).kind == LGSM_NULL);              // then the pointer ...
  CHECK(lgsm_check_set(5, cls.data(), 0).kind == LGSM_NO_ROWS);        // ... then the rows ...
  CHECK(lgsm_check_set(LG_SOFTMAX_MIN, cls.data(), n).kind == LGSM_OK && lgsm_check_set(LG_SOFTMAX_MAX, cls.data(), n).kind == LGSM_OK);
  cls[3] = 4, cls[7] = 200;                                            // ... then every byte; the first offender is named
  CHECK(lgsm_check_set(5, cls.data(), 7).kind == LGSM_OK);
  const LgsmCheck v = lgsm_check_set(4, cls.data(), n);
  CHECK(v.kind == LGSM_ENTRY && v.row == 3 && v.value == 4);
  const LgsmCheck u = lgsm_check_set(128, cls.data(), n);
  CHECK(u.kind == LGSM_ENTRY && u.row == 7 && u.value == 200);
  // the planes the wide setter accepts: +1 at the row's class, -1 elsewhere
  cls[7] = 2;
  std::vector<int8_t> planes(5 * n, 0);
  lgsm_one_hot(cls.data(), 5, n, planes.data());
  CHECK(lgtw_check_set(5, planes.data(), n).kind == LGT_OK);
  for (long long i = 0; i < n; ++i)
    for (int c = 0; c < 5; ++c) CHECK(planes[c * n + i] == (cls[i] == c ? 1 : -1));
}

static void test_sizes() {                                             // (lgsm_eval_hw's rule and lgc_plan / lgtc_refusal themselves: the topics' host tests)
  CHECK(lgsm_eval_lds_floats(0, 128) == 4 + 16 + 64 + 2 && lgsm_eval_hw(1 << 20, LGT_LDS_FLOATS, 128) == 256);
  for (int C : {2, 33, 128}) CHECK(lgsm_eval_hw(100, LGT_LDS_FLOATS, C) <= 1024 && lgsm_eval_hw(1 << 20, LGT_LDS_FLOATS, C) >= lgtw_eval_hw(1 << 20, LGT_LDS_FLOATS, C));
  CHECK(lgsm_eval_lds_floats(lgsm_eval_hw(1 << 20, LGT_LDS_FLOATS, 33), 33) <= LGT_LDS_FLOATS && lgsm_eval_red_at(1, 5) % 2 == 0);
  CHECK(LGSM_EVAL_CHAINS == 32 && lgsm_eval_blocks(1, 256) == 1 && lgsm_eval_blocks(33, 256) == 2 && lgsm_eval_blocks(1 << 20, 256) == 256);
  // what dsgd_lg_softmax_sync_steps_ranges refuses before any weight moves, as the call asks: one configuration over each limit
  LgcPlan plan;
  long long base[1];
  const int64_t b1[1] = {0}, e1[1] = {1000}, eb[1] = {(1LL << 31) + 5};
  auto why = [&](const int64_t* re, long long n_ent) {
    const LgcFault f = lgc_plan(b1, re, 1, n_ent, 47237, lgt_acc_stride(47237), 256, &plan, base);
    return lgtc_refusal(f, f == LGC_OK ? lgtc_table_words(plan.positions, 128) : -1);
  };
  CHECK(!why(e1, 75000) && why(e1, 0) && why(e1, 1LL << 31) && why(eb, 75000));   // served; no entries; 2^31 entries; 2^31 rows
  CHECK(lgtc_refusal(LGC_OK, lgtc_table_words((1LL << 30) + 1, 128)) && lgtc_refusal(LGC_KEYS, 0));   // the table beyond 2^37 doubles; the keys
}

int main() {
  test_set();
  test_sizes();
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::fprintf(stderr, "all checks passed\n");
  return failures ? 1 : 0;
}
