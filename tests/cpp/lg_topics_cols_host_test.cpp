// csrc/dsgd_lg_topics_cols_host.hpp alone (pure host C++): the lane groups' runs at every (share, group width), the coefficient
// table's words and its refusal, the accumulator word of a slot.  Built with ASan and UBSan by tests/test_lg_topics_cols_host.py.
#include <cstdio>
#include <initializer_list>
#include "dsgd_lg_topics_cols_host.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main() {
  for (int share = LGC_MIN_SHARE; share <= LGC_MAX_SHARE; share += LGC_THREADS) {   // every share lgc_share gives
    for (int gw : {16, 32, 64}) {
      const int run = lgtc_group_entries(share, gw);
      // the groups' runs tile the share, in whole fetches of sixteen; the flag count's lanes divide a run
      CHECK(run * lgtc_groups(gw) == share && run % gw == 0 && run % LG_GROUP == 0 && run >= LG_GROUP);
    }
  }
  CHECK(lgtc_groups(16) == 16 && lgtc_groups(32) == 8 && lgtc_groups(64) == 4 && lgtc_group_entries(256, 16) == 16 && lgtc_group_entries(256, 64) == 64 && lgtc_group_entries(2048, 16) == 128 && lgtc_group_entries(2048, 64) == 512);
  // the table: positions x TP doubles, the limit itself served, beyond it refused without overflow
  CHECK(lgtc_table_words(0, 4) == 0 && lgtc_table_words(23149, 104) == 23149LL * 104 && lgtc_table_words(1LL << 30, 128) == LGTC_MAX_WORDS);
  CHECK(lgtc_table_words((1LL << 30) + 1, 128) == -1 && lgtc_table_words((1LL << 31) - 1, 128) == -1);   // lgc_plan's most positions x 128
  CHECK(lgtc_table_words((1LL << 31) - 1, 64) == ((1LL << 31) - 1) * 64 && lgtc_table_words((1LL << 31) - 1, 4) == ((1LL << 31) - 1) * 4);
  CHECK(lgtc_table_words(1LL << 31, 4) == -1 && lgtc_table_words(-1, 4) == -1);                          // positions lgc_plan would not give
  CHECK(lgtc_refusal(LGC_OK, 5) == nullptr && lgtc_refusal(LGC_OK, -1) && lgtc_refusal(LGC_NO_ENTRIES, 5) && lgtc_refusal(LGC_KEYS, 5));
  CHECK(lgtc_table_words(10, 0) == -1 && lgtc_table_words(10, 6) == -1 && lgtc_table_words(10, 132) == -1);   // TP is lgti_tp's
  // the accumulator word of the layout's slot k * lg_stride + rank
  const unsigned int dp = 47237, lg_stride = 47296;
  for (int tp : {4, 32, 104, 128}) {
    const long long acc_stride = lgti_acc_stride((int)dp, tp);
    CHECK(lgtc_acc_word(0, lg_stride, acc_stride, tp) == 0 && lgtc_acc_word(5, lg_stride, acc_stride, tp) == 5LL * tp);
    CHECK(lgtc_acc_word(3 * lg_stride + dp - 1, lg_stride, acc_stride, tp) == 3 * acc_stride + (long long)(dp - 1) * tp);
    CHECK((long long)dp * tp <= acc_stride);                            // the last rank's topics end inside the worker's words
  }
  const unsigned int wide = 1u << 20;                                   // the largest slot lgc_plan lets through: no 32-bit arithmetic on the way
  CHECK(lgtc_acc_word((1u << 31) - 1, wide, (long long)wide * 128, 128) == 2047LL * wide * 128 + (long long)(wide - 1) * 128);
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::fprintf(stderr, "all checks passed\n");
  return failures ? 1 : 0;
}
