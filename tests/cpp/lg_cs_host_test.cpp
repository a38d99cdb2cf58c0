// csrc/dsgd_lg_cs_host.hpp alone (pure host C++): lg_cs_pick_G on both sides of every limit -- the LDS budget (K = 6 / 7 at
// D + 1 = 47,237, and the last width that fits for every K), dp = 63 / 64, the slice-columns cap, the worker cap -- and the LDS
// words it counts against the carve the kernel uses (lg_cs_lds): every array inside, none overlapping, the 8-byte ones
// aligned.  Built with AddressSanitizer and UBSan by tests/test_lg_cs_host.py and run as a program of its own.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "dsgd_lg_cs_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void test_constants() {
  static_assert(LG_CS_G == 16, "sixteen slices");
  static_assert(lg_cs_sp(47237, 16) == 2956 && lg_cs_sp(64, 16) == 8 && lg_cs_sp(65, 16) == 8, "1 .. 4 columns of padding, whole float4s");
  static_assert(lg_cs_pick_G(47237, 3) == 16 && lg_cs_pick_G(47237, 4) == 16, "the reference's own worker counts are served");
}

static void test_lds_budget() {
  const int dp = 47237;
  for (int K = 1; K <= 6; ++K) CHECK(lg_cs_pick_G(dp, K) == 16);
  CHECK(lg_cs_pick_G(dp, 7) == 0 && lg_cs_pick_G(dp, 8) == 0);
  CHECK(lg_cs_lds_words(dp, 16, 6) <= DSGD_LDS_FLOATS && lg_cs_lds_words(dp, 16, 7) > DSGD_LDS_FLOATS);
  // eight slices would not hold three workers at this width (why the family runs sixteen)
  CHECK(lg_cs_lds_words(dp, 8, 2) <= DSGD_LDS_FLOATS && lg_cs_lds_words(dp, 8, 3) > DSGD_LDS_FLOATS);
  // for every worker count: the widest model that fits, and the first that does not
  for (int K = 1; K <= CS_MAX_K; ++K) {
    int last = 0;
    for (int d = 64; d < 16 * 16000; ++d)
      if (lg_cs_pick_G(d, K)) last = d;
    CHECK(last > 0 && lg_cs_pick_G(last, K) == 16 && lg_cs_pick_G(last + 1, K) == 0);
    CHECK(lg_cs_lds_words(last, 16, K) <= DSGD_LDS_FLOATS && lg_cs_lds_words(last + 1, 16, K) > DSGD_LDS_FLOATS);
    for (int d = last + 1; d < last + 200; ++d) CHECK(lg_cs_pick_G(d, K) == 0);   // (monotone beyond it)
  }
}

static void test_narrow_and_wide() {
  CHECK(lg_cs_pick_G(64, 1) == 16 && lg_cs_pick_G(63, 1) == 0);
  CHECK(lg_cs_pick_G(64, 8) == 16 && lg_cs_pick_G(63, 8) == 0);
  CHECK(lg_cs_pick_G(1, 1) == 0 && lg_cs_pick_G(0, 1) == 0 && lg_cs_pick_G(-5, 1) == 0);
  // the worker cap (slot_meta's field, the builder's limit) and no workers
  CHECK(lg_cs_pick_G(1000, CS_MAX_K) == 16 && lg_cs_pick_G(1000, CS_MAX_K + 1) == 0 && lg_cs_pick_G(1000, 0) == 0 && lg_cs_pick_G(1000, -1) == 0);
  // the slice-columns cap: 16-bit slice-local columns.  LDS gives out long before it on this device, so the cap is asked
  // for itself: at it a width passes the cap's term (and fails on LDS alone), one column beyond it fails the cap's term
  const int at_cap = 16 * LG_CS_MAX_SLICE_COLS;
  CHECK((at_cap + 16 - 1) / 16 == LG_CS_MAX_SLICE_COLS && (at_cap + 1 + 16 - 1) / 16 == LG_CS_MAX_SLICE_COLS + 1);
  CHECK(!lg_cs_fits(at_cap, 16, 1) && lg_cs_lds_words(at_cap, 16, 1) > DSGD_LDS_FLOATS);
  CHECK(!lg_cs_fits(at_cap + 1, 16, 1));
  CHECK(lg_cs_pick_G(at_cap, 1) == 0 && lg_cs_pick_G(at_cap + 1, 1) == 0 && lg_cs_pick_G(INT_MAX, 1) == 0 && lg_cs_pick_G(INT_MAX, 8) == 0);
}

static void test_carve() {
  for (int dp : {64, 65, 100, 4097, 47237, 100000})
    for (int K = 1; K <= CS_MAX_K; ++K) {
      const LgCsLds l = lg_cs_lds(dp, 16, K);
      CHECK(l.sp == lg_cs_sp(dp, 16) && l.sp % 4 == 0 && l.sp > (dp + 15) / 16 && l.sp <= (dp + 15) / 16 + 4);
      // in order, back to back, nothing overlapping: accumulators, weights, slot partials, row dots, label bits, scales, flags
      CHECK(l.acc == 0 && l.w == l.acc + 2 * K * l.sp && l.ps == l.w + l.sp && l.d == l.ps + CS_MAX_SLOTS && l.ymask == l.d + CS_MAX_SLOTS);
      CHECK(l.scale == l.ymask + CS_MAX_SLOTS / 32 && l.red == l.scale + 4 * CS_MAX_K && l.words == l.red + 32);
      CHECK(l.acc % 2 == 0 && l.scale % 2 == 0 && l.w % 4 == 0);   // 8-byte words at even offsets, the float4 copy at a multiple of four
      // what lg_cs_pick_G counts covers what the kernel's carve asks for
      CHECK(lg_cs_lds_words(dp, 16, K) == l.words);
      if (lg_cs_pick_G(dp, K)) CHECK(l.words <= DSGD_LDS_FLOATS);
    }
}

int main() {
  test_constants();
  test_lds_budget();
  test_narrow_and_wide();
  test_carve();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
