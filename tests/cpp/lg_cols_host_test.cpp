// csrc/dsgd_lg_cols_host.hpp alone (pure host C++): the share size rule with both sides of its clamps, the padding to whole
// shares, the workers' position bases (K = 1, K = 16, one row), and the decision to decline: 2^31 - 1 positions or entries
// are laid out, 2^31 are not.  Built with AddressSanitizer and UBSan by tests/test_lg_cols_host.py and run as a program of
// its own.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_lg_cols_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void test_constants() {
  static_assert(LGC_THREADS == 4 * 64 && LGC_WAVES == 4, "a wave walks a quarter of a share");
  static_assert(LGC_MAX_SHARE == LGC_THREADS * LGC_NU && LGC_MAX_SHARE % LGC_THREADS == 0 && LGC_MIN_SHARE % LGC_THREADS == 0, "whole rounds");
  static_assert(LGC_MAX_SHARE * 8 * LGC_PER_CU <= 160 * 1024, "eight workgroups' tables fit a compute unit's LDS");
  static_assert(LGC_LIMIT == 2147483648LL, "31-bit positions under the flag");
}

static void test_share() {
  const int cu = 256;   // 2,048 workgroup slots
  CHECK(lgc_share(1, cu) == LGC_MIN_SHARE);
  CHECK(lgc_share(2048LL * 256, cu) == 256);          // the lower clamp's last: 256 entries per slot
  CHECK(lgc_share(2048LL * 256 + 1, cu) == 512);      // one more: the next whole workgroup
  CHECK(lgc_share(2048LL * 1792, cu) == 1792);
  CHECK(lgc_share(2048LL * 1792 + 1, cu) == 2048);
  CHECK(lgc_share(2048LL * 2048, cu) == LGC_MAX_SHARE);       // the upper clamp's first exact fit
  CHECK(lgc_share(2048LL * 2048 + 1, cu) == LGC_MAX_SHARE);   // ... and beyond it
  CHECK(lgc_share(LGC_LIMIT - 1, cu) == LGC_MAX_SHARE);
  CHECK(lgc_share(1400000, cu) == 768);               // about 18,519 RCV1-like rows
  CHECK(lgc_share(48000000, cu) == 2048);             // about RCV1's train split
  CHECK(lgc_share(5000, 1) == 768 && lgc_share(5000, 0) == 768);   // no compute unit reported: one
  for (long long n : {1LL, 255LL, 256LL, 257LL, 100000LL, 7777777LL, LGC_LIMIT - 1}) {
    const int s = lgc_share(n, 304);
    CHECK(s % LGC_THREADS == 0 && s >= LGC_MIN_SHARE && s <= LGC_MAX_SHARE);
  }
}

static void test_plan() {
  LgcPlan p;
  {   // one row, one worker
    const int64_t b[1] = {77}, e[1] = {78};
    long long base[1] = {-1};
    CHECK(lgc_plan(b, e, 1, 75, 47237, 47296, 256, &p, base) == LGC_OK);
    CHECK(base[0] == 0 && p.positions == 1 && p.share == 256 && p.n_shares == 1 && p.n_pad == 256);
    CHECK(lgc_plan(b, e, 1, 0, 47237, 47296, 256, &p, base) == LGC_NO_ENTRIES && p.n_shares == 0);
  }
  {   // padding: whole shares, the last one partly filled or exactly full
    const int64_t b[1] = {0}, e[1] = {4096};
    long long base[1];
    CHECK(lgc_plan(b, e, 1, 256, 100, 128, 256, &p, base) == LGC_OK && p.n_shares == 1 && p.n_pad == 256);
    CHECK(lgc_plan(b, e, 1, 257, 100, 128, 256, &p, base) == LGC_OK && p.n_shares == 2 && p.n_pad == 512);
    CHECK(lgc_plan(b, e, 1, 307200, 47237, 47296, 256, &p, base) == LGC_OK && p.share == 256 && p.n_shares == 1200 && p.n_pad == 307200);
    CHECK(lgc_plan(b, e, 1, 48000001, 47237, 47296, 256, &p, base) == LGC_OK && p.share == 2048 && p.n_shares == 23438 &&
          p.n_pad == 23438LL * 2048 && p.n_pad - 48000001 < 2048);
  }
  {   // K = 16: uneven workers, overlapping ones, a one-row worker; the bases are the rows in front
    int64_t b[16], e[16];
    long long want = 0, base[16];
    std::vector<long long> bases;
    for (int k = 0; k < 16; ++k) {
      b[k] = 10 * k;
      e[k] = b[k] + (k == 5 ? 1 : 100 + k);   // (they overlap: positions are per worker, not per row)
      bases.push_back(want);
      want += e[k] - b[k];
    }
    CHECK(lgc_plan(b, e, 16, 123456, 47237, 47296, 256, &p, base) == LGC_OK && p.positions == want);
    for (int k = 0; k < 16; ++k) CHECK(base[k] == bases[(size_t)k]);
    CHECK(base[6] == base[5] + 1);
  }
  {   // positions: 2^31 - 1 rows are laid out, 2^31 are declined -- in one worker and across two
    long long base[2];
    const int64_t b1[1] = {0}, e_ok[1] = {LGC_LIMIT - 1}, e_no[1] = {LGC_LIMIT};
    CHECK(lgc_plan(b1, e_ok, 1, 1000, 100, 128, 256, &p, base) == LGC_OK && p.positions == LGC_LIMIT - 1);
    CHECK(lgc_plan(b1, e_no, 1, 1000, 100, 128, 256, &p, base) == LGC_POSITIONS && p.n_shares == 0);
    const int64_t b2[2] = {0, 5}, e2_ok[2] = {LGC_LIMIT - 2, 6}, e2_no[2] = {LGC_LIMIT - 2, 7};
    CHECK(lgc_plan(b2, e2_ok, 2, 1000, 100, 128, 256, &p, base) == LGC_OK && base[1] == LGC_LIMIT - 2 && p.positions == LGC_LIMIT - 1);
    CHECK(lgc_plan(b2, e2_no, 2, 1000, 100, 128, 256, &p, base) == LGC_POSITIONS);
    const int64_t bl[2] = {0, 0}, el[2] = {LG_MAX_LIST, LG_MAX_LIST};   // the longest lists lg_check_ranges lets through
    CHECK(lgc_plan(bl, el, 2, 1000, 100, 128, 256, &p, base) == LGC_POSITIONS);
  }
  {   // entries: 2^31 - 1 are laid out, 2^31 are declined
    long long base[1];
    const int64_t b[1] = {0}, e[1] = {1000000};
    CHECK(lgc_plan(b, e, 1, LGC_LIMIT - 1, 100, 128, 256, &p, base) == LGC_OK && p.share == 2048 && p.n_shares == 1048576 &&
          p.n_pad == LGC_LIMIT);
    CHECK(lgc_plan(b, e, 1, LGC_LIMIT, 100, 128, 256, &p, base) == LGC_ENTRIES && p.n_shares == 0);
  }
  {   // keys: workers x columns and workers x stride stay ints
    std::vector<int64_t> b(50000, 0), e(50000, 1);
    std::vector<long long> base(50000);
    CHECK(lgc_plan(b.data(), e.data(), 45405, 1000, 47237, 47296, 256, &p, base.data()) == LGC_OK);
    CHECK(lgc_plan(b.data(), e.data(), 45406, 1000, 47237, 47296, 256, &p, base.data()) == LGC_KEYS);   // 45,406 x 47,296 >= 2^31
    CHECK(lgc_plan(b.data(), e.data(), 50000, 1000, 47237, 47296, 256, &p, base.data()) == LGC_KEYS);
  }
}

int main() {
  test_constants();
  test_share();
  test_plan();
  if (failures) {
    std::fprintf(stderr, "%d checks FAILED\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
