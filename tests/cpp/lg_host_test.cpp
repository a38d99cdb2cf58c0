// csrc/dsgd_lg_host.hpp alone (pure host C++): the shift, the grids, and every refusal of the list, range and offset
// validation.  Built with AddressSanitizer and UBSan by tests/test_lg_host.py and run as a program of its own.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_lg_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void test_shift() {
  CHECK(lg_shift(1) == 62);
  CHECK(lg_shift(2) == 61);
  CHECK(lg_shift(3) == 60);
  for (int k = 2; k <= 40; ++k) {
    const long long p = 1LL << k;
    CHECK(lg_shift(p - 1) == 62 - k);
    CHECK(lg_shift(p) == 62 - k);
    CHECK(lg_shift(p + 1) == 62 - k - 1);
    // n entries of magnitude <= 2^S stay inside 2^62
    CHECK(p <= (1LL << (62 - lg_shift(p))));
    CHECK(p + 1 <= (1LL << (62 - lg_shift(p + 1))));
  }
  CHECK(lg_shift(LG_MAX_LIST) == 22);
  static_assert(lg_shift(100) == 55 && lg_shift(4096) == 50 && lg_shift(4097) == 49, "the tests' lists");
}

static void test_grids() {
  CHECK(lg_blocks_per_worker(1, 1, 256, 2) == 1);
  CHECK(lg_blocks_per_worker(16, 1, 256, 2) == 1);
  CHECK(lg_blocks_per_worker(17, 1, 256, 2) == 2);
  CHECK(lg_blocks_per_worker(100, 3, 256, 2) == 7);
  CHECK(lg_blocks_per_worker(65536, 1, 256, 2) == 512);
  CHECK(lg_blocks_per_worker(65536, 3, 256, 2) == 170);
  CHECK(lg_blocks_per_worker(643531, 1, 256, 4) == 1024);
  CHECK(lg_blocks_per_worker(100, 4000, 256, 2) == 1);   // more workers than workgroups: one each
  CHECK(lg_blocks_per_worker(0, 1, 256, 2) == 1);
  CHECK(lg_finish_blocks(1) == 1 && lg_finish_blocks(256) == 1 && lg_finish_blocks(257) == 2 && lg_finish_blocks(47237) == 185);
  CHECK(lg_eval_blocks(1, 256) == 1 && lg_eval_blocks(64, 256) == 1 && lg_eval_blocks(65, 256) == 2);
  CHECK(lg_eval_blocks(4096, 256) == 64 && lg_eval_blocks(1 << 20, 256) == 256);
}

static void test_lists() {
  const long long n_rows = 10;
  std::vector<int32_t> a = {0, 9, 3}, b = {5}, bad_hi = {1, 10}, bad_lo = {2, 2, -1};
  {
    const int32_t* l[2] = {a.data(), b.data()};
    const int64_t n[2] = {3, 1};
    const LgCheck v = lg_check_lists(l, n, 2, n_rows);
    CHECK(v.kind == LG_OK && v.longest == 3 && v.total == 4);
    CHECK(lg_check_lists(l, n, 0, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_lists(nullptr, n, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_lists(l, nullptr, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_lists(l, n, 2, 9).kind == LG_INDEX);   // fewer rows loaded: 9 is outside
  }
  {
    const int32_t* l[2] = {a.data(), b.data()};
    const int64_t n[2] = {3, 0};
    const LgCheck v = lg_check_lists(l, n, 2, n_rows);
    CHECK(v.kind == LG_EMPTY && v.worker == 1);
    const int64_t neg[2] = {-1, 1};
    CHECK(lg_check_lists(l, neg, 2, n_rows).kind == LG_EMPTY);
  }
  {
    const int32_t* l[2] = {a.data(), nullptr};
    const int64_t n[2] = {3, 1};
    const LgCheck v = lg_check_lists(l, n, 2, n_rows);
    CHECK(v.kind == LG_EMPTY && v.worker == 1);
  }
  {
    const int32_t* l[2] = {bad_hi.data(), bad_lo.data()};
    const int64_t n[2] = {2, 3};
    LgCheck v = lg_check_lists(l, n, 2, n_rows);
    CHECK(v.kind == LG_INDEX && v.worker == 0 && v.pos == 1 && v.value == 10);
    const int32_t* l2[2] = {a.data(), bad_lo.data()};
    const int64_t n2[2] = {3, 3};
    v = lg_check_lists(l2, n2, 2, n_rows);
    CHECK(v.kind == LG_INDEX && v.worker == 1 && v.pos == 2 && v.value == -1);
    // an empty list is refused as such even when another list holds a bad index
    const int64_t n3[2] = {2, 0};
    CHECK(lg_check_lists(l, n3, 2, n_rows).kind == LG_EMPTY);
  }
  {
    const int32_t* l[1] = {a.data()};
    const int64_t n[1] = {LG_MAX_LIST + 1};   // (refused before any entry is read)
    CHECK(lg_check_lists(l, n, 1, n_rows).kind == LG_TOO_LONG);
  }
}

static void test_ranges() {
  const long long n_rows = 100;
  {
    const int64_t b[2] = {0, 40}, e[2] = {40, 100};
    const LgCheck v = lg_check_ranges(b, e, 2, n_rows);
    CHECK(v.kind == LG_OK && v.longest == 60 && v.total == 100);
    CHECK(lg_check_ranges(b, e, 0, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_ranges(nullptr, e, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_ranges(b, nullptr, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_ranges(b, e, 2, 99).kind == LG_INDEX);
  }
  {
    const int64_t b[2] = {0, 50}, e[2] = {40, 50};
    const LgCheck v = lg_check_ranges(b, e, 2, n_rows);
    CHECK(v.kind == LG_EMPTY && v.worker == 1);
  }
  {
    const int64_t b[1] = {9}, e[1] = {3};
    CHECK(lg_check_ranges(b, e, 1, n_rows).kind == LG_EMPTY);
  }
  {
    const int64_t b[1] = {-1}, e[1] = {3};
    const LgCheck v = lg_check_ranges(b, e, 1, n_rows);
    CHECK(v.kind == LG_INDEX && v.value == -1);
    const int64_t b2[1] = {99}, e2[1] = {101};
    CHECK(lg_check_ranges(b2, e2, 1, n_rows).kind == LG_INDEX);
    const int64_t b3[1] = {99}, e3[1] = {100};
    CHECK(lg_check_ranges(b3, e3, 1, n_rows).kind == LG_OK);
  }
}

static void test_flat() {
  const long long n_rows = 10;
  std::vector<int32_t> idx = {0, 1, 2, 3, 4, 9};
  {
    const int64_t off[5] = {0, 1, 3, 4, 6};   // 2 steps x 2 workers
    const LgCheck v = lg_check_flat(idx.data(), 6, off, 2, 2, n_rows);
    CHECK(v.kind == LG_OK && v.longest == 2 && v.total == 6);
    CHECK(lg_check_flat(nullptr, 6, off, 2, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_flat(idx.data(), 6, nullptr, 2, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_flat(idx.data(), 6, off, 0, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_flat(idx.data(), 6, off, 2, 0, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_flat(idx.data(), 0, off, 2, 2, n_rows).kind == LG_NO_WORKERS);
    CHECK(lg_check_flat(idx.data(), 6, off, 2, 2, 9).kind == LG_INDEX);
    CHECK(lg_check_flat(idx.data(), 5, off, 2, 2, n_rows).kind == LG_END);
  }
  {
    const int64_t off[5] = {1, 1, 3, 4, 6};
    CHECK(lg_check_flat(idx.data(), 6, off, 2, 2, n_rows).kind == LG_FIRST_OFFSET);
  }
  {
    const int64_t off[5] = {0, 3, 2, 4, 6};
    const LgCheck v = lg_check_flat(idx.data(), 6, off, 2, 2, n_rows);
    CHECK(v.kind == LG_OFFSETS && v.worker == 1);
  }
  {
    const int64_t off[5] = {0, 7, 7, 7, 6};
    CHECK(lg_check_flat(idx.data(), 6, off, 2, 2, n_rows).kind == LG_OFFSETS);
  }
  {
    const int64_t off[5] = {0, 1, 1, 4, 6};
    const LgCheck v = lg_check_flat(idx.data(), 6, off, 2, 2, n_rows);
    CHECK(v.kind == LG_EMPTY && v.worker == 1);
  }
  {
    std::vector<int32_t> bad = {0, 1, -3, 3, 4, 9};
    const int64_t off[5] = {0, 1, 3, 4, 6};
    const LgCheck v = lg_check_flat(bad.data(), 6, off, 2, 2, n_rows);
    CHECK(v.kind == LG_INDEX && v.pos == 2 && v.value == -3);
  }
  {
    const int64_t off[2] = {0, 6};
    CHECK(lg_check_flat(idx.data(), 6, off, INT64_MAX / 2, 4, n_rows).kind == LG_NO_WORKERS);   // n_steps * n_workers overflows
  }
}

int main() {
  test_shift();
  test_grids();
  test_lists();
  test_ranges();
  test_flat();
  if (failures) {
    std::fprintf(stderr, "%d checks FAILED\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
