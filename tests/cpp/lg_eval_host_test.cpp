// lg_pred_table and lg_pred_owner of csrc/dsgd_lg_host.hpp alone (pure host C++): the ranges-to-workgroups table of
// dsgd_lg_predict_ranges and the bisection its kernel runs over it.  Built with AddressSanitizer and UBSan by
// tests/test_lg_eval_host.py and run as a program of its own.
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

struct Table {
  std::vector<long long> first_block, begin, out_off;   // exactly as long as the function may write: the sanitizer watches the ends
  LgPredTable t;
};
static Table table_of(const std::vector<int64_t>& b, const std::vector<int64_t>& e, int n_cu, long long n_rows = -1) {
  Table T;
  const int K = (int)b.size();
  const int cap = K >= 1 && K <= LG_PRED_MAX_RANGES ? K : 0;   // (a refused count writes nothing)
  T.first_block.assign((size_t)cap + 1, -7);
  T.begin.assign((size_t)cap + 1, -7);   // (one spare word: data() of an empty vector may be null, and null is refused)
  T.out_off.assign((size_t)cap + 1, -7);
  T.t = lg_pred_table(b.data(), e.data(), K, n_cu, n_rows, T.first_block.data(), T.begin.data(), T.out_off.data());
  return T;
}

// every property of a table that was accepted
static void check_table(const std::vector<int64_t>& b, const std::vector<int64_t>& e, int n_cu, const Table& T) {
  const int K = (int)b.size();
  CHECK(T.t.fault == LGP_OK && T.t.n == K);
  CHECK(T.first_block[0] == 0 && T.out_off[0] == 0);
  long long longest = 0, total = 0;
  for (int r = 0; r < K; ++r) {
    const long long rows = e[r] - b[r];
    CHECK(T.begin[r] == b[r]);
    // a run is lg_eval_blocks of its rows, behind the run before it; an empty range has no workgroup and no output
    CHECK(T.first_block[r + 1] - T.first_block[r] == (rows ? lg_eval_blocks(rows, n_cu) : 0));
    CHECK(T.out_off[r + 1] - T.out_off[r] == rows);
    total += rows;
    if (rows > longest) longest = rows;
  }
  CHECK(T.t.grid == T.first_block[K] && T.t.total == total && T.t.total == T.out_off[K] && T.t.longest == longest);
  // the bisection finds the owner of EVERY workgroup, and the owner is never an empty range
  int owner = 0;
  for (long long blk = 0; blk < T.t.grid; ++blk) {
    while (T.first_block[owner + 1] <= blk) ++owner;   // (the linear walk: the first range whose run ends behind blk)
    const int got = lg_pred_owner(T.first_block.data(), K, blk);
    CHECK(got == owner);
    CHECK(e[got] > b[got] && T.first_block[got] <= blk && blk < T.first_block[got + 1]);
  }
}

static void test_single_ranges() {
  for (int n_cu : {1, 2, 256})
    for (long long rows : {1LL, 63LL, 64LL, 65LL, 4095LL, 4096LL, 20000LL, 64LL * 256, 64LL * 256 + 1, 1LL << 20}) {
      const std::vector<int64_t> b = {5}, e = {5 + rows};
      const Table T = table_of(b, e, n_cu);
      CHECK(T.t.fault == LGP_OK && T.t.grid == lg_eval_blocks(rows, n_cu) && T.t.longest == rows && T.t.total == rows);
      check_table(b, e, n_cu, T);
    }
}

static unsigned long long lcg(unsigned long long& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// a few dozen tables of uneven lengths, empty ranges among them (in front, between, at the end), in shuffled order
static void test_many_tables() {
  unsigned long long s = 12345;
  int tables = 0;
  for (int K : {1, 2, 3, 7, 16, 17, 100, 255, 256})
    for (int n_cu : {1, 3, 256})
      for (int variant = 0; variant < 2; ++variant) {
        std::vector<int64_t> b((size_t)K), e((size_t)K);
        long long at = (long long)(lcg(s) % 50);
        for (int r = 0; r < K; ++r) {
          const unsigned long long kind = lcg(s) % 6;
          long long rows = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? 64 + (long long)(lcg(s) % 3) - 1 : kind == 3 ? (long long)(lcg(s) % 700)
                                                                                                       : (long long)(lcg(s) % 30000);
          if (variant == 1 && (r == 0 || r == K - 1)) rows = 0;   // empty ranges at both ends
          if (K == 1 || (variant == 0 && r == K / 2)) rows = rows ? rows : 65;   // (never a table without rows)
          b[(size_t)r] = at;
          e[(size_t)r] = at + rows;
          at += rows + (long long)(lcg(s) % 3);   // (ranges may touch; they never overlap)
        }
        if (K > 2 && variant == 1) {   // two ranges trade places: the order of the ranges is the caller's, not the rows'
          std::swap(b[0], b[(size_t)K - 1]), std::swap(e[0], e[(size_t)K - 1]);
          std::swap(b[1], b[(size_t)K / 2]), std::swap(e[1], e[(size_t)K / 2]);
        }
        long long total = 0;
        for (int r = 0; r < K; ++r) total += e[(size_t)r] - b[(size_t)r];
        const Table T = table_of(b, e, n_cu);
        if (total == 0) {
          CHECK(T.t.fault == LGP_NO_ROWS);
          continue;
        }
        check_table(b, e, n_cu, T);
        ++tables;
      }
  CHECK(tables >= 36);
}

static void test_empty_between() {
  const std::vector<int64_t> b = {0, 100, 100, 300}, e = {100, 100, 165, 300};
  const Table T = table_of(b, e, 256);
  check_table(b, e, 256, T);
  CHECK(T.first_block[1] == 2 && T.first_block[2] == 2 && T.first_block[3] == 4 && T.first_block[4] == 4);
  CHECK(T.out_off[1] == 100 && T.out_off[2] == 100 && T.out_off[3] == 165 && T.out_off[4] == 165);
  CHECK(lg_pred_owner(T.first_block.data(), 4, 1) == 0 && lg_pred_owner(T.first_block.data(), 4, 2) == 2 && lg_pred_owner(T.first_block.data(), 4, 3) == 2);
}

static void test_refusals() {
  {   // 256 ranges are served, 257 refused
    std::vector<int64_t> b(256), e(256);
    for (int r = 0; r < 256; ++r) b[(size_t)r] = 10 * r, e[(size_t)r] = 10 * r + 1 + r % 9;
    Table T = table_of(b, e, 256);
    check_table(b, e, 256, T);
    CHECK(T.t.grid == 256);
    b.push_back(5000), e.push_back(5001);
    T = table_of(b, e, 256);
    CHECK(T.t.fault == LGP_TOO_MANY && T.first_block[0] == -7);   // (nothing written)
  }
  {
    const std::vector<int64_t> b = {0, 9}, e = {5, 7};
    const Table T = table_of(b, e, 4);
    CHECK(T.t.fault == LGP_REVERSED && T.t.range == 1);
  }
  {   // overlaps: partly, one inside the other, the same range twice, far apart in the table
    CHECK(table_of({0, 4}, {5, 9}, 4).t.fault == LGP_OVERLAP);
    CHECK(table_of({0, 2}, {9, 3}, 4).t.fault == LGP_OVERLAP);
    CHECK(table_of({3, 3}, {8, 8}, 4).t.fault == LGP_OVERLAP);
    const Table T = table_of({20, 0, 10, 24}, {25, 5, 15, 30}, 4);
    CHECK(T.t.fault == LGP_OVERLAP && T.t.range == 0 && T.t.other == 3);
    CHECK(table_of({0, 5}, {5, 9}, 4).t.fault == LGP_OK);          // touching is not overlapping
    CHECK(table_of({0, 3, 3}, {9, 3, 3}, 4).t.fault == LGP_OK);    // an empty range lies inside another: it holds no row
  }
  {
    CHECK(table_of({4}, {4}, 4).t.fault == LGP_NO_ROWS);
    CHECK(table_of({4, 0, 9}, {4, 0, 9}, 4).t.fault == LGP_NO_ROWS);
  }
  {   // the loaded rows
    CHECK(table_of({0, 50}, {50, 100}, 4, 100).t.fault == LGP_OK);
    const Table T = table_of({0, 50}, {50, 101}, 4, 100);
    CHECK(T.t.fault == LGP_OUTSIDE && T.t.range == 1);
    CHECK(table_of({-1}, {5}, 4, 100).t.fault == LGP_OUTSIDE);
    CHECK(table_of({0, 200}, {50, 200}, 4, 100).t.fault == LGP_OK);   // an empty range is nowhere
  }
  {   // bad arguments
    const int64_t b[1] = {0}, e[1] = {5};
    long long fb[2], bg[1], oo[2];
    CHECK(lg_pred_table(b, e, 0, 4, -1, fb, bg, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, e, -3, 4, -1, fb, bg, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(nullptr, e, 1, 4, -1, fb, bg, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, nullptr, 1, 4, -1, fb, bg, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, e, 1, 0, -1, fb, bg, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, e, 1, 4, -1, nullptr, bg, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, e, 1, 4, -1, fb, nullptr, oo).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, e, 1, 4, -1, fb, bg, nullptr).fault == LGP_ARGS);
    CHECK(lg_pred_table(b, e, 1, 4, -1, fb, bg, oo).fault == LGP_OK);
  }
}

int main() {
  test_single_ranges();
  test_many_tables();
  test_empty_between();
  test_refusals();
  if (failures) {
    std::fprintf(stderr, "%d checks FAILED\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
