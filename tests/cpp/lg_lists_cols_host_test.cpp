// csrc/dsgd_lg_lists_cols_host.hpp alone, as a program of its own (tests/test_lg_lists_cols_host.py builds it under ASan and UBSan):
// the owner word at its limits, the repeat check, the route at every limit.
#include "dsgd_lg_lists_cols_host.hpp"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(x) \
  if (!(x)) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x), ++failures

int main() {
  // the owner word: round trips at the limits, and never LGL_NONE
  const int workers[] = {0, 1, LGL_MAX_WORKERS - 1};
  const long long positions[] = {0, 1, LGL_MAX_POS / 2, LGL_MAX_POS - 1};
  for (int k : workers)
    for (long long p : positions) {
      const unsigned int w = lgl_pack(k, p);
      CHECK(lgl_worker(w) == k && lgl_pos(w) == p && w != LGL_NONE);
    }
  CHECK(lgl_worker(LGL_NONE) == LGL_MAX_WORKERS);   // what no worker of a served step compares equal to
  CHECK(LGL_MAX_POS == 1LL << 24 && LGL_MAX_WORKERS == 255);

  // the repeat check: none, one inside a list, one across lists (the lists of a step lie one behind the other); the bitmap
  // comes back clear, so the next step starts fresh
  const long long n_rows = 200;
  std::vector<uint64_t> seen((size_t)lgl_seen_words(n_rows), 0);
  CHECK(lgl_seen_words(64) == 1 && lgl_seen_words(65) == 2 && seen.size() == 4);
  auto clear = [&] {
    for (uint64_t w : seen)
      if (w) return false;
    return true;
  };
  const int32_t none[] = {0, 63, 64, 199, 5, 128};
  const int32_t inside[] = {7, 9, 7, 130, 131, 132};    // lists [0, 3) and [3, 6): 7 twice in the first
  const int32_t across[] = {7, 9, 11, 130, 9, 132};     // 9 in both
  CHECK(!lgl_step_repeats(none, 0, 6, seen.data()) && clear());
  CHECK(lgl_step_repeats(inside, 0, 6, seen.data()) && clear());
  CHECK(lgl_step_repeats(across, 0, 6, seen.data()) && clear());
  CHECK(!lgl_step_repeats(across, 0, 4, seen.data()) && clear());   // (a window without the second 9)
  CHECK(!lgl_step_repeats(inside, 1, 6, seen.data()) && clear());   // (the same row in TWO steps is no repeat)
  CHECK(!lgl_step_repeats(none, 3, 3, seen.data()) && clear());     // (no rows)

  // the route at each limit
  CHECK(lgl_route(1, 1, false, true) == LGL_COLS);
  CHECK(lgl_route(LGL_MAX_POS - 1, LGL_MAX_WORKERS, false, true) == LGL_COLS);
  CHECK(lgl_route(LGL_MAX_POS, 1, false, true) == LGL_LISTS_POSITIONS);
  CHECK(lgl_route(1, LGL_MAX_WORKERS + 1, false, true) == LGL_LISTS_WORKERS);
  CHECK(lgl_route(2, 1, true, true) == LGL_LISTS_REPEAT);
  CHECK(lgl_route(1, 1, false, false) == LGL_LISTS_NO_LAYOUT);
  CHECK(lgl_route(LGL_MAX_POS, LGL_MAX_WORKERS + 1, true, false) == LGL_LISTS_NO_LAYOUT);
  // the mark grid: one lane per row of the longest list, capped, never empty
  CHECK(lgl_mark_blocks(257, 1, 256) == 2 && lgl_mark_blocks(0, 3, 0) == 1 && lgl_mark_blocks(1LL << 30, 4, 256) == 512);

  if (failures) return 1;
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
