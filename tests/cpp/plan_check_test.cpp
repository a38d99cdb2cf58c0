// csrc/dsgd_plan_check.hpp on its own, on the CPU: the questions a plan is asked again after dsgd_load_csr replaced the data
// under it -- is every index a loaded row, does every list fit the staged sub-batch of the one-workgroup kernel given THESE
// row starts.  Built with -fsanitize=address,undefined and run directly by tests/test_plan_check.py: the row starts live in
// vectors of exactly n_rows + 1 entries, so a check that reads row_ptr[r + 1] for a row that is not loaded is a heap overflow
// the sanitizer reports.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_plan_check.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checks;                                                          \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

// row starts of rows with the given lengths (exactly n + 1 entries on the heap)
static std::vector<long long> starts(const std::vector<long long>& len) {
  std::vector<long long> rp(len.size() + 1, 0);
  for (size_t i = 0; i < len.size(); ++i) rp[i + 1] = rp[i] + len[i];
  return rp;
}
static std::vector<long long> uniform(long long n_rows, long long len) { return starts(std::vector<long long>((size_t)n_rows, len)); }
static PlanCheck check(const std::vector<int32_t>& idx, const std::vector<long long>& off, const std::vector<long long>& rp) {
  return plan_check_lists(idx.data(), off.data(), (long long)off.size() - 1, rp.data(), (long long)rp.size() - 1);
}

int main() {
  const int CAP = PLAN_STAGE_CAP, CH = PLAN_STAGE_CH;
  CHECK(CAP == 192 && CH == 128);   // (the kernel's own: static_assert in dsgd_hip.hip ties them to PLAN_CAP / BT_CH)

  // ---- inside and outside the rows ----
  {
    const std::vector<long long> rp = uniform(10, 3);
    const std::vector<int32_t> in = {0, 9, 4, 4, 0};
    CHECK(plan_first_outside(in.data(), (long long)in.size(), 10) == -1);
    const std::vector<int32_t> hi = {0, 9, 10, 11};
    CHECK(plan_first_outside(hi.data(), (long long)hi.size(), 10) == 2);   // the FIRST one
    const std::vector<int32_t> neg = {3, -1, 12};
    CHECK(plan_first_outside(neg.data(), (long long)neg.size(), 10) == 1);
    const std::vector<int32_t> big = {0x7fffffff};
    CHECK(plan_first_outside(big.data(), 1, 10) == 0);
    CHECK(plan_first_outside(big.data(), 1, 0x80000000LL) == -1);          // (compared as 64-bit: no wrap at 2^31 rows)
    CHECK(plan_list_fits_staged(rp.data(), 10, in.data(), (long long)in.size()));
    CHECK(!plan_list_fits_staged(rp.data(), 10, hi.data(), (long long)hi.size()));   // refused BEFORE row_ptr[11] is read
    CHECK(!plan_list_fits_staged(rp.data(), 10, neg.data(), (long long)neg.size()));
    CHECK(!plan_list_fits_staged(nullptr, 10, in.data(), (long long)in.size()));     // no host copy of the rows
    PlanCheck v = check(hi, {0, 2, 4}, rp);
    CHECK(v.bad_at == 2 && !v.fits);
    v = check(in, {0, 2, 5}, rp);
    CHECK(v.bad_at == -1 && v.fits);
  }

  // ---- the empty and the one-row edges ----
  {
    const std::vector<long long> none = {0};   // no rows loaded
    const std::vector<int32_t> z = {0};
    CHECK(plan_first_outside(z.data(), 1, 0) == 0);
    CHECK(plan_first_outside(z.data(), 0, 0) == -1);       // an empty list holds no bad index
    CHECK(plan_list_fits_staged(none.data(), 0, z.data(), 0));
    CHECK(!plan_list_fits_staged(none.data(), 0, z.data(), 1));
    PlanCheck v = plan_check_lists(z.data(), none.data(), 0, none.data(), 0);   // a plan of no lists
    CHECK(v.bad_at == -1 && v.fits);
    const std::vector<long long> one = starts({1});        // one row (an empty row owns one explicit zero)
    const std::vector<int32_t> rep(CAP, 0);
    CHECK(plan_first_outside(rep.data(), CAP, 1) == -1);
    CHECK(plan_list_fits_staged(one.data(), 1, rep.data(), CAP));   // CAP times the one row: CAP items
    const std::vector<int32_t> second = {0, 1};
    v = check(second, {0, 2}, one);
    CHECK(v.bad_at == 1 && !v.fits);
    const std::vector<long long> zero_len = starts({0});   // (a row of no entries at all: no item)
    CHECK(plan_list_fits_staged(zero_len.data(), 1, rep.data(), CAP));
  }

  // ---- the staged sub-batch: rows and work items at the limit, one below, one above ----
  {
    // rows: CAP rows of one item each fit; CAP + 1 rows never do
    const std::vector<long long> rp = uniform(CAP + 1, CH);
    std::vector<int32_t> idx((size_t)CAP + 1);
    for (int i = 0; i <= CAP; ++i) idx[(size_t)i] = i;
    CHECK(plan_list_fits_staged(rp.data(), CAP + 1, idx.data(), CAP - 1));
    CHECK(plan_list_fits_staged(rp.data(), CAP + 1, idx.data(), CAP));
    CHECK(!plan_list_fits_staged(rp.data(), CAP + 1, idx.data(), CAP + 1));
    // items: 100 rows; row 0 carries what brings the sum to CAP - 1, CAP, CAP + 1 items (the other 99 rows: one item each)
    for (int extra = -1; extra <= 1; ++extra) {
      std::vector<long long> len(100, 1);
      len[0] = (long long)(CAP - 99 + extra) * CH;            // exactly that many items ...
      std::vector<long long> r2 = starts(len);
      std::vector<int32_t> l100(100);
      for (int i = 0; i < 100; ++i) l100[(size_t)i] = i;
      CHECK(plan_list_fits_staged(r2.data(), 100, l100.data(), 100) == (extra <= 0));
      len[0] += 1;                                            // ... and one non-zero more opens one more item
      r2 = starts(len);
      CHECK(plan_list_fits_staged(r2.data(), 100, l100.data(), 100) == (extra < 0));
    }
    // every list of a plan is asked: one list over the limit among lists that fit
    std::vector<long long> len(300, 75);
    len[250] = (long long)CAP * CH;
    const std::vector<long long> r3 = starts(len);
    std::vector<int32_t> all(300);
    for (int i = 0; i < 300; ++i) all[(size_t)i] = i;
    PlanCheck v = check(all, {0, 100, 200, 300}, r3);
    CHECK(v.bad_at == -1 && !v.fits);                         // list 2: 99 + CAP items
    v = check(all, {0, 100, 200}, r3);
    CHECK(v.bad_at == -1 && v.fits);
  }

  // ---- the rows shrink under a plan, grow back, and grow LONGER at the same count ----
  {
    std::vector<int32_t> idx(100);
    for (int i = 0; i < 100; ++i) idx[(size_t)i] = 80 * i + 7;    // reaches row 7,927
    const std::vector<long long> off = {0, 100};
    const std::vector<long long> a = uniform(12000, 75);
    PlanCheck v = check(idx, off, a);
    CHECK(v.bad_at == -1 && v.fits);                              // 100 items
    {
      const std::vector<long long> b = uniform(6000, 150);        // fewer rows: index 75 of the list is 6,007
      v = check(idx, off, b);
      CHECK(v.bad_at == 75 && !v.fits);
      CHECK(idx[(size_t)v.bad_at] == 6007);
    }
    {
      const std::vector<long long> c = uniform(7928, 150);        // just enough rows again; two items per row now: over
      v = check(idx, off, c);
      CHECK(v.bad_at == -1 && !v.fits);
      const std::vector<long long> c1 = uniform(7927, 150);       // one row short
      v = check(idx, off, c1);
      CHECK(v.bad_at == 99);
    }
    v = check(idx, off, a);                                       // the first data again
    CHECK(v.bad_at == -1 && v.fits);
    std::vector<long long> len(12000, 75);                        // the same row count, the listed rows 3,000 entries long
    for (int32_t r : idx) len[(size_t)r] = 3000;
    v = check(idx, off, starts(len));
    CHECK(v.bad_at == -1 && !v.fits);                             // 2,400 items: the stale "fits" was the fault
  }

  // ---- the caller's flat lists of n_steps x n_workers workers (dsgd_sync_steps_f64, dsgd_plan_create_rp64_n) ----
  {
    auto flat = [](const std::vector<int32_t>& idx, const std::vector<int64_t>& off, long long n_steps, long long n_workers, long long n_rows) {
      return flat_lists_check(idx.data(), (long long)idx.size(), off.data(), n_steps, n_workers, n_rows);   // (off: exactly n_lists + 1 entries)
    };
    const std::vector<int32_t> idx = {0, 9, 4, 4, 0, 7};
    const std::vector<int64_t> off = {0, 2, 3, 5, 6};   // two steps of two workers
    FlatListsCheck v = flat(idx, off, 2, 2, 10);
    CHECK(v.kind == FLAT_LISTS_OK && v.list == -1 && v.pos == -1);
    v = flat(idx, {1, 2, 3, 5, 6}, 2, 2, 10);
    CHECK(v.kind == FLAT_LISTS_FIRST_OFFSET && v.value == 1);
    v = flat(idx, {0, 2, 3, 5, 5}, 2, 2, 10);            // the end disagrees with n_idx: judged before any list
    CHECK(v.kind == FLAT_LISTS_END && v.value == 5);
    v = flat(idx, {0, 2, 3, 5, 7}, 2, 2, 10);
    CHECK(v.kind == FLAT_LISTS_END && v.value == 7);
    v = flat(idx, {0, 3, 2, 5, 6}, 2, 2, 10);            // a decreasing offset: list 1 is worker 1 of step 0
    CHECK(v.kind == FLAT_LISTS_OFFSETS && v.list == 1 && v.list / 2 == 0 && v.list % 2 == 1 && v.value == 2);
    v = flat(idx, {0, 2, 9, 5, 6}, 2, 2, 10);            // an offset that leaves idx (idx[9] is never read)
    CHECK(v.kind == FLAT_LISTS_OFFSETS && v.list == 1 && v.value == 9);
    v = flat(idx, {0, 2, 2, 5, 6}, 2, 2, 10);            // an empty list in the middle ...
    CHECK(v.kind == FLAT_LISTS_EMPTY && v.list == 1);
    v = flat(idx, {0, 2, 3, 6, 6}, 2, 2, 10);            // ... and as the last list: worker 1 of step 1
    CHECK(v.kind == FLAT_LISTS_EMPTY && v.list == 3 && v.list / 2 == 1 && v.list % 2 == 1);
    v = flat(idx, {0, 0, 3, 5, 6}, 2, 2, 10);            // ... and as the first
    CHECK(v.kind == FLAT_LISTS_EMPTY && v.list == 0);
    // indices outside the rows, at the first and the last position: -1 and n_rows
    for (const int32_t bad : {-1, 10}) {
      std::vector<int32_t> first = idx, last = idx;
      first.front() = bad;
      last.back() = bad;
      v = flat(first, off, 2, 2, 10);
      CHECK(v.kind == FLAT_LISTS_INDEX && v.pos == 0 && v.value == bad);
      v = flat(last, off, 2, 2, 10);
      CHECK(v.kind == FLAT_LISTS_INDEX && v.pos == 5 && v.value == bad);
      CHECK(flat(first, off, 2, 2, -1).kind == FLAT_LISTS_OK);   // the rows are not known: the indices are not judged
      CHECK(flat(last, off, 2, 2, -1).kind == FLAT_LISTS_OK);
      CHECK(flat(last, off, 2, 2, 11).kind == (bad < 0 ? FLAT_LISTS_INDEX : FLAT_LISTS_OK));   // one row more
    }
    CHECK(flat(idx, {0, 2, 2, 5, 6}, 2, 2, -1).kind == FLAT_LISTS_EMPTY);   // (the offsets are judged either way)
    // no entries at all with one step: the one list is empty (idx may be an empty array: nothing of it is read)
    v = flat({}, {0, 0}, 1, 1, 10);
    CHECK(v.kind == FLAT_LISTS_EMPTY && v.list == 0);
    v = flat({}, {0, 0, 0}, 1, 2, -1);
    CHECK(v.kind == FLAT_LISTS_EMPTY && v.list == 0);
  }

  std::fprintf(stderr, "plan_check_test: all checks passed (%d)\n", g_checks);
  return 0;
}
