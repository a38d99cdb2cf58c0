// The host arithmetic behind logistic plans and the several-ranges evaluation, on the CPU: the ranges-to-workgroups table of
// dsgd_lg_loss_acc_ranges (csrc/dsgd_lg_host.hpp: lg_eval_table) and the plan-info code of a logistic plan
// (csrc/dsgd_route.hpp).  Built with AddressSanitizer and UBSan by tests/test_lg_plan_host.py and run as a program of its own.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_lg_host.hpp"
#include "dsgd_route.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// every range's run of workgroups is lg_eval_blocks of its rows, the runs are contiguous, disjoint and in the ranges' order,
// and the grid is their sum
static void check_table(const std::vector<int64_t>& b, const std::vector<int64_t>& e, int n_cu) {
  LgEvalTable t;
  const int n = (int)b.size();
  CHECK(lg_eval_table(b.data(), e.data(), n, n_cu, &t));
  CHECK(t.n == n);
  int at = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(t.r[i].row_begin == b[(size_t)i] && t.r[i].row_end == e[(size_t)i]);
    CHECK(t.r[i].first_block == at);
    CHECK(t.r[i].n_blocks == lg_eval_blocks(e[(size_t)i] - b[(size_t)i], n_cu));
    CHECK(t.r[i].n_blocks >= 1 && t.r[i].n_blocks <= n_cu);
    at += t.r[i].n_blocks;
  }
  CHECK(t.grid == at);
  for (int i = n; i < LG_MAX_RANGES; ++i) CHECK(t.r[i].n_blocks == 0 && t.r[i].row_begin == 0 && t.r[i].row_end == 0);
}

static void test_table() {
  static_assert(LG_MAX_RANGES == 16 && LG_EVAL_THREADS / LG_GROUP == 64, "16 ranges; 64 rows per pass of a 1,024-lane workgroup");
  for (int n_cu : {1, 256}) {
    const long long full = 64LL * n_cu;
    const long long sizes[5] = {1, 64, 65, full, full + 1};
    // one range of every size
    for (long long s : sizes) check_table({7}, {7 + s}, n_cu);
    // the block counts themselves
    LgEvalTable t;
    const int64_t b5[5] = {0, 0, 0, 0, 0}, e5[5] = {1, 64, 65, full, full + 1};
    CHECK(lg_eval_table(b5, e5, 5, n_cu, &t));
    CHECK(t.r[0].n_blocks == 1 && t.r[1].n_blocks == 1);
    CHECK(t.r[2].n_blocks == (n_cu == 1 ? 1 : 2));
    CHECK(t.r[3].n_blocks == n_cu && t.r[4].n_blocks == n_cu);   // (capped: the persistent loop takes a second pass)
    // 16 ranges: every size, overlapping and repeated ranges among them
    std::vector<int64_t> b, e;
    for (int i = 0; i < LG_MAX_RANGES; ++i) {
      b.push_back(i % 3);
      e.push_back(i % 3 + sizes[i % 5]);
    }
    check_table(b, e, n_cu);
    CHECK(lg_eval_table(b.data(), e.data(), 16, n_cu, &t) && t.grid <= 16 * n_cu);
    // 17 are refused, as are none, null tables and no compute unit
    b.push_back(0);
    e.push_back(1);
    CHECK(!lg_eval_table(b.data(), e.data(), 17, n_cu, &t));
    CHECK(!lg_eval_table(b.data(), e.data(), 0, n_cu, &t));
    CHECK(!lg_eval_table(nullptr, e.data(), 1, n_cu, &t));
    CHECK(!lg_eval_table(b.data(), nullptr, 1, n_cu, &t));
    CHECK(!lg_eval_table(b.data(), e.data(), 1, n_cu, nullptr));
  }
  const int64_t b[1] = {0}, e[1] = {1};
  LgEvalTable t;
  CHECK(!lg_eval_table(b, e, 1, 0, &t));
  // the same range twice: two runs of the same length, one behind the other
  const int64_t b2[2] = {10, 10}, e2[2] = {210, 210};
  CHECK(lg_eval_table(b2, e2, 2, 256, &t));
  CHECK(t.r[0].n_blocks == 4 && t.r[1].n_blocks == 4 && t.r[1].first_block == 4 && t.grid == 8);
}

static void test_plan_code() {
  const Knobs k{};
  RouteFacts f{};
  PlanFacts p;
  p.lg = true;
  CHECK(route_plan(k, f, p) == PLAN_LG);
  // whatever else is known of the plan or the context: the model decides
  p.cs_current = p.fits_here = p.vt_current = true;
  p.max_step_rows = 300;
  p.n_workers = 1;
  CHECK(route_plan(k, f, p) == PLAN_LG);
  CHECK(plan_info_code(PLAN_LG, false) == 7 && plan_info_code(PLAN_LG, true) == 7);
  // ... and a logistic plan lays nothing out at its creation (the callers pass rp64 || lg)
  CHECK(!plan_lays_out_at_creation(k, f, true, true, true));
  // the codes of the other kinds stay
  CHECK(plan_info_code(PLAN_RP64, false) == 6 && plan_info_code(PLAN_CS64, false) == 5 && plan_info_code(PLAN_CS, false) == 1);
  CHECK(plan_info_code(PLAN_ONE_WG, false) == 2 && plan_info_code(PLAN_VT, false) == 3);
  CHECK(plan_info_code(PLAN_ROWWISE, false) == 0 && plan_info_code(PLAN_ROWWISE, true) == 4);
  p.lg = false;
  p.rp64 = true;
  CHECK(route_plan(k, f, p) == PLAN_RP64);
}

int main() {
  test_table();
  test_plan_code();
  if (failures) {
    std::fprintf(stderr, "%d checks FAILED\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
