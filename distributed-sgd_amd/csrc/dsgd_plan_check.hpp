// A plan's lists against the data that is loaded NOW (pure host C++, no HIP: tests/cpp/plan_check_test.cpp compiles it alone).
//
// A plan (dsgd_plan_create / _from_seed / dsgd_async_plan_create) keeps row indices, and two things derived from the data
// loaded when it was made: "every index is a loaded row" (device-drawn lists are trusted for it: they were drawn inside the
// caller's ranges of THAT data) and "every list fits the staged sub-batch of dsgd_plan_kernel" (summed from THAT data's row
// lengths).  dsgd_load_csr may replace the data under a live plan, with fewer rows or longer ones, so both are asked again
// at the plan's first use after every load (dsgd_hip.hip: plan_revalidate, keyed by the context's load counter):
//
//   plan_first_outside     the first position whose index is not a row of the loaded data (-1: none)
//   plan_list_fits_staged  one list: at most PLAN_STAGE_CAP rows and PLAN_STAGE_CAP work items of PLAN_STAGE_CH non-zeros
//   plan_check_lists       both over all lists of a plan
#pragma once

#include <cstddef>
#include <cstdint>

constexpr int PLAN_STAGE_CAP = 192;   // = PLAN_CAP of csrc/dsgd_batch.hpp (item slots of a staged sub-batch; asserted in dsgd_hip.hip)
constexpr int PLAN_STAGE_CH = 128;    // = BT_CH: non-zeros per work item

inline long long plan_first_outside(const int32_t* idx, long long n, long long n_rows) {
  for (long long t = 0; t < n; ++t)
    if (idx[t] < 0 || (long long)idx[t] >= n_rows) return t;
  return -1;
}

// row_ptr: the n_rows + 1 row starts of the loaded data as the library holds them (an empty row owns one explicit zero); NULL
// (no host copy) answers false, as does any index outside the rows
inline bool plan_list_fits_staged(const long long* row_ptr, long long n_rows, const int32_t* idx, long long n) {
  if (n > PLAN_STAGE_CAP || !row_ptr) return false;
  long long items = 0;
  for (long long t = 0; t < n; ++t) {
    const long long r = idx[t];
    if (r < 0 || r >= n_rows) return false;
    items += (row_ptr[r + 1] - row_ptr[r] + PLAN_STAGE_CH - 1) / PLAN_STAGE_CH;
  }
  return items <= PLAN_STAGE_CAP;
}

struct PlanCheck {
  long long bad_at = -1;   // position in idx of the first index outside [0, n_rows) (-1: every index is a loaded row)
  bool fits = false;       // every list fits the staged sub-batch (false whenever bad_at >= 0)
};

// offsets: n_lists + 1 ascending positions into idx
inline PlanCheck plan_check_lists(const int32_t* idx, const long long* offsets, long long n_lists, const long long* row_ptr, long long n_rows) {
  PlanCheck v;
  v.bad_at = plan_first_outside(idx, n_lists > 0 ? offsets[n_lists] : 0, n_rows);
  if (v.bad_at >= 0) return v;
  v.fits = true;
  for (long long i = 0; i < n_lists && v.fits; ++i)
    v.fits = plan_list_fits_staged(row_ptr, n_rows, idx + offsets[i], offsets[i + 1] - offsets[i]);
  return v;
}
