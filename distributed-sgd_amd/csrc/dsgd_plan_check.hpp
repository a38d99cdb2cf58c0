// A plan's lists against the data that is loaded NOW, and a caller's flat lists before they are kept (pure host C++, no HIP: tests/cpp/plan_check_test.cpp compiles it alone).
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
//
// and the caller's flat lists of n_steps x n_workers workers (dsgd_sync_steps_f64, dsgd_plan_create_rp64_n), before any of it
// is kept:
//
//   flat_lists_check       the offsets start at 0, end at n_idx, never decrease, leave no list empty; every index is a row
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

// What is wrong with flat lists, and where: plain data, the callers word their own messages.  List i is worker i % n_workers
// of step i / n_workers.
enum FlatListsFault {
  FLAT_LISTS_OK = 0,
  FLAT_LISTS_FIRST_OFFSET,   // offsets[0] != 0                                  value: offsets[0]
  FLAT_LISTS_END,            // offsets[n_lists] != n_idx                        value: offsets[n_lists]
  FLAT_LISTS_OFFSETS,        // list `list` ends before it begins or behind idx  value: its end
  FLAT_LISTS_EMPTY,          // list `list` is empty                             value: its begin
  FLAT_LISTS_INDEX,          // idx[pos] is not a row                            value: idx[pos]
};
struct FlatListsCheck {
  FlatListsFault kind = FLAT_LISTS_OK;
  long long list = -1, pos = -1, value = 0;
};

// offsets: n_steps * n_workers + 1 positions into idx (the product fits: the callers refuse an overflow first); n_rows < 0:
// the rows are not known (no data loaded) and the indices are not judged
inline FlatListsCheck flat_lists_check(const int32_t* idx, long long n_idx, const int64_t* offsets, long long n_steps, long long n_workers,
                                       long long n_rows) {
  FlatListsCheck v;
  const long long n_lists = n_steps * n_workers;
  auto bad = [&v](FlatListsFault kind, long long list, long long pos, long long value) {
    v.kind = kind;
    v.list = list;
    v.pos = pos;
    v.value = value;
    return v;
  };
  if (offsets[0] != 0) return bad(FLAT_LISTS_FIRST_OFFSET, 0, 0, offsets[0]);
  if (offsets[n_lists] != n_idx) return bad(FLAT_LISTS_END, n_lists, n_lists, offsets[n_lists]);
  for (long long i = 0; i < n_lists; ++i) {
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] > n_idx) return bad(FLAT_LISTS_OFFSETS, i, i + 1, offsets[i + 1]);
    if (offsets[i + 1] == offsets[i]) return bad(FLAT_LISTS_EMPTY, i, i + 1, offsets[i]);
  }
  const long long t = n_rows < 0 ? -1 : plan_first_outside(idx, n_idx, n_rows);
  if (t >= 0) return bad(FLAT_LISTS_INDEX, -1, t, idx[t]);
  return v;
}
