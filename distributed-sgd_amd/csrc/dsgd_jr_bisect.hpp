// Which raw value of a shuffle serves its draw m (csrc/dsgd_shuffle.hpp, phase 1 of the two slice kernels).
//
// `rej` holds the raw values rejected inside the shuffle as offsets from its first raw value, ascending.  Rejection i
// happened while draw T_i = rej[i] - i was being served, and T is non-decreasing (rej is strictly ascending), so draw m is
// served by raw offset m + #{i : T_i <= m}: an upper bound over T by bisection, 10 probes for the 512 rejections the job
// form keeps where the linear walk below takes one probe per rejection in front of the draw.
//
// No device type and no library call, so that the kernel and a host test compile the same lines
// (tests/test_seed_job_abi.py compares it with the linear walk on hand-made lists).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSGD_JRB_HD __host__ __device__
#else
#define DSGD_JRB_HD
#endif

DSGD_JRB_HD inline long long dsgd_jr_raw_of_draw_bisect(long long m, const int* rej, int n_rej) {
  int lo = 0, hi = n_rej;   // T_i <= m for every i < lo, T_i > m for every i >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)rej[mid] - (long long)mid <= m) lo = mid + 1;
    else hi = mid;
  }
  return m + (long long)lo;
}
// the linear walk the bisection replaces: what dsgd_jr_slice_kernel calls (at most JR_MAX_REJ = 64 rejections)
DSGD_JRB_HD inline long long dsgd_jr_raw_of_draw_linear(long long m, const int* rej, int n_rej) {
  long long x = m;
  for (int i = 0; i < n_rej; ++i) {
    if ((long long)rej[i] <= x) ++x;
    else break;
  }
  return x;
}
