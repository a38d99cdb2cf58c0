// The limits of the kernel families that the host's choice of a family depends on (csrc/dsgd_route.hpp) and the kernels
// themselves are written for: LDS budgets, the column slices' and the column lists' capacities.  No HIP type and no library
// call, like csrc/dsgd_layout_types.hpp: the kernel headers, the route header and a host test (tests/test_route.py) compile
// the same numbers.
#pragma once

#include "dsgd_layout_types.hpp"

#ifdef __HIPCC__
#define DSGD_HD __host__ __device__
#else
#define DSGD_HD
#endif

#define DSGD_LDS_FLOATS 40960  // 160 KiB / 4

// the split streams: the most hot ranks a workgroup holds (2 * hsplit words of LDS beside the waves' strips; < 65536: 16-bit ranks)
constexpr int HSPLIT_MAX = (DSGD_LDS_FLOATS - 16 * WS_COEF_STRIDE - 4 - 64) / 2;
// the cold tile walk (csrc/dsgd_kernels.hpp)
constexpr int CT_STRIP = 256;        // floats per wave: [0, CT_MAXROWS + 2) by local row, [192, 256) per-lane dummy slots

// column slices (csrc/dsgd_cs.hpp)
constexpr int CS_THREADS_NARROW = 256;   // (tuning runs: DSGD_CS_NT=256)
constexpr int CS_MAX_K = 8;         // hosted workers
constexpr int CS_MAX_SLOTS = 1024;   // per (step, slice); also the most rows of a step

DSGD_HD constexpr int cs_lds_words(int dp, int G, int K) {
  return (2 + K) * ((((dp + G - 1) / G) + 4) & ~3) + 2 * CS_MAX_SLOTS + 32;   // (a slice is padded by 1 .. 4 columns)
}

// a per-request launch: the builder's scratch sits where the accumulators, partial dots and coefficients go afterwards
DSGD_HD constexpr int cs_req_lds_words(int dp, int G, int K) {
  const int sp = (((dp + G - 1) / G) + 4) & ~3;
  const int rest = K * sp + 2 * CS_MAX_SLOTS;
  return 2 * sp + (rest > 7000 ? rest : 7000) + 32;   // 7000 >= CS_BUILD_WORDS (static_assert in csrc/dsgd_cs.hpp)
}

// column lists (csrc/dsgd_tcol.hpp)
constexpr int TC_MAX_SHARE = 8192;       // entries per workgroup of the gradient kernel: 64 KB of LDS for its 64-bit table
constexpr int TC_DC_BITS = 13;           // packed entry: relative column (< TC_MAX_SHARE) below, bit of the row above
constexpr int TC_MAX_BITS = 1 << (32 - TC_DC_BITS);   // 524,288 bits of bitmap (every worker's range padded to 64 rows)

// the fp64 row-parallel family (csrc/dsgd_rp64.hpp)
constexpr bool RP64_FUSED_DEFAULT = false;   // (DSGD_RP64_FUSED=1 selects the fused form: not measured yet)
