// The logistic model's column slices (csrc/dsgd_lg_cs.hpp): how many slices serve a model of dp columns and K hosted workers,
// and where a slice's workgroup keeps what in LDS.  Pure C++, no HIP: tests/cpp/lg_cs_host_test.cpp compiles it alone, the
// kernel and csrc/dsgd_lg_calls.hpp compile the same numbers.
//
// A slice holds, per column, the weight (one word) and one int64 accumulator per hosted worker (two words): 1 + 2 K words,
// beside the scratch of a step -- against the SVM's 2 + K (csrc/dsgd_limits.hpp: cs_lds_words).  With dp = 47,237 eight slices
// do not fit three workers; sixteen serve six.  The logistic family therefore always runs LG_CS_G = 16 slices, or declines:
//   lg_cs_pick_G(dp, K)   16, or 0 = none: the plan keeps the two-launch row form (plan code 7)
// bounded by DSGD_LDS_FLOATS (the words of lg_cs_lds), dp >= 4 G (no slice without columns to spare), LG_CS_MAX_SLICE_COLS
// (16-bit slice-local columns) and CS_MAX_K (slot_meta's worker field, the builder's limit).
#pragma once

#include "dsgd_limits.hpp"

constexpr int LG_CS_G = 16;                     // = CS_MAX_G (static_assert in csrc/dsgd_lg_cs.hpp)
constexpr int LG_CS_MAX_SLICE_COLS = 65536;     // = CS_MAX_SLICE_COLS (csrc/dsgd_route.hpp; static_assert in csrc/dsgd_hip.hip)

// padded columns of a slice, as dsgd_cs_slice_kernel lays the weights out (csrc/dsgd_cs.hpp: 1 .. 4 columns of padding)
DSGD_HD constexpr int lg_cs_sp(int dp, int G) { return (((dp + G - 1) / G) + 4) & ~3; }

// The carve of a slice's LDS, in 32-bit words from the (16-byte aligned) base.  The int64 accumulators come first and the
// doubles sit at even offsets: every 8-byte access is naturally aligned.
struct LgCsLds {
  int sp;        // padded columns
  int acc;       // [K][sp] int64: a worker's fixed-point column sums, zero between steps
  int w;         // [sp] float: the slice's weights
  int ps;        // [CS_MAX_SLOTS] float: partial x.w per slot
  int d;         // [CS_MAX_SLOTS] float: x.w per row of the step, the G partials added in slice order
  int ymask;     // [CS_MAX_SLOTS / 32] bit r: the label of row r is +1
  int scale;     // [2][CS_MAX_K] double: 2^(S_k - vexp), then 2^(vexp - S_k), of the step's workers
  int red;       // [32]: [17] the step's "given up" flag
  int words;     // all of it
};
DSGD_HD constexpr LgCsLds lg_cs_lds(int dp, int G, int K) {
  LgCsLds l{};
  l.sp = lg_cs_sp(dp, G);
  l.acc = 0;
  l.w = 2 * K * l.sp;
  l.ps = l.w + l.sp;
  l.d = l.ps + CS_MAX_SLOTS;
  l.ymask = l.d + CS_MAX_SLOTS;
  l.scale = l.ymask + CS_MAX_SLOTS / 32;
  l.red = l.scale + 2 * 2 * CS_MAX_K;
  l.words = l.red + 32;
  return l;
}
// the words lg_cs_pick_G counts: (1 + 2 K) per padded column, the row and exchange scratch
DSGD_HD constexpr int lg_cs_lds_words(int dp, int G, int K) { return (1 + 2 * K) * lg_cs_sp(dp, G) + 2 * CS_MAX_SLOTS + CS_MAX_SLOTS / 32 + 4 * CS_MAX_K + 32; }

DSGD_HD constexpr bool lg_cs_fits(int dp, int G, int K) {
  // (the slice-columns cap first, in 64 bits: behind it nothing below leaves 32 bits)
  return K >= 1 && K <= CS_MAX_K && dp >= 4 * G && ((long long)dp + G - 1) / G <= LG_CS_MAX_SLICE_COLS &&
         lg_cs_lds_words(dp, G, K) <= DSGD_LDS_FLOATS;
}
DSGD_HD constexpr int lg_cs_pick_G(int dp, int K) { return (dp >= 1 && lg_cs_fits(dp, LG_CS_G, K)) ? LG_CS_G : 0; }
