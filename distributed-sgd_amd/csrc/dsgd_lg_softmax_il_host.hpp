// The host arithmetic of SOFTMAX regression over few classes, the lanes across the non-zeros (include/dsgd.h "THE LOGISTIC
// MODEL": SOFTMAX, FEW CLASSES; pure C++, no HIP: tests/cpp/lg_softmax_il_host_test.cpp compiles it alone;
// csrc/dsgd_lg_softmax_il.hpp and csrc/dsgd_lg_softmax_il_calls.hpp compile the same numbers).  The layout, the gradient's head
// and grid are the interleaved topics' (csrc/dsgd_lg_topics_il_host.hpp), the evaluation's grid, carve and fold the wide
// softmax's (csrc/dsgd_lg_softmax_host.hpp), all unchanged.
//
//   lgsi_check_set       dsgd_lg_softmax_set_il's arguments: lgsm_check_set's refusals in its order, C up to LG_SOFTMAX_IL_MAX
//   lgsi_quads           the kernels' template argument for TP: the smallest of 1, 2, 4, 8 quads that holds TP / 4
//   lgsi_quad_in         whether quad q of such a kernel lies inside TP (the kernels' guard: nothing beyond a rank's TP words
//                        is ever loaded); known without TP for the quads every TP of the bucket has
#pragma once

#include "dsgd_lg_softmax_host.hpp"

constexpr int LG_SOFTMAX_IL_MAX = LG_TOPICS_IL_MAX;

inline LgsmCheck lgsi_check_set(int32_t C, const uint8_t* cls, long long n_rows) {
  if (C > LG_SOFTMAX_IL_MAX) {
    LgsmCheck v;
    v.kind = LGSM_BAD_C, v.value = C;
    return v;
  }
  return lgsm_check_set(C, cls, n_rows);
}

// The reduce-scatter that brings the lanes' partial sums into the wide placement halves the classes a lane holds at every step:
// it runs over a power of two of them.  TP = 4, 8, 16, 32 fill their bucket; TP = 12 runs in the bucket of 16 and TP = 20, 24, 28
// in the bucket of 32, their missing quads never loaded (sums of nothing: +0.0f, in lanes that own no class).
LG_HD constexpr int lgsi_quads(int tp) { return tp <= 4 ? 1 : (tp <= 8 ? 2 : (tp <= 16 ? 4 : 8)); }
// a bucket of NQ quads serves NQ / 2 < TP / 4 <= NQ: its first NQ / 2 + 1 quads are inside every such TP
LG_HD constexpr bool lgsi_quad_in(int nq, int q, int tp) { return q <= nq / 2 || 4 * q < tp; }
