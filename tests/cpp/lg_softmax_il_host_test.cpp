// csrc/dsgd_lg_softmax_il_host.hpp alone under ASan and UBSan: the refusals with 32 in 128's place; the buckets and their guard
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_lg_softmax_il_host.hpp"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

int main() {
  std::vector<uint8_t> cls(64);
  for (size_t i = 0; i < cls.size(); ++i) cls[i] = (uint8_t)(i % 32);
  for (int C : {-1, 1, 33, 128}) CHECK(lgsi_check_set(C, cls.data(), 64).kind == LGSM_BAD_C);   // (nothing read before C is in range)
  CHECK(lgsi_check_set(33, nullptr, 0).kind == LGSM_BAD_C && lgsi_check_set(0, nullptr, 0).kind == LGSM_OK);
  CHECK(lgsi_check_set(32, cls.data(), 64).kind == LGSM_OK && lgsi_check_set(32, nullptr, 64).kind == LGSM_NULL);
  const LgsmCheck v = lgsi_check_set(31, cls.data(), 64);
  CHECK(lgsi_check_set(32, cls.data(), 0).kind == LGSM_NO_ROWS);
  CHECK(v.kind == LGSM_ENTRY && v.row == 31 && v.value == 31);
  for (int C = LG_SOFTMAX_MIN; C <= LG_SOFTMAX_IL_MAX; ++C) {
    const int tp = lgti_tp(C), nq = lgsi_quads(tp);
    CHECK((nq == 1 || nq == 2 || nq == 4 || nq == 8) && 4 * nq >= tp && (nq == 1 || 2 * nq < tp));   // the smallest bucket that holds TP
    for (int q = 0; q < nq; ++q) CHECK(lgsi_quad_in(nq, q, tp) == (4 * q < tp));
    CHECK(lgtw_group_width(tp) == LG_GROUP);   // the wide form serves the same TP with 16 lanes per row: lgsm_row<16> on both sides
  }
  fprintf(stderr, "all checks passed\n");
  return 0;
}
