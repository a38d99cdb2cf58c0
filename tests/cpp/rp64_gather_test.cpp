// csrc/dsgd_rp64_gather.hpp on its own, on the CPU: the layout of the fp64 mode's gather slots (one plane per word of a column
// sum) and the rank word's encoding, checked at compile time and again at run time.  Built and run directly by
// tests/test_fp64v_comm_abi.py.
#include <cstdio>

#include "dsgd_rp64_gather.hpp"

static int g_bad = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);           \
      ++g_bad;                                                          \
    }                                                                   \
  } while (0)

// the layout of a slot of `words` planes at one dp
static void check_slot(int dp, int words) {
  const long long stride = rp64_gather_stride(dp), slot = rp64_gather_slot_words(dp, words);
  CHECK(stride % 64 == 0 && stride >= (long long)dp + RP64_HDR_WORDS && stride < (long long)dp + RP64_HDR_WORDS + 64);
  CHECK(slot == stride * words);
  for (int i = 0; i < words; ++i) {
    const long long at = rp64_gather_plane(dp, i);
    CHECK(at == stride * i);
    // the plane's sums [0, dp) and its header positions lie inside the slot ...
    for (int h = 0; h < RP64_HDR_WORDS; ++h) {
      const long long w = at + rp64_gather_header(dp, h);
      CHECK(w >= at + dp && w < at + stride && w < slot);
    }
    // ... and in front of the next plane: the planes do not overlap
    if (i + 1 < words) CHECK(at + rp64_gather_header(dp, RP64_HDR_WORDS - 1) < rp64_gather_plane(dp, i + 1));
  }
  // the kernels' addressing: acc[i] + k * acc_stride with acc[1] = acc[0] + stride, acc_stride = the slot
  for (long long k = 0; k < 3; ++k)
    for (int i = 0; i < words; ++i) {
      const long long first = rp64_gather_plane(dp, i) + k * slot, last = first + dp - 1;
      CHECK(first >= k * slot && last < (k + 1) * slot);
      if (i == 0) CHECK(first + rp64_gather_header(dp, RP64_HDR_ACTIVE) < k * slot + (words > 1 ? rp64_gather_plane(dp, 1) : slot));
    }
  // a message never leaves its plane
  for (long long off = 0; off < stride; off += RP64_MSG_WORDS) {
    const long long n = RP64_MSG_WORDS < stride - off ? RP64_MSG_WORDS : stride - off;
    CHECK(n > 0 && off + n <= stride && n * (long long)sizeof(unsigned long long) <= (1LL << 20));
  }
}

static void check_rank_word(int k) {
  for (int v = 0; v < 2; ++v) {
    const unsigned long long w = rp64_rank_word(k, v != 0);
    CHECK(rp64_rank_word_k(w) == k);
    CHECK(rp64_rank_word_v64(w) == (v != 0));
    CHECK((w >> (RP64_RANK_V64_BIT + 1)) == 0ull);
  }
  CHECK(rp64_rank_word(k, false) == (unsigned long long)k);                // float data: the plain count
  CHECK(rp64_rank_word(k, true) != rp64_rank_word(k, false));             // the value type alone is a disagreement
  CHECK(rp64_rank_word(k, true) != rp64_rank_word(k == 1 ? 2 : 1, true)); // ... and so is the count alone
}

// the same at compile time (the helpers are constexpr: the kernels and the host fold them)
static_assert(rp64_gather_stride(1) == 64 && rp64_gather_stride(62) == 64 && rp64_gather_stride(63) == 128, "stride");
static_assert(rp64_gather_stride(47237) == 47296 && rp64_gather_slot_words(47237, 2) == 2 * 47296, "stride at RCV1's D + 1");
static_assert(rp64_gather_plane(63, 1) == 128 && rp64_gather_header(63, RP64_HDR_ACTIVE) == 64, "planes");
static_assert(rp64_rank_word_k(rp64_rank_word(0x7fffffff, true)) == 0x7fffffff && rp64_rank_word_v64(rp64_rank_word(0x7fffffff, true)), "rank word");
static_assert(rp64_rank_word(1, true) == ((1ull << 32) | 1ull), "bit 32");

int main() {
  const int dps[] = {1, 62, 63, 47237};
  for (int dp : dps)
    for (int words = 1; words <= 2; ++words) check_slot(dp, words);
  check_rank_word(1);
  check_rank_word(0x7fffffff);
  if (g_bad) {
    std::fprintf(stderr, "%d checks failed\n", g_bad);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
