// Stand-alone host program over csrc/dsgd_lg_gather.hpp (plain C++, no HIP): the offsets of the agreement record, the header
// block and the slots of the logistic model's buffer across ranks, that no two blocks overlap, that a step's message does not
// depend on the buffer's capacity, and the judgement of an agreement record.  tests/test_logistic_ranks_abi.py compiles it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsgd_lg_gather.hpp"
#include "dsgd_lg_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

// every word of the buffer is claimed by exactly one of: a rank's record words, a header word, a slot's column, padding
static void layout(int world, int cap, int dp) {
  const long long total = lgg_total_words(world, cap, dp);
  const long long stride = lgg_stride(dp);
  std::vector<int> owner((size_t)total, 0);   // 0: padding
  CHECK(stride % 64 == 0 && stride >= dp && stride - dp < 64);
  for (int r = 0; r < world; ++r)
    for (int h = 0; h < LGG_REC_WORDS; ++h) {
      const long long at = lgg_record_at(r) + h;
      CHECK(at >= 0 && at < lgg_record_words(world));
      CHECK(owner[(size_t)at] == 0);
      owner[(size_t)at] = 1;
    }
  CHECK(lgg_header_at(world) == lgg_record_words(world) && lgg_header_at(world) % 64 == 0);
  for (int g = 0; g < cap; ++g) {
    const long long at = lgg_step_header_at(world, cap, cap) + g;
    CHECK(at >= lgg_header_at(world) && at < lgg_slots_at(world, cap));
    CHECK(owner[(size_t)at] == 0);
    owner[(size_t)at] = 2;
  }
  CHECK(lgg_slots_at(world, cap) % 64 == 0);
  for (int g = 0; g < cap; ++g) {
    CHECK(lgg_slot_at(world, cap, dp, g) == lgg_slots_at(world, cap) + (long long)g * stride);
    for (int j = 0; j < dp; j += (dp > 4096 ? 997 : 1)) {
      const long long at = lgg_slot_at(world, cap, dp, g) + j;
      CHECK(at < total);
      CHECK(owner[(size_t)at] == 0);
      owner[(size_t)at] = 3;
    }
    const long long last = lgg_slot_at(world, cap, dp, g) + dp - 1;   // the last column stays inside its slot
    CHECK(last < lgg_slot_at(world, cap, dp, g + 1) && last < total);
  }
  CHECK(lgg_slot_at(world, cap, dp, cap) == total);
  // a step of K <= cap workers: its header words end where the slots start, and the run [header, slot K) depends on K and dp alone
  for (long long K = 1; K <= cap; ++K) {
    const long long h = lgg_step_header_at(world, cap, K);
    CHECK(h >= lgg_header_at(world));
    CHECK(h + lgg_pad64(K) == lgg_slots_at(world, cap));
    CHECK(lgg_step_words(dp, K) == lgg_slot_at(world, cap, dp, K) - h);
    CHECK(h + lgg_step_words(dp, K) <= total);
    CHECK(lgg_step_words(dp, K) == lgg_slot_at(world, cap + 64, dp, K) - lgg_step_header_at(world, cap + 64, K));   // (another capacity)
    CHECK(lgg_messages(lgg_step_words(dp, K)) * LGG_MSG_WORDS >= lgg_step_words(dp, K));
    CHECK((lgg_messages(lgg_step_words(dp, K)) - 1) * LGG_MSG_WORDS < lgg_step_words(dp, K));
  }
}

static void workers() {
  // rank-major: the K = k * world global workers are each hit once
  for (int world : {1, 2, 3, 64})
    for (int k : {1, 3, 5}) {
      std::vector<int> seen((size_t)(k * world), 0);
      for (int r = 0; r < world; ++r)
        for (int j = 0; j < k; ++j) {
          const long long g = lgg_global_worker(r, k, j);
          CHECK(g >= 0 && g < (long long)k * world);
          seen[(size_t)g]++;
        }
      for (int s : seen) CHECK(s == 1);
      CHECK(lgg_global_worker(1 % world, k, 0) == (world > 1 ? k : 0));
    }
}

static std::vector<long long> record(int world, const long long* k, const long long* steps, const long long* vexp) {
  // what the all-reduce leaves: every rank's words in its own position (sum of one value and zeros)
  std::vector<long long> rec((size_t)lgg_record_words(world), 0);
  for (int r = 0; r < world; ++r) {
    rec[(size_t)lgg_record_at(r) + LGG_REC_K] += k[r];
    rec[(size_t)lgg_record_at(r) + LGG_REC_STEPS] += steps[r];
    rec[(size_t)lgg_record_at(r) + LGG_REC_VEXP] += vexp[r];
  }
  return rec;
}

static void judgement() {
  {
    const long long k[3] = {3, 3, 3}, steps[3] = {5, 5, 5}, vexp[3] = {-2, 4, 0};
    const auto rec = record(3, k, steps, vexp);
    for (int self = 0; self < 3; ++self) {
      const LggVerdict v = lgg_judge(rec.data(), 3, self);
      CHECK(v.fault == LGG_OK && v.vexp == 4);   // the maximum, whoever asks
    }
  }
  {
    const long long k[2] = {1, 1}, steps[2] = {1, 1}, vexp[2] = {-30, -31};   // (negative exponents: the maximum, not the magnitude)
    const auto rec = record(2, k, steps, vexp);
    CHECK(lgg_judge(rec.data(), 2, 0).vexp == -30 && lgg_judge(rec.data(), 2, 1).vexp == -30);
  }
  {
    const long long k[2] = {1, 2}, steps[2] = {1, 1}, vexp[2] = {0, 0};
    const auto rec = record(2, k, steps, vexp);
    const LggVerdict a = lgg_judge(rec.data(), 2, 0), b = lgg_judge(rec.data(), 2, 1);
    CHECK(a.fault == LGG_K_DIFFERS && a.bad_rank == 1 && a.theirs == 2);
    CHECK(b.fault == LGG_K_DIFFERS && b.bad_rank == 0 && b.theirs == 1);   // EVERY rank sees the mismatch
  }
  {
    const long long k[3] = {2, 2, 2}, steps[3] = {5, 5, 4}, vexp[3] = {1, 1, 1};
    const auto rec = record(3, k, steps, vexp);
    for (int self = 0; self < 3; ++self) CHECK(lgg_judge(rec.data(), 3, self).fault == LGG_STEPS_DIFFER);
    CHECK(lgg_judge(rec.data(), 3, 0).bad_rank == 2 && lgg_judge(rec.data(), 3, 0).theirs == 4);
    CHECK(lgg_judge(rec.data(), 3, 2).bad_rank == 0 && lgg_judge(rec.data(), 3, 2).theirs == 5);
  }
  {
    const long long k[1] = {7}, steps[1] = {0}, vexp[1] = {10};   // world = 1, an empty run
    const auto rec = record(1, k, steps, vexp);
    const LggVerdict v = lgg_judge(rec.data(), 1, 0);
    CHECK(v.fault == LGG_OK && v.vexp == 10);
  }
}

int main() {
  // dp = 0, 1, 62 and 63 (mod 64), narrow and at RCV1's width (47,237 = 738 * 64 + 5 is none of them: 47,232 + r)
  for (int dp : {64, 1, 62, 63, 128, 65, 126, 127, 47232, 47233, 47294, 47295, 47237})
    for (int world : {1, 2, 64})
      for (int cap : {4, 6, 64, 65, 192}) layout(world, cap, dp);
  CHECK(lgg_stride(64) == 64 && lgg_stride(1) == 64 && lgg_stride(62) == 64 && lgg_stride(63) == 64 && lgg_stride(65) == 128);
  CHECK(LGG_MAX_WORLD * LGG_REC_WORDS <= lgg_record_words(LGG_MAX_WORLD));
  CHECK(LGG_MSG_WORDS * 8 == (1 << 20));
  CHECK(lgg_stride(47237) == (((long long)47237 + 63) & ~63LL));   // the stride the column-list layouts were built with
  workers();
  judgement();
  CHECK(lg_shift(1) == 62 && lg_shift(4096) == 50);   // (the header words' meaning: a worker's n gives its shift)
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
