// The layout of the logistic model's accumulator buffer (d_lg_acc) and of the words its steps send across ranks (a communicator
// attached with dsgd_comm_init_lg; include/dsgd.h "THE LOGISTIC MODEL -- ACROSS RANKS"): constexpr helpers
// only, shared by the kernels, the host side and a stand-alone host program (tests/cpp/lg_gather_test.cpp compiles this
// header with a plain C++ compiler).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LGG_HD __host__ __device__
#else
#define LGG_HD
#endif

// The buffer for `cap` worker slots in a world of W ranks, 64-bit words, ALL zero between calls:
//   [W * LGG_REC_WORDS, padded to 64]   the agreement record: rank r's words at r * LGG_REC_WORDS -- the hosted workers k of its
//                                       call, the steps of the call and the vexp of its own data (signed)
//   [cap, padded to 64]                 the header block: one length word n per global worker (its shift is lg_shift(n)); the
//                                       finish of a step across ranks cannot read the WorkSegs of a remote rank's workers.  A
//                                       step of K workers uses the LAST lgg_pad64(K) words of the block, so that its header
//                                       words and its slots are one run of words whose length depends on K and dp alone --
//                                       ranks whose buffers have grown to different capacities still send equal messages
//   [cap][stride]                       the slots, stride = lgg_stride(dp) = the context's lg_stride: global worker g's fixed-point
//                                       column sums in rank order.  The column-list layouts bake `worker * stride + column`
//                                       into their cached tables, so the header words are NOT inside the slots.
// Without a communicator W = 1, the record and the header block stay zero and the local workers are the slots 0 .. k - 1.
// Across ranks global worker r * k + j is rank r's worker j: the gradient kernels get the slots' base moved to slot r * k
// (nothing is copied), a rank's own n words go to the step's header positions r * k + j, and ONE in-place
// ncclAllReduce(ncclInt64, ncclSum) from the step's first header word to the end of slot K - 1 is the exact all-gather (every
// word is non-zero on at most one rank).  The messages are cut at LGG_MSG_WORDS.
constexpr int LGG_REC_K = 0, LGG_REC_STEPS = 1, LGG_REC_VEXP = 2, LGG_REC_WORDS = 3;
constexpr int LGG_MAX_WORLD = 64;
constexpr long long LGG_MSG_WORDS = (1LL << 20) / (long long)sizeof(unsigned long long);   // 1 MiB, as RP64_MSG_WORDS

LGG_HD constexpr long long lgg_pad64(long long n) { return (n + 63) & ~63LL; }
LGG_HD constexpr long long lgg_stride(int dp) { return lgg_pad64((long long)dp); }
// where the blocks start, in words from the buffer's first
LGG_HD constexpr long long lgg_record_at(int rank) { return (long long)rank * LGG_REC_WORDS; }
LGG_HD constexpr long long lgg_record_words(int world) { return lgg_pad64((long long)world * LGG_REC_WORDS); }
LGG_HD constexpr long long lgg_header_at(int world) { return lgg_record_words(world); }
LGG_HD constexpr long long lgg_header_words(int cap) { return lgg_pad64((long long)cap); }
LGG_HD constexpr long long lgg_slots_at(int world, int cap) { return lgg_header_at(world) + lgg_header_words(cap); }
LGG_HD constexpr long long lgg_slot_at(int world, int cap, int dp, long long g) { return lgg_slots_at(world, cap) + g * lgg_stride(dp); }
LGG_HD constexpr long long lgg_total_words(int world, int cap, int dp) { return lgg_slot_at(world, cap, dp, cap); }
// global worker of rank `rank`'s hosted worker j when every rank hosts k
LGG_HD constexpr long long lgg_global_worker(int rank, int k, int j) { return (long long)rank * k + j; }
// ONE step of K <= cap workers: where its header words start (they end where the slots start) and the words its all-reduce
// covers, the header words and the first K slots
LGG_HD constexpr long long lgg_step_header_at(int world, int cap, long long K) { return lgg_slots_at(world, cap) - lgg_pad64(K); }
LGG_HD constexpr long long lgg_step_words(int dp, long long K) { return lgg_pad64(K) + K * lgg_stride(dp); }
LGG_HD constexpr long long lgg_messages(long long words) { return (words + LGG_MSG_WORDS - 1) / LGG_MSG_WORDS; }

// The judgement of an agreement record that has been all-reduced: every rank hosts the same k >= 1 and runs the same number of
// steps; the call then runs on the largest vexp.  `bad_rank` is the first rank that differs from rank `self`.
enum LggFault { LGG_OK = 0, LGG_K_DIFFERS, LGG_STEPS_DIFFER };
struct LggVerdict {
  LggFault fault = LGG_OK;
  int bad_rank = -1;
  long long theirs = 0;   // the differing rank's k or steps
  int vexp = 0;           // LGG_OK: the maximum over the ranks
};
inline LggVerdict lgg_judge(const long long* rec, int world, int self) {
  LggVerdict v;
  const long long k = rec[lgg_record_at(self) + LGG_REC_K], steps = rec[lgg_record_at(self) + LGG_REC_STEPS];
  long long vmax = rec[lgg_record_at(self) + LGG_REC_VEXP];
  for (int r = 0; r < world; ++r) {
    const long long* w = rec + lgg_record_at(r);
    if (w[LGG_REC_K] != k) {
      v.fault = LGG_K_DIFFERS;
      v.bad_rank = r;
      v.theirs = w[LGG_REC_K];
      return v;
    }
    if (w[LGG_REC_STEPS] != steps) {
      v.fault = LGG_STEPS_DIFFER;
      v.bad_rank = r;
      v.theirs = w[LGG_REC_STEPS];
      return v;
    }
    if (w[LGG_REC_VEXP] > vmax) vmax = w[LGG_REC_VEXP];
  }
  v.vexp = (int)vmax;
  return v;
}
