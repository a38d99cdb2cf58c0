// The layout of the fp64 mode's gather buffer across ranks (a communicator attached with dsgd_comm_init_f64 or
// dsgd_comm_init_f64v; csrc/dsgd_rp64.hpp "across ranks"): constexpr helpers only, shared by the kernels, the
// host side and a stand-alone host program (tests/cpp/rp64_gather_test.cpp compiles this header with a plain C++ compiler).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RP64_HD __host__ __device__
#else
#define RP64_HD
#endif

// The gather buffer of a step of k hosted workers in a world of W ranks, K = k * W, 64-bit words, zero between calls:
//   [W (padded to 64)]        one word per rank: the k it was called with and the value type of its data (rp64_rank_word;
//                             the ranks must agree on both before the slots travel)
//   [K][words][stride]        global worker r * k + j's slot, `words` planes of `stride` = rp64_gather_stride(dp) words:
//     float values, words = 1   [0, dp) its fixed-point column sums, rank order, then its header words -- the list length n
//                               (its shift is 62 - ceil(log2 n)) and its active count
//     Double values, words = 2  plane 0 (HI, signed): the high words of the column sums and the two header words, laid out
//                               as the one plane of float values is; plane 1 (LO, unsigned) directly behind it: the low
//                               words of the column sums in [0, dp) and nothing else (its header positions stay zero)
// Both planes are reached through the kernels' `acc[i] + k * acc_stride`: acc[1] = acc[0] + stride, acc_stride = words * stride.
// A slot is non-zero on exactly ONE rank, so ncclAllReduce(ncclInt64, ncclSum) over the buffer IS the all-gather: exact,
// whatever the order of the sum (HI in two's complement, LO below 2^63: no carry between the words on the wire either).
// Behind it every rank holds every worker's integers and folds them in worker order with the single context's own finish
// (dsgd_rp64_finish_kernel<true>, on Double values dsgd_rp64v_finish_kernel<RP64_STEP>) -- the bits of ONE process that
// hosts the K workers.
constexpr int RP64_HDR_N = 0, RP64_HDR_ACTIVE = 1, RP64_HDR_WORDS = 2;
// one message of the gather: at most 1 MiB (a plane is 378 KB at RCV1's D; wider planes are cut)
constexpr long long RP64_MSG_WORDS = (1LL << 20) / (long long)sizeof(unsigned long long);
RP64_HD constexpr long long rp64_gather_stride(int dp) { return ((long long)dp + RP64_HDR_WORDS + 63) & ~63LL; }
// a slot of `words` planes, where plane i starts inside it, and where header word h (of plane 0) lies inside it
RP64_HD constexpr long long rp64_gather_slot_words(int dp, int words) { return rp64_gather_stride(dp) * words; }
RP64_HD constexpr long long rp64_gather_plane(int dp, int i) { return rp64_gather_stride(dp) * i; }
RP64_HD constexpr long long rp64_gather_header(int dp, int h) { return (long long)dp + h; }

// A rank's word: the hosted workers k in bits 0..31, the value type in bit 32 (1: Double values, two planes per slot).
// Float data under either entry point gives the plain k of dsgd_comm_init_f64's first form.
constexpr int RP64_RANK_V64_BIT = 32;
RP64_HD constexpr unsigned long long rp64_rank_word(int k, bool v64) {
  return (unsigned long long)(unsigned int)k | ((v64 ? 1ull : 0ull) << RP64_RANK_V64_BIT);
}
RP64_HD constexpr int rp64_rank_word_k(unsigned long long w) { return (int)(unsigned int)(w & 0xffffffffull); }
RP64_HD constexpr bool rp64_rank_word_v64(unsigned long long w) { return ((w >> RP64_RANK_V64_BIT) & 1ull) != 0ull; }

// A plan run's word (dsgd_plan_run_f64 on a row-parallel plan under a communicator: ONE agreement per call, in front of the
// first slot message; the steps behind it travel without rank words).  The ranks all-reduce the [W] words in front of the
// slots with each rank's own word in its own position, and every rank reads all of them back:
//   bits 0..30   the hosted workers k of the rank's plan (1 <= k <= 2^31 - 1)
//   bit  31      the value type (1: Double values, two planes per slot)
//   bits 32..63  the steps of the call, step_end - step_begin (0: an empty run, which still takes part)
// A call runs at most RP64_CALL_MAX_STEPS = 2^32 - 1 steps: a longer range is refused before the agreement and is cut by the
// caller.
constexpr int RP64_CALL_V64_BIT = 31, RP64_CALL_STEPS_SHIFT = 32;
constexpr long long RP64_CALL_MAX_STEPS = 0xffffffffLL;
RP64_HD constexpr unsigned long long rp64_call_word(int k, bool v64, long long steps) {
  return ((unsigned long long)(unsigned int)k & 0x7fffffffull) | ((v64 ? 1ull : 0ull) << RP64_CALL_V64_BIT) |
         ((unsigned long long)steps << RP64_CALL_STEPS_SHIFT);
}
RP64_HD constexpr int rp64_call_word_k(unsigned long long w) { return (int)(w & 0x7fffffffull); }
RP64_HD constexpr bool rp64_call_word_v64(unsigned long long w) { return ((w >> RP64_CALL_V64_BIT) & 1ull) != 0ull; }
RP64_HD constexpr long long rp64_call_word_steps(unsigned long long w) { return (long long)(w >> RP64_CALL_STEPS_SHIFT); }
