// The JOB's evaluation of the logistic model on every rank (dsgd_lg_eval_job; include/dsgd.h "THE LOGISTIC MODEL", ACROSS RANKS;
// DESIGN.md 3.13 and 7.5): the gather record's layout and the host's fold as constexpr / inline helpers that a stand-alone host
// program compiles with a plain C++ compiler (tests/cpp/lg_eval_job_test.cpp), and -- under hipcc only -- the one kernel that
// fills this rank's positions of the record.  Included by dsgd_hip.hip after dsgd_lg_eval.hpp.
//
// A job of K = n_local * world ranges; rank r's range j takes position lgg_global_worker(r, n_local, j) = r * n_local + j, the
// global worker order of the steps.  The record, 64-bit words, in a device buffer of its own (NOT inside d_lg_acc):
//   [K][LGE_WORDS]   per position: the three tallies (signum(d) == y, == 0, == -y), the fp64 BIT PATTERN of the range's sum of
//                    l_i (its workgroups' words added from 0.0 in block order), and a writer count of 1
//   padded to 64 words with zeros
// Every word is non-zero on at most one rank, so ONE in-place ncclAllReduce(ncclInt64, ncclSum) over lge_words(K) words is an
// exact all-gather: a double's bit pattern added to zeros is itself.  A position whose writer count is not 1 behind the gather
// was written by no rank or by two -- the ranks disagree about the layout: DSGD_ESTATE.
#pragma once

#include <cstdint>
#include <cstring>

#include "dsgd_lg_gather.hpp"

constexpr int LGE_RIGHT = 0, LGE_ZERO = 1, LGE_WRONG = 2, LGE_SUM = 3, LGE_WRITERS = 4, LGE_WORDS = 5;

// the words the all-reduce covers, and where position pos's block of LGE_WORDS words starts
LGG_HD constexpr long long lge_words(long long K) { return lgg_pad64((long long)LGE_WORDS * K); }
LGG_HD constexpr long long lge_at(long long pos) { return (long long)LGE_WORDS * pos; }

// The fold of a gathered record, in POSITION order, with the expressions of dsgd_lg_predict_ranges (csrc/dsgd_lg_calls.hpp): the
// bits that call returns on one context holding every rank's rows.  nsq: the sum of the |w|^2 words.  Outputs may be null.
// bad_pos >= 0: the first position whose writer count is not 1 (`writers` holds it); nothing was written.
struct LgeFold {
  int bad_pos = -1;
  long long writers = 1;
  long long total = 0;   // rows of the job's ranges
};
inline LgeFold lge_fold(const unsigned long long* rec, int K, double lambda, double nsq, int64_t* counts_out, double* range_loss_out, double* loss,
                        double* acc) {
  LgeFold f;
  for (int r = 0; r < K; ++r) {   // (before anything is written)
    const unsigned long long* b = rec + lge_at(r);
    if (b[LGE_WRITERS] != 1ull) {
      f.bad_pos = r;
      f.writers = (long long)b[LGE_WRITERS];
      return f;
    }
    f.total += (long long)(b[LGE_RIGHT] + b[LGE_ZERO] + b[LGE_WRONG]);
  }
  double ls_all = 0.0;   // (in order: the same bits on every rank)
  unsigned long long right = 0;
  for (int r = 0; r < K; ++r) {
    const unsigned long long* b = rec + lge_at(r);
    const long long rows = (long long)(b[LGE_RIGHT] + b[LGE_ZERO] + b[LGE_WRONG]);
    double ls;
    memcpy(&ls, &b[LGE_SUM], sizeof(ls));
    ls_all += ls;
    right += b[LGE_RIGHT];
    if (range_loss_out) range_loss_out[r] = rows ? lambda * nsq + ls / (double)rows : 0.0;   // (dsgd_lg_loss_acc's expression)
    for (int j = 0; counts_out && j < 3; ++j) counts_out[3 * r + j] = (int64_t)b[j];
  }
  if (loss) *loss = lambda * nsq + ls_all / (double)f.total;
  if (acc) *acc = (double)right / (double)f.total;
  return f;
}

#if defined(__HIPCC__)
constexpr int LGE_THREADS = 256;

struct LgeArgs {
  const long long* first_block;       // [k + 1] lg_pred_table's: local range j owns loss_part[first_block[j] .. first_block[j + 1])
  const double* loss_part;            // dsgd_lg_predict_ranges_kernel's per-workgroup sums of l_i
  const unsigned long long* tally;    // [k][LG_TALLY_WORDS] its tallies
  unsigned long long* rec;            // the gather record, lge_words(K) words
  int k, K, first;                    // the local ranges, the job's, this rank's first position
};

// Behind dsgd_lg_predict_ranges_kernel over the k local ranges.  grid: k workgroups, one per local range.  Lane 0 adds the range's
// loss_part words from 0.0 in block order, contraction off -- the loop dsgd_lg_predict_ranges runs on the host, the same bits --
// and writes the range's LGE_WORDS words at its global position.  All lanes of the grid together zero every word of the record
// outside this rank's block (the words of the previous call are gone), as dsgd_lg_header_kernel does for a step's header words.
// Plain vector stores; no LDS.
__global__ void __launch_bounds__(LGE_THREADS) dsgd_lg_eval_fold_kernel(LgeArgs a) {
#pragma clang fp contract(off)
  const long long own0 = lge_at(a.first), own1 = lge_at((long long)a.first + a.k), words = lge_words(a.K);
  for (long long i = (long long)blockIdx.x * LGE_THREADS + threadIdx.x; i < words; i += (long long)gridDim.x * LGE_THREADS)
    if (i < own0 || i >= own1) a.rec[i] = 0ull;
  if (threadIdx.x == 0) {
    const int j = blockIdx.x;
    double ls = 0.0;
    for (long long b = a.first_block[j]; b < a.first_block[j + 1]; ++b) ls = ls + a.loss_part[b];
    unsigned long long* out = a.rec + lge_at((long long)a.first + j);
    const unsigned long long* t = a.tally + (long long)j * LG_TALLY_WORDS;
    out[LGE_RIGHT] = t[0];
    out[LGE_ZERO] = t[1];
    out[LGE_WRONG] = t[2];
    out[LGE_SUM] = (unsigned long long)__double_as_longlong(ls);
    out[LGE_WRITERS] = 1ull;
  }
}
#endif
