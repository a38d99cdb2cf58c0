// Device code of libdsgd_hip, part 15 (gfx950 only): the logistic model over SEVERAL TOPICS -- one-vs-rest over T <= 8 label
// planes on the same resident rows, ONE pass over the rows and ONE launch pair per step whatever T (include/dsgd.h "THE
// LOGISTIC MODEL": SEVERAL TOPICS).  Included by dsgd_hip.hip after dsgd_logistic.hpp.
//
// The contract: topic t's weights, losses, tallies and probabilities are the BITS the single-model kernels give on a context
// whose labels are plane t.  It holds because the kernels here ARE the single model's bodies (csrc/dsgd_logistic.hpp),
// instantiated with a topic loop:
//   the dot        lgt_row_load + lgt_row_dot, row_dot split at the fetch: a row's first LG_UNR * 16 non-zeros are fetched ONCE
//                  and reused by every topic
//   the gradient   lg_grad_body<true, true>.  Integer sums do not depend on their order, so how the LDS head is shared moves no
//                  bit: topic t owns lgt_hot(T) = LG_HOT / T words of the single model's 16 KiB head (its hottest ranks; the
//                  others go to global vector atomics) -- a workgroup's LDS does not grow with T and never lowers the six waves
//                  per SIMD the registers allow.  (The whole head for a few topics per sweep would re-read the rows once per
//                  sweep: the pass over the rows is what the topics are here to share.)
//   the finish     lg_finish_body<LG_STEP, false, true>: the topic on the grid's y, |w_t'|^2 into nsq_part[t][block]; weights the
//                  finish did not write: dsgd_lg_nsq_kernel with the same grid
//   the evaluation dsgd_lg_eval_kernel's grid, stride and fixed-order tree, per row and topic lg_row_loss.  A group's lane 0 adds
//                  topic t's losses in row order into its own word of LDS (a register per topic would be an indexed array:
//                  scratch), the words then go through lg_block_tally3 and lg_block_sum topic by topic.  The hot-weight tile is
//                  smaller per topic; the tile's size moves no bit
//   predict        lg_predict_body<true>: p_out[t][position]
//
// What the gfx950 compile reports (hipcc -O3, tools/isa.sh; every kernel: no scratch, no spill):
//   dsgd_lg_topics_grad_kernel     79 VGPRs, 103 SGPRs, 16,384 B LDS, 6 waves per SIMD (dsgd_lg_grad_kernel: 78 VGPRs, 6 waves)
//   dsgd_lg_topics_finish_kernel   22 VGPRs,  30 SGPRs,     32 B LDS, 8 waves per SIMD
//   dsgd_lg_topics_eval_kernel    110 VGPRs,  97 SGPRs, dynamic LDS,  4 waves per SIMD (what ONE 1024-lane workgroup per CU needs)
//   dsgd_lg_topics_predict_kernel  58 VGPRs,  70 SGPRs,      0 B LDS, 8 waves per SIMD
//
// Plain C++ and vector atomics only.
#pragma once
#include "dsgd_lg_topics_host.hpp"

static_assert(LGT_HOT_WORDS == LG_HOT, "the topics share the single model's LDS head");
static_assert(LGT_LDS_FLOATS == DSGD_LDS_FLOATS, "one LDS budget");

struct LgtArgs {
  const float* w;                  // [T][w_stride] the topics' weights, rank order
  long long w_stride;
  const signed char* planes;       // [T][n_rows] +1 / -1
  int T, hot;                      // hot = lgt_hot(T): the ranks of the LDS head each topic owns
  int dp, vexp, K;
  const int* idx;                  // the lists, concatenated
  const WorkSeg* segs;             // [K] each worker's [begin, end) in idx
  long long blocks_per_worker;     // grid = K * blocks_per_worker
  unsigned long long* acc;         // [T][K][acc_stride] fixed-point column sums, rank order; zero on entry
  long long acc_stride;
  DevScalars* sc;                  // err (1: a row index outside the data)
};

// grid: K x blocks_per_worker workgroups, one 16-lane group per listed position
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_grad_kernel(CsrView m, LgtArgs a) { lg_grad_body<true, true>(m, a); }

struct LgtFinishArgs {
  unsigned long long* acc;   // [T][K][acc_stride], zeroed here
  long long acc_stride;
  const WorkSeg* segs;       // [K]: the lengths give each worker's shift
  int K, dp, vexp;
  float* w;                  // [T][w_stride] rank order, updated
  long long w_stride;
  double lr, lambda;
  double* nsq_part;          // [T][gridDim.x] |w_t'|^2 of each workgroup's columns
};

// grid: (lg_finish_blocks(dp), T) workgroups -- ONE column per lane, the topic on y
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_finish_kernel(LgtFinishArgs a) { lg_finish_body<LG_STEP, false, true>(a); }

// grid: lg_eval_blocks(rows, n_cu) workgroups; dynamic LDS: lgt_eval_lds_floats(hw, T) floats (csrc/dsgd_lg_topics_host.hpp).
// tally: [T][LG_TALLY_WORDS], zero on entry; loss_part: [T][part_stride], topic t's word of workgroup b at [t][b]
__global__ void __launch_bounds__(LG_EVAL_THREADS) dsgd_lg_topics_eval_kernel(CsrView m, const float* __restrict__ w, long long w_stride,
                                                                             const signed char* __restrict__ planes, int T, long long row_begin,
                                                                             long long row_end, unsigned long long* tally, int hw, double* loss_part,
                                                                             long long part_stride) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  double* sums = reinterpret_cast<double*>(lds + lgt_eval_sums_at(hw, T));        // [T][LGT_EVAL_GROUPS]
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + lgt_eval_cnt_at(hw, T));   // [T][3][LGT_EVAL_GROUPS]
  for (int tp = 0; tp < T; ++tp)
    for (int j = threadIdx.x; j < hw; j += LG_EVAL_THREADS) lds[tp * hw + j] = w[(long long)tp * w_stride + j];
  for (int j = threadIdx.x; j < T * LGT_EVAL_GROUPS; j += LG_EVAL_THREADS) sums[j] = 0.0;
  for (int j = threadIdx.x; j < 3 * T * LGT_EVAL_GROUPS; j += LG_EVAL_THREADS) cnt[j] = 0u;
  __syncthreads();
  const int sub = threadIdx.x % LG_GROUP;
  const int g = threadIdx.x / LG_GROUP;
  const long long group = ((long long)blockIdx.x * LG_EVAL_THREADS + threadIdx.x) / LG_GROUP;
  const long long n_groups = (long long)gridDim.x * LG_EVAL_THREADS / LG_GROUP;
  for (long long row = row_begin + group; row < row_end; row += n_groups) {
    const long long st = m.row_ptr[row], en = m.row_ptr[row + 1];
    RowRegs<LG_GROUP, LG_UNR> r;
    lgt_row_load<LG_GROUP, LG_UNR>(m, st, en, sub, r);
    for (int tp = 0; tp < T; ++tp) {
      const float d = lgt_row_dot<LG_GROUP, LG_UNR, true>(m, st, en, lds + tp * hw, w + (long long)tp * w_stride, hw, sub, r);
      if (sub == 0) {   // (this group's own words: nobody else touches them)
        int which;
        const double l = lg_row_loss((double)planes[(long long)tp * m.n_rows + row], d, which);
        cnt[(tp * 3 + which) * LGT_EVAL_GROUPS + g] += 1u;
        sums[tp * LGT_EVAL_GROUPS + g] = sums[tp * LGT_EVAL_GROUPS + g] + l;
      }
    }
  }
  __syncthreads();
  for (int tp = 0; tp < T; ++tp) {
    const bool own = sub == 0;
    const unsigned int c0 = own ? cnt[(tp * 3 + 0) * LGT_EVAL_GROUPS + g] : 0u;
    const unsigned int c1 = own ? cnt[(tp * 3 + 1) * LGT_EVAL_GROUPS + g] : 0u;
    const unsigned int c2 = own ? cnt[(tp * 3 + 2) * LGT_EVAL_GROUPS + g] : 0u;
    const double ls = own ? sums[tp * LGT_EVAL_GROUPS + g] : 0.0;
    lg_block_tally3(c0, c1, c2, tally + tp * LG_TALLY_WORDS, reinterpret_cast<unsigned int*>(lds + T * hw));
    const double s = lg_block_sum(ls, reinterpret_cast<double*>(lds + lgt_eval_red_at(hw, T)), LG_EVAL_THREADS / 64);
    if (threadIdx.x == 0) loss_part[(long long)tp * part_stride + blockIdx.x] = s;
  }
}

// p_out: [T][n], topic-major
__global__ void __launch_bounds__(LG_THREADS) dsgd_lg_topics_predict_kernel(CsrView m, const float* __restrict__ w, long long w_stride, int T,
                                                                           const int* __restrict__ idx, long long n, float* p_out, DevScalars* sc) {
  lg_predict_body<true>(m, w, w_stride, T, idx, n, p_out, sc);
}
