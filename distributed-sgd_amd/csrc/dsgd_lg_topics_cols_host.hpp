// The host arithmetic of the topics' whole-split steps by COLUMN LISTS (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS, ROW
// RANGES; pure C++, no HIP: tests/cpp/lg_topics_cols_host_test.cpp compiles it alone; csrc/dsgd_lg_topics_cols.hpp and
// csrc/dsgd_lg_topics_cols_calls.hpp compile the same numbers).  The layout of the entries is the single model's, unchanged
// (csrc/dsgd_lg_cols_host.hpp: lgc_share, lgc_plan); the interleaved shapes and the group width are those of the list forms
// (csrc/dsgd_lg_topics_il_host.hpp, csrc/dsgd_lg_topics_wide_host.hpp).
//
//   lgtc_groups          lane groups of a workgroup of dsgd_lg_topics_cgrad_kernel<GW>: 256 / GW
//   lgtc_group_entries   the contiguous run of a share's entries ONE lane group walks: share * GW / 256 -- a multiple of GW, and
//                        so of the sixteen entries a fetch hands round, because a share is a multiple of 256
//   lgtc_table_words     doubles of the step's coefficient table cq[position][TP]; -1: more than LGTC_MAX_WORDS (refused)
//   lgtc_refusal         why a ranges configuration cannot be served (lgc_plan's fault, the table's words), or nullptr: it can
//   lgtc_acc_word        the topics' accumulator word of a layout's slot `k * lg_stride + rank`: k * acc_stride + rank * TP (+ 2l
//                        for lane l)
#pragma once

#include "dsgd_lg_cols_host.hpp"
#include "dsgd_lg_topics_wide_host.hpp"

// The table stays below 2^37 doubles (1 TiB): beyond any device, and a byte offset into it keeps 23 bits of a 64-bit word
// free.  What is below the limit and does not fit the device fails at the allocation.
constexpr long long LGTC_MAX_WORDS = 1LL << 37;

LG_HD constexpr int lgtc_groups(int gw) { return LGC_THREADS / gw; }
LG_HD constexpr int lgtc_group_entries(int share, int gw) { return share / LGC_THREADS * gw; }
static_assert(LGC_THREADS == LG_THREADS, "the coefficient and the gradient kernel split one workgroup size into lane groups");
static_assert(LGC_MIN_SHARE % LGC_THREADS == 0 && LGC_MAX_SHARE % LGC_THREADS == 0, "shares are whole workgroups' worth of lanes");

// positions: lgc_plan's (below LGC_LIMIT); tp: lgti_tp(T)
inline long long lgtc_table_words(long long positions, int tp) {
  if (positions < 0 || tp < 4 || tp > LG_TOPICS_WIDE_MAX || tp % 4) return -1;
  const long long words = positions * (long long)tp;   // (below 2^31 * 2^7: no overflow)
  return positions >= LGC_LIMIT || words > LGTC_MAX_WORDS ? -1 : words;
}

// what lgc_plan and lgtc_table_words said about a configuration: nullptr = it can be laid out, else why not (the call fails
// with DSGD_EUNSUPPORTED: the topics have no row form over ranges to fall back to)
inline const char* lgtc_refusal(LgcFault plan, long long table_words) {
  switch (plan) {
    case LGC_OK: return table_words < 0 ? "the coefficient table rows x TP would pass 2^37 doubles" : nullptr;
    case LGC_NO_ENTRIES: return "their rows have no entries";
    case LGC_ENTRIES: return "2^31 entries or more";
    case LGC_POSITIONS: return "2^31 rows or more";
    case LGC_KEYS: return "workers x columns reach 2^31";
  }
  return "an unknown fault";
}

// (slot and lg_stride are below 2^31 -- lgc_plan's LGC_KEYS: one 32-bit division per flushed column)
LG_HD constexpr long long lgtc_acc_word(unsigned int slot, unsigned int lg_stride, long long acc_stride, int tp) {
  return (long long)(slot / lg_stride) * acc_stride + (long long)(slot % lg_stride) * tp;
}
