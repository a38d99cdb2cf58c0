// The host's part of an epoch's device-drawn lists (csrc/dsgd_shuffle.hpp; the calls are in csrc/dsgd_seed_host.hpp): the
// epoch's frame and the sequential walk over the rejection candidates that dsgd_jr_scan_kernel delivers, which fixes the raw
// index every shuffle starts at and the raw values rejected inside it.
//
// Pure host arithmetic -- no device type, no library call but <vector> -- so that the library and a host test compile the
// same lines (tests/test_jr_walk.py runs it under AddressSanitizer and UBSan against a draw-by-draw java.util.Random).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

struct JrShuf {            // per (batch, worker), from the walk over the candidates
  long long raw0;          // raw index of the shuffle's first raw value
  int rej_begin, rej_end;  // its rejected raw values (offsets from raw0, ascending) in the flat rejection list
};

// steps the reference runs before an empty slice (core/Master.scala:184-188; the slave's Vec.sum throws on it)
inline long long jr_epoch_steps(const std::vector<long long>& len, long long max_samples, int batch_size) {
  long long n_steps = 0;
  for (long long b = 0; b < max_samples; b += batch_size) {
    bool ok = true;
    for (size_t k = 0; k < len.size(); ++k) ok = ok && b < len[k];
    if (!ok) break;
    ++n_steps;
  }
  return n_steps;
}

// An epoch of n_steps steps of a job whose workers have `len` rows each, seen from a context that hosts the workers
// first .. first + n_local - 1.  Shuffle q = step * n_splits + worker takes len - 1 draws (none for a split of one row).
struct JrFrame {
  long long n_steps = 0, n_shuf = 0, n_lists = 0;   // shuffles of the job; lists of the hosted workers
  int n_splits = 0, first = 0, n_local = 0;
  std::vector<long long> start;                     // n_shuf + 1: nominal raw index of every shuffle's start (no rejections)
  std::vector<int64_t> offsets;                     // n_lists + 1: prefix offsets of the hosted workers' lists, step-major
  long long nominal = 0;                            // draws of the epoch = raw values it takes without a rejection
};
inline JrFrame jr_frame(const std::vector<long long>& len, int first, int n_local, long long n_steps, int batch_size) {
  JrFrame f;
  f.n_steps = n_steps;
  f.n_splits = (int)len.size();
  f.first = first;
  f.n_local = n_local;
  f.n_shuf = n_steps * f.n_splits;
  f.n_lists = n_steps * n_local;
  f.start.assign((size_t)f.n_shuf + 1, 0);
  f.offsets.assign((size_t)f.n_lists + 1, 0);
  for (long long q = 0; q < f.n_shuf; ++q) {
    const long long l = len[(size_t)(q % f.n_splits)];
    f.start[(size_t)q + 1] = f.start[(size_t)q] + (l >= 2 ? l - 1 : 0);
  }
  for (long long q = 0; q < f.n_lists; ++q) {
    const long long l = len[(size_t)(first + q % n_local)], b = (q / n_local) * (long long)batch_size;
    f.offsets[(size_t)q + 1] = f.offsets[(size_t)q] + std::min<long long>(batch_size, l - b);
  }
  f.nominal = f.start[(size_t)f.n_shuf];
  return f;
}

// The candidates as dsgd_jr_scan_kernel leaves them: raw values that SOME bound <= the longest split can reject.  Workgroup
// w looked at raw indices [w * span, (w + 1) * span); its candidates are entries [wg_base[w] >> 16, + (wg_base[w] & 0xffff))
// of cand_i (raw index) / cand_u (raw value), in raw order; the blocks lie in the order the workgroups arrived.
struct JrCandidates {
  const long long* cand_i;
  const unsigned int* cand_u;
  const unsigned long long* wg_base;
  long long n_wg;
};
struct JrWalked {
  std::vector<JrShuf> shuf;       // one per shuffle (after jr_select_hosted: per list)
  std::vector<int> rej;           // the flat rejection list the records point into
  long long rej_total = 0;        // rejections of the epoch: it takes nominal + rej_total raw values
  long long scan_at_least = 0;    // jr_walk returned false: the stream outran the scan -- scan this far at least
};
// Walks the candidates in raw order (workgroup by workgroup, each block in order) with `rej` = the rejections so far: raw
// index i serves draw d = i - rej of the epoch; draw d belongs to shuffle j (start[j] <= d < start[j + 1]) and its bound
// is len_j - (d - start[j]).  `scan` raw values were looked at: false when the epoch needs more than that.
inline bool jr_walk(const JrFrame& f, const std::vector<long long>& len, const JrCandidates& c, long long scan, JrWalked* out) {
  const std::vector<long long>& start = f.start;
  std::vector<JrShuf>& shuf = out->shuf;
  std::vector<int>& rej_list = out->rej;
  long long rej = 0, j = 0;
  bool beyond = false;
  rej_list.clear();
  shuf.resize((size_t)f.n_shuf);
  for (long long q = 0; q < f.n_shuf; ++q) shuf[(size_t)q] = JrShuf{start[(size_t)q], 0, 0};
  long long next_begin = 0;   // shuffles < next_begin have their record closed
  // Called with jj = the shuffle of the candidate in hand, BEFORE that candidate is judged: every rejection counted so far
  // lies in a shuffle before jj (candidates come in raw order), so each shuffle in [next_begin, jj) ends its rejections
  // where the list ends now, and each shuffle up to jj starts `rej` raw values behind its nominal start with an empty run
  // of rejections.  After it, shuf[jj].raw0 and .rej_begin are final and shuffles < jj are closed.
  auto close_upto = [&](long long jj) {
    for (; next_begin < jj; ++next_begin) {
      shuf[(size_t)next_begin].rej_end = (int)rej_list.size();
      if (next_begin + 1 < f.n_shuf) {
        shuf[(size_t)next_begin + 1].raw0 = start[(size_t)next_begin + 1] + rej;
        shuf[(size_t)next_begin + 1].rej_begin = (int)rej_list.size();
      }
    }
  };
  for (long long w = 0; w < c.n_wg && !beyond; ++w) {
    const unsigned long long bw = c.wg_base[(size_t)w];
    const unsigned long long at = bw >> 16, cnt = bw & 0xffffULL;
    for (unsigned long long t = 0; t < cnt; ++t) {
      const long long d = c.cand_i[(size_t)(at + t)] - rej;
      if (d >= f.nominal) {
        beyond = true;
        break;
      }
      while (start[(size_t)j + 1] <= d) ++j;
      close_upto(j);
      const long long l = len[(size_t)(j % f.n_splits)];
      const unsigned int n = (unsigned int)(l - (d - start[(size_t)j]));
      if ((n & (n - 1)) != 0 && c.cand_u[(size_t)(at + t)] >= (0x80000000u / n) * n) {
        rej_list.push_back((int)(c.cand_i[(size_t)(at + t)] - shuf[(size_t)j].raw0));
        ++rej;
      }
    }
  }
  close_upto(f.n_shuf);
  out->rej_total = rej;
  out->scan_at_least = f.nominal + rej;
  return f.nominal + rej <= scan;   // (else: more rejections than the margin scanned)
}

// the hosted workers' records and rejections alone, step-major, hosted-worker-minor (the identity for a job hosted whole)
inline void jr_select_hosted(const JrFrame& f, JrWalked* w) {
  if (f.first == 0 && f.n_local == f.n_splits) return;
  std::vector<JrShuf> mine((size_t)f.n_lists);
  std::vector<int> rej_mine;
  for (long long q = 0; q < f.n_lists; ++q) {
    const JrShuf& s = w->shuf[(size_t)((q / f.n_local) * f.n_splits + f.first + q % f.n_local)];
    mine[(size_t)q] = JrShuf{s.raw0, (int)rej_mine.size(), (int)rej_mine.size() + (s.rej_end - s.rej_begin)};
    rej_mine.insert(rej_mine.end(), w->rej.begin() + s.rej_begin, w->rej.begin() + s.rej_end);
  }
  w->shuf.swap(mine);
  w->rej.swap(rej_mine);
}
