// Stand-alone host program over csrc/dsgd_lg_eval_job.hpp (plain C++, no HIP): the gather record of dsgd_lg_eval_job -- its
// offsets for K = 1, 2, 12, 13, 255, 256 (disjoint blocks, padded to 64, a rank's positions exactly r k .. r k + k - 1) -- and
// the host's fold: in position order, not in a rank-minor order and not as a pairwise tree, and a writer count of 0 or 2 is
// reported with nothing written.  tests/test_lg_eval_job_host.py compiles it with -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dsgd_lg_eval_job.hpp"
#include "dsgd_lg_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static unsigned long long bits_of(double x) {
  unsigned long long b;
  std::memcpy(&b, &x, sizeof(b));
  return b;
}

static void layout(int K) {
  const long long words = lge_words(K);
  CHECK(words % 64 == 0 && words >= (long long)LGE_WORDS * K && words - (long long)LGE_WORDS * K < 64);
  CHECK(words <= lge_words(LG_PRED_MAX_RANGES));
  std::vector<int> owner((size_t)words, -1);
  for (int p = 0; p < K; ++p)
    for (int h = 0; h < LGE_WORDS; ++h) {
      const long long at = lge_at(p) + h;
      CHECK(at >= 0 && at < words);
      CHECK(owner[(size_t)at] == -1);
      owner[(size_t)at] = p;
    }
  // every way of cutting K into world x k: rank r's positions are r k .. r k + k - 1, every position is one rank's
  for (int world = 1; world <= K && world <= LGG_MAX_WORLD; ++world) {
    if (K % world) continue;
    const int k = K / world;
    std::vector<int> rank_of((size_t)K, -1);
    for (int r = 0; r < world; ++r)
      for (int j = 0; j < k; ++j) {
        const long long g = lgg_global_worker(r, k, j);
        CHECK(g == (long long)r * k + j && g >= 0 && g < K);
        CHECK(rank_of[(size_t)g] == -1);
        rank_of[(size_t)g] = r;
        CHECK(owner[(size_t)lge_at(g)] == (int)g && owner[(size_t)(lge_at(g) + LGE_WORDS - 1)] == (int)g);
      }
    for (int p = 0; p < K; ++p) CHECK(rank_of[(size_t)p] == p / k);
  }
}

// a record of K positions whose sums are v; position 0 holds the job's one row (total = 1: loss = the folded sum itself at
// lambda = 0), so that the order of the fold is the only thing the loss depends on
static std::vector<unsigned long long> record(const std::vector<double>& v) {
  const int K = (int)v.size();
  std::vector<unsigned long long> rec((size_t)lge_words(K), 0ull);
  for (int p = 0; p < K; ++p) {
    unsigned long long* b = rec.data() + lge_at(p);
    b[LGE_RIGHT] = p == 0 ? 1ull : 0ull;
    b[LGE_SUM] = bits_of(v[(size_t)p]);
    b[LGE_WRITERS] = 1ull;
  }
  return rec;
}
static double left_fold(const std::vector<double>& v) {
  double s = 0.0;
  for (double x : v) s += x;
  return s;
}
static double rank_minor_fold(const std::vector<double>& v, int world) {   // worker j of every rank, then worker j + 1
  const int k = (int)v.size() / world;
  double s = 0.0;
  for (int j = 0; j < k; ++j)
    for (int r = 0; r < world; ++r) s += v[(size_t)(r * k + j)];
  return s;
}
static double pairwise(const std::vector<double>& v, size_t lo, size_t hi) {
  if (hi - lo == 1) return v[lo];
  const size_t mid = lo + (hi - lo) / 2;
  return pairwise(v, lo, mid) + pairwise(v, mid, hi);
}

static void fold_order(int K, int world) {
  const double e = std::ldexp(1.0, -53);
  // (a) 1.0, then 2^-53 many times: from the left every 2^-53 is half an ulp of 1.0 and is rounded away; a tree adds them to
  //     one another first
  std::vector<double> a((size_t)K, e);
  a[0] = 1.0;
  // (b) the 1.0 at rank 1's first position: in position order rank 0's k words of 2^-53 add up exactly before they meet it; a
  //     rank-minor order puts the first 2^-53 and the 1.0 together and loses it
  std::vector<double> b((size_t)K, e);
  b[(size_t)(K / world)] = 1.0;
  for (const std::vector<double>* v : {&a, &b}) {
    const std::vector<unsigned long long> rec = record(*v);
    double loss = -1.0, acc = -1.0;
    std::vector<double> rl((size_t)K, -1.0);
    std::vector<int64_t> counts((size_t)(3 * K), -1);
    const LgeFold f = lge_fold(rec.data(), K, 0.0, 0.0, counts.data(), rl.data(), &loss, &acc);
    CHECK(f.bad_pos == -1 && f.total == 1);
    CHECK(bits_of(loss) == bits_of(left_fold(*v)));
    CHECK(bits_of(loss) != bits_of(pairwise(*v, 0, v->size())));
    CHECK(acc == 1.0 && counts[0] == 1 && counts[1] == 0 && counts[3] == 0);
    CHECK(bits_of(rl[0]) == bits_of((*v)[0]) && rl[1] == 0.0);   // (a range without rows reports 0.0)
  }
  CHECK(bits_of(left_fold(a)) == bits_of(1.0));
  CHECK(bits_of(left_fold(b)) != bits_of(rank_minor_fold(b, world)));
  {   // the regulariser and the division, with dsgd_lg_predict_ranges' expressions
    std::vector<unsigned long long> rec = record(a);
    rec[(size_t)(lge_at(1) + LGE_WRONG)] = 2ull;
    rec[(size_t)(lge_at(1) + LGE_ZERO)] = 4ull;
    double loss = 0.0, acc = 0.0;
    std::vector<double> rl((size_t)K, -1.0);
    const double lambda = 1e-5, nsq = 3.25;
    const LgeFold f = lge_fold(rec.data(), K, lambda, nsq, nullptr, rl.data(), &loss, &acc);
    CHECK(f.bad_pos == -1 && f.total == 7);
    CHECK(bits_of(loss) == bits_of(lambda * nsq + left_fold(a) / 7.0));
    CHECK(bits_of(acc) == bits_of(1.0 / 7.0));
    CHECK(bits_of(rl[1]) == bits_of(lambda * nsq + e / 6.0));
  }
}

static void writers(int K) {
  std::vector<double> v((size_t)K, 0.5);
  for (unsigned long long count : {0ull, 2ull})
    for (int bad : {0, K / 2, K - 1}) {
      std::vector<unsigned long long> rec = record(v);
      rec[(size_t)(lge_at(bad) + LGE_WRITERS)] = count;
      double loss = -1.0, acc = -1.0;
      std::vector<double> rl((size_t)K, -1.0);
      std::vector<int64_t> counts((size_t)(3 * K), -1);
      const LgeFold f = lge_fold(rec.data(), K, 0.0, 0.0, counts.data(), rl.data(), &loss, &acc);
      CHECK(f.bad_pos == bad && f.writers == (long long)count);
      CHECK(loss == -1.0 && acc == -1.0 && rl[0] == -1.0 && counts[0] == -1);   // nothing written
    }
}

int main() {
  for (int K : {1, 2, 12, 13, 255, 256}) layout(K);
  fold_order(12, 2);
  fold_order(12, 3);
  fold_order(256, 2);
  fold_order(256, 64);
  for (int K : {1, 2, 12, 13, 255, 256}) writers(K);
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
