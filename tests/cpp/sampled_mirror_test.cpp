// Drives the sampled evaluation of include/dsgd.hpp (Master::localSampledLoss / localSampledAccuracy, SparseSVM::lossAccList /
// lossAccSampled; core/Master.scala:109-118) against a list drawn by csrc/jrand.c (dsgd_jrand_shuffle).
//   usage: sampled_mirror_test cpu | gpu        exit code 0 = all checks passed
//   cpu: the refusals that need no device and the mirror's shuffle against jrand.c's
//   gpu: 500 synthetic rows; both windows, several sample sizes, DSGD_SAMPLED_DEVICE unset and = 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "dsgd.hpp"

extern "C" int64_t dsgd_jrand_shuffle(uint64_t* state, int32_t* buf, int64_t len);   // csrc/jrand.c (lib/libdsgd_host.so)

static int failures = 0;
#define CHECK(...)                                                         \
  do {                                                                     \
    if (!(__VA_ARGS__)) {                                                  \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

// `Random.shuffle(0 until len) take k`, each entry + lo, by jrand.c; *state advances
static std::vector<int32_t> jrand_take(uint64_t* state, int64_t lo, int64_t len, int64_t k) {
  std::vector<int32_t> buf((size_t)len);
  std::iota(buf.begin(), buf.end(), 0);
  dsgd_jrand_shuffle(state, buf.data(), len);
  buf.resize((size_t)std::min(k, len));
  for (int32_t& r : buf) r += (int32_t)lo;
  return buf;
}

static void cpu_checks() {
  using namespace dsgd;
  for (int len : {1, 2, 7, 1024, 5000}) {   // the mirror's shuffle is jrand.c's, entry for entry and draw for draw
    JavaRandom r(31);
    uint64_t st = r.state();
    std::vector<int32_t> xs((size_t)len);
    std::iota(xs.begin(), xs.end(), 0);
    CHECK(shuffle(xs, r) == jrand_take(&st, 0, len, len) && r.state() == st);
  }
  double l = -1, a = -1;
  int64_t counts[3] = {-1, -1, -1}, n = -1, draws = -1;
  uint64_t st = 12345;
  const int32_t idx[2] = {0, 1};
  CHECK(dsgd_loss_acc_list(nullptr, nullptr, idx, 2, &l, &a, counts) == DSGD_EINVAL);
  CHECK(dsgd_loss_acc_list_f64(nullptr, nullptr, idx, 2, &l, &a, counts) == DSGD_EINVAL);
  CHECK(dsgd_loss_acc_sampled(nullptr, nullptr, &st, 0, 10, 5, &l, &a, counts, nullptr, &n, &draws) == DSGD_EINVAL);
  CHECK(dsgd_loss_acc_sampled_f64(nullptr, nullptr, &st, 0, 10, 5, &l, &a, counts, nullptr, &n, &draws) == DSGD_EINVAL);
  CHECK(l == -1 && a == -1 && counts[0] == -1 && counts[2] == -1 && n == -1 && draws == -1 && st == 12345);
}

static void gpu_checks() {
  using namespace dsgd;
  const int D = 40, N = 500, N_TRAIN = 400;
  Data d;
  JavaRandom gen(5);
  for (int i = 0; i < N; ++i) {
    std::vector<std::pair<int32_t, float>> x;
    for (int j = 0; j < 1 + i % 5; ++j) x.emplace_back(1 + (i * 7 + j * 11) % D, (float)(gen.nextInt(2001) - 1000) / 1000.0f);
    std::sort(x.begin(), x.end());
    x.erase(std::unique(x.begin(), x.end(), [](const auto& p, const auto& q) { return p.first == q.first; }), x.end());
    d.add(x, i % 3 == 0 ? -1 : +1);
  }
  SparseSVM model(1e-3, D);
  model.load(d);
  model.buildDimSparsity(N_TRAIN);
  Vec w((size_t)D + 1);
  for (int j = 0; j <= D; ++j) w[(size_t)j] = (float)(gen.nextInt(2001) - 1000) / 500.0f;

  for (const char* device : {"0", "1"}) {
    setenv("DSGD_SAMPLED_DEVICE", device, 1);
    Master master(model, N_TRAIN, N, 3, JavaRandom(9));
    uint64_t st = JavaRandom(9).state();
    for (bool test : {false, true})
      for (int k : {1, 50, 99, 100, 101, 400, 1000}) {
        const int64_t lo = test ? N_TRAIN : 0, len = test ? N - N_TRAIN : N_TRAIN;
        const auto want_l = model.lossAccList(w, jrand_take(&st, lo, len, k));
        const double got_l = master.localSampledLoss(w, k, test);
        CHECK(got_l == want_l.loss && master.random().state() == st && want_l.n == std::min<int64_t>(k, len));
        const auto want_a = model.lossAccList(w, jrand_take(&st, lo, len, k));   // (a second shuffle: another sample)
        const double got_a = master.localSampledAccuracy(w, k, test);
        CHECK(got_a == want_a.accuracy && master.random().state() == st);
        CHECK(want_a.counts[0] + want_a.counts[1] + want_a.counts[2] == want_a.n);
      }
    bool threw = false;
    try {
      master.localSampledLoss(w, 0);
    } catch (const IllegalArgumentException&) {
      threw = true;
    }
    CHECK(threw && master.random().state() == st);
  }
  {   // the device draw itself: the list, the draws and the state are jrand.c's
    JavaRandom r(77);
    uint64_t st = r.state();
    const auto want = jrand_take(&st, 100, 300, 64);
    const auto got = model.lossAccSampled(w, r, 100, 400, 64, true);
    CHECK(got.idx == want && r.state() == st && got.n == 64 && got.draws >= 299);
    const auto by_list = model.lossAccList(w, want);
    CHECK(got.loss == by_list.loss && got.accuracy == by_list.accuracy && std::memcmp(got.counts, by_list.counts, sizeof(got.counts)) == 0);
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  try {
    cpu_checks();
    if (mode == "gpu") gpu_checks();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (failures) return 1;
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
