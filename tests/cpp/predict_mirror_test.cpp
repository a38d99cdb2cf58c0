// Drives Master::predict / distributedLoss / distributedAccuracy of include/dsgd.hpp (core/Master.scala:61-98 over
// dsgd_predict_ranges): at w = 0 and after a few steps they must equal what dsgd_loss_acc returns for the same rows.
//   usage: predict_mirror_test cpu | gpu        exit code 0 = all checks passed
#include <cstdio>
#include <cstring>
#include <string>

#include "dsgd.hpp"

static int failures = 0;
#define CHECK(...)                                                         \
  do {                                                                     \
    if (!(__VA_ARGS__)) {                                                  \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static dsgd::Data kat_rows() {  // D = 6, 1-based ids
  dsgd::Data d;
  const std::vector<std::pair<std::vector<std::pair<int32_t, float>>, int>> rows = {
      {{{1, .6f}, {3, .8f}}, +1}, {{{2, 1.f}}, -1}, {{{3, .6f}, {4, .8f}}, -1},
      {{{1, .8f}, {6, .6f}}, +1}, {{{1, .6f}, {3, .8f}}, -1}, {{{2, .6f}, {6, .8f}}, +1}};
  for (const auto& r : rows) d.add(r.first, r.second);
  return d;
}

static void cpu_checks() {
  // the argument checks that need no device: a null context is refused, nothing is written
  int8_t pred[4] = {7, 7, 7, 7};
  const int64_t b[1] = {0}, e[1] = {4};
  double loss = -1, acc = -1;
  CHECK(dsgd_predict_ranges(nullptr, nullptr, b, e, 1, pred, nullptr, &loss, &acc) == DSGD_EINVAL);
  CHECK(dsgd_predict_ranges_f64(nullptr, nullptr, b, e, 1, pred, nullptr, &loss, &acc) == DSGD_EINVAL);
  CHECK(pred[0] == 7 && loss == -1 && acc == -1);
  bool threw = false;
  try {
    dsgd::check(dsgd_predict_ranges(nullptr, nullptr, b, e, 1, pred, nullptr, nullptr, nullptr));
  } catch (const dsgd::IllegalArgumentException&) {
    threw = true;
  }
  CHECK(threw);
}

static void compare(dsgd::SparseSVM& model, dsgd::Master& master, const dsgd::Vec& w, int64_t nTrain) {
  using namespace dsgd;
  const double dl = master.distributedLoss(w), da = master.distributedAccuracy(w);
  CHECK(dl == master.localLoss(w) && da == master.localAccuracy(w));   // integer tallies, the same |w|^2: exact
  double l = 0, a = 0;
  int64_t counts[3] = {0, 0, 0};
  check(dsgd_loss_acc(model.ctx(), w.data(), 0, nTrain, &l, &a, counts));
  CHECK(dl == l && da == a);
  // the map itself: every train row once, in split order, and its predictions are the ones the tallies were made from
  const auto preds = master.predict(w);
  CHECK((int64_t)preds.size() == nTrain);
  const int y[6] = {1, -1, -1, 1, -1, 1};
  int64_t c[3] = {0, 0, 0};
  for (size_t i = 0; i < preds.size(); ++i) {
    CHECK(preds[i].first == (int64_t)i && preds[i].second >= -1 && preds[i].second <= 1);
    ++c[preds[i].second == 0 ? 1 : (preds[i].second == y[preds[i].first] ? 0 : 2)];
  }
  CHECK(c[0] == counts[0] && c[1] == counts[1] && c[2] == counts[2]);
  std::vector<int32_t> idx;
  for (int64_t i = 0; i < nTrain; ++i) idx.push_back((int32_t)i);
  const std::vector<float> f = model.forward(w, idx);
  for (size_t i = 0; i < preds.size(); ++i) CHECK((float)preds[i].second == f[i]);
}

static void gpu_checks() {
  using namespace dsgd;
  for (int nodeCount : {1, 2, 4}) {   // (4: SplitStrategy.vanilla yields 3 groups of 2)
    SparseSVM model(0.1, 6);
    model.load(kat_rows());
    model.buildDimSparsity(6);
    Master master(model, /*nTrain=*/6, /*nRows=*/6, nodeCount, JavaRandom(0));
    Vec w(7, 0.f);
    CHECK(master.distributedLoss(w) == 1.0 && master.distributedAccuracy(w) == 0.0);   // Main.scala:75-78's first two lines
    compare(model, master, w, 6);
    Slave slave(model, /*async=*/false);
    for (int step = 0; step < 3; ++step) {   // KAT-1's steps: two workers with fixed batches, lr 0.25
      const GradUpdate a = slave.gradient(GradientRequest{w, {0, 1, 2}});
      const GradUpdate b = slave.gradient(GradientRequest{w, {3, 4, 5}});
      for (int j = 0; j < 7; ++j) w[(size_t)j] -= 0.25f * 0.5f * (a.gradUpdate[(size_t)j] + b.gradUpdate[(size_t)j]);
      compare(model, master, w, 6);
    }
    CHECK(master.distributedAccuracy(w) == 5. / 6);
  }
  {   // what the reference's fold throws on, and what the entry refuses
    SparseSVM model(0.1, 6);
    model.load(kat_rows());
    model.buildDimSparsity(6);
    const Vec w(7, 0.f);
    auto refused = [&](const std::vector<std::pair<int64_t, int64_t>>& ranges) {
      try {
        model.predictRanges(w, ranges);
      } catch (const IllegalArgumentException&) {
        return 1;
      } catch (const IndexOutOfBoundsException&) {
        return 2;
      }
      return 0;
    };
    CHECK(refused({{0, 3}, {2, 6}}) == 1 && refused({{3, 1}}) == 1 && refused({{2, 2}}) == 1 && refused({}) == 1);
    CHECK(refused({{0, 7}}) == 2);
    const auto r = model.predictRanges(w, {{0, 1}, {3, 3}, {1, 6}});
    CHECK(r.predictions.size() == 6 && r.counts.size() == 9 && r.counts[1] == 1 && r.counts[3] + r.counts[4] + r.counts[5] == 0 && r.counts[7] == 5);
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  cpu_checks();
  if (mode == "gpu") gpu_checks();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::fprintf(stderr, "predict mirror (%s): all checks passed\n", mode.c_str());
  return 0;
}
