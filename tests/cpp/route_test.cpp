// csrc/dsgd_route.hpp on its own, on the CPU: the switches dsgd_create reads and which kernel family serves a call.  Built
// with -fsanitize=address,undefined and run directly by tests/test_route.py.
//
// Two kinds of check:
//   (a) outright assertions: every knob's default and clamp, both sides of every threshold of the row ranges' route at the
//       default knobs and RCV1's shape, the order of precedence of the plan and request routes, the slice count against the
//       host builder's wording, the column lists' back-off step by step, both sides of every threshold of the evaluation
//       kernels' lanes per row (eval_group) against the expression dsgd_load_csr held;
//   (b) a 64-bit FNV-1a digest of every function's outputs over a fixed grid (the edge values x each knob changed alone x the
//       context's facts), held to constants recorded from the lines these functions replaced in csrc/dsgd_hip.hip at commit
//       09dd9cb: the same grid driver (digest_grid below) ran over those lines, pasted around a stand-in context, in a
//       recorder that was not kept.  The constants are the parent's: nothing here prints the header's own digests in
//       their place.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "dsgd_route.hpp"

static int g_checks = 0;
static void check_(bool ok, const char* file, int line, const char* what) {
  ++g_checks;
  if (!ok) {
    std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", file, line, what);
    std::exit(1);
  }
}
#define CHECK(cond) check_((cond), __FILE__, __LINE__, #cond)   // (an expression: the checks below chain it behind a comma)

struct Fnv {
  uint64_t h = 1469598103934665603ULL;
  void num(long long v) {
    unsigned char b[sizeof v];
    std::memcpy(b, &v, sizeof v);
    for (size_t i = 0; i < sizeof v; ++i) h = (h ^ b[i]) * 1099511628211ULL;
  }
};

typedef std::vector<std::pair<std::string, std::string>> Env;   // name -> value: the lookup knobs_read is given

// every name of the table, in the order the digest lists the values
static const char* const NAMES[] = {
    "DSGD_FIX_SHIFT", "DSGD_FIX_BOUND", "DSGD_PLAN_KERNEL", "DSGD_VT", "DSGD_CS", "DSGD_CS_G", "DSGD_CS_MAX_MB", "DSGD_CS_HOST_LAYOUT",
    "DSGD_CS_REQ", "DSGD_CACHE_MB", "DSGD_TEST_CS_SKIP_PUBLISH", "DSGD_REQ_MAPPED", "DSGD_REQ_PLAN", "DSGD_STREAM_MIN", "DSGD_FSTEP",
    "DSGD_FSTEP_MIN", "DSGD_FSTEP_MAX", "DSGD_FSTEP_ROWS", "DSGD_FSTEP_REBALANCE", "DSGD_TCOL", "DSGD_TCOL_MIN", "DSGD_TCOL_MAX",
    "DSGD_TCOL_MAX_NNZ", "DSGD_TCOL_SHARE", "DSGD_REQ_SPIN", "DSGD_CS_NT", "DSGD_VT_TPW", "DSGD_VT_PACK_MB", "DSGD_HSPLIT",
    "DSGD_RP64_FUSED", "DSGD_PLAN_PROF"};
constexpr int N_NAMES = (int)(sizeof(NAMES) / sizeof(NAMES[0]));

struct PlanIn {
  bool rp64, cs_current, fits_here, vt_current, layout_tried;
  long long max_step_rows;
  int n_workers;
};

// ---- the header under test as the grid driver calls it: knobs from a lookup, facts, every function's outputs as integers ----
struct HeaderImpl {
  Knobs k;
  RouteFacts f;
  void set_env(const Env& env) {
    k = Knobs();
    knobs_read(k, [&](const char* name) -> const char* {
      for (const auto& e : env)
        if (e.first == name) return e.second.c_str();
      return nullptr;
    });
  }
  void set_facts(const RouteFacts& facts) { f = facts; }
  // the values in the order of NAMES (DSGD_CACHE_MB as the bytes of the plans' cache, as dsgd_create sets it)
  std::vector<long long> knob_values() const {
    return {k.max_shift, k.fix_bound, k.plan_kernel, k.vt_enable, k.cs_enable, k.cs_g, k.cs_max_mb, k.cs_host_layout, k.cs_req,
            (long long)((size_t)k.cache_mb << 20), k.cs_test_skip, k.req_mapped, k.req_plan, k.stream_min, k.fstep_enable, k.fstep_min,
            k.fstep_max, k.fstep_rows, k.fstep_rebalance, k.tcol_enable, k.tcol_min, k.tcol_max, k.tcol_max_nnz, k.tcol_share,
            k.req_spin, k.cs_nt, k.vt_tpw, k.vt_pack_mb, k.hsplit, k.rp64_fused, k.plan_prof};
  }
  int possible() const { return fstep_possible(k, f); }
  int grid(int nw, long long tot, long long ent, long long smallest) const { return fstep_grid(k, f, nw, tot, ent, smallest); }
  int wanted(long long tot, int nw) const { return tcol_wanted(k, f, tot, nw); }
  int one_wg_ok(long long rows, int nw) const { return plan_kernel_ok(k, f, rows, nw); }
  int pick_G(int K, bool request) const { return cs_pick_G(k, f, K, request); }
  void ranges(int nw, long long tot, long long ent, long long smallest, int out[3]) const {
    const RangesRoute r = route_ranges(k, f, nw, tot, ent, smallest);
    out[0] = r.try_tcol, out[1] = r.then, out[2] = r.fstep_wg;
  }
  PlanFacts plan_facts(const PlanIn& p) const {
    PlanFacts pf;
    pf.rp64 = p.rp64, pf.cs_current = p.cs_current, pf.fits_here = p.fits_here, pf.vt_current = p.vt_current;
    pf.max_step_rows = p.max_step_rows, pf.n_workers = p.n_workers;
    return pf;
  }
  int plan_info(const PlanIn& p) const { return plan_info_code(route_plan(k, f, plan_facts(p)), p.layout_tried); }
  // the arm dsgd_plan_run takes, as plan_info's code for it (-1: an fp64 context refuses the plan)
  int plan_run(const PlanIn& p) const {
    const PlanRoute r = route_plan(k, f, plan_facts(p));
    if (f.fp64 && r != PLAN_RP64 && r != PLAN_CS64) return -1;
    return plan_info_code(r, true);
  }
  int lays_out(bool rp64, bool have_data, bool have_ds) const { return plan_lays_out_at_creation(k, f, rp64, have_data, have_ds); }
  void request(int K, long long rows, bool fit, bool valid, int out[3]) const {
    const RequestRoute r = route_request(k, f, K, rows, [&] { return fit; }, [&] { return valid; });
    out[0] = r.first, out[1] = r.first == REQ_CS ? r.rowwise : -1, out[2] = r.G;
  }
};

// ---- the grid -----------------------------------------------------------------------------------------------------------
static RouteFacts rcv1_facts() {
  RouteFacts f;
  f.dp = 47237;
  f.n_rows = 804414;
  f.n_cu = 256;
  f.hsplit = HSPLIT_MAX & ~3;
  f.cold_col16 = true;
  f.coldm_nnz = 1000000;
  return f;
}
static std::vector<RouteFacts> layout_facts() {   // the layouts the row ranges' route distinguishes
  std::vector<RouteFacts> v;
  v.push_back(rcv1_facts());
  RouteFacts f = rcv1_facts();
  f.cold_col16 = false, v.push_back(f);
  f = rcv1_facts(), f.coldm_nnz = 0, v.push_back(f);
  f = rcv1_facts(), f.n_rows = (1LL << 31) - 1, v.push_back(f);
  f = rcv1_facts(), f.n_rows = 1LL << 31, v.push_back(f);
  f = rcv1_facts(), f.dp = 70001, v.push_back(f);                       // more cold columns than the LDS tile holds
  f = rcv1_facts(), f.dp = f.hsplit + (DSGD_LDS_FLOATS - 16 * CT_STRIP - 64 - 4), v.push_back(f);       // ... exactly as many
  f = rcv1_facts(), f.dp = f.hsplit + (DSGD_LDS_FLOATS - 16 * CT_STRIP - 64 - 4) + 1, v.push_back(f);   // ... one more
  f = rcv1_facts(), f.dp = f.hsplit, v.push_back(f);                    // no cold column
  f = rcv1_facts(), f.dp = 100, v.push_back(f);
  f = rcv1_facts(), f.n_cu = 64, v.push_back(f);
  f = rcv1_facts(), f.dp = 262143, v.push_back(f);                      // 64 workers x dp = 2^24 - 64
  f = rcv1_facts(), f.dp = 262144, v.push_back(f);                      // ... = 2^24
  return v;
}
static std::vector<Env> knob_envs() {   // nothing set, then each knob that bears on a route changed alone
  std::vector<Env> v;
  v.push_back({});
  const char* one[][2] = {{"DSGD_FSTEP", "0"},          {"DSGD_TCOL", "0"},           {"DSGD_CS", "0"},          {"DSGD_CS_REQ", "1"},
                          {"DSGD_REQ_PLAN", "1"},       {"DSGD_PLAN_KERNEL", "0"},    {"DSGD_VT", "0"},          {"DSGD_CS_G", "8"},
                          {"DSGD_CS_G", "16"},          {"DSGD_CS_G", "12"},          {"DSGD_STREAM_MIN", "1"},  {"DSGD_STREAM_MIN", "98304"},
                          {"DSGD_FSTEP_MIN", "1"},      {"DSGD_FSTEP_MIN", "9000"},   {"DSGD_FSTEP_MAX", "100000"}, {"DSGD_FSTEP_ROWS", "1"},
                          {"DSGD_FSTEP_ROWS", "100000"}, {"DSGD_TCOL_MIN", "1"},      {"DSGD_TCOL_MIN", "100000"}, {"DSGD_TCOL_MAX", "1000"},
                          {"DSGD_TCOL_MAX", "600000"},  {"DSGD_TCOL_MAX_NNZ", "1"},   {"DSGD_TCOL_MAX_NNZ", "100000"}, {"DSGD_HSPLIT", "64"},
                          {"DSGD_FIX_SHIFT", "12"},     {"DSGD_CS_HOST_LAYOUT", "1"}, {"DSGD_REQ_SPIN", "0"},    {"DSGD_REQ_MAPPED", "0"}};
  for (const auto& e : one) v.push_back({{e[0], e[1]}});
  v.push_back({{"DSGD_CS_REQ", "1"}, {"DSGD_REQ_PLAN", "1"}});
  v.push_back({{"DSGD_CS_REQ", "1"}, {"DSGD_CS_G", "16"}});
  v.push_back({{"DSGD_TCOL", "0"}, {"DSGD_FSTEP", "0"}});
  return v;
}
static const char* const PARSE_STRINGS[] = {"", "abc", "0", "1", "-1", "-5", "7", "8", "9", "12", "16", "20", "21", "22", "99", "255", "256", "257",
                                            "8191", "100000", "2147483647", "-2147483648", "4500001", "9000000000", "12abc", " 3", "+4", "1e3"};

static void digest_grid(uint64_t out[8]) {
  HeaderImpl m;
  Fnv d_knobs, d_pred, d_ranges, d_plan, d_request, d_G, d_gate, d_create;
  // the knobs: nothing set, then every name alone with every string
  m.set_env({});
  for (long long v : m.knob_values()) d_knobs.num(v);
  for (int n = 0; n < N_NAMES; ++n)
    for (const char* s : PARSE_STRINGS) {
      if (!std::strcmp(s, "9000000000") && !(!std::strcmp(NAMES[n], "DSGD_STREAM_MIN") || !std::strncmp(NAMES[n], "DSGD_FSTEP_M", 12) ||
                                             !std::strcmp(NAMES[n], "DSGD_FSTEP_ROWS") || !std::strncmp(NAMES[n], "DSGD_TCOL_M", 11)))
        continue;   // (atoi beyond int is undefined: that string goes only to the names atoll reads)
      m.set_env({{NAMES[n], s}});
      for (long long v : m.knob_values()) d_knobs.num(v);
    }
  const std::vector<Env> envs = knob_envs();
  const std::vector<RouteFacts> layouts = layout_facts();
  // row ranges
  const long long TOT[] = {1, 511, 512, 8191, 8192, 65535, 65536, 98303, 98304, 131071, 131072, 524224, 524225, 1LL << 31, (1LL << 31) + 1};
  const int NW[] = {1, 3, 64, 65, 256, 257};
  for (const Env& env : envs) {
    m.set_env(env);
    for (const RouteFacts& f : layouts) {
      m.set_facts(f);
      d_pred.num(m.possible());
      for (long long tot : TOT)
        for (int nw : NW) {
          d_pred.num(m.wanted(tot, nw));
          const long long ENT[] = {tot * 75, 100000, 100001, 4500000, 4500001};
          const long long SMALL[] = {std::max<long long>(1, tot / nw), 1, 511, 512, 1024, tot};
          for (long long ent : ENT)
            for (long long sm : SMALL) {
              if (sm > tot) continue;   // (the smallest range is no longer than all of them)
              int r[3];
              m.ranges(nw, tot, ent, sm, r);
              d_ranges.num(r[0]), d_ranges.num(r[1]), d_ranges.num(r[2]);
              d_pred.num(m.grid(nw, tot, ent, sm));
            }
        }
    }
  }
  // plans and requests: every combination of the boolean facts
  for (const Env& env : envs) {
    m.set_env(env);
    for (int fb = 0; fb < 32; ++fb) {
      RouteFacts f = rcv1_facts();
      f.comm = fb & 1, f.prof = fb & 2, f.fp64 = fb & 4, f.val64 = fb & 8, f.async_running = fb & 16;
      if (f.val64 && !f.fp64) continue;   // (Double data is loaded into fp64 contexts only)
      m.set_facts(f);
      for (int K : {1, 2, 8, 9})
        for (long long rows : {192LL, 1024LL, 1025LL, 2048LL, 2049LL}) {
          d_pred.num(m.one_wg_ok(rows, K));
          for (int pb = 0; pb < 32; ++pb) {
            // (a layout that is current was tried: bit 4 says so for one that was tried and declined)
            const PlanIn p{(pb & 1) != 0, (pb & 2) != 0, (pb & 4) != 0, (pb & 8) != 0, (pb & (16 | 2 | 8)) != 0, rows, K};
            if (p.rp64 && !f.fp64) continue;   // (row-parallel plans exist in fp64 contexts only)
            d_plan.num(m.plan_info(p));
            if (!(f.fp64 && f.comm && !p.rp64)) d_plan.num(m.plan_run(p));   // (an fp64 context under a communicator refuses other plans before the route)
          }
          for (int qb = 0; qb < 4; ++qb) {
            int r[3];
            m.request(K, rows, (qb & 1) != 0, (qb & 2) != 0, r);
            d_request.num(r[0]), d_request.num(r[1]), d_request.num(r[2]);
          }
        }
      for (int cb = 0; cb < 8; ++cb) d_create.num(m.lays_out((cb & 1) != 0, (cb & 2) != 0, (cb & 4) != 0));
    }
  }
  // the slice count (a coarse walk here: the whole domain is compared with the host builder's wording in the checks)
  for (const char* g : {"", "8", "16"}) {
    m.set_env(*g ? Env{{"DSGD_CS_G", g}} : Env{});
    for (int dp = 1; dp <= (1 << 21); dp += (dp < 4096 ? 1 : 997)) {
      RouteFacts f = rcv1_facts();
      f.dp = dp;
      m.set_facts(f);
      for (int K = 1; K <= CS_MAX_K; ++K) d_G.num(m.pick_G(K, false)), d_G.num(m.pick_G(K, true));
    }
  }
  // the back-off: a fixed script of hits, misses and resets
  {
    TcolGate g;
    unsigned int x = 12345u;
    for (int i = 0; i < 4000; ++i) {
      x = x * 1664525u + 1013904223u;
      const unsigned int op = (x >> 16) % 97u;
      if (op == 0)
        g.reset(), d_gate.num(-1);
      else if (op < 4 && i > 1000)
        g.hit(), d_gate.num(-2);
      else
        d_gate.num(g.miss());
    }
  }
  const Fnv* all[8] = {&d_knobs, &d_pred, &d_ranges, &d_plan, &d_request, &d_G, &d_gate, &d_create};
  for (int i = 0; i < 8; ++i) out[i] = all[i]->h;
}

// recorded from csrc/dsgd_hip.hip at 09dd9cb (see the head of this file)
static const uint64_t PARENT_DIGESTS[8] = {
    0x943f594559b5a6afULL,   // knobs
    0x92ad94f40a43be1cULL,   // predicates
    0xfbecbb40e25d99c4ULL,   // route_ranges
    0x48ab8c771e5df783ULL,   // route_plan
    0x4892cbb5ddac68c3ULL,   // route_request
    0xe05edb06d9296483ULL,   // cs_pick_G
    0x25a2540c3c46db5bULL,   // TcolGate
    0x471bbdc7af1a4583ULL,   // plan_lays_out_at_creation
};
static const char* const DIGEST_NAMES[8] = {"knobs", "predicates", "route_ranges", "route_plan", "route_request", "cs_pick_G", "TcolGate", "plan_lays_out_at_creation"};

static Knobs parse(const Env& env) {
  HeaderImpl m;
  m.set_env(env);
  return m.k;
}
static long long value_of(const Knobs& k, const char* name) {
  HeaderImpl m;
  m.k = k;
  const std::vector<long long> v = m.knob_values();
  for (int n = 0; n < N_NAMES; ++n)
    if (!std::strcmp(NAMES[n], name)) return v[(size_t)n];
  CHECK(!"a name of the table");
  return 0;
}
static long long parsed(const char* name, const char* s) { return value_of(parse({{name, s}}), name); }

static void test_knobs() {
  // nothing set: the documented defaults (README.md, the comments of struct Knobs)
  const Knobs d = parse({});
  CHECK(d.max_shift == 21 && d.fix_bound && d.hsplit == 18398 && d.stream_min == 131072 && d.fstep_enable && !d.fstep_rebalance);
  CHECK(d.fstep_min == 65536 && d.fstep_max == (1LL << 31) && d.fstep_rows == 512);
  CHECK(d.tcol_enable && d.tcol_min == 512 && d.tcol_max == 98303 && d.tcol_max_nnz == 4500000 && d.tcol_share == 0);
  CHECK(d.cs_enable && d.cs_g == 0 && d.cs_max_mb == 8192 && d.cs_nt == 0 && !d.cs_host_layout && d.cache_mb == 8192);
  CHECK(d.plan_kernel && d.vt_enable && d.vt_pack_mb == 2048 && d.vt_tpw == 1 && !d.plan_prof);
  CHECK(!d.cs_req && d.req_mapped && d.req_spin && !d.req_plan && d.rp64_fused == RP64_FUSED_DEFAULT && d.cs_test_skip == 0);
  // every name of the table is one the digest lists, and the other way round
  CHECK((int)(sizeof(KNOBS) / sizeof(KNOBS[0])) == N_NAMES);
  for (const KnobSpec& s : KNOBS) {
    bool found = false;
    for (const char* n : NAMES) found = found || !std::strcmp(n, s.name);
    CHECK(found);
  }
  // the clamps, at, below and above
  CHECK(parsed("DSGD_FIX_SHIFT", "0") == 8 && parsed("DSGD_FIX_SHIFT", "7") == 8 && parsed("DSGD_FIX_SHIFT", "8") == 8 && parsed("DSGD_FIX_SHIFT", "9") == 9);
  CHECK(parsed("DSGD_FIX_SHIFT", "20") == 20 && parsed("DSGD_FIX_SHIFT", "21") == 21 && parsed("DSGD_FIX_SHIFT", "22") == 21 && parsed("DSGD_FIX_SHIFT", "99") == FIX_SHIFT);
  CHECK(parsed("DSGD_FIX_SHIFT", "abc") == 8 && parsed("DSGD_FIX_SHIFT", "") == 8);
  CHECK(parsed("DSGD_CS_G", "8") == 8 && parsed("DSGD_CS_G", "16") == 16 && parsed("DSGD_CS_G", "12") == 0 && parsed("DSGD_CS_G", "abc") == 0 && parsed("DSGD_CS_G", "") == 0);
  CHECK(parsed("DSGD_CS_NT", "256") == CS_THREADS_NARROW && parsed("DSGD_CS_NT", "255") == 0 && parsed("DSGD_CS_NT", "257") == 0 && parsed("DSGD_CS_NT", "") == 0);
  for (const char* n : {"DSGD_STREAM_MIN", "DSGD_FSTEP_MIN", "DSGD_FSTEP_MAX", "DSGD_FSTEP_ROWS", "DSGD_TCOL_MIN", "DSGD_TCOL_MAX", "DSGD_TCOL_MAX_NNZ"}) {
    CHECK(parsed(n, "0") == 1 && parsed(n, "-5") == 1 && parsed(n, "1") == 1 && parsed(n, "7") == 7 && parsed(n, "abc") == 1 && parsed(n, "") == 1);
    CHECK(parsed(n, "9000000000") == 9000000000LL);
  }
  for (const char* n : {"DSGD_CS_MAX_MB", "DSGD_VT_PACK_MB", "DSGD_TCOL_SHARE"})
    CHECK(parsed(n, "-5") == 0 && parsed(n, "-1") == 0 && parsed(n, "0") == 0 && parsed(n, "1") == 1 && parsed(n, "abc") == 0 && parsed(n, "") == 0);
  CHECK(parsed("DSGD_CACHE_MB", "-5") == 0 && parsed("DSGD_CACHE_MB", "1") == (1 << 20) && parsed("DSGD_CACHE_MB", "abc") == 0);
  CHECK(parsed("DSGD_VT_TPW", "0") == 1 && parsed("DSGD_VT_TPW", "-5") == 1 && parsed("DSGD_VT_TPW", "1") == 1 && parsed("DSGD_VT_TPW", "7") == 7 && parsed("DSGD_VT_TPW", "abc") == 1);
  CHECK(parsed("DSGD_HSPLIT", "-5") == -5 && parsed("DSGD_HSPLIT", "0") == 0 && parsed("DSGD_HSPLIT", "100000") == 100000 && parsed("DSGD_HSPLIT", "abc") == 0);
  for (const KnobSpec& s : KNOBS)
    if (s.kind == KNOB_FLAG) {
      CHECK(parsed(s.name, "0") == 0 && parsed(s.name, "1") == 1 && parsed(s.name, "7") == 1 && parsed(s.name, "-1") == 1);
      CHECK(parsed(s.name, "abc") == 0 && parsed(s.name, "") == 0);
    }
    // the test-only name: this program is built without the seam define
#ifndef DSGD_TEST_COLLECTIVE_SEAM
  CHECK(parsed("DSGD_TEST_CS_SKIP_PUBLISH", "7") == 0);
#else
  CHECK(parsed("DSGD_TEST_CS_SKIP_PUBLISH", "7") == 7 && parsed("DSGD_TEST_CS_SKIP_PUBLISH", "-5") == 0);
#endif
  // a name changes its own field and no other
  for (int n = 0; n < N_NAMES; ++n) {
    HeaderImpl a, b;
    a.set_env({});
    b.set_env({{NAMES[n], "7"}});
    const std::vector<long long> va = a.knob_values(), vb = b.knob_values();
    for (int i = 0; i < N_NAMES; ++i)
      if (i != n) CHECK(va[(size_t)i] == vb[(size_t)i]);
  }
}

// the row ranges' route at the default knobs, RCV1's dp and 256 CUs
struct R3 {
  bool tcol;
  RangesThen then;
  int wg;
};
static R3 ranges_of(const Knobs& k, const RouteFacts& f, int nw, long long tot, long long ent, long long smallest) {
  const RangesRoute r = route_ranges(k, f, nw, tot, ent, smallest);
  return {r.try_tcol, r.then, r.fstep_wg};
}
static void test_route_ranges() {
  const Knobs k;
  const RouteFacts f = rcv1_facts();
  auto one = [&](long long tot, long long ent) { return ranges_of(k, f, 1, tot, ent, tot); };
  // 511 / 512 rows: the column lists begin
  CHECK(!one(511, 511 * 75).tcol && one(511, 511 * 75).then == RANGES_ROWWISE);
  CHECK(one(512, 512 * 75).tcol && one(512, 512 * 75).then == RANGES_ROWWISE);
  // 98,303 / 98,304 rows of few non-zeros: they end (row chunks from 65,536 rows on are their fall-back, then their successor)
  CHECK(one(98303, 98303 * 10).tcol && one(98303, 98303 * 10).then == RANGES_FSTEP);
  CHECK(!one(98304, 98304 * 10).tcol && one(98304, 98304 * 10).then == RANGES_FSTEP);
  // 65,535 / 65,536 rows: the row chunks begin (behind the column lists, which still want both)
  CHECK(one(65535, 65535 * 10).tcol && one(65535, 65535 * 10).then == RANGES_ROWWISE && one(65535, 65535 * 10).wg == 0);
  CHECK(one(65536, 65536 * 10).tcol && one(65536, 65536 * 10).then == RANGES_FSTEP && one(65536, 65536 * 10).wg == 128);
  // 131,071 / 131,072 rows with row chunks off: the streaming launches begin
  {
    Knobs off;
    off.fstep_enable = false;
    CHECK(ranges_of(off, f, 1, 131071, 131071 * 75, 131071).then == RANGES_ROWWISE && !ranges_of(off, f, 1, 131071, 131071 * 75, 131071).tcol);
    CHECK(ranges_of(off, f, 1, 131072, 131072 * 75, 131072).then == RANGES_STREAM && ranges_of(off, f, 1, 131072, 131072 * 75, 131072).wg == 0);
    CHECK(ranges_of(off, f, 1, 98303, 98303LL * 75, 98303).tcol);   // (more entries than DSGD_TCOL_MAX_NNZ, and nobody to hand over to)
  }
  // the hand-over by entries: from 8,192 rows on, more than tcol_max_nnz entries go to the row chunks
  CHECK(one(8191, k.tcol_max_nnz + 1).tcol && one(8191, k.tcol_max_nnz + 1).then == RANGES_ROWWISE && one(8191, k.tcol_max_nnz + 1).wg == 0);
  CHECK(!one(8192, k.tcol_max_nnz + 1).tcol && one(8192, k.tcol_max_nnz + 1).then == RANGES_FSTEP && one(8192, k.tcol_max_nnz + 1).wg == 16);
  CHECK(one(8192, k.tcol_max_nnz).tcol && one(8192, k.tcol_max_nnz).then == RANGES_ROWWISE);
  CHECK(one(70000, k.tcol_max_nnz).tcol && one(70000, k.tcol_max_nnz).then == RANGES_FSTEP);   // (chunks possible, the lists keep it)
  CHECK(!one(70000, k.tcol_max_nnz + 1).tcol && one(70000, k.tcol_max_nnz + 1).then == RANGES_FSTEP);
  // 64 / 65 workers: the column lists' limit; 256 / 257: the row chunks' (one workgroup per worker at least, n_cu in all)
  CHECK(ranges_of(k, f, 64, 70000, 700000, 1000).tcol && !ranges_of(k, f, 65, 70000, 700000, 1000).tcol);
  CHECK(ranges_of(k, f, 256, 200000, 200000 * 75, 700).then == RANGES_FSTEP && ranges_of(k, f, 256, 200000, 200000 * 75, 700).wg == 1);
  CHECK(ranges_of(k, f, 257, 200000, 200000 * 75, 700).then == RANGES_STREAM && ranges_of(k, f, 257, 200000, 200000 * 75, 700).wg == 0);
  // the bitmap: tot + 64 x workers at TC_MAX_BITS and one above (the row limit raised to let the rows through)
  {
    Knobs wide;
    wide.tcol_max = 1LL << 30;
    CHECK(tcol_wanted(wide, f, TC_MAX_BITS - 64 * 3, 3) && !tcol_wanted(wide, f, TC_MAX_BITS - 64 * 3 + 1, 3));
  }
  // workers x dp at 2^24 - 1 and 2^24 (a model of 2^18 columns, 64 workers; 2^24 - 1 itself at one worker)
  {
    RouteFacts g = f;
    g.dp = (1 << 24) - 1;
    CHECK(tcol_wanted(k, g, 1000, 1));
    g.dp = 1 << 24;
    CHECK(!tcol_wanted(k, g, 1000, 1));
    g.dp = 1 << 18;
    CHECK(tcol_wanted(k, g, 10000, 63) && !tcol_wanted(k, g, 10000, 64));
  }
  // the grid: smallest range / fstep_rows = 0 (one workgroup all the same), 1, and more than n_cu / workers
  CHECK(fstep_grid(k, f, 4, 100000, 7500000, 511) == 1 && fstep_grid(k, f, 4, 100000, 7500000, 512) == 1 && fstep_grid(k, f, 4, 100000, 7500000, 1024) == 2);
  CHECK(fstep_grid(k, f, 4, 100000, 7500000, 25000) == 48 && fstep_grid(k, f, 4, 1000000, 75000000, 250000) == 64);
  // fstep_possible, each reason in turn
  {
    CHECK(fstep_possible(k, f));
    Knobs off;
    off.fstep_enable = false;
    CHECK(!fstep_possible(off, f));
    RouteFacts g = f;
    g.dp = g.hsplit, CHECK(!fstep_possible(k, g));   // no cold column
    g.dp = g.hsplit - 5, CHECK(!fstep_possible(k, g));
    g = f, g.dp = g.hsplit + (DSGD_LDS_FLOATS - 16 * CT_STRIP - 64 - 4), CHECK(fstep_possible(k, g));
    g.dp += 1, CHECK(!fstep_possible(k, g));         // a cold column beyond the LDS tile
    g = f, g.cold_col16 = false, CHECK(!fstep_possible(k, g));
    g = f, g.coldm_nnz = 0, CHECK(!fstep_possible(k, g));
    g = f, g.n_rows = (1LL << 31) - 1, CHECK(fstep_possible(k, g));
    g.n_rows = 1LL << 31, CHECK(!fstep_possible(k, g));
    CHECK(fstep_grid(k, f, 1, k.fstep_max, 75 * k.fstep_max, k.fstep_max) > 0 && fstep_grid(k, f, 1, k.fstep_max + 1, 75 * k.fstep_max, k.fstep_max) == 0);
  }
  // Whole-split steps of RCV1-like rows (75 non-zeros), one worker, at the sizes the thresholds' comments quote.  The family is
  // the one profiles/r06_dispatch_table.txt records under its second table, "after (DSGD_TCOL_MAX_NNZ = 4.5 M)": column
  // lists up to 4.5 M entries (60,000 rows), row chunks beyond.  (Its third section, the crossover scan that SET the
  // threshold, still shows 80,441 rows on the column lists: it was measured before the threshold existed.)
  CHECK(one(4800, 4800 * 75).tcol && one(18519, 18519 * 75).tcol && one(60000, 60000 * 75).tcol);
  for (long long n : {80441LL, 160000LL, 643531LL, 6710886LL}) CHECK(!one(n, n * 75).tcol && one(n, n * 75).then == RANGES_FSTEP);
  CHECK(one(80441, 80441 * 75).wg == 157 && one(160000, 160000 * 75).wg == 256 && one(6710886, 6710886LL * 75).wg == 256);
  // ... and the rows of that second table whose model size it states: D = 20,000 (row chunks possible) and D = 70,000 (51,604
  // cold columns do not fit the LDS tile: the streaming launches take the large ranges)
  {
    RouteFacts g = f;
    g.dp = 20001;
    const struct { long long rows; double nnz; bool tcol; } t20[] = {{2000, 76.6, true}, {20000, 75.3, true}, {80000, 75.2, false}, {200000, 75.1, false}, {800000, 75.0, false}};
    for (const auto& t : t20) {
      const R3 r = ranges_of(k, g, 1, t.rows, (long long)(t.rows * t.nnz), t.rows);
      CHECK(r.tcol == t.tcol && (t.tcol || r.then == RANGES_FSTEP));
    }
    g.dp = 70001;
    const struct { long long rows; bool tcol; RangesThen then; } t70[] = {{2000, true, RANGES_ROWWISE}, {20000, true, RANGES_ROWWISE}, {80000, true, RANGES_ROWWISE}, {200000, false, RANGES_STREAM}, {800000, false, RANGES_STREAM}};
    for (const auto& t : t70) {
      const R3 r = ranges_of(k, g, 1, t.rows, t.rows * 75, t.rows);
      CHECK(r.tcol == t.tcol && r.then == t.then && r.wg == 0);
    }
  }
}

static void test_route_plan_and_request() {
  // plan_info's code for every arm, once
  CHECK(plan_info_code(PLAN_RP64, false) == 6 && plan_info_code(PLAN_CS64, false) == 5 && plan_info_code(PLAN_CS, false) == 1);
  CHECK(plan_info_code(PLAN_ONE_WG, false) == 2 && plan_info_code(PLAN_VT, false) == 3);
  CHECK(plan_info_code(PLAN_ROWWISE, false) == 0 && plan_info_code(PLAN_ROWWISE, true) == 4 && plan_info_code(PLAN_CS, true) == 1);
  const Knobs k;
  Knobs k_req = k;
  k_req.req_plan = true, k_req.cs_req = true;
  for (int fb = 0; fb < 16; ++fb) {
    RouteFacts f = rcv1_facts();
    f.comm = fb & 1, f.prof = fb & 2, f.fp64 = fb & 4, f.val64 = fb & 8;
    for (int K : {1, 2, 8, 9})
      for (long long rows : {192LL, 2048LL, 2049LL}) {
        // plans: the order of precedence, outright
        for (int pb = 0; pb < 16; ++pb) {
          PlanFacts p;
          p.rp64 = pb & 1, p.cs_current = pb & 2, p.fits_here = pb & 4, p.vt_current = pb & 8;
          p.max_step_rows = rows, p.n_workers = K;
          const PlanRoute r = route_plan(k, f, p);
          const bool one = K == 1 && rows <= 2048 && !f.comm && p.fits_here;
          const PlanRoute want = p.rp64 ? PLAN_RP64 : (p.cs_current && !f.comm) ? (f.fp64 ? PLAN_CS64 : PLAN_CS) : one ? PLAN_ONE_WG : p.vt_current ? PLAN_VT : PLAN_ROWWISE;
          CHECK(r == want);
          Knobs off = k;
          off.cs_enable = false, off.plan_kernel = false, off.vt_enable = false;   // (an fp64 context has its slices whatever DSGD_CS says)
          CHECK(route_plan(off, f, p) == (p.rp64 ? PLAN_RP64 : (p.cs_current && !f.comm && f.fp64) ? PLAN_CS64 : PLAN_ROWWISE));
        }
        // requests: fp64 first (ranks, Double data, slices), then one workgroup, the column-slice request, row-wise
        for (int qb = 0; qb < 4; ++qb) {
          const bool fit = qb & 1, valid = qb & 2;
          int asked = 0;
          const RequestRoute r = route_request(k_req, f, K, rows, [&] { return ++asked, fit; }, [&] { return ++asked, valid; });
          const RequestArm rowwise = (f.comm || f.prof) ? REQ_ROWWISE_READBACK : REQ_ROWWISE_MAIL;
          RequestArm want = rowwise;
          if (f.fp64)
            want = f.comm ? REQ_F64_RANKS : f.val64 ? REQ_F64_ROWS : REQ_F64_CS;
          else if (K == 1 && rows <= 2048 && !f.comm && fit)
            want = f.prof ? REQ_ONE_WG_READBACK : REQ_ONE_WG_MAIL;
          else if (!f.comm && !f.prof && K <= 8 && rows <= 1024 && valid)
            want = REQ_CS;
          CHECK(r.first == want && r.rowwise == rowwise && (r.G != 0) == (want == REQ_CS));
          if (want == REQ_CS) CHECK(r.G == cs_pick_G(k_req, f, K, true) && r.rowwise == REQ_ROWWISE_MAIL);
          if (f.fp64) CHECK(asked == 0);   // (the lists are scanned only where the answer decides)
          // at the default knobs neither the one-workgroup kernel nor the column-slice request serves a request
          const RequestRoute d = route_request(k, f, K, rows, [&] { return fit; }, [&] { return valid; });
          CHECK(d.first == (f.fp64 ? want : rowwise) && d.G == 0);
        }
      }
  }
  // a plan's slices are laid out at creation: every condition in turn
  {
    RouteFacts f = rcv1_facts();
    CHECK(plan_lays_out_at_creation(k, f, false, true, true));
    CHECK(!plan_lays_out_at_creation(k, f, true, true, true) && !plan_lays_out_at_creation(k, f, false, false, true) && !plan_lays_out_at_creation(k, f, false, true, false));
    Knobs off = k;
    off.cs_enable = false;
    CHECK(!plan_lays_out_at_creation(off, f, false, true, true));
    f.fp64 = true, CHECK(plan_lays_out_at_creation(off, f, false, true, true));
    f.comm = true, CHECK(!plan_lays_out_at_creation(k, f, false, true, true));
    f.comm = false, f.async_running = true, CHECK(!plan_lays_out_at_creation(k, f, false, true, true));
  }
}

// the slice count as the host builder of the column slices worded it before it called cs_pick_G
static int host_builder_G(int cs_g, int dp, int K) {
  int G = cs_g ? cs_g : (K <= 4 ? 8 : 16);
  if (!cs_g && G == 8 && cs_lds_words(dp, 8, K) > DSGD_LDS_FLOATS) G = 16;
  if (dp < 4 * G || cs_lds_words(dp, G, K) > DSGD_LDS_FLOATS || (dp + G - 1) / G > 65536) return 0;
  return G;
}
static void test_slice_count() {
  long long differing = 0;
  for (int cs_g : {0, 8, 16}) {
    Knobs k;
    k.cs_g = cs_g;
    RouteFacts f = rcv1_facts();
    for (int dp = 1; dp <= (1 << 21); ++dp) {
      f.dp = dp;
      for (int K = 1; K <= CS_MAX_K; ++K) differing += cs_pick_G(k, f, K, false) != host_builder_G(cs_g, dp, K);
    }
  }
  CHECK(differing == 0);
  const Knobs k;
  RouteFacts f = rcv1_facts();
  CHECK(cs_pick_G(k, f, 3, false) == 8 && cs_pick_G(k, f, 4, false) == 8 && cs_pick_G(k, f, 5, false) == 16 && cs_pick_G(k, f, 8, false) == 16);
  f.dp = 31, CHECK(cs_pick_G(k, f, 1, false) == 0);
  f.dp = 32, CHECK(cs_pick_G(k, f, 1, false) == 8);
}

static void test_tcol_gate() {
  CHECK(TcolGate::MISSES == 12 && TcolGate::COOLDOWN == 256 && TcolGate::RESUME == 8);
  TcolGate g;
  for (int i = 1; i <= 12; ++i) CHECK(g.miss());   // misses 1-12 build
  CHECK(!g.miss());                                // the 13th starts the cooldown
  for (int i = 0; i < 256; ++i) CHECK(!g.miss());  // 256 declined steps
  CHECK(g.streak == 8 && g.cooldown == 0);
  for (int i = 0; i < 4; ++i) CHECK(g.miss());     // four more builds
  CHECK(!g.miss() && g.cooldown == 256);           // ... and out again
  g.reset();
  CHECK(g.streak == 0 && g.cooldown == 0);
  for (int i = 0; i < 12; ++i) CHECK(g.miss());
  g.hit();                                         // a hit clears the streak
  CHECK(g.streak == 0);
  for (int i = 0; i < 12; ++i) CHECK(g.miss());
  CHECK(!g.miss());
  g.hit();                                         // ... and not the cooldown
  CHECK(g.cooldown == 256 && !g.miss());
}

// lanes per row of the fp32 row-wise evaluation kernels: the expression dsgd_load_csr held, `mean > 192.0 ? 64 : (mean > 96.0 ?
// 32 : (mean > 12.0 ? 16 : 8))` with mean = (double)nnz / (double)n_rows, restated here and compared over a grid; both sides of
// every threshold at 1, 7 and 2^31 rows (the quotient of 12 n + 1 and n = 2^31 is 12 + 2^-31: a double holds it, a float would
// not); the degenerate inputs.
static int load_csr_group(long long nnz, long long n_rows) {
  const double mean = (double)nnz / (double)n_rows;
  return mean > 192.0 ? 64 : (mean > 96.0 ? 32 : (mean > 12.0 ? 16 : 8));
}
static void test_eval_group() {
  for (long long n : {1LL, 7LL, 1LL << 31}) {
    CHECK(eval_group(12 * n, n) == 8 && eval_group(12 * n + 1, n) == 16);
    CHECK(eval_group(96 * n, n) == 16 && eval_group(96 * n + 1, n) == 32);
    CHECK(eval_group(192 * n, n) == 32 && eval_group(192 * n + 1, n) == 64);
    CHECK(eval_group(12 * n - 1, n) == 8 && eval_group(96 * n - 1, n) == 16 && eval_group(192 * n - 1, n) == 32);
    CHECK(eval_group(0, n) == 8 && eval_group(n, n) == 8 && eval_group(75 * n, n) == 16 && eval_group(1000 * n, n) == 64);
  }
  // no rows (dsgd_load_csr refuses them; the expression's own answer): 0 / 0 is no number and compares false, n / 0 is +inf
  CHECK(eval_group(0, 0) == 8 && eval_group(5, 0) == 64);
  long long differing = 0;
  for (long long n : {1LL, 2LL, 3LL, 7LL, 100LL, 4095LL, 804414LL, (1LL << 31) - 1, 1LL << 31, 1LL << 40})
    for (long long per : {0LL, 1LL, 11LL, 12LL, 13LL, 95LL, 96LL, 97LL, 191LL, 192LL, 193LL, 5000LL})
      for (long long d = -2; d <= 2; ++d) {
        const long long nnz = per * n + d;
        if (nnz >= 0) differing += eval_group(nnz, n) != load_csr_group(nnz, n);
      }
  CHECK(differing == 0);
}

int main() {
  uint64_t got[8];
  digest_grid(got);
  test_eval_group();
  test_knobs();
  test_route_ranges();
  test_route_plan_and_request();
  test_slice_count();
  test_tcol_gate();
  for (int i = 0; i < 8; ++i) {
    if (got[i] != PARENT_DIGESTS[i])
      std::fprintf(stderr, "digest %s: 0x%016llx, the parent's 0x%016llx\n", DIGEST_NAMES[i], (unsigned long long)got[i], (unsigned long long)PARENT_DIGESTS[i]);
    CHECK(got[i] == PARENT_DIGESTS[i]);
  }
  std::fprintf(stderr, "route_test: all checks passed (%d)\n", g_checks);
  return 0;
}
