// Which kernel family serves a call, and the switches that bear on it.  Host only: no HIP type, no library call beyond
// atoi / atoll, so the same code runs under the sanitizers in tests/test_route.py (tests/cpp/route_test.cpp), which also
// holds every function here to digests recorded from the code this header replaced in csrc/dsgd_hip.hip.
//
//   Knobs          every switch dsgd_create reads from the environment, one table that parses them
//   RouteFacts     what a route needs from the context, as plain values (dsgd_hip.hip: route_facts)
//   route_ranges   dsgd_sync_step_ranges[_async], the ranges of a grouped step     -> column lists / row chunks / streaming / row-wise
//   route_plan     dsgd_plan_run and dsgd_plan_info                                 -> fp64 families / column slices / one workgroup /
//                                                                                     virtual tiles / row-wise
//   route_request  dsgd_sync_step                                                   -> the same families for ONE step of index lists
//   TcolGate       the column lists' back-off from callers that never repeat a configuration
//   eval_group     dsgd_load_csr[_f64]: lanes per row of the fp32 row-wise evaluation kernels
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>

#include "dsgd_limits.hpp"

// ------------------------------------------------------------------------------------------------
// knobs: fixed at dsgd_create
// ------------------------------------------------------------------------------------------------
constexpr bool FSTEP_PACKED_DEFAULT = true;   // (measured: every run of five faster than every run of the parent's library, profiles/fstep_packed_ab.txt)
struct Knobs {
  // -- the fixed-point grid
  int max_shift = FIX_SHIFT;         // DSGD_FIX_SHIFT: cap of the per-launch fixed-point shift of the split layout
  bool fix_bound = true;             // DSGD_FIX_BOUND=0: keep the data-independent bound (rows per workgroup x largest value)
  int hsplit = HSPLIT_MAX;           // DSGD_HSPLIT: hot/cold split rank as asked for (tests: wide models); dsgd_create clamps it to
                                     //   [1, HSPLIT_MAX] and aligns it: the context's hsplit is the one the layout uses
  // -- row ranges (dsgd_sync_step_ranges)
  long long stream_min = 131072;     // DSGD_STREAM_MIN: row ranges with at least this many rows use the streaming kernels.  Four
                                     //   launches of the split streams cost ~50 us whatever the range; the row-wise kernel + reduce
                                     //   take 37 us for 18,519 rows and 57 us for 80,000 (streaming: 49 / 63 us;
                                     //   profiles/r04_stream_min.txt)
  bool fstep_enable = true;          // DSGD_FSTEP=0: row ranges through the three streaming launches / the row-wise kernel
  bool fstep_rebalance = false;      // DSGD_FSTEP_REBALANCE=1: the chunks re-cut by their workgroups' measured durations (measured: 98.4 ->
                                     //   97.5 us at N = 804,414, nothing at 2 M / 6.7 M rows, and two layout rebuilds per configuration --
                                     //   which workgroup is slow is not a stable property of its chunk: OFF, profiles/r06_fstep_wg_times.txt)
  long long fstep_min = 65536;       // DSGD_FSTEP_MIN / DSGD_FSTEP_MAX: row ranges of this many rows in total take the chunked launch
  long long fstep_max = 1LL << 31;   //   (measured, whole-split steps, us: 80 K rows 56 -> 50-54, 643 K 118 -> 105, 1.6 M 213 -> 199,
                                     //    3.2 M 374 -> 343, 6.7 M 699 -> 663; at 18.5 K rows the row-wise kernel stays ahead: 37 vs 35-41)
  long long fstep_rows = 512;        // DSGD_FSTEP_ROWS: a chunk holds at least this many rows (fewer workgroups for small ranges:
                                     //   every workgroup moves 378 KB of LDS tiles in and out whatever its chunk)
  bool fstep_packed = FSTEP_PACKED_DEFAULT;   // DSGD_FSTEP_PACKED=0: the chunked launch on the plain streams.  Default: on packed copies of the split streams (row starts in
                                     //   bit 15 of the hot rank words, y * x as values: no hot lane tables, 128 bytes and one request per
                                     //   lane less per hot tile; 6 bytes per hot slot + 4 per cold slot of extra device memory).  Read
                                     //   by knobs_read beside the table below; the measurement behind the default: profiles/fstep_packed_ab.txt
  bool tcol_enable = true;           // DSGD_TCOL=0: such ranges through the row-wise kernel
  long long tcol_min = 512;          // DSGD_TCOL_MIN / DSGD_TCOL_MAX: row ranges of this many rows in total take the column lists
  long long tcol_max = 98303;        //   (above: row chunks, dsgd_fstep.hpp.  Measured, whole-split steps, us, row-wise / chunks / columns:
                                     //    4,800 rows 22.7 / 27.4 / 18.1; 18,519: 30.9 / 34.8 / 20.6; 40,000: 36.6 / 42.7 / 31.7; 80,441: 49 / 48 / 42.8;
                                     //    160,000: 73 / 57.5 / 73; 320,000: 117 / 65 / 162 -- profiles/r05_tcol_probe_*.json)
  long long tcol_max_nnz = 4500000;  // DSGD_TCOL_MAX_NNZ: ... and of at most this many non-zeros where row chunks can take over (round 6: the
                                     //   crossover is a matter of ENTRIES -- 80 K rows of 150 non-zeros: columns 67.8 us, chunks 51.7; of 40: 33.3 / 37.8;
                                     //   RCV1-like rows of 75: columns win up to ~60 K rows = 4.5 M entries, profiles/r06_dispatch_table.txt)
  int tcol_share = 0;                // DSGD_TCOL_SHARE: entries per workgroup of the gradient kernel (0: entries / CUs, within [1024, 8192])
  // -- resident plans (dsgd_plan_run).  The three budgets in MiB are ints, as atoi reads them: a use widens before it scales
  //    (`(long long)k.cs_max_mb << 20`, never `k.cs_max_mb << 20`)
  bool cs_enable = true;             // DSGD_CS=0: small steps of resident plans through the row-parallel kernels
  int cs_g = 0;                      // DSGD_CS_G: slices (8 or 16; 0 = 8 up to four hosted workers, 16 beyond)
  int cs_max_mb = 8192;              // DSGD_CS_MAX_MB: largest column-slice layout of one plan (device-built; the host
                                     //   builder of DSGD_CS_HOST_LAYOUT=1 holds a copy of it in host memory as well)
  int cs_nt = 0;                     // DSGD_CS_NT=256: tuning runs with 256 lanes per slice where a plan's steps fit them
  bool cs_host_layout = false;       // DSGD_CS_HOST_LAYOUT=1: a plan's slices laid out by the host (rounds 1-4; kept as the cross-check)
  int cache_mb = 8192;               // DSGD_CACHE_MB: device blocks kept across plans (PlanCache::cache_cap; dsgd_cache_trim gives them back)
  bool plan_kernel = true;           // DSGD_PLAN_KERNEL=0: the multi-launch small-batch path
  bool vt_enable = true;             // DSGD_VT=0: index-list steps of resident plans through dsgd_mb_grad_kernel
  int vt_pack_mb = 2048;             // DSGD_VT_PACK_MB: plans whose packed copy fits get one (0: descriptors only)
  int vt_tpw = 1;                    // DSGD_VT_TPW: virtual tiles per wave the grid is sized for (measured: 1 beats 2-4 up to B = 65,536)
  bool plan_prof = false;            // DSGD_PLAN_PROF=1: phase cycle counters of dsgd_plan_kernel and the chunked launch (tuning runs)
  // -- per-request steps (dsgd_sync_step)
  bool cs_req = false;               // DSGD_CS_REQ=1: per-request steps of the reference's sizes through dsgd_cs_request_kernel.  OFF by
                                     //   default: a slice's workgroup lays the step out before it runs it, one dependent trip to
                                     //   memory per row and wave -- measured 126 us per 3 x 100 request against 40 us through the
                                     //   row-parallel kernels (profiles/r05_probe_v1.json); the kernel is kept, tested, and is what
                                     //   the abort-path test drives
  bool req_mapped = true;            // DSGD_REQ_MAPPED=0: always the copy on the stream
  bool req_spin = true;              // DSGD_REQ_SPIN=0: wait for the stream instead of polling the mailbox
  bool req_plan = false;             // DSGD_REQ_PLAN=1: one-worker requests of <= 192 rows through the one-workgroup kernel (its
                                     //   launch re-derives s in fp64 and sets up 147 KB of LDS for ONE step: 37 us per request at the
                                     //   C ABI against 32 us through the row-parallel kernels -- profiles/r04_boundary_latency.json)
  // -- the fp64 mode
  bool rp64_fused = RP64_FUSED_DEFAULT;   // DSGD_RP64_FUSED: dsgd_sync_steps_f64, 1 = one fused launch per step, 0 = two
  // -- test builds (-DDSGD_TEST_COLLECTIVE_SEAM) only; dsgd_test_cs_skip_publish sets it as well
  int cs_test_skip = 0;              // DSGD_TEST_CS_SKIP_PUBLISH: slice 1 goes silent from this step of a launch on
};

// One table drives the parsing.  A value is read with atoi (flags, ints, choices) or atoll: text that is no number reads as 0, and
// then the clamp applies.  Classes: PRODUCT -- what a deployment may set (budgets, the way out of a family); TUNING -- A/B
// switches and measured thresholds, defaults are what the published numbers use; TEST -- there for the tests alone.
// Read elsewhere, where they are used, and not part of Knobs: DSGD_RCCL_LIB (test builds: the collective library),
// DSGD_COLD_UNPACKED (32-bit cold ids; tests), DSGD_FSTEP_DUMP (tuning: per-workgroup clocks), DSGD_SEED_PROF (tuning:
// csrc/dsgd_seed_host.hpp), DSGD_DENSE_MFMA (the dense engine), and csrc/jrand.c's DSGD_HOST_THREADS / DSGD_HOST_SPECULATE.
enum KnobKind { KNOB_FLAG, KNOB_INT, KNOB_LL, KNOB_CHOICE };
enum KnobClass { KNOB_PRODUCT, KNOB_TUNING, KNOB_TEST };
struct KnobSpec {
  const char* name;
  KnobKind kind;
  KnobClass cls;
  bool Knobs::*b;
  int Knobs::*i;
  long long Knobs::*l;
  long long lo, hi;    // KNOB_INT / KNOB_LL: the clamp; KNOB_CHOICE: the two values accepted (anything else reads as 0)
  bool seam_only;      // honoured only by the tests' build (-DDSGD_TEST_COLLECTIVE_SEAM)
};
constexpr KnobSpec knob_flag(const char* n, KnobClass c, bool Knobs::*f) { return {n, KNOB_FLAG, c, f, nullptr, nullptr, 0, 1, false}; }
constexpr KnobSpec knob_int(const char* n, KnobClass c, int Knobs::*f, long long lo, long long hi = INT_MAX, bool seam = false) {
  return {n, KNOB_INT, c, nullptr, f, nullptr, lo, hi, seam};
}
constexpr KnobSpec knob_ll(const char* n, KnobClass c, long long Knobs::*f, long long lo) {
  return {n, KNOB_LL, c, nullptr, nullptr, f, lo, LLONG_MAX, false};
}
constexpr KnobSpec knob_choice(const char* n, KnobClass c, int Knobs::*f, int a, int b) {
  return {n, KNOB_CHOICE, c, nullptr, f, nullptr, a, b, false};
}
constexpr KnobSpec KNOBS[] = {
    knob_flag("DSGD_CS", KNOB_PRODUCT, &Knobs::cs_enable),
    knob_int("DSGD_CS_MAX_MB", KNOB_PRODUCT, &Knobs::cs_max_mb, 0),
    knob_int("DSGD_CACHE_MB", KNOB_PRODUCT, &Knobs::cache_mb, 0),
    knob_int("DSGD_VT_PACK_MB", KNOB_PRODUCT, &Knobs::vt_pack_mb, 0),
    knob_int("DSGD_HSPLIT", KNOB_PRODUCT, &Knobs::hsplit, INT_MIN),
    knob_flag("DSGD_RP64_FUSED", KNOB_PRODUCT, &Knobs::rp64_fused),
    knob_int("DSGD_FIX_SHIFT", KNOB_TUNING, &Knobs::max_shift, 8, FIX_SHIFT),
    knob_flag("DSGD_FIX_BOUND", KNOB_TUNING, &Knobs::fix_bound),
    knob_flag("DSGD_PLAN_KERNEL", KNOB_TUNING, &Knobs::plan_kernel),
    knob_flag("DSGD_PLAN_PROF", KNOB_TUNING, &Knobs::plan_prof),
    knob_flag("DSGD_VT", KNOB_TUNING, &Knobs::vt_enable),
    knob_int("DSGD_VT_TPW", KNOB_TUNING, &Knobs::vt_tpw, 1),
    knob_choice("DSGD_CS_G", KNOB_TUNING, &Knobs::cs_g, 8, 16),
    knob_choice("DSGD_CS_NT", KNOB_TUNING, &Knobs::cs_nt, CS_THREADS_NARROW, CS_THREADS_NARROW),
    knob_flag("DSGD_CS_REQ", KNOB_TUNING, &Knobs::cs_req),
    knob_flag("DSGD_REQ_MAPPED", KNOB_TUNING, &Knobs::req_mapped),
    knob_flag("DSGD_REQ_PLAN", KNOB_TUNING, &Knobs::req_plan),
    knob_flag("DSGD_REQ_SPIN", KNOB_TUNING, &Knobs::req_spin),
    knob_ll("DSGD_STREAM_MIN", KNOB_TUNING, &Knobs::stream_min, 1),
    knob_flag("DSGD_FSTEP", KNOB_TUNING, &Knobs::fstep_enable),
    knob_ll("DSGD_FSTEP_MIN", KNOB_TUNING, &Knobs::fstep_min, 1),
    knob_ll("DSGD_FSTEP_MAX", KNOB_TUNING, &Knobs::fstep_max, 1),
    knob_ll("DSGD_FSTEP_ROWS", KNOB_TUNING, &Knobs::fstep_rows, 1),
    knob_flag("DSGD_FSTEP_REBALANCE", KNOB_TUNING, &Knobs::fstep_rebalance),
    knob_flag("DSGD_TCOL", KNOB_TUNING, &Knobs::tcol_enable),
    knob_ll("DSGD_TCOL_MIN", KNOB_TUNING, &Knobs::tcol_min, 1),
    knob_ll("DSGD_TCOL_MAX", KNOB_TUNING, &Knobs::tcol_max, 1),
    knob_ll("DSGD_TCOL_MAX_NNZ", KNOB_TUNING, &Knobs::tcol_max_nnz, 1),
    knob_int("DSGD_TCOL_SHARE", KNOB_TUNING, &Knobs::tcol_share, 0),
    knob_flag("DSGD_CS_HOST_LAYOUT", KNOB_TEST, &Knobs::cs_host_layout),
    knob_int("DSGD_TEST_CS_SKIP_PUBLISH", KNOB_TEST, &Knobs::cs_test_skip, 0, INT_MAX, true),
};

// lookup: const char* (const char* name), nullptr where the name is not set (dsgd_create passes getenv)
template <class Lookup>
inline void knobs_read(Knobs& k, Lookup lookup) {
  for (const KnobSpec& s : KNOBS) {
#ifndef DSGD_TEST_COLLECTIVE_SEAM
    if (s.seam_only) continue;
#endif
    const char* e = lookup(s.name);
    if (!e) continue;
    switch (s.kind) {
      case KNOB_FLAG: k.*s.b = atoi(e) != 0; break;
      case KNOB_INT: k.*s.i = (int)std::max<long long>(s.lo, std::min<long long>(s.hi, atoi(e))); break;
      case KNOB_LL: k.*s.l = std::max(s.lo, std::min(s.hi, atoll(e))); break;
      case KNOB_CHOICE: {
        const int v = atoi(e);
        k.*s.i = (v == s.lo || v == s.hi) ? v : 0;
        break;
      }
    }
  }
  // (a flag like the table's; outside it: the table's names are the ones tests/cpp/route_test.cpp digests)
  if (const char* e = lookup("DSGD_FSTEP_PACKED")) k.fstep_packed = atoi(e) != 0;
}

// ------------------------------------------------------------------------------------------------
// what a route needs from the context
// ------------------------------------------------------------------------------------------------
struct RouteFacts {
  int dp = 0;                 // D + 1
  long long n_rows = 0;
  int n_cu = 256;
  int hsplit = HSPLIT_MAX;    // clamped and aligned (dsgd_create)
  bool cold_col16 = false;    // the cold stream carries 16-bit ranks
  long long coldm_nnz = 0;    // slots of the cold stream
  bool comm = false;          // a communicator is attached
  bool prof = false;          // the gradient kernels are bracketed by profiling events
  bool fp64 = false;          // DSGD_F_FP64
  bool val64 = false;         // ... on Double feature values
  bool async_running = false; // the persistent Hogwild engine is resident
};

constexpr long long PLAN_MAX_ROWS = 2048;   // steps with more rows in total use the multi-workgroup kernels
constexpr long long ROWS_32BIT = 1LL << 31;         // the row chunks and the column lists carry 32-bit row numbers: n_rows below this
constexpr long long FSTEP_HANDOVER_ROWS = 8192;     // ranges of more entries than tcol_max_nnz go to the row chunks from this many rows on
constexpr int TC_MAX_WORKERS = 64;                  // column lists: hosted workers of one step
constexpr long long TC_MAX_KEYS = 1LL << 24;        // ... and workers x dp, the (worker, column) keys the device sorts by, below this
constexpr int CS_MAX_SLICE_COLS = 65536;            // column slices: columns of one slice (16-bit slice-local ids)

// can the chunked launch serve this context's layout at all?  (16-bit cold ids, every cold column inside the LDS tile)
inline bool fstep_possible(const Knobs& k, const RouteFacts& f) {
  const int H = std::min(f.hsplit, f.dp);
  const int nc = f.dp - H;
  const int nc_lds = std::min(nc, DSGD_LDS_FLOATS - 16 * CT_STRIP - 64 - 4);
  return k.fstep_enable && nc > 0 && nc <= nc_lds && f.cold_col16 && f.coldm_nnz > 0 && f.n_rows < ROWS_32BIT;
}
// workgroups per worker of the chunked launch for ranges of tot rows and ent non-zeros, the smallest of smallest rows (0: not this path)
inline int fstep_grid(const Knobs& k, const RouteFacts& f, int n_workers, long long tot, long long ent, long long smallest) {
  // (from DSGD_FSTEP_MIN rows on -- or from FSTEP_HANDOVER_ROWS on when the range holds more entries than the column lists take)
  if (!fstep_possible(k, f) || tot > k.fstep_max || (tot < k.fstep_min && !(ent > k.tcol_max_nnz && tot >= FSTEP_HANDOVER_ROWS))) return 0;
  if (n_workers > f.n_cu) return 0;
  const long long per_worker = std::max<long long>(1, f.n_cu / n_workers);
  return (int)std::max<long long>(1, std::min(per_worker, std::min(smallest, tot) / std::max<long long>(1, k.fstep_rows)));
}
// may a chunked launch (fstep_grid > 0) run its PACKED form?  The hot ranks must leave bit 15 of their 16-bit words free; the
// extra memory is asked for where the copies are built (csrc/dsgd_fstep_host.hpp: no memory -> the plain form).
constexpr int FSTEP_PACKED_MAX_HOT = 32768;
inline bool fstep_packed_wanted(const Knobs& k, const RouteFacts& f) {
  return k.fstep_packed && std::min(f.hsplit, f.dp) <= FSTEP_PACKED_MAX_HOT;
}
inline bool tcol_wanted(const Knobs& k, const RouteFacts& f, long long tot, int n_workers) {
  return k.tcol_enable && tot >= k.tcol_min && tot <= k.tcol_max && n_workers <= TC_MAX_WORKERS && f.n_rows < ROWS_32BIT &&
         (long long)n_workers * f.dp < TC_MAX_KEYS && tot + 64LL * n_workers <= TC_MAX_BITS;
}
inline bool plan_kernel_ok(const Knobs& k, const RouteFacts& f, long long step_rows, int n_workers) {
  // (several hosted workers: their batches would run one after the other in the one workgroup -- 44 us for 3 x 100 --
  //  while dsgd_mb_grad_kernel gives every worker its own workgroups: 32 us with the four-launch finish, less fused)
  return k.plan_kernel && !f.comm && n_workers == 1 && step_rows <= PLAN_MAX_ROWS;
}
// slices for K hosted workers: 8 up to four (wider slices, fewer peers in the exchange), 16 beyond or for a wide model; 0: none fits
inline int cs_pick_G(const Knobs& k, const RouteFacts& f, int K, bool request) {
  auto fits = [&](int G) {
    const int words = request ? cs_req_lds_words(f.dp, G, K) : cs_lds_words(f.dp, G, K);
    return f.dp >= 4 * G && words <= DSGD_LDS_FLOATS && (f.dp + G - 1) / G <= CS_MAX_SLICE_COLS;
  };
  int G = k.cs_g ? k.cs_g : (K <= 4 ? 8 : 16);
  if (!k.cs_g && G == 8 && !fits(8)) G = 16;
  return fits(G) ? G : 0;
}

// lanes per row of the fp32 row-wise evaluation kernels (dsgd_forward_kernel, dsgd_eval_kernel, dsgd_predict_kernel,
// dsgd_eval_list_kernel) for data of nnz non-zeros in n_rows rows, chosen when the data is loaded: a row of mean length
// gives a lane at most 6 products (below 64 lanes).  The mean is taken in double; a mean ON a threshold keeps the narrower
// group.  nnz is the count the context HOLDS (dsgd_n_rows): a row without a non-zero owns one explicit zero there, so six
// empty rows weigh six entries.  (No rows: 0 / 0 compares false everywhere, 8.)  dsgd_tuning_info reports it in slot [7].
inline int eval_group(long long nnz, long long n_rows) {
  const double mean = (double)nnz / (double)n_rows;
  return mean > 192.0 ? 64 : (mean > 96.0 ? 32 : (mean > 12.0 ? 16 : 8));
}

// ---- row ranges: column lists first where they are wanted, then row chunks / the streaming launches / the row-wise kernel ----
enum RangesThen { RANGES_FSTEP, RANGES_STREAM, RANGES_ROWWISE };
struct RangesRoute {
  bool try_tcol;      // column lists (which may decline softly: no memory, the back-off -- then `then`)
  RangesThen then;
  int fstep_wg;       // RANGES_FSTEP: workgroups per worker
};
inline RangesRoute route_ranges(const Knobs& k, const RouteFacts& f, int n_workers, long long tot, long long ent, long long smallest) {
  RangesRoute r;
  r.fstep_wg = fstep_grid(k, f, n_workers, tot, ent, smallest);
  // the hand-over: 10^3 .. 10^5 rows are the column lists' unless row chunks could run and the ranges hold more entries than
  // DSGD_TCOL_MAX_NNZ
  r.try_tcol = tcol_wanted(k, f, tot, n_workers) && !(r.fstep_wg > 0 && ent > k.tcol_max_nnz);
  r.then = r.fstep_wg > 0 ? RANGES_FSTEP : (tot >= k.stream_min ? RANGES_STREAM : RANGES_ROWWISE);
  return r;
}

// ---- resident plans ----
struct PlanFacts {
  bool rp64 = false;         // a row-parallel fp64 plan
  bool lg = false;           // a logistic plan (csrc/dsgd_lg_calls.hpp: plan_run_lg)
  bool lg_cs_current = false;   // ... created with its column slices, and they are laid out for the current column ranking
  bool cs_current = false;   // its column slices are laid out for the current column ranking
  bool fits_here = false;    // every list fits the staged sub-batch of the one-workgroup kernel, on the rows loaded now
  bool vt_current = false;   // its virtual tiles are laid out for the current split streams
  long long max_step_rows = 0;
  int n_workers = 0;
};
enum PlanRoute { PLAN_RP64, PLAN_CS64, PLAN_CS, PLAN_ONE_WG, PLAN_VT, PLAN_ROWWISE, PLAN_LG, PLAN_LG_CS };
inline PlanRoute route_plan(const Knobs& k, const RouteFacts& f, const PlanFacts& p) {
  // (the model and the entry point that made the plan decide, not a knob: the lists and their ranges only, as PLAN_RP64 --
  //  or, asked for at creation and current, the logistic column slices of csrc/dsgd_lg_cs.hpp)
  if (p.lg) return p.lg_cs_current ? PLAN_LG_CS : PLAN_LG;
  if (p.rp64) return PLAN_RP64;
  if ((k.cs_enable || f.fp64) && !f.comm && p.cs_current) return f.fp64 ? PLAN_CS64 : PLAN_CS;
  if (plan_kernel_ok(k, f, p.max_step_rows, p.n_workers) && p.fits_here) return PLAN_ONE_WG;
  if (k.vt_enable && p.vt_current) return PLAN_VT;
  return PLAN_ROWWISE;
}
// dsgd_plan_info's first word (include/dsgd.h); a row-wise plan says whether a layout was tried for the current ranking
inline int plan_info_code(PlanRoute r, bool layout_tried) {
  switch (r) {
    case PLAN_LG: return 7;
    case PLAN_LG_CS: return 8;
    case PLAN_RP64: return 6;
    case PLAN_CS64: return 5;
    case PLAN_CS: return 1;
    case PLAN_ONE_WG: return 2;
    case PLAN_VT: return 3;
    case PLAN_ROWWISE: break;
  }
  return layout_tried ? 4 : 0;
}
// are a plan's column slices laid out when it is created (on the build stream), not inside its first run?
inline bool plan_lays_out_at_creation(const Knobs& k, const RouteFacts& f, bool rp64, bool have_data, bool have_ds) {
  return !rp64 && (k.cs_enable || f.fp64) && !f.comm && have_data && have_ds && !f.async_running;
}

// ---- per-request steps: K lists of `rows` rows in all ----
enum RequestArm {
  REQ_F64_RANKS,        // fp64 across ranks
  REQ_F64_ROWS,         // fp64 on Double data: the row-parallel pair
  REQ_F64_CS,           // fp64: a one-step column-slice plan
  REQ_ONE_WG_READBACK,  // one workgroup, statistics read back (profiling)
  REQ_ONE_WG_MAIL,      // ... through the mailbox
  REQ_CS,               // the column-slice request; a step that does not fit its one-step layout falls through to `rowwise`
  REQ_ROWWISE_READBACK, // row-wise, statistics read back (a communicator, profiling)
  REQ_ROWWISE_MAIL,     // ... through the mailbox
};
struct RequestRoute {
  RequestArm first;
  RequestArm rowwise;   // the row-wise arm of this context (where `first` ends up, or falls through to)
  int G;                // REQ_CS: slices
};
// lists_fit(): every list non-null and inside the one-workgroup kernel's staged sub-batch; lists_valid(): every list non-empty,
// non-null and inside the loaded rows.  Both scan the lists, so they are asked only where the answer decides.
template <class Fit, class Valid>
inline RequestRoute route_request(const Knobs& k, const RouteFacts& f, int K, long long rows, Fit lists_fit, Valid lists_valid) {
  RequestRoute r;
  r.rowwise = (f.comm || f.prof) ? REQ_ROWWISE_READBACK : REQ_ROWWISE_MAIL;
  r.first = r.rowwise;
  r.G = 0;
  if (f.fp64) {
    r.first = f.comm ? REQ_F64_RANKS : (f.val64 ? REQ_F64_ROWS : REQ_F64_CS);
  } else if (k.req_plan && plan_kernel_ok(k, f, rows, K) && lists_fit()) {
    r.first = f.prof ? REQ_ONE_WG_READBACK : REQ_ONE_WG_MAIL;
  } else if (k.cs_enable && k.cs_req && !f.comm && !f.prof && K <= CS_MAX_K && rows <= CS_MAX_SLOTS) {
    const int G = cs_pick_G(k, f, K, true);
    if (G && lists_valid()) {
      r.first = REQ_CS;
      r.G = G;
    }
  }
  return r;
}

// ------------------------------------------------------------------------------------------------
// The column lists' back-off.  A caller that never repeats a configuration (mini-batches over ever new row ranges) would pay
// a layout -- milliseconds -- for every 20 us step: more misses in a row than the cache holds, and the column lists leave such
// a context alone.  Not for good: after COOLDOWN declined steps they try again -- a fit that settles on fixed
// splits after a phase of ever new ranges gets its column lists back; a context that keeps changing pays 4 layouts per 256 steps.
// ------------------------------------------------------------------------------------------------
struct TcolGate {
  static constexpr int MISSES = 12;      // layouts built in a row without one being used again, before the lists sit out
  static constexpr int COOLDOWN = 256;   // steps they sit out
  static constexpr int RESUME = 8;       // the streak they come back with: MISSES - RESUME builds, then out again
  int streak = 0, cooldown = 0;
  void hit() { streak = 0; }             // a cached layout was used again
  bool miss() {                          // no cached layout: may this step build one?
    if (cooldown > 0) {
      if (--cooldown == 0) streak = RESUME;
      return false;
    }
    if (++streak > MISSES) {
      cooldown = COOLDOWN;
      return false;
    }
    return true;
  }
  void reset() { streak = cooldown = 0; }   // (data loaded: the misses were about the old rows' ranges)
};
