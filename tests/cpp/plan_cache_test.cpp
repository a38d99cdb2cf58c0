// csrc/dsgd_plan_cache.hpp on its own, on the CPU: PlanCache and CacheBuf compiled (behind csrc/dsgd_buf.hpp) against
// stand-ins for the HIP calls they use -- malloc / free that count live blocks and can fail the next allocations, events
// that count creates, records, waits and synchronises, can fail the next create or record, and can be "not ready".
// Every rule of the cache is checked by name.  Built with -fsanitize=address,undefined and run directly by
// tests/test_plan_cache.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

// ---- the stand-ins ----
typedef int hipError_t;
typedef void* hipEvent_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorNotReady = 600, hipErrorUnknown = 999 };
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipEventDisableTiming = 2 };
enum { DSGD_OK = 0, DSGD_EHIP = -5 };
static int g_live = 0, g_frees = 0, g_allocs = 0, g_fail_allocs = 0;   // (g_fail_allocs: the next so many allocations fail)
static size_t g_last_alloc_bytes = 0;
static int g_ev_live = 0, g_ev_creates = 0, g_records = 0, g_waits = 0, g_syncs = 0, g_errors_cleared = 0;
static bool g_fail_create = false, g_fail_record = false, g_none_ready = false;
static std::set<hipEvent_t> g_not_ready;
static hipStream_t g_last_record_stream = nullptr, g_last_wait_stream = nullptr, g_last_sync_stream = nullptr;
static hipEvent_t g_last_wait_event = nullptr;
static hipError_t stub_alloc(void** p, size_t bytes) {
  if (g_fail_allocs > 0) {
    --g_fail_allocs;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  g_last_alloc_bytes = bytes;
  ++g_live, ++g_allocs;
  return hipSuccess;
}
static hipError_t stub_free(void* p) {
  std::free(p);
  --g_live, ++g_frees;
  return hipSuccess;
}
static hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
static hipError_t hipFree(void* p) { return stub_free(p); }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes); }
static hipError_t hipHostFree(void* p) { return stub_free(p); }
static hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
  *d = h;
  return hipSuccess;
}
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int) {
  if (g_fail_create) {
    g_fail_create = false;
    return hipErrorOutOfMemory;
  }
  *e = new int(0);   // (a block of its own: a lost or twice-destroyed event is the sanitizer's finding)
  ++g_ev_live, ++g_ev_creates;
  return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
  delete static_cast<int*>(e);
  g_not_ready.erase(e);
  --g_ev_live;
  return hipSuccess;
}
static hipError_t hipEventRecord(hipEvent_t, hipStream_t s) {
  if (g_fail_record) {
    g_fail_record = false;
    return hipErrorUnknown;
  }
  g_last_record_stream = s;
  ++g_records;
  return hipSuccess;
}
static hipError_t hipEventQuery(hipEvent_t e) { return (g_none_ready || g_not_ready.count(e)) ? hipErrorNotReady : hipSuccess; }
static hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
  g_last_wait_stream = s, g_last_wait_event = e;
  ++g_waits;
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) {
  g_last_sync_stream = s;
  ++g_syncs;
  return hipSuccess;
}
static hipError_t hipGetLastError() {
  ++g_errors_cleared;
  return hipSuccess;
}
static const char* hipGetErrorString(hipError_t) { return "stub error"; }
static char g_err[256];
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#include "dsgd_buf.hpp"
#include "dsgd_plan_cache.hpp"

static int g_bad = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_bad;                                                            \
    }                                                                     \
  } while (0)

// a context's two streams and its cache, wired the way dsgd_create wires them
static int g_stream_a, g_stream_b;
namespace {
struct Ctx {
  hipStream_t stream = &g_stream_a;
  hipStream_t build_stream = &g_stream_b;
  PlanCache pc;
  Ctx() { pc.launch = &stream, pc.build = &build_stream; }
  void* take(size_t bytes, size_t* got = nullptr) {   // a take that must succeed
    void* q = nullptr;
    size_t g = 0;
    CHECK(pc.take(&q, bytes, &g) == DSGD_OK && q != nullptr);
    if (got) *got = g;
    return q;
  }
  void* cached(size_t bytes) {   // a block of `bytes` (a multiple of 4096) put into the cache; its address
    void* q = take(bytes);
    pc.give(q, bytes);
    return q;
  }
};
}  // namespace

static void take_rounds_to_4096() {
  Ctx c;
  size_t got = 0;
  void* a = c.take(0, &got);
  CHECK(got == 4096 && g_last_alloc_bytes == 4096);
  void* b = c.take(1, &got);
  CHECK(got == 4096 && g_last_alloc_bytes == 4096);
  void* d = c.take(4096, &got);
  CHECK(got == 4096 && g_last_alloc_bytes == 4096);
  void* e = c.take(4097, &got);
  CHECK(got == 8192 && g_last_alloc_bytes == 8192);
  c.pc.give(a, 4096), c.pc.give(b, 4096), c.pc.give(d, 4096), c.pc.give(e, 8192);
  CHECK(c.pc.cache.size() == 4 && c.pc.cache_bytes == 3 * 4096 + 8192);
}

static void take_smallest_fit_within_twice_plus_64k() {
  Ctx c;
  const size_t req = 4096, top = 2 * req + 65536;
  void *too_big = c.take(top + 4096), *at_bound = c.take(top), *small = c.take(8192);
  c.pc.give(too_big, top + 4096);
  int allocs = g_allocs;
  size_t got = 0;
  void* fresh = c.take(req, &got);   // the block just beyond the bound is not taken: a fresh one is allocated
  CHECK(fresh != too_big && got == req && g_allocs == allocs + 1 && c.pc.cache.size() == 1 && c.pc.cache_bytes == top + 4096);
  c.pc.give(at_bound, top), c.pc.give(small, 8192);
  allocs = g_allocs;
  CHECK(c.take(req, &got) == small && got == 8192);      // the smallest that fits, not the first
  CHECK(c.take(req, &got) == at_bound && got == top);    // the bound itself is inside
  CHECK(g_allocs == allocs && c.pc.cache.size() == 1 && c.pc.cache_bytes == top + 4096);
  void* again = c.take(req, &got);                        // only the too-big block is left
  CHECK(again != too_big && got == req && g_allocs == allocs + 1);
  // a block smaller than the request is no hit either
  allocs = g_allocs;
  void* big = c.take(top + 8192, &got);
  CHECK(big != too_big && got == top + 8192 && g_allocs == allocs + 1 && c.pc.cache.size() == 1);
  // the caller learns the block's full size: what it gives back is what the cache counts
  CHECK(c.take(top + 4096 - 100, &got) == too_big && got == top + 4096 && c.pc.cache_bytes == 0);
  c.pc.give(fresh, req), c.pc.give(small, 8192), c.pc.give(at_bound, top), c.pc.give(again, req), c.pc.give(big, top + 8192);
  c.pc.give(too_big, top + 4096);
}

static void hit_waits_once_on_the_build_stream_and_pools_the_event() {
  Ctx c;
  void* a = c.cached(4096);
  CHECK(g_last_record_stream == c.stream && c.pc.cache.size() == 1 && c.pc.ev_pool.empty());
  const hipEvent_t ev = c.pc.cache[0].ev;
  const int waits = g_waits, creates = g_ev_creates;
  CHECK(c.take(4096) == a);
  CHECK(g_waits == waits + 1 && g_last_wait_stream == c.build_stream && g_last_wait_event == ev);
  CHECK(c.pc.ev_pool.size() == 1 && c.pc.ev_pool[0] == ev);
  const int records = g_records;
  c.pc.give(a, 4096);   // the next give reuses the pooled event
  CHECK(g_ev_creates == creates && g_records == records + 1 && c.pc.ev_pool.empty() && c.pc.cache[0].ev == ev);
  // no build stream yet: nothing to wait on, the event still goes to the pool
  c.build_stream = nullptr;
  CHECK(c.take(4096) == a && g_waits == waits + 1 && c.pc.ev_pool.size() == 1);
  c.pc.give(a, 4096);
}

static void failed_allocation_flushes_and_retries_once() {
  Ctx c;
  c.cached(4096), c.cached(8192);
  CHECK(c.pc.cache.size() == 2 && g_live == 2);
  // fails with blocks cached: all of them go back to the device, their events to the pool, the retry succeeds
  int frees = g_frees, cleared = g_errors_cleared;
  g_fail_allocs = 1;
  void* q = c.take(1 << 20);
  CHECK(g_frees == frees + 2 && g_errors_cleared == cleared + 1 && c.pc.cache.empty() && c.pc.cache_bytes == 0 && c.pc.ev_pool.size() == 2);
  CHECK(g_live == 1 && g_fail_allocs == 0);
  // fails with nothing cached: soft, the error text untouched
  void* out = nullptr;
  size_t got = 0;
  g_err[0] = 0, g_fail_allocs = 1;
  CHECK(c.pc.take(&out, 4096, &got) == 1 && out == nullptr && g_err[0] == 0 && g_fail_allocs == 0);
  // fails twice: soft, and the cache is empty
  c.pc.give(q, 1 << 20);
  c.cached(4096);
  CHECK(c.pc.cache.size() == 2);
  frees = g_frees, g_fail_allocs = 2;
  CHECK(c.pc.take(&out, 64 << 20, &got) == 1 && out == nullptr && g_err[0] == 0 && g_fail_allocs == 0);
  CHECK(g_frees == frees + 2 && c.pc.cache.empty() && c.pc.cache_bytes == 0 && g_live == 0);
}

static void give_keeps_or_frees() {
  {   // null does nothing
    Ctx c;
    c.pc.give(nullptr, 4096);
    CHECK(c.pc.cache_tick == 0 && c.pc.cache.empty());
  }
  {   // the cap on bytes
    Ctx c;
    c.pc.cache_cap = 8192;
    void *a = c.take(4096), *b = c.take(4096), *d = c.take(4096);
    const int frees = g_frees;
    c.pc.give(a, 4096), c.pc.give(b, 4096);
    CHECK(c.pc.cache.size() == 2 && c.pc.cache_bytes == 8192 && g_frees == frees);
    c.pc.give(d, 4096);   // would pass the cap: freed
    CHECK(c.pc.cache.size() == 2 && c.pc.cache_bytes == 8192 && g_frees == frees + 1 && c.pc.cache_tick == 3);
  }
  {   // at most 256 blocks (their events "not ready", so that the aged trim of every 16th give leaves them alone)
    Ctx c;
    std::vector<void*> held;
    for (int i = 0; i < 257; ++i) held.push_back(c.take(4096));
    g_none_ready = true;
    const int frees = g_frees;
    for (void* q : held) c.pc.give(q, 4096);
    g_none_ready = false;
    CHECK(c.pc.cache.size() == 256 && c.pc.cache_bytes == 256 * 4096 && g_frees == frees + 1 && g_live == 256);
  }
  {   // a block of size 0 (allocated outside the cache) is freed, and counts as a hand-back
    Ctx c;
    void* a = c.take(4096);
    const int frees = g_frees, events = g_ev_live;
    c.pc.give(a, 0);
    CHECK(c.pc.cache.empty() && c.pc.cache_bytes == 0 && g_frees == frees + 1 && g_ev_live == events && c.pc.cache_tick == 1);
  }
  {   // no event to be had: the block is freed
    Ctx c;
    void* a = c.take(4096);
    const int frees = g_frees, events = g_ev_live;
    g_fail_create = true;
    c.pc.give(a, 4096);
    CHECK(!g_fail_create && c.pc.cache.empty() && c.pc.cache_bytes == 0 && g_frees == frees + 1 && g_ev_live == events);
  }
  {   // the record fails: the launch stream is synchronised instead, the block is kept
    Ctx c;
    void* a = c.take(4096);
    const int syncs = g_syncs, frees = g_frees;
    g_fail_record = true;
    c.pc.give(a, 4096);
    CHECK(!g_fail_record && g_syncs == syncs + 1 && g_last_sync_stream == c.stream && g_frees == frees);
    CHECK(c.pc.cache.size() == 1 && c.pc.cache[0].p == a && c.pc.cache_bytes == 4096);
  }
}

static void trim_frees_aged_or_over_blocks_once_ready() {
  {   // aged: only when its last reader is done
    Ctx c;
    void* a = c.cached(4096);
    const hipEvent_t ev = c.pc.cache[0].ev;
    c.pc.cache_tick += PlanCache::CACHE_MAX_AGE;   // exactly CACHE_MAX_AGE hand-backs later: not aged yet
    int frees = g_frees;
    c.pc.trim(c.pc.cache_cap, true);
    CHECK(c.pc.cache.size() == 1 && g_frees == frees);
    c.pc.cache_tick += 1;
    g_not_ready.insert(ev);
    const int cleared = g_errors_cleared;
    c.pc.trim(c.pc.cache_cap, true);   // aged, still being read: stays, the query's error cleared
    CHECK(c.pc.cache.size() == 1 && c.pc.cache[0].p == a && g_frees == frees && g_errors_cleared == cleared + 1);
    g_not_ready.erase(ev);
    c.pc.trim(c.pc.cache_cap, true);
    CHECK(c.pc.cache.empty() && c.pc.cache_bytes == 0 && g_frees == frees + 1 && c.pc.ev_pool.size() == 1 && c.pc.ev_pool[0] == ev);
  }
  {   // over keep_bytes: oldest first, down to the limit; aged_only leaves them
    Ctx c;
    void *a = c.take(4096), *b = c.take(8192), *d = c.take(4096);
    c.pc.give(a, 4096), c.pc.give(b, 8192), c.pc.give(d, 4096);
    int frees = g_frees;
    c.pc.trim(8192, true);
    CHECK(c.pc.cache.size() == 3 && g_frees == frees);
    c.pc.trim(8192, false);
    CHECK(c.pc.cache.size() == 1 && c.pc.cache[0].p == d && c.pc.cache_bytes == 4096 && g_frees == frees + 2);
    c.pc.trim(4096, false);   // at the limit: nothing more
    CHECK(c.pc.cache.size() == 1 && g_frees == frees + 2);
  }
  {   // over keep_bytes, the oldest still being read: it stays, the next one goes
    Ctx c;
    void *a = c.take(4096), *b = c.take(4096);
    c.pc.give(a, 4096), c.pc.give(b, 4096);
    g_not_ready.insert(c.pc.cache[0].ev);
    const int frees = g_frees;
    c.pc.trim(4096, false);
    CHECK(c.pc.cache.size() == 1 && c.pc.cache[0].p == a && c.pc.cache_bytes == 4096 && g_frees == frees + 1);
    g_not_ready.clear();
    c.pc.trim(0, false);
    CHECK(c.pc.cache.empty() && c.pc.cache_bytes == 0 && g_frees == frees + 2);
  }
}

static void every_16th_give_trims_aged_blocks() {
  Ctx c;
  void* old = c.cached(4096);   // tick 1
  void *x = c.take(8192), *y = c.take(8192), *z = c.take(8192);
  c.pc.cache_tick = 77;
  const int frees = g_frees;
  c.pc.give(x, 8192);   // tick 78: `old` is aged, but no trim runs
  c.pc.give(y, 8192);   // tick 79
  CHECK(c.pc.cache.size() == 3 && c.pc.cache[0].p == old && g_frees == frees);
  c.pc.give(z, 8192);   // tick 80 (a multiple of 16, not of 32): the aged trim
  CHECK(c.pc.cache_tick == 80 && g_frees == frees + 1 && c.pc.cache.size() == 3 && c.pc.cache[0].p == x && c.pc.cache_bytes == 3 * 8192);
}

static void cache_buf_owns_one_block() {
  Ctx c;
  {
    CacheBuf<int> a;
    CHECK(a.get() == nullptr && !a);
    CHECK(a.take(c.pc, 1000) == DSGD_OK && a.get() != nullptr && g_last_alloc_bytes == 4096);
    int* raw = a;   // the implicit conversion the launch sites rely on
    raw[999] = 7;
    CHECK(a[999] == 7 && a + 1 == raw + 1);
    // a move leaves the source empty and gives nothing
    const unsigned long long tick = c.pc.cache_tick;
    CacheBuf<int> b(std::move(a));
    CHECK(a.get() == nullptr && b.get() == raw && c.pc.cache_tick == tick && c.pc.cache.empty());
    CacheBuf<int> d;
    d = std::move(b);
    CHECK(b.get() == nullptr && d.get() == raw && c.pc.cache_tick == tick && c.pc.cache.empty());
    a.reset(), b.reset();   // empty: nothing
    CHECK(c.pc.cache_tick == tick);
    // take on a held buffer gives the old block first (here: and takes it straight back)
    const int allocs = g_allocs;
    CHECK(d.take(c.pc, 1000) == DSGD_OK && d.get() == raw && c.pc.cache_tick == tick + 1 && g_allocs == allocs && c.pc.cache.empty());
    // ... a larger one: the old block is in the cache, a new one allocated
    CHECK(d.take(c.pc, 100000) == DSGD_OK && d.get() != raw && g_allocs == allocs + 1);
    CHECK(c.pc.cache.size() == 1 && c.pc.cache[0].p == raw && c.pc.cache[0].bytes == 4096);
    // a move assignment hands the target's old block back, once
    CacheBuf<int> e;
    CHECK(e.take(c.pc, 5000) == DSGD_OK && c.pc.cache.size() == 1);
    int* e_raw = e;
    e = std::move(d);
    CHECK(d.get() == nullptr && c.pc.cache.size() == 2 && c.pc.cache[1].p == e_raw && c.pc.cache[1].bytes == 20480);
    // a failed take: soft, the buffer empty, the old block handed back
    g_fail_allocs = 2;
    CHECK(e.take(c.pc, 1 << 24) == 1 && e.get() == nullptr && g_fail_allocs == 0);
    e.reset();
    CHECK(c.pc.cache.empty() && g_live == 0);   // (the failed allocation flushed the cache, the old block with it)
    // the destructor gives exactly once
    CHECK(e.take(c.pc, 10) == DSGD_OK);
  }
  CHECK(c.pc.cache.size() == 1 && c.pc.cache_bytes == 4096 && g_live == 1);
  {   // alloc_uncached followed by reset frees and does not cache
    CacheBuf<double> u;
    const int frees = g_frees;
    const unsigned long long tick = c.pc.cache_tick;
    CHECK(u.alloc_uncached(c.pc, 100) == hipSuccess && u.get() != nullptr && g_last_alloc_bytes == 800 && g_live == 2);
    u.reset();
    CHECK(u.get() == nullptr && g_frees == frees + 1 && g_live == 1 && c.pc.cache.size() == 1 && c.pc.cache_tick == tick + 1);
    g_fail_allocs = 1;
    CHECK(u.alloc_uncached(c.pc, 100) == hipErrorOutOfMemory && u.get() == nullptr);
    CHECK(u.alloc_uncached(c.pc, 100) == hipSuccess);   // left to the destructor
  }
  CHECK(c.pc.cache.size() == 1 && g_live == 1);
}

// the device builder of the column slices (cs_build_device_impl): six takes, the fourth fails softly; the caller's cs_free
// resets all six
static void builder_failure_loses_nothing() {
  Ctx c;
  CacheBuf<int> hdr, meta, rf, col, val, cl;
  CHECK(hdr.take(c.pc, 100) == DSGD_OK && meta.take(c.pc, 5000) == DSGD_OK && rf.take(c.pc, 3000) == DSGD_OK);
  g_fail_allocs = 1;
  CHECK(col.take(c.pc, 40000) == 1 && col.get() == nullptr && g_live == 3);
  const int frees = g_frees;
  hdr.reset(), meta.reset(), rf.reset(), col.reset(), val.reset(), cl.reset();
  CHECK(g_frees == frees && g_live == 3 && c.pc.cache.size() == 3 && c.pc.cache_bytes == 4096 + 20480 + 12288);
  hdr.reset(), meta.reset(), rf.reset();   // (again: nothing twice)
  CHECK(g_live == 3 && c.pc.cache.size() == 3);
}

int main() {
  take_rounds_to_4096();
  CHECK(g_live == 0 && g_ev_live == 0);   // (every Ctx's cache lets go of its blocks and events when it goes)
  take_smallest_fit_within_twice_plus_64k();
  hit_waits_once_on_the_build_stream_and_pools_the_event();
  failed_allocation_flushes_and_retries_once();
  give_keeps_or_frees();
  trim_frees_aged_or_over_blocks_once_ready();
  every_16th_give_trims_aged_blocks();
  cache_buf_owns_one_block();
  builder_failure_loses_nothing();
  CHECK(g_live == 0 && g_ev_live == 0);
  {   // drop_all: blocks and events, cached and pooled, all gone
    Ctx c;
    void* a = c.cached(4096);
    c.cached(8192);
    CHECK(c.take(4096) == a && c.pc.ev_pool.size() == 1 && c.pc.cache.size() == 1 && g_live == 2 && g_ev_live == 2);
    c.pc.give(a, 4096);
    CHECK(c.take(4096) == a);
    c.pc.drop_all();
    CHECK(c.pc.cache.empty() && c.pc.ev_pool.empty() && c.pc.cache_bytes == 0 && g_live == 1 && g_ev_live == 0);
    c.pc.give(a, 4096);
    c.pc.drop_all();
    CHECK(g_live == 0 && g_ev_live == 0);
  }
  CHECK(g_live == 0 && g_ev_live == 0);
  if (g_bad) return 1;
  std::fprintf(stderr, "all checks passed (%d allocations, %d releases, %d events)\n", g_allocs, g_frees, g_ev_creates);
  return 0;
}
