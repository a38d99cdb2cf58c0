// csrc/dsgd_layout_cache.hpp on its own, on the CPU: LayoutCache compiled (behind csrc/dsgd_buf.hpp) against stand-ins for the
// HIP allocation calls -- malloc / free that count live blocks.  The payload owns a DevBuf, so a layout that is lost or
// released twice is the sanitizer's finding.  Every rule of the cache is checked by name.  Built with
// -fsanitize=address,undefined and run directly by tests/test_layout_cache.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

// ---- the stand-ins ----
typedef int hipError_t;
typedef void* hipEvent_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2 };
enum { DSGD_OK = 0, DSGD_EHIP = -5 };
static int g_live = 0, g_allocs = 0, g_frees = 0;
static hipError_t stub_alloc(void** p, size_t bytes) {
  *p = std::malloc(bytes ? bytes : 1);
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
static hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
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
#include "dsgd_layout_cache.hpp"

static int g_bad = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_bad;                                                            \
    }                                                                     \
  } while (0)

namespace {
struct Layout {   // what the three families keep: device tables and a few numbers
  DevBuf<int> d_table;
  int tag = 0;
};
typedef LayoutCache<Layout> Cache;
typedef std::vector<long long> Key;

int g_idle = 0;
bool idle() {
  ++g_idle;
  return true;
}
Key key(long long i) { return Key{i * 100, i * 100 + 50}; }
// what a caller does on a miss: make_room, build, insert
Cache::Entry* add(Cache& c, const Key& k, int n_wg, long long gen, int tag) {
  CHECK(c.make_room(gen, idle));
  Layout L;
  CHECK(L.d_table.try_alloc(16) == hipSuccess);
  L.tag = tag;
  return c.insert(k, n_wg, gen, std::move(L));
}
bool has(Cache& c, long long i, long long gen) {   // (without a stamp: find would change the order under test)
  for (const Cache::Entry& e : c.entries)
    if (e.gen == gen && e.n_wg == 0 && e.ranges == key(i)) return true;
  return false;
}
}  // namespace

static void a_hit_restamps_and_protects_from_eviction() {
  Cache c;
  for (int i = 0; i < 8; ++i) add(c, key(i), 0, 1, i);
  Cache::Entry* e = c.find(key(0), 0, 1);   // the oldest becomes the youngest
  CHECK(e && !e->declined && e->layout.tag == 0 && e->used == c.clock);
  add(c, key(8), 0, 1, 8);
  CHECK(c.entries.size() == 8 && has(c, 0, 1) && !has(c, 1, 1) && has(c, 8, 1) && g_live == 8);
}

static void the_ninth_insert_evicts_the_least_recently_used() {
  Cache c;
  for (int i = 0; i < 8; ++i) add(c, key(i), 0, 1, i);
  for (int i : {0, 1, 2, 4, 5, 6, 7}) CHECK(c.find(key(i), 0, 1) != nullptr);   // all but 3
  add(c, key(8), 0, 1, 8);
  CHECK(c.entries.size() == 8 && !has(c, 3, 1) && g_live == 8);
  for (int i : {0, 1, 2, 4, 5, 6, 7, 8}) CHECK(has(c, i, 1));
  CHECK(c.find(key(3), 0, 1) == nullptr);
}

static void entries_of_another_gen_go_first_and_no_live_one_needlessly() {
  Cache c;
  for (int i = 0; i < 5; ++i) add(c, key(i), 0, 1, i);
  add(c, key(5), 0, 2, 5);   // a new ranking: all five go, though there was room
  CHECK(c.entries.size() == 1 && has(c, 5, 2) && g_live == 1);
  Cache d;   // (a mix of generations never builds up through make_room: made by hand)
  for (int i = 0; i < 8; ++i) add(d, key(i), 0, 1, i);
  for (int i = 0; i < 5; ++i) d.entries[(size_t)i].gen = 0;   // five of an earlier ranking, the three youngest live
  CHECK(d.find(key(0), 0, 1) == nullptr);                     // (stale: not found under the current gen)
  g_idle = 0;
  add(d, key(8), 0, 1, 8);
  CHECK(g_idle == 1 && d.entries.size() == 4 && g_live == 1 + 4);   // (c's one, d's four)
  for (int i : {5, 6, 7, 8}) CHECK(has(d, i, 1));   // the sweep made the room: no live entry went
}

static void idle_runs_once_per_make_room_that_erases_and_never_otherwise() {
  Cache c;
  g_idle = 0;
  c.clear(idle);   // an empty cache
  CHECK(c.make_room(1, idle));
  CHECK(g_idle == 0);
  for (int i = 0; i < 8; ++i) add(c, key(i), 0, 1, i);
  CHECK(g_idle == 0);   // (room all along)
  add(c, key(8), 0, 1, 8);
  CHECK(g_idle == 1);   // one erasure
  for (Cache::Entry& e : c.entries) e.gen = 0;
  g_idle = 0;
  CHECK(c.make_room(1, idle));
  CHECK(g_idle == 1 && c.entries.empty() && g_live == 0);   // eight erasures
  for (int i = 0; i < 12; ++i) {   // overfilled by hand, four stale and eight live: the sweep AND an eviction in one make_room
    Layout L;
    CHECK(L.d_table.try_alloc(16) == hipSuccess);
    c.entries.push_back(Cache::Entry{key(i), 0, i < 4 ? 0 : 1, ++c.clock, false, std::move(L)});
  }
  g_idle = 0;
  CHECK(c.make_room(1, idle));
  CHECK(g_idle == 1 && c.entries.size() == 7 && !has(c, 4, 1) && has(c, 5, 1) && g_live == 7);
  g_idle = 0;
  c.clear(idle);
  CHECK(g_idle == 1 && c.entries.empty() && g_live == 0);
  // an idle() that fails: nothing goes
  for (int i = 0; i < 8; ++i) add(c, key(i), 0, 1, i);
  CHECK(!c.make_room(1, [] { return false; }) && c.entries.size() == 8 && g_live == 8);
  CHECK(!c.make_room(2, [] { return false; }) && c.entries.size() == 8 && g_live == 8);
}

static void a_declined_entry_is_an_entry() {
  Cache c;
  CHECK(c.make_room(1, idle));
  c.insert_declined(key(0), 0, 1);
  Cache::Entry* e = c.find(key(0), 0, 1);
  CHECK(e && e->declined && !e->layout.d_table && c.entries.size() == 1 && g_live == 0);   // found as declined; a slot, no memory
  CHECK(c.find(key(0), 0, 2) == nullptr);                                                   // not under another gen
  for (int i = 1; i < 8; ++i) add(c, key(i), 0, 1, i);
  for (int i = 1; i < 8; ++i) CHECK(c.find(key(i), 0, 1) != nullptr);
  add(c, key(8), 0, 1, 8);   // the declined one is the least recently used: evicted like any other
  CHECK(c.entries.size() == 8 && !has(c, 0, 1) && c.find(key(0), 0, 1) == nullptr);
  CHECK(c.make_room(1, idle));
  c.insert_declined(key(0), 0, 1);
  CHECK(c.make_room(2, idle) && c.entries.empty() && g_live == 0);   // ... and swept with its gen
}

static void the_same_ranges_with_another_n_wg_are_another_entry() {
  Cache c;
  Cache::Entry* a = add(c, key(0), 4, 1, 40);
  CHECK(a->layout.tag == 40);
  CHECK(c.find(key(0), 8, 1) == nullptr && c.find(key(0), 0, 1) == nullptr);
  add(c, key(0), 8, 1, 80);
  CHECK(c.entries.size() == 2 && c.find(key(0), 4, 1)->layout.tag == 40 && c.find(key(0), 8, 1)->layout.tag == 80);
  CHECK(c.find(Key{0, 50, 50, 60}, 4, 1) == nullptr);   // (more ranges: another key)
}

static void size_never_exceeds_the_capacity() {
  Cache c;
  unsigned long long x = 12345;   // (a fixed script: the same 100 operations on every run)
  long long gen = 1;
  for (int step = 0; step < 100; ++step) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const int op = (int)((x >> 33) % 10), k = (int)((x >> 40) % 12), n_wg = (int)((x >> 50) % 2) * 4;
    if (op == 0) ++gen;                    // a new ranking: what is cached is stale from here on
    else if (op == 1 && step % 7 == 0) c.clear(idle);
    else if (Cache::Entry* e = c.find(key(k), n_wg, gen)) CHECK(e->gen == gen && e->n_wg == n_wg && e->ranges == key(k));
    else if (op < 4) {
      CHECK(c.make_room(gen, idle));
      c.insert_declined(key(k), n_wg, gen);
    } else add(c, key(k), n_wg, gen, step);
    CHECK(c.entries.size() <= Cache::CAP);
    int live = 0;
    for (const Cache::Entry& e : c.entries) live += !e.declined;
    CHECK(g_live == live);   // every built layout holds its block, nothing else does
  }
}

static void clear_and_destruction_release_everything() {
  {
    Cache c;
    for (int i = 0; i < 6; ++i) add(c, key(i), 0, 1, i);
    CHECK(g_live == 6);
    g_idle = 0;
    c.clear(idle);
    CHECK(g_idle == 1 && g_live == 0 && c.entries.empty());
    c.clear(idle);
    CHECK(g_idle == 1);   // (empty: nothing to wait for)
    for (int i = 0; i < 6; ++i) add(c, key(i), 0, 1, i);
    CHECK(g_live == 6);
  }
  CHECK(g_live == 0);   // (the destructor: the way of dsgd_destroy)
}

static void a_pointer_from_find_survives_further_finds() {
  Cache c;
  for (int i = 0; i < 8; ++i) add(c, key(i), 0, 1, i);
  Cache::Entry* e = c.find(key(2), 0, 1);
  int* const table = e->layout.d_table;
  for (int round = 0; round < 3; ++round)
    for (int i = 0; i < 8; ++i) CHECK(c.find(key(i), 0, 1) != nullptr);
  CHECK(c.find(key(9), 0, 1) == nullptr);
  CHECK(e == c.find(key(2), 0, 1) && e->layout.tag == 2 && e->layout.d_table == table);
  table[15] = 7;   // (still the entry's block: the sanitizer would say otherwise)
}

int main() {
  a_hit_restamps_and_protects_from_eviction();
  CHECK(g_live == 0);   // (every cache lets go of its layouts when it goes)
  the_ninth_insert_evicts_the_least_recently_used();
  entries_of_another_gen_go_first_and_no_live_one_needlessly();
  idle_runs_once_per_make_room_that_erases_and_never_otherwise();
  a_declined_entry_is_an_entry();
  the_same_ranges_with_another_n_wg_are_another_entry();
  size_never_exceeds_the_capacity();
  clear_and_destruction_release_everything();
  a_pointer_from_find_survives_further_finds();
  CHECK(g_live == 0 && g_allocs == g_frees);
  if (g_bad) return 1;
  std::fprintf(stderr, "all checks passed (%d allocations, %d releases)\n", g_allocs, g_frees);
  return 0;
}
