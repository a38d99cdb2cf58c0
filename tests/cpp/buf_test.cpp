// csrc/dsgd_buf.hpp on its own, on the CPU: the header compiled against a stand-in for the handful of HIP calls it uses --
// plain malloc / free that count live blocks and releases, and fail the next allocation on request.  Built with
// -fsanitize=address,undefined and run directly by tests/test_buf_helper.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>

// ---- the stand-ins ----
typedef int hipError_t;
typedef void* hipEvent_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2 };
enum { DSGD_OK = 0, DSGD_EHIP = -5 };
static int g_live = 0, g_frees = 0, g_events = 0;
static bool g_fail_next = false, g_fail_next_map = false;
static hipError_t stub_alloc(void** p, size_t bytes) {
  if (g_fail_next) {
    g_fail_next = false;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  ++g_live;
  return hipSuccess;
}
static hipError_t stub_free(void* p) {
  std::free(p);
  --g_live;
  ++g_frees;
  return hipSuccess;
}
static hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
static hipError_t hipFree(void* p) { return stub_free(p); }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes); }
static hipError_t hipHostFree(void* p) { return stub_free(p); }
static hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
  if (g_fail_next_map) {
    g_fail_next_map = false;
    return hipErrorOutOfMemory;
  }
  *d = h;
  return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t) {
  --g_events;
  return hipSuccess;
}
static const char* hipGetErrorString(hipError_t) { return "stub: out of memory"; }
static char g_err[256];
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#include "dsgd_buf.hpp"

static int g_bad = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_bad;                                                            \
    }                                                                     \
  } while (0)

template <typename Buf>
static void owner_checks() {
  const int frees0 = g_frees;
  {
    Buf a;
    CHECK(a.get() == nullptr && a.cap() == 0 && !a);
    CHECK(a.alloc(100) == DSGD_OK && a.get() != nullptr && a.cap() == 100 && g_live == 1);
    int* raw = a;   // the implicit conversion the call sites rely on
    raw[99] = 7;
    CHECK(a[99] == 7 && a + 1 == raw + 1);
    // move: the source is left empty, nothing is released
    Buf b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == raw && b.cap() == 100 && g_live == 1 && g_frees == frees0);
    Buf c;
    CHECK(c.alloc(5) == DSGD_OK && g_live == 2);
    c = std::move(b);   // the target's old block goes, once
    CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == raw && c.cap() == 100 && g_live == 1 && g_frees == frees0 + 1);
    // reserve below or at the capacity does nothing
    CHECK(c.reserve(100) == DSGD_OK && c.reserve(1) == DSGD_OK && c.get() == raw && g_frees == frees0 + 1);
    // reserve above it releases the old block exactly once
    CHECK(c.reserve(101) == DSGD_OK && c.cap() == 101 && g_live == 1 && g_frees == frees0 + 2);
    // a failed allocation: null, capacity 0, the old block released
    g_fail_next = true;
    CHECK(c.reserve(1000) == DSGD_EHIP && c.get() == nullptr && c.cap() == 0 && g_live == 0 && g_frees == frees0 + 3);
    CHECK(g_err[0] != 0);
    // try_alloc: the runtime's own error, the error text untouched
    g_err[0] = 0, g_fail_next = true;
    CHECK(c.try_alloc(8) == hipErrorOutOfMemory && g_err[0] == 0 && c.get() == nullptr && c.cap() == 0 && g_live == 0);
    CHECK(c.try_alloc(8) == hipSuccess && c.cap() == 8 && g_live == 1);
    c.reset();
    g_fail_next = true;
    CHECK(c.alloc(8) == DSGD_EHIP && c.get() == nullptr && c.cap() == 0 && g_live == 0 && g_frees == frees0 + 4);
    // reset releases once, and only once
    CHECK(c.alloc(8) == DSGD_OK && g_live == 1);
    c.reset();
    c.reset();
    CHECK(c.get() == nullptr && c.cap() == 0 && g_live == 0 && g_frees == frees0 + 5);
    CHECK(c.alloc(3) == DSGD_OK && g_live == 1);   // left to the destructor
  }
  CHECK(g_live == 0 && g_frees == frees0 + 6);
}

int main() {
  owner_checks<DevBuf<int>>();
  owner_checks<HostBuf<int>>();
  {   // growth by doubling (the index staging): at least twice the capacity, never less than asked
    DevBuf<char> d;
    CHECK(d.reserve(10, Grow::twice) == DSGD_OK && d.cap() == 10);
    CHECK(d.reserve(11, Grow::twice) == DSGD_OK && d.cap() == 20);
    CHECK(d.reserve(100, Grow::twice) == DSGD_OK && d.cap() == 100);
    DevBuf<void> v;   // untyped: bytes
    CHECK(v.alloc(16) == DSGD_OK && v.cap() == 16);
  }
  {   // pinned: the flags are kept; mapped memory hands out the device's address
    HostBuf<double> h;
    CHECK(h.alloc(4) == DSGD_OK && h.flags() == hipHostMallocDefault && h.dev() == nullptr);
    CHECK(h.alloc(4, hipHostMallocMapped) == DSGD_OK && h.flags() == hipHostMallocMapped && h.dev() == h.get());
    HostBuf<double> k(std::move(h));
    CHECK(h.dev() == nullptr && k.dev() == k.get() && k.flags() == hipHostMallocMapped);
    g_fail_next = true;
    CHECK(k.alloc(9, hipHostMallocMapped) == DSGD_EHIP && k.get() == nullptr && k.dev() == nullptr && k.cap() == 0);
    // the pinned block is there but its device address is not to be had: released again, once, and empty
    CHECK(k.alloc(4, hipHostMallocMapped) == DSGD_OK && g_live == 1);
    const int frees = g_frees;
    g_fail_next_map = true;
    CHECK(k.alloc(9, hipHostMallocMapped) == DSGD_EHIP && k.get() == nullptr && k.dev() == nullptr && k.cap() == 0);
    CHECK(g_live == 0 && g_frees == frees + 2);   // the old block and the new one
  }
  {   // events: destroyed once, by the last owner
    int dummy = 0;
    Event e;
    e.e = &dummy, g_events = 1;
    Event f(std::move(e));
    CHECK(e.e == nullptr && f.e == &dummy && g_events == 1);
    f.reset();
    f.reset();
    CHECK(g_events == 0);
  }
  CHECK(g_live == 0 && g_events == 0);
  if (g_bad) return 1;
  std::fprintf(stderr, "all checks passed (%d releases)\n", g_frees);
  return 0;
}
