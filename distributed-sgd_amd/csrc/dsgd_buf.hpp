// Owning buffers of the host side (csrc/dsgd_hip.hip): DevBuf<T> owns device memory, HostBuf<T> pinned host memory, Event a
// hipEvent_t its owner created.  All are move-only, null (capacity 0) when empty, and release in their destructor; nothing
// here knows about streams -- who replaces or drops a buffer that a stream may still use synchronises that stream first.
//
// Every allocation of the library goes through the two function pairs below (the plan cache, which keeps blocks by its own
// rules, included): the only callers of the four HIP allocation calls.
//
// Expects, declared before this header: the HIP runtime's allocation calls, hipGetErrorString, and the project's
// `int fail(int code, const char* fmt, ...)` with DSGD_OK / DSGD_EHIP (tests/cpp/buf_test.cpp brings stand-ins).
#pragma once

#include <cstddef>

#pragma GCC visibility push(hidden)   // (host plumbing: nothing of it belongs in the library's dynamic symbols)

#ifdef DSGD_TEST_COLLECTIVE_SEAM   // test builds only: the bytes currently held, by block (dsgd_test_live_bytes)
#include <mutex>
#include <unordered_map>
struct LiveBytes {
  std::mutex mu;
  std::unordered_map<void*, size_t> blocks;
  long long bytes = 0;
  void took(void* p, size_t n) {
    std::lock_guard<std::mutex> lk(mu);
    blocks[p] = n, bytes += (long long)n;
  }
  void gives(void* p) {   // BEFORE the release: afterwards the address may already be another thread's new block
    std::lock_guard<std::mutex> lk(mu);
    bytes -= (long long)blocks[p], blocks.erase(p);
  }
};
static LiveBytes g_live_dev, g_live_pin;
#define DSGD_LIVE(call) call
#else
#define DSGD_LIVE(call) ((void)0)
#endif

static hipError_t dev_alloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) *p = nullptr;
  else if (*p) DSGD_LIVE(g_live_dev.took(*p, bytes));
  return e;
}
static void dev_free(void* p) {
  if (!p) return;
  DSGD_LIVE(g_live_dev.gives(p));
  (void)hipFree(p);
}
static hipError_t pin_alloc(void** p, size_t bytes, unsigned int flags) {
  const hipError_t e = hipHostMalloc(p, bytes, flags);
  if (e != hipSuccess) *p = nullptr;
  else if (*p) DSGD_LIVE(g_live_pin.took(*p, bytes));
  return e;
}
static void pin_release(void* p) {
  if (!p) return;
  DSGD_LIVE(g_live_pin.gives(p));
  (void)hipHostFree(p);
}

template <typename T> struct BufElem { static constexpr size_t size = sizeof(T); };
template <> struct BufElem<void> { static constexpr size_t size = 1; };   // untyped buffers count bytes

enum class Grow { exact, twice };   // reserve: to what was asked for / to at least twice the present capacity

template <typename T>
class DevBuf {
  T* p_ = nullptr;
  size_t cap_ = 0;   // elements

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) reset(), p_ = o.p_, cap_ = o.cap_, o.p_ = nullptr, o.cap_ = 0;
    return *this;
  }
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t cap() const { return cap_; }
  void reset() { dev_free(p_), p_ = nullptr, cap_ = 0; }
  // drops what it held, then takes n elements; empty after a failure.  try_alloc hands the runtime's error back and leaves the
  // thread's error text alone (builders that fall back to another path); alloc reports through fail()
  hipError_t try_alloc(size_t n) {
    reset();
    const hipError_t e = dev_alloc((void**)&p_, BufElem<T>::size * n);
    if (e == hipSuccess) cap_ = n;
    return e;
  }
  int alloc(size_t n) {
    const hipError_t e = try_alloc(n);
    return e == hipSuccess ? DSGD_OK : fail(DSGD_EHIP, "device allocation of %zu bytes: %s", BufElem<T>::size * n, hipGetErrorString(e));
  }
  int reserve(size_t n, Grow g = Grow::exact) {   // grow-only; the contents do not survive a grow
    return n <= cap_ ? DSGD_OK : alloc(g == Grow::twice && 2 * cap_ > n ? 2 * cap_ : n);
  }
};

template <typename T>
class HostBuf {
  T* p_ = nullptr;
  size_t cap_ = 0;   // elements
  T* dev_ = nullptr;   // mapped memory: the device's address of it
  unsigned int flags_ = 0;

 public:
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : p_(o.p_), cap_(o.cap_), dev_(o.dev_), flags_(o.flags_) { o.p_ = o.dev_ = nullptr, o.cap_ = 0; }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) reset(), p_ = o.p_, cap_ = o.cap_, dev_ = o.dev_, flags_ = o.flags_, o.p_ = o.dev_ = nullptr, o.cap_ = 0;
    return *this;
  }
  ~HostBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  T* dev() const { return dev_; }
  size_t cap() const { return cap_; }
  unsigned int flags() const { return flags_; }   // the hipHostMalloc flags of the last alloc
  void reset() { pin_release(p_), p_ = dev_ = nullptr, cap_ = 0; }
  hipError_t try_alloc(size_t n, unsigned int flags = hipHostMallocDefault) {   // (as DevBuf's)
    reset();
    flags_ = flags;
    hipError_t e = pin_alloc((void**)&p_, BufElem<T>::size * n, flags);
    if (e == hipSuccess && (flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer((void**)&dev_, p_, 0)) != hipSuccess) reset();
    if (e == hipSuccess) cap_ = n;
    return e;
  }
  int alloc(size_t n, unsigned int flags = hipHostMallocDefault) {
    const hipError_t e = try_alloc(n, flags);
    return e == hipSuccess ? DSGD_OK : fail(DSGD_EHIP, "pinned allocation of %zu bytes: %s", BufElem<T>::size * n, hipGetErrorString(e));
  }
  int reserve(size_t n, unsigned int flags = hipHostMallocDefault) { return n <= cap_ ? DSGD_OK : alloc(n, flags); }   // grow-only
};

struct Event {   // (instead of a destroy line per owner: Pinned, FstepLayout -- pin_free and fstep_free went with it)
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) reset(), e = o.e, o.e = nullptr;
    return *this;
  }
  ~Event() { reset(); }
  operator hipEvent_t() const { return e; }
  void reset() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
};

#pragma GCC visibility pop
