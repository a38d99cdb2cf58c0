// The device blocks of plans, cached across plans (host only; after dsgd_buf.hpp).  A plan (dsgd_plan_create) takes its
// blocks here and hands them back when it goes (dsgd_plan_destroy): an epoch of the reference is one plan
// (core/Master.scala:179-199), so plans come and go with every epoch -- hipMalloc / hipFree per plan (the latter
// synchronises the device) would sit in the fit loop.  PlanCache keeps the blocks, CacheBuf<T> is a plan's hold on one.
//
// Expects, beyond what dsgd_buf.hpp does: hipEventCreateWithFlags / hipEventRecord / hipEventQuery, hipStreamWaitEvent,
// hipStreamSynchronize and hipGetLastError (tests/cpp/plan_cache_test.cpp brings stand-ins).
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

struct PlanCache {
  struct Block {
    void* p = nullptr;
    size_t bytes = 0;
    Event ev;                      // recorded on the launch stream when the block came back: its last reader
    unsigned long long tick = 0;   // cache_tick when it came back: a block no plan took for CACHE_MAX_AGE hand-backs is freed
  };
  static constexpr unsigned long long CACHE_MAX_AGE = 48;   // (an epoch's plan hands back ~10 blocks: blocks unused for ~5 plans)
  static constexpr size_t MAX_BLOCKS = 256;
  std::vector<Block> cache;
  size_t cache_bytes = 0;
  unsigned long long cache_tick = 0;
  size_t cache_cap = (size_t)8 << 30;   // DSGD_CACHE_MB (dsgd_cache_trim gives blocks back on request)
  std::vector<Event> ev_pool;           // events of blocks in use, for the next ones
  // the context's streams (dsgd_create sets both): blocks come back behind the LAUNCH stream's work and are taken on the
  // BUILD stream, which the context creates with its first plan (null until then)
  const hipStream_t* launch = nullptr;
  const hipStream_t* build = nullptr;
  PlanCache() = default;
  PlanCache(const PlanCache&) = delete;
  PlanCache& operator=(const PlanCache&) = delete;
  ~PlanCache() { drop_all(); }
  // take: the smallest cached block of at least `bytes` and at most twice that (+ 64 KiB); the BUILD stream waits for the
  // block's last reader on the launch stream (the event recorded when it came back).  Otherwise a fresh allocation.
  // *got: the block's full size, for give.  Returns 1 for a soft failure (memory; the error text untouched): the caller
  // falls back.
  int take(void** out, size_t bytes, size_t* got) {
    bytes = (std::max<size_t>(bytes, 1) + 4095) & ~(size_t)4095;
    int best = -1;
    for (int i = 0; i < (int)cache.size(); ++i)
      if (cache[i].bytes >= bytes && cache[i].bytes <= 2 * bytes + (1u << 16) && (best < 0 || cache[i].bytes < cache[best].bytes)) best = i;
    if (best >= 0) {
      Block blk = std::move(cache[(size_t)best]);
      cache.erase(cache.begin() + best);
      cache_bytes -= blk.bytes;
      if (blk.ev) {
        const hipError_t e = *build ? hipStreamWaitEvent(*build, blk.ev, 0) : hipSuccess;
        ev_pool.push_back(std::move(blk.ev));
        if (e != hipSuccess) {
          dev_free(blk.p);   // (nobody could order a use of it: back to the device, which waits for its last reader)
          return fail(DSGD_EHIP, "hipStreamWaitEvent (a cached block's last reader): %s", hipGetErrorString(e));
        }
      }
      *out = blk.p;
      *got = blk.bytes;
      return DSGD_OK;
    }
    void* q = nullptr;
    hipError_t e = dev_alloc(&q, bytes);
    if (e != hipSuccess && !cache.empty()) {   // (memory is tight: give the cached blocks back and try once more)
      (void)hipGetLastError();
      flush();
      e = dev_alloc(&q, bytes);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return 1;   // soft: the caller falls back
    }
    *out = q;
    *got = bytes;
    return DSGD_OK;
  }
  // give back: the block's last reader is whatever the launch stream holds now.  `bytes` is what take handed out; 0 marks a
  // block allocated outside the cache (CacheBuf::alloc_uncached), which is freed -- as is any block the cache has no room for
  void give(void* q, size_t bytes) {
    if (!q) return;
    ++cache_tick;
    if ((cache_tick & 15) == 0) trim(cache_cap, true);
    if (bytes == 0 || cache_bytes + bytes > cache_cap || cache.size() >= MAX_BLOCKS) {
      dev_free(q);
      return;
    }
    Block blk;
    blk.p = q;
    blk.bytes = bytes;
    if (!ev_pool.empty()) {
      blk.ev = std::move(ev_pool.back());
      ev_pool.pop_back();
    } else if (hipEventCreateWithFlags(&blk.ev.e, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      dev_free(q);
      return;
    }
    if (hipEventRecord(blk.ev, *launch) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(*launch);
    }
    blk.tick = cache_tick;
    cache.push_back(std::move(blk));
    cache_bytes += bytes;
  }
  // blocks beyond `keep_bytes` (oldest first) or older than CACHE_MAX_AGE hand-backs go back to the device: a block whose
  // last reader has finished is freed at once, one still being read stays (hipFree would wait for the device)
  void trim(size_t keep_bytes, bool aged_only) {
    for (size_t i = 0; i < cache.size();) {
      Block& b = cache[i];
      const bool aged = cache_tick - b.tick > CACHE_MAX_AGE;
      const bool over = !aged_only && cache_bytes > keep_bytes;
      if ((aged || over) && (!b.ev || hipEventQuery(b.ev) == hipSuccess)) {
        dev_free(b.p);
        if (b.ev) ev_pool.push_back(std::move(b.ev));
        cache_bytes -= b.bytes;
        cache.erase(cache.begin() + (long)i);
      } else {
        (void)hipGetLastError();   // (hipErrorNotReady of the query)
        ++i;
      }
    }
  }
  void drop_all() {   // (dsgd_destroy, after the live plans gave their blocks back: the streams are idle)
    flush();
    ev_pool.clear();
  }
 private:
  void flush() {   // every cached block back to the device, its event to the pool
    for (Block& b : cache) {
      dev_free(b.p);
      if (b.ev) ev_pool.push_back(std::move(b.ev));
    }
    cache.clear();
    cache_bytes = 0;
  }
};

// A plan's hold on one block: move-only, null when empty; reset() (and the destructor) hands the block back to the cache it
// came from, behind an event on the launch stream.
template <typename T>
class CacheBuf {
  T* p_ = nullptr;
  size_t bytes_ = 0;   // the block's size as the cache handed it out (0: alloc_uncached)
  PlanCache* cache_ = nullptr;

 public:
  CacheBuf() = default;
  CacheBuf(const CacheBuf&) = delete;
  CacheBuf& operator=(const CacheBuf&) = delete;
  CacheBuf(CacheBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_), cache_(o.cache_) { o.p_ = nullptr, o.bytes_ = 0; }
  CacheBuf& operator=(CacheBuf&& o) noexcept {
    if (this != &o) reset(), p_ = o.p_, bytes_ = o.bytes_, cache_ = o.cache_, o.p_ = nullptr, o.bytes_ = 0;
    return *this;
  }
  ~CacheBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  void reset() {
    if (p_) cache_->give(p_, bytes_);
    p_ = nullptr, bytes_ = 0;
  }
  // drops what it held, then takes n elements from the cache: DSGD_OK, or 1 for a soft failure (PlanCache::take); empty after
  // a failure
  int take(PlanCache& cache, size_t n) {
    reset();
    void* q = nullptr;
    const int rc = cache.take(&q, BufElem<T>::size * n, &bytes_);
    if (rc == DSGD_OK) p_ = static_cast<T*>(q), cache_ = &cache;
    else bytes_ = 0;
    return rc;
  }
  // ... n elements of its own, outside the cache (the host builder of the column slices, whose synchronous copies are not
  // ordered behind a cached block's last reader): reset() counts as a hand-back of `cache` but frees the block
  hipError_t alloc_uncached(PlanCache& cache, size_t n) {
    reset();
    cache_ = &cache;
    return dev_alloc((void**)&p_, BufElem<T>::size * n);
  }
};

#pragma GCC visibility pop
