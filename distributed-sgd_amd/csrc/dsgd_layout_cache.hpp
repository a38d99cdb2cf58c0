// The device layouts a gradient family keeps per row-range configuration (host only; after dsgd_buf.hpp): the row chunks'
// tile tables (csrc/dsgd_fstep_host.hpp), the SVM's column lists (csrc/dsgd_tcol_host.hpp) and the logistic model's
// (csrc/dsgd_lg_calls.hpp).  LayoutCache<L> holds at most CAP of them and owns every rule they share -- the key, the
// generation, least-recently-used eviction, "declined for good" -- so that a caller is: find, make_room, build, insert.
//
// The cache knows nothing of streams: whoever drops a layout that a stream may still read makes the stream idle first.
// make_room and clear take that as a callable `bool idle()` (true: idle now) and call it ONCE, before the first entry
// goes, and not at all when none does.
//
// An Entry* is valid until the next make_room, insert, insert_declined or clear; find moves nothing.
// (tests/cpp/layout_cache_test.cpp holds every rule by name, against stand-ins for the HIP calls of dsgd_buf.hpp.)
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

template <class L>
struct LayoutCache {
  static constexpr size_t CAP = 8;
  struct Entry {
    std::vector<long long> ranges;   // the key: row_begin, row_end per worker ...
    int n_wg = 0;                    // ... and one int (the row chunks' workgroups per worker; 0 for the others)
    long long gen = -1;              // the context's layout_gen the layout was built under
    unsigned long long used = 0;     // the clock at its last find or insert
    bool declined = false;           // no layout to be had for this key, for good: `layout` is empty, the caller's other path
    L layout;
  };
  std::vector<Entry> entries;
  unsigned long long clock = 0;

  // the entry of this key under this generation (declined ones too: the caller asks), stamped; or null
  Entry* find(const std::vector<long long>& ranges, int n_wg, long long gen) {
    for (Entry& e : entries)
      if (e.gen == gen && e.n_wg == n_wg && e.ranges == ranges) {
        e.used = ++clock;
        return &e;
      }
    return nullptr;
  }
  // room for one insert under `gen`: every entry of another generation goes, then the least recently used ones while CAP
  // are left.  false: idle() failed -- nothing went
  template <class Idle>
  bool make_room(long long gen, Idle&& idle) {
    size_t stale = 0;
    for (const Entry& e : entries) stale += e.gen != gen;
    if (stale == 0 && entries.size() < CAP) return true;
    if (!idle()) return false;
    for (size_t i = 0; i < entries.size();)
      if (entries[i].gen != gen) entries.erase(entries.begin() + (long)i);
      else ++i;
    while (entries.size() >= CAP) {
      size_t v = 0;
      for (size_t i = 1; i < entries.size(); ++i)
        if (entries[i].used < entries[v].used) v = i;
      entries.erase(entries.begin() + (long)v);
    }
    return true;
  }
  // (behind make_room) a built layout; a key remembered as declined
  Entry* insert(std::vector<long long> ranges, int n_wg, long long gen, L&& layout) {
    entries.push_back(Entry{std::move(ranges), n_wg, gen, ++clock, false, std::move(layout)});
    return &entries.back();
  }
  void insert_declined(std::vector<long long> ranges, int n_wg, long long gen) {
    entries.push_back(Entry{std::move(ranges), n_wg, gen, ++clock, true, L()});
  }
  template <class Idle>
  void clear(Idle&& idle) {
    if (entries.empty()) return;
    (void)idle();
    entries.clear();
  }
};

#pragma GCC visibility pop
