// csrc/dsgd_layout_host.hpp on its own, on the CPU: the arithmetic behind every table the gradient kernels read -- wave tiles
// and lane descriptors, the split streams' offsets, tile ranges, row chunks, virtual tiles, fixed-point shifts.  Built with
// -fsanitize=address,undefined and run directly by tests/test_layout_host.py.  Every input vector has exactly the length the
// functions are entitled to read (n_rows + 1 offsets, n_rows labels, ...), so an over-read is a heap overflow the sanitizer
// reports.
//
// Two kinds of check:
//   (a) a slow decoder of its own, written from the comments on WTile, on the 16-bit lane descriptor, on VtLane, FChunk and
//       StreamSeg (csrc/dsgd_layout_types.hpp) and not from the builders, recovers rows, slot ranges and label signs from the
//       tables and holds them to the inputs;
//   (b) a 64-bit FNV-1a digest of every output table, held to constants recorded from the functions as they stood inside
//       csrc/dsgd_hip.hip at commit e936d6a (the parent of the commit that moved them), on the same inputs with equal
//       shares: the move changed no byte.  (`layout_host_test --print` prints the digests instead of comparing them.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "dsgd_layout_host.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checks;                                                          \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

typedef std::vector<long long> VLL;

// ---- digests ---------------------------------------------------------------------------------------------------------
struct Fnv {
  uint64_t h = 1469598103934665603ULL;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ULL;
  }
  void num(long long v) { bytes(&v, sizeof v); }
  template <typename T>
  void vec(const std::vector<T>& v) {   // (every record hashed here is free of padding: the sizes are asserted in the types header)
    num((long long)v.size());
    if (!v.empty()) bytes(v.data(), sizeof(T) * v.size());
  }
};
static Fnv d_tiles, d_split, d_cold_shift, d_locate, d_stream, d_chunks, d_vt, d_shift;

// ---- inputs ----------------------------------------------------------------------------------------------------------
static VLL starts(const VLL& len) {   // exactly n + 1 entries on the heap
  VLL rp(len.size() + 1, 0);
  for (size_t i = 0; i < len.size(); ++i) rp[i + 1] = rp[i] + len[i];
  return rp;
}
static std::vector<signed char> labels(size_t n) {
  std::vector<signed char> y(n);
  for (size_t i = 0; i < n; ++i) y[i] = (signed char)((i * 7 + 3) % 5 < 2 ? 1 : -1);
  return y;
}
struct Lcg {
  uint32_t s;
  uint32_t next(uint32_t m) {
    s = s * 1664525u + 1013904223u;
    return (s >> 8) % m;
  }
};

// a ranked CSR as the split sees it: hot and cold entries per row
struct Data {
  VLL hot, cold;
  bool has_cold = true;
  // what split_offsets makes of it
  VLL rp, hrp, ctp, crp, long_rows, long_weight;
  std::vector<signed char> y;
  HostTiles ht, hc;
  long long n() const { return (long long)hot.size(); }
};
static void add(Data& d, long long hot, long long cold) {
  d.hot.push_back(hot);
  d.cold.push_back(cold);
}
static bool is_long(long long hot, long long cold) { return hot > WS_MAXNNZ || cold > WS_MAXNNZ; }

// ---- the decoder (from the comments on WTile and the lane descriptor) ----------------------------------------------------
struct DecRow {
  long long row, begin, end;   // global row, its slots [begin, end) of the stream
  bool ypos;
};
// Lane l owns the slots [8l, 8l + 8) of the window at pos0; bit k of its descriptor marks a row start at slot 8l + k, bit
// 8 + k the label sign of the row ENDING there.  The first start opens local row 1 (global row r0), every later one closes a
// row, the last one (start number rows + 1) is the end mark, at the slot count of info's upper half.
static std::vector<DecRow> decode_tile(const WTile& t, const unsigned short* meta) {
  const int nrows = (int)(short)(t.info & 0xffff);
  const long long nslots = (long long)((unsigned int)t.info >> 16);
  CHECK(nrows >= 1);
  CHECK(t.pos0 % 8 == 0);
  CHECK(nslots >= 1 && nslots - 1 < WS_SLOTS);   // the last slot lies below pos0 + WS_SLOTS
  std::vector<DecRow> rows;
  long long open = -1;
  int starts_seen = 0;
  for (int slot = 0; slot < WS_SLOTS; ++slot) {
    const unsigned int m = meta[slot / 8];
    const bool st = (m >> (slot % 8)) & 1u, ys = (m >> (8 + slot % 8)) & 1u;
    if (!st) {
      CHECK(!ys);
      continue;
    }
    ++starts_seen;
    if (open >= 0) rows.push_back(DecRow{t.r0 + (long long)rows.size(), t.pos0 + open, t.pos0 + slot, ys});
    else CHECK(!ys);   // nothing ends at the first start
    open = slot;
  }
  CHECK(starts_seen == nrows + 1);
  CHECK((int)rows.size() == nrows);
  CHECK(open == nslots);
  return rows;
}
// the tiles [tb, te) of a table hold exactly the rows of [rb, re) with 1 .. WS_MAXNNZ slots, whole and in order
static void check_tiles(const VLL& sp, const std::vector<signed char>& y, long long rb, long long re, const std::vector<WTile>& wt,
                        const std::vector<unsigned short>& meta, size_t tb, size_t te, int max_rows) {
  std::vector<DecRow> got;
  for (size_t t = tb; t < te; ++t) {
    CHECK(meta.size() >= (t + 1) * 64);
    const std::vector<DecRow> rows = decode_tile(wt[t], &meta[t * 64]);
    CHECK((long long)rows.size() <= max_rows);
    got.insert(got.end(), rows.begin(), rows.end());
  }
  size_t g = 0;
  for (long long i = rb; i < re; ++i) {
    const long long len = sp[(size_t)i + 1] - sp[(size_t)i];
    if (len < 1 || len > WS_MAXNNZ) continue;   // no empty row and no row longer than a tile in any tile
    CHECK(g < got.size());
    CHECK(got[g].row == i && got[g].begin == sp[(size_t)i] && got[g].end == sp[(size_t)i + 1]);
    CHECK(got[g].ypos == (y[(size_t)i] > 0));
    ++g;
  }
  CHECK(g == got.size());
}
static void check_host_tiles(const VLL& sp, const std::vector<signed char>& y, const HostTiles& ht, int max_rows) {
  const long long n = (long long)sp.size() - 1;
  long long tileable = 0;
  for (long long i = 0; i < n; ++i) tileable += sp[(size_t)i + 1] - sp[(size_t)i] >= 1 && sp[(size_t)i + 1] - sp[(size_t)i] <= WS_MAXNNZ;
  CHECK(!ht.r0.empty() && ht.r0.back() == (int)n);   // the sentinel
  if (tileable == 0) {
    CHECK(ht.wt.size() == 1 && ht.wt[0].info == 0xffff && ht.wt[0].pos0 == 0 && ht.wt[0].r0 == 0);
    CHECK(ht.r0.size() == 1);
    CHECK(ht.meta16 == std::vector<unsigned short>(64, 0));
    return;
  }
  CHECK(ht.r0.size() == ht.wt.size() + 1 && ht.meta16.size() == ht.wt.size() * 64);
  for (size_t t = 0; t < ht.wt.size(); ++t) CHECK(ht.r0[t] == ht.wt[t].r0);
  check_tiles(sp, y, 0, n, ht.wt, ht.meta16, 0, ht.wt.size(), max_rows);
}
static void digest_host_tiles(const HostTiles& ht) {
  d_tiles.vec(ht.wt);
  d_tiles.vec(ht.r0);
  d_tiles.vec(ht.meta16);
}
static size_t tiles_of(const VLL& len, int max_rows) {
  const VLL sp = starts(len);
  const std::vector<signed char> y = labels(len.size());
  HostTiles ht;
  build_wave_tiles(sp.data(), (long long)len.size(), y.data(), ht, max_rows);
  check_host_tiles(sp, y, ht, max_rows);
  digest_host_tiles(ht);
  return ht.r0.size() - 1;
}

static void test_tiles() {
  // every length around a lane (8) and around a tile (504); 0 and 505 stay out and close the open tile
  CHECK(tiles_of({0, 1, 7, 8, 9, 503, 504, 505, 1, 0, 9, 505, 505, 8, 7}, WS_MAXROWS) >= 4);
  // a window filled to exactly 511 slots is one tile; to 512, the last row opens the next
  CHECK(tiles_of({500, 11}, WS_MAXROWS) == 1);
  CHECK(tiles_of({500, 12}, WS_MAXROWS) == 2);
  CHECK(tiles_of({3, 500, 8}, WS_MAXROWS) == 1);
  CHECK(tiles_of({3, 500, 9}, WS_MAXROWS) == 2);
  // a row start at slot 8k + 7, inside a tile and as a tile's first row (window at 504, row at 511)
  CHECK(tiles_of({7, 504, 3, 20}, WS_MAXROWS) == 2);
  CHECK(tiles_of({15, 9, 487, 1, 1}, WS_MAXROWS) == 2);
  // the row caps: 254 rows for hot tiles, 128 for cold tiles
  for (int n : {254, 255, 256}) {
    CHECK(tiles_of(VLL((size_t)n, 1), WS_MAXROWS) == (n <= 254 ? 1u : 2u));
    CHECK(tiles_of(VLL((size_t)n, 1), CT_MAXROWS) == 2u);
  }
  CHECK(tiles_of(VLL(257, 1), CT_MAXROWS) == 3u);
  // a long row first, last, and between two tiles
  CHECK(tiles_of({505, 4, 4, 0, 4, 4, 600}, WS_MAXROWS) == 2);
  // nothing to tile: the single unused record
  CHECK(tiles_of({}, WS_MAXROWS) == 0);
  CHECK(tiles_of({0, 505, 0}, WS_MAXROWS) == 0);
}

// ---- the split -----------------------------------------------------------------------------------------------------------
static void split(Data& d) {
  VLL len(d.hot.size());
  std::vector<int> cnt(d.hot.size());
  for (size_t i = 0; i < len.size(); ++i) {
    len[i] = d.hot[i] + d.cold[i];
    cnt[i] = (int)d.cold[i];
  }
  d.rp = starts(len);
  d.y = labels(len.size());
  split_offsets(d.rp, cnt, d.has_cold, d.hrp, d.ctp, d.crp, d.long_rows, d.long_weight);
  const size_t n = len.size();
  CHECK(d.hrp.size() == n + 1 && d.ctp.size() == n + 1 && d.crp.size() == n + 1);
  CHECK(d.long_weight.size() == d.long_rows.size() + 1 && d.long_weight[0] == 0);
  size_t nl = 0;
  for (size_t i = 0; i < n; ++i) {
    const long long hs = d.hrp[i + 1] - d.hrp[i], cs = d.ctp[i + 1] - d.ctp[i], ce = d.crp[i + 1] - d.crp[i];
    if (is_long(d.hot[i], d.cold[i])) {   // on the list, and in neither stream
      CHECK(nl < d.long_rows.size() && d.long_rows[nl] == (long long)i);
      CHECK(d.long_weight[nl + 1] - d.long_weight[nl] == len[i] + 1300);
      ++nl;
      CHECK(hs == 0 && cs == 0 && ce == 0);
    } else {   // at least one slot in each stream: an explicit zero where the row has no entry
      CHECK(hs == std::max(d.hot[i], 1LL) && ce == d.cold[i]);
      CHECK(cs == (d.has_cold ? std::max(d.cold[i], 1LL) : 0));
    }
  }
  CHECK(nl == d.long_rows.size());
  d_split.vec(d.hrp);
  d_split.vec(d.ctp);
  d_split.vec(d.crp);
  d_split.vec(d.long_rows);
  d_split.vec(d.long_weight);
  build_wave_tiles(d.hrp.data(), d.n(), d.y.data(), d.ht);
  build_wave_tiles(d.ctp.data(), d.n(), d.y.data(), d.hc, CT_MAXROWS);
  check_host_tiles(d.hrp, d.y, d.ht, WS_MAXROWS);
  check_host_tiles(d.ctp, d.y, d.hc, CT_MAXROWS);
  digest_host_tiles(d.ht);
  digest_host_tiles(d.hc);
}
// every length at a lane's and a tile's edge in both streams, long rows first, last and between tiles, filler in between
static Data mixed() {
  Data d;
  Lcg g{12345u};
  add(d, 505, 3);   // long, first
  for (long long h : {0, 1, 7, 8, 9, 503, 504}) add(d, h, 1 + h % 3);
  add(d, 4, 504);
  add(d, 4, 505);   // long by its cold part
  for (int i = 0; i < 60; ++i) add(d, 1 + g.next(40), g.next(9));
  add(d, 9, 64);    // the most cold entries a virtual tile takes
  add(d, 9, 65);    // one more
  add(d, 700, 0);   // long, between two tiles
  add(d, 0, 0);     // an empty row: one explicit zero in each stream
  for (int i = 0; i < 150; ++i) add(d, 1 + g.next(90), g.next(12));
  add(d, 3, 600);   // long, last
  return d;
}
static Data one_slot(int n) {   // 254 / 128 rows fill a tile long before its slots do; 300 rows of one cold slot are refitted
  Data d;
  for (int i = 0; i < n; ++i) add(d, 1, 1);
  return d;
}
static Data long_run() {   // a stretch of nothing but long rows
  Data d;
  for (int i = 0; i < 20; ++i) add(d, 10 + i, 2);
  for (int i = 0; i < 6; ++i) add(d, 600 + i, 1);
  for (int i = 0; i < 20; ++i) add(d, 30 - i, 0);
  return d;
}
static Data no_cold() {   // every column hot: no cold stream at all
  Data d;
  d.has_cold = false;
  Lcg g{99u};
  for (int i = 0; i < 80; ++i) add(d, i == 40 ? 505 : g.next(30), 0);
  return d;
}

// ---- locate_segs and the streaming launch's worst rows ----------------------------------------------------------------------
static void check_located(const HostTiles& ht, long long rb, long long re, long long tb, long long te) {
  const long long n_tiles = (long long)ht.r0.size() - 1;
  CHECK(0 <= tb && tb <= te && te <= n_tiles);
  int before = 0;
  for (long long t = 0; t < n_tiles; ++t) {
    const long long r0 = ht.wt[(size_t)t].r0, r1 = r0 + (short)(ht.wt[(size_t)t].info & 0xffff);   // its rows [r0, r1)
    const bool meets = r0 < re && r1 > rb && rb < re;
    if (meets) CHECK(tb <= t && t < te);
    if (tb <= t && t < te && !meets) {   // wholly before the range (a long row sits in between), never behind it
      CHECK(r0 <= rb);
      if (rb < re) CHECK(r1 <= rb);      // (around an EMPTY range: the tile it lies in)
      ++before;
    }
  }
  CHECK(before <= 1);
}
static void test_locate(const Data& d) {
  const long long n = d.n();
  VLL marks = {0, 1, 2, 9, 10, 11, n / 3, n / 2, n / 2 + 1, n - 2, n - 1, n};
  for (long long r : d.long_rows) {   // ranges that begin and end at, before and behind every long row
    marks.push_back(r);
    marks.push_back(r + 1);
  }
  for (size_t t = 0; t + 1 < d.ht.r0.size(); t += 3) marks.push_back(d.ht.r0[t] + 1);   // ... and inside tiles
  std::vector<StreamSeg> segs;
  for (long long a : marks)
    for (long long b : marks)
      if (0 <= a && a <= b && b <= n) {
        StreamSeg s{};
        s.row_begin = a;
        s.row_end = b;
        segs.push_back(s);
      }
  long long max_tiles = -1, max_long = -1, max_ctiles = -1, mt = 1, ml = 0, mc = 0;
  locate_segs(d.ht.r0, d.hc.r0, d.long_rows, segs, &max_tiles, &max_long, &max_ctiles);
  for (const StreamSeg& s : segs) {
    check_located(d.ht, s.row_begin, s.row_end, s.tile_begin, s.tile_end);
    if (d.hc.r0.size() > 1) check_located(d.hc, s.row_begin, s.row_end, s.ctile_begin, s.ctile_end);
    else CHECK(s.ctile_begin == 0 && s.ctile_end == 0);
    CHECK(0 <= s.long_begin && s.long_begin <= s.long_end && s.long_end <= (long long)d.long_rows.size());
    for (long long k = 0; k < (long long)d.long_rows.size(); ++k)   // exactly the listed rows of the range
      CHECK((s.long_begin <= k && k < s.long_end) == (s.row_begin <= d.long_rows[(size_t)k] && d.long_rows[(size_t)k] < s.row_end));
    mt = std::max(mt, s.tile_end - s.tile_begin);
    ml = std::max(ml, s.long_end - s.long_begin);
    mc = std::max(mc, s.ctile_end - s.ctile_begin);
  }
  CHECK(max_tiles == mt && max_long == ml && max_ctiles == mc);
  d_locate.vec(segs);
  // the rows one workgroup of the streaming launch can meet: workgroup b owns the 16-tile groups b, b + gx, ... and, of the
  // long rows, sixteen at a time with the other workgroups
  for (long long gx : {1, 2, 5}) {
    long long rows_max = 1;
    for (const StreamSeg& s : segs) {
      const long long n_long = s.long_end - s.long_begin, long_rows = (n_long + 16 * gx - 1) / (16 * gx) * 16;
      for (long long b = 0; b < gx; ++b) {
        long long rows = 0;
        for (long long t = s.tile_begin; t < s.tile_end; ++t)
          if ((t - s.tile_begin) / 16 % gx == b && d.ht.r0.size() > 1) rows += (short)(d.ht.wt[(size_t)t].info & 0xffff);
        rows_max = std::max(rows_max, rows + long_rows);
      }
    }
    const long long worst = stream_worst_rows(segs, d.ht.r0, gx);
    CHECK(worst >= rows_max);
    d_stream.num(worst);
  }
}

// ---- row chunks ----------------------------------------------------------------------------------------------------------
static long long row_weight(const Data& d, long long i) {   // slots in the two streams + 2, or a long row's own
  if (is_long(d.hot[(size_t)i], d.cold[(size_t)i])) return d.hot[(size_t)i] + d.cold[(size_t)i] + 1300 + 2;
  return (d.hrp[(size_t)i + 1] - d.hrp[(size_t)i]) + (d.ctp[(size_t)i + 1] - d.ctp[(size_t)i]) + 2;
}
static void check_chunks(const Data& d, const std::vector<std::pair<long long, long long>>& ranges, int n_wg,
                         const std::vector<double>& share, bool digest, ChunkTables* keep = nullptr) {
  std::vector<StreamSeg> segs;
  for (const auto& r : ranges) {
    StreamSeg s{};
    s.row_begin = r.first;
    s.row_end = r.second;
    segs.push_back(s);
  }
  ChunkTables T;
  cut_row_chunks(segs, n_wg, share, d.hrp, d.ctp, d.long_rows, d.long_weight, d.y.data(), T);
  CHECK(T.chunks.size() == ranges.size() * (size_t)n_wg);
  long long tile = 0, ctile = 0, largest = 1;
  for (size_t k = 0; k < ranges.size(); ++k) {
    const long long rb = ranges[k].first, re = ranges[k].second;
    long long row = rb, wtot = 0, wmax = 0;
    for (long long i = rb; i < re; ++i) {
      wtot += row_weight(d, i);
      wmax = std::max(wmax, row_weight(d, i));
    }
    long long lng = std::lower_bound(d.long_rows.begin(), d.long_rows.end(), rb) - d.long_rows.begin();
    for (int b = 0; b < n_wg; ++b) {
      const FChunk& ch = T.chunks[k * (size_t)n_wg + (size_t)b];
      // the chunks partition the range in order (an empty chunk is allowed); so do their tiles and long rows
      CHECK(ch.row_begin == row && ch.row_end >= ch.row_begin && ch.row_end <= re);
      CHECK(ch.tile_begin == tile && ch.tile_end >= tile && ch.ctile_begin == ctile && ch.ctile_end >= ctile);
      CHECK(ch.long_begin == lng && ch.long_end >= lng);
      for (long long q = ch.long_begin; q < ch.long_end; ++q)
        CHECK(ch.row_begin <= d.long_rows[(size_t)q] && d.long_rows[(size_t)q] < ch.row_end);
      // a chunk's tiles hold its rows and no others
      check_tiles(d.hrp, d.y, ch.row_begin, ch.row_end, T.wt, T.meta, (size_t)ch.tile_begin, (size_t)ch.tile_end, WS_MAXROWS);
      check_tiles(d.ctp, d.y, ch.row_begin, ch.row_end, T.ct, T.cmeta, (size_t)ch.ctile_begin, (size_t)ch.ctile_end, CT_MAXROWS);
      if (share.empty()) {   // equal shares: no chunk outweighs the mean by more than the heaviest single row
        long long w = 0;
        for (long long i = ch.row_begin; i < ch.row_end; ++i) w += row_weight(d, i);
        CHECK((double)w <= (double)wtot / n_wg + (double)wmax);
      }
      row = ch.row_end;
      tile = ch.tile_end;
      ctile = ch.ctile_end;
      lng = ch.long_end;
      largest = std::max(largest, (long long)ch.row_end - ch.row_begin);
    }
    CHECK(row == re);
    CHECK(lng == std::lower_bound(d.long_rows.begin(), d.long_rows.end(), re) - d.long_rows.begin());
  }
  CHECK(T.worst_rows == largest);
  // the tables end where the last chunk does, or hold the one unused record
  CHECK(T.wt.size() == (size_t)std::max(tile, 1LL) && T.ct.size() == (size_t)std::max(ctile, 1LL));
  if (tile == 0) CHECK(T.wt[0].info == 0xffff);
  if (ctile == 0) CHECK(T.ct[0].info == 0xffff);
  CHECK(T.meta.size() == T.wt.size() * 64 && T.cmeta.size() == T.ct.size() * 64);
  if (digest) {
    d_chunks.vec(T.chunks);
    d_chunks.vec(T.wt);
    d_chunks.vec(T.ct);
    d_chunks.vec(T.meta);
    d_chunks.vec(T.cmeta);
    d_chunks.num(T.worst_rows);
  }
  if (keep) *keep = T;
}
static void test_chunks(const Data& d) {
  const long long n = d.n();
  for (int n_wg : {1, 3, 7}) check_chunks(d, {{0, n}}, n_wg, {}, true);
  check_chunks(d, {{3, 8}}, 8, {}, true);                                   // more workgroups than rows
  check_chunks(d, {{0, n / 6}, {n / 6, n / 2 + 5}, {n / 2 + 5, n}}, 4, {}, true);   // three workers of unequal size
  check_chunks(d, {{n / 3, n / 3}}, 2, {}, true);                           // an empty range
  if (d.ht.r0.size() > 2) check_chunks(d, {{d.ht.r0[1] + 1, n}}, 3, {}, true);   // a range that begins inside a tile
  for (long long r : d.long_rows) check_chunks(d, {{r, r + 1}}, 2, {}, true);   // ... that holds only long rows
  // unequal shares (a re-cut by measured times): still a partition; how a compiler rounds the double products may move a cut,
  // so no digest
  std::vector<double> share;
  for (int i = 0; i < 3 * 4; ++i) share.push_back(0.85 + 0.05 * (i % 7));
  check_chunks(d, {{0, n / 6}, {n / 6, n / 2 + 5}, {n / 2 + 5, n}}, 4, share, false);
}

// ---- virtual tiles -------------------------------------------------------------------------------------------------------
static VtTables check_vt(const Data& d, const std::vector<unsigned short>& ccol, const std::vector<int>& idx, const VLL& off, long long n_steps,
                         int n_workers, int n_cu, int tpw) {
  const VtStreams m{d.n(), d.hrp.data(), d.ctp.data(), d.crp.data(), d.rp.data(), d.y.data(), ccol.data()};
  VtTables T;
  CHECK(vt_tables(idx.data(), off.data(), n_steps, n_workers, n_cu, tpw, m, T));
  const long long n_lists = n_steps * n_workers;
  CHECK((long long)T.vt_off.size() == n_lists + 1 && T.vt_off[0] == 0 && (long long)T.segs.size() == 2 * n_lists);
  CHECK(T.lanes.size() == T.tile_rows.size() * 64 && (long long)T.tile_rows.size() == T.vt_off[(size_t)n_lists]);   // padded to 64 lanes
  CHECK((long long)T.grid.size() == n_steps && (long long)T.gxt.size() == n_steps && (long long)T.shift.size() == n_steps);
  size_t lr = 0;
  for (long long li = 0; li < n_lists; ++li) {
    const WorkSeg ts = T.segs[(size_t)li], ls = T.segs[(size_t)(n_lists + li)];
    CHECK(ts.begin == T.vt_off[(size_t)li] && ts.end == T.vt_off[(size_t)li + 1] && ts.end > ts.begin);   // every list starts a tile
    CHECK(ls.begin == (long long)lr);
    long long tile = ts.begin;
    int lane = 0, local = 0;
    for (long long t = off[(size_t)li]; t < off[(size_t)li + 1]; ++t) {   // in list order: consecutive lanes of one tile, or one record
      const size_t r = (size_t)idx[(size_t)t];
      const long long hot = d.hrp[r + 1] - d.hrp[r], cold = d.crp[r + 1] - d.crp[r];
      if (is_long(d.hot[r], d.cold[r]) || cold > 64) {
        CHECK(lr < T.long_rows.size());
        const MbRec& rec = T.long_rows[lr++];
        CHECK(rec.st == d.rp[r] && rec.len == d.rp[r + 1] - d.rp[r] && rec.y == (float)d.y[r]);
        continue;
      }
      const int nl = (int)std::max(std::max((hot + 7) / 8, cold), 1LL);
      if (lane + nl > 64) {   // the row does not fit behind the others: the rest of the tile is padding
        for (; lane < 64; ++lane) {
          const VtLane& L = T.lanes[(size_t)tile * 64 + (size_t)lane];
          CHECK(L.hp == 0 && L.info == 0 && L.cp == 0 && L.crank == 0);
        }
        CHECK(T.tile_rows[(size_t)tile] == local);
        ++tile;
        lane = local = 0;
        CHECK(tile < ts.end);
      }
      long long hot_next = d.hrp[r], cold_next = d.ctp[r];
      for (int j = 0; j < nl; ++j, ++lane) {
        const VtLane& L = T.lanes[(size_t)tile * 64 + (size_t)lane];
        const long long cnt = L.info & 0xf;
        CHECK(cnt == std::min(8LL, d.hrp[r + 1] - hot_next));   // the row's hot slots, eight to a lane, in order
        CHECK(L.hp == (cnt ? hot_next : 0));
        hot_next += cnt;
        CHECK(((L.info & VT_START) != 0) == (j == 0) && ((L.info & VT_LAST) != 0) == (j == nl - 1));
        CHECK(((L.info & VT_YPOS) != 0) == (d.y[r] > 0));
        CHECK((int)((L.info >> 16) & 0x3f) == local && (L.info & ~(0xfu | VT_START | VT_LAST | VT_YPOS | VT_COLD | (0x3fu << 16))) == 0);
        CHECK(((L.info & VT_COLD) != 0) == (j < cold));   // one cold entry per lane, with its rank
        if (j < cold) {
          CHECK(L.cp == cold_next && L.crank == ccol[(size_t)cold_next]);
          ++cold_next;
        } else {
          CHECK(L.cp == 0 && L.crank == 0);
        }
      }
      CHECK(hot_next == d.hrp[r + 1] && cold_next == d.ctp[r] + cold);
      ++local;
    }
    for (; lane < 64; ++lane) {
      const VtLane& L = T.lanes[(size_t)tile * 64 + (size_t)lane];
      CHECK(L.hp == 0 && L.info == 0 && L.cp == 0 && L.crank == 0);
    }
    CHECK(T.tile_rows[(size_t)tile] == local && tile + 1 == ts.end);
    CHECK(ls.end == (long long)lr);
  }
  CHECK(lr == T.long_rows.size());
  // a step's shift covers the rows ONE workgroup can meet under its grid: the first gxt workgroups of a worker walk its tiles
  // (workgroup b the 16-tile groups b, b + gxt, ...), the others its long rows, sixteen at a time
  const long long per_worker = std::max(1, n_cu / n_workers);
  for (long long s = 0; s < n_steps; ++s) {
    const long long gx = T.gxt[(size_t)s], gl = T.grid[(size_t)s] - gx;
    CHECK(gx >= 1 && gl >= 0 && (gx + gl <= per_worker || (gx == 1 && gl <= 1)));
    // tile workgroups: as many as give every wave at most tpw tiles of the step's longest list and no more, unless the worker's
    // share of the CUs caps them
    long long max_t = 1;
    for (int k = 0; k < n_workers; ++k) max_t = std::max(max_t, T.segs[(size_t)(s * n_workers + k)].end - T.segs[(size_t)(s * n_workers + k)].begin);
    CHECK((gx * 16 * tpw >= max_t && (gx - 1) * 16 * tpw < max_t) || (gx * 16 * tpw < max_t && gx == std::max(1LL, per_worker - gl)));
    long long worst = 1;
    for (int k = 0; k < n_workers; ++k) {
      const WorkSeg ts = T.segs[(size_t)(s * n_workers + k)], ls = T.segs[(size_t)(n_lists + s * n_workers + k)];
      for (long long b = 0; b < gx; ++b) {
        long long rows = 0;
        for (long long t = ts.begin; t < ts.end; ++t)
          if ((t - ts.begin) / 16 % gx == b)
            for (int l = 0; l < 64; ++l) rows += (T.lanes[(size_t)t * 64 + (size_t)l].info & VT_START) != 0;
        worst = std::max(worst, rows);
      }
      CHECK(ls.end == ls.begin || gl > 0);
      if (gl) worst = std::max(worst, (ls.end - ls.begin + 16 * gl - 1) / (16 * gl) * 16);
    }
    // the bound, and the finest shift that keeps it (never finer than 21)
    const int shift = T.shift[(size_t)s];
    CHECK(shift <= 21 && shift >= 0 && (1LL << (30 - shift)) >= worst);
    CHECK(shift == 21 || (1LL << (30 - shift - 1)) < worst);
  }
  d_vt.vec(T.lanes);
  d_vt.vec(T.tile_rows);
  d_vt.vec(T.long_rows);
  d_vt.vec(T.vt_off);
  d_vt.vec(T.segs);
  d_vt.vec(T.grid);
  d_vt.vec(T.gxt);
  d_vt.vec(T.shift);
  return T;
}
static void test_vt(const Data& d) {
  std::vector<unsigned short> ccol((size_t)d.ctp.back());   // the cold stream's ranks, exactly ctp[n_rows] of them
  for (size_t i = 0; i < ccol.size(); ++i) ccol[i] = (unsigned short)(i * 2654435761u >> 17);
  const long long n = d.n();
  long long r64 = -1, r65 = -1, r504 = -1;
  for (long long i = 0; i < n; ++i) {
    if (d.cold[(size_t)i] == 64) r64 = i;
    if (d.cold[(size_t)i] == 65) r65 = i;
    if (d.hot[(size_t)i] == 504) r504 = i;
  }
  CHECK(r64 >= 0 && r65 >= 0 && r504 >= 0);
  // two steps of two workers: a repeated row, the rows of 64 and of 65 cold entries, long rows, an empty list, and a list of
  // forty 63-lane rows (forty tiles: more than one 16-tile group, more than one workgroup)
  std::vector<int> idx;
  VLL off = {0};
  for (int i = 0; i < 30; ++i) idx.push_back((int)((i * 37) % n));
  for (int r : {5, 5, (int)r64, (int)r65, 5, 0, (int)n - 1, (int)r64}) idx.push_back(r);
  off.push_back((long long)idx.size());
  off.push_back((long long)idx.size());   // (an empty list)
  for (int i = 0; i < 40; ++i) idx.push_back((int)r504);
  off.push_back((long long)idx.size());
  for (long long r : d.long_rows) idx.push_back((int)r);   // nothing but long rows
  for (int i = 0; i < 40; ++i) idx.push_back((int)d.long_rows[0]);
  off.push_back((long long)idx.size());
  check_vt(d, ccol, idx, off, 2, 2, 8, 1);
  check_vt(d, ccol, idx, off, 2, 2, 256, 2);
  check_vt(d, ccol, idx, off, 1, 4, 64, 1);
  check_vt(d, ccol, idx, off, 4, 1, 2, 1);
  // Shifts below 21: one workgroup meets more than 512 rows.  A row of one lane, one of three lanes (21 to a tile) and a
  // long row, each repeated.
  long long r1 = -1, r3 = -1;
  for (long long i = 0; i < n; ++i) {
    if (is_long(d.hot[(size_t)i], d.cold[(size_t)i])) continue;
    if (d.hot[(size_t)i] >= 1 && d.hot[(size_t)i] <= 8 && d.cold[(size_t)i] <= 1) r1 = i;
    if (d.hot[(size_t)i] >= 17 && d.hot[(size_t)i] <= 24 && d.cold[(size_t)i] <= 3) r3 = i;
  }
  CHECK(r1 >= 0 && r3 >= 0);
  const int rl = (int)d.long_rows[0];
  {   // 1,100 one-lane rows in one workgroup (18 tiles, gx = 1): 2^11 rows, shift 19
    const VtTables T = check_vt(d, ccol, std::vector<int>(1100, (int)r1), {0, 1100}, 1, 1, 1, 1);
    CHECK(T.gxt[0] == 1 && T.grid[0] == 1 && T.shift[0] == 19);
  }
  {   // 66 tiles of 21 rows over three workgroups: the 16-tile groups 0 and 3 meet in one, 32 tiles = 672 rows, shift 20
    const VtTables T = check_vt(d, ccol, std::vector<int>(66 * 21, (int)r3), {0, 66 * 21}, 1, 1, 3, 1);
    CHECK(T.gxt[0] == 3 && T.grid[0] == 3 && T.shift[0] == 20);
  }
  {   // 600 long rows in one long-row workgroup, sixteen at a time: 608 rows, shift 20; with two workers, the longer list counts
    const VtTables T = check_vt(d, ccol, std::vector<int>(600, rl), {0, 600}, 1, 1, 4, 1);
    CHECK(T.gxt[0] == 1 && T.grid[0] == 2 && T.shift[0] == 20);
    std::vector<int> two(1700, rl);
    std::fill(two.begin(), two.begin() + 600, (int)r1);
    const VtTables U = check_vt(d, ccol, two, {0, 600, 1700}, 1, 2, 2, 1);   // 600 tiled rows | 1,100 long rows
    CHECK(U.gxt[0] == 1 && U.grid[0] == 2 && U.shift[0] == 19);
    const VtTables V = check_vt(d, ccol, two, {0, 600, 1700}, 2, 1, 64, 1);  // the same lists as two steps: 600 rows in one workgroup; the long rows over eight
    CHECK(V.shift[0] == 20 && V.shift[1] == 21);
  }
  // A tile filled to exactly 64 lanes stays one tile: 63 lanes + 1, the 64-cold-entry row first in its list, 64 one-lane rows
  {
    std::vector<int> fill = {(int)r504, (int)r1, (int)r64, (int)r1, (int)r1, (int)r64};
    fill.insert(fill.end(), 64, (int)r1);
    const VtTables T = check_vt(d, ccol, fill, {0, 2, 6, 70}, 1, 3, 12, 1);
    CHECK(T.vt_off == VLL({0, 1, 4, 5}) && T.tile_rows == std::vector<int>({2, 1, 2, 1, 64}));
  }
  // lists of exactly 16 and 32 tiles: one and two workgroups at one tile per wave, one at two
  for (int tiles : {16, 32}) {
    const VtTables T = check_vt(d, ccol, std::vector<int>((size_t)tiles, (int)r504), {0, tiles}, 1, 1, 8, 1);
    CHECK(T.gxt[0] == tiles / 16);
    const VtTables U = check_vt(d, ccol, std::vector<int>((size_t)tiles, (int)r504), {0, tiles}, 1, 1, 8, 2);
    CHECK(U.gxt[0] == 1);
  }
  // an index at n_rows: not possible (and nothing read behind the offsets)
  std::vector<int> bad = {1, 2, (int)n};
  const VtStreams m{n, d.hrp.data(), d.ctp.data(), d.crp.data(), d.rp.data(), d.y.data(), ccol.data()};
  VtTables T;
  CHECK(!vt_tables(bad.data(), VLL{0, 3}.data(), 1, 1, 8, 1, m, T));
  bad[2] = -1;
  CHECK(!vt_tables(bad.data(), VLL{0, 3}.data(), 1, 1, 8, 1, m, T));
}

// ---- shifts --------------------------------------------------------------------------------------------------------------
static void test_shifts() {
  CHECK(rows_bits(0) == 0 && rows_bits(1) == 0 && rows_bits(2) == 1 && rows_bits(3) == 2);
  for (int k = 2; k <= 40; ++k) {
    CHECK(rows_bits(1LL << k) == k && rows_bits((1LL << k) + 1) == k + 1 && rows_bits((1LL << k) - 1) == k);
    d_shift.num(rows_bits((1LL << k) + 1));
  }
  for (long long worst : {1LL, 1000LL, 804414LL, 1LL << 20}) {
    const long long room = (1LL << 30) - worst;
    for (int shift0 : {1, 9, 20}) {
      CHECK(refine_shift(shift0, 21, 0u, worst) == 21);        // nothing measured: as fine as allowed
      CHECK(refine_shift(shift0, shift0, 0u, worst) == shift0);
      const unsigned int edge = (unsigned int)(room / 2);      // the largest sum that still admits one more step
      CHECK(refine_shift(shift0, 21, edge, worst) == shift0 + 1);
      CHECK(refine_shift(shift0, 21, edge + 1u, worst) == shift0);
      CHECK(refine_shift(shift0, 21, (unsigned int)(room / 4), worst) == std::min(21, shift0 + 2));
      for (unsigned int amax : {0u, 1u, 4096u, edge / 1024u, edge, edge + 1u, 0xffffffffu}) d_shift.num(refine_shift(shift0, 21, amax, worst));
    }
  }
  // the cold words' scale: the finest s <= 21 with 2^28 + 2^s + 32 (2^(s - 21) A + 256) < 2^30
  auto fits = [](int s, unsigned int a) { return 268435456.0 + std::ldexp(1.0, s) + 32.0 * (std::ldexp((double)a, s - 21) + 256.0) < 1073741824.0; };
  CHECK(cold_shift_for(0u) == 21 && cold_shift_for(1000u) == 21);
  for (unsigned int a : {0u, 1u, 1000u, 1u << 24, 25000000u, 25100000u, 25200000u, 1u << 25, 1u << 28, 0xffffffffu}) {
    const int s = cold_shift_for(a);
    CHECK(s >= 1 && s <= 21 && (fits(s, a) || s == 1) && (s == 21 || !fits(s + 1, a)));
    d_cold_shift.num(s);
  }
}

// recorded from the functions inside csrc/dsgd_hip.hip at commit e936d6a (see the top of this file)
static const struct {
  const char* name;
  const Fnv* got;
  uint64_t want;
} DIGESTS[] = {
    {"tiles", &d_tiles, 0x9bfe77b62b4d6fa9ULL},
    {"split", &d_split, 0x70f3cc75b66cba4aULL},
    {"cold_shift", &d_cold_shift, 0x25ccb02d0b51565fULL},
    {"locate", &d_locate, 0xbc16101d56ff3158ULL},
    {"stream", &d_stream, 0xff486a5f9c1d37caULL},
    {"chunks", &d_chunks, 0x33f88dd8c14f2935ULL},
    {"vt", &d_vt, 0x84e9ea3276f67413ULL},
    {"shift", &d_shift, 0x588c1be11d1d4621ULL},
};

int main(int argc, char** argv) {
  test_tiles();
  test_shifts();
  Data sets[] = {mixed(), one_slot(300), long_run(), no_cold()};
  for (Data& d : sets) {
    split(d);
    test_locate(d);
    test_chunks(d);
  }
  {   // 300 rows of one cold slot in one chunk: three tiles of <= 128 rows are refitted to sixteen of <= 19
    ChunkTables T;
    check_chunks(sets[1], {{0, 300}}, 1, {}, false, &T);
    CHECK(T.chunks[0].ctile_end - T.chunks[0].ctile_begin == 16 && T.chunks[0].tile_end - T.chunks[0].tile_begin == 2);
  }
  test_vt(sets[0]);
  const bool print = argc > 1 && std::string(argv[1]) == "--print";
  for (const auto& d : DIGESTS) {
    if (print) std::printf("%s 0x%016llxULL\n", d.name, (unsigned long long)d.got->h);
    else if (d.got->h != d.want) {
      std::fprintf(stderr, "digest %s: 0x%016llx, recorded 0x%016llx\n", d.name, (unsigned long long)d.got->h, (unsigned long long)d.want);
      return 1;
    }
  }
  std::fprintf(stderr, "all checks passed (%d)\n", g_checks);
  return 0;
}
