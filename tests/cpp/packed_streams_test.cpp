// The packed copies of the split streams (csrc/dsgd_layout_host.hpp: packed_streams_ref, packed_lane_bits) against the lane
// descriptors the existing builders write.  Built with AddressSanitizer and UBSan and run by tests/test_packed_streams.py.
//
// For every tile of build_wave_tiles and of cut_row_chunks' chunked tile table:
//   (a) the start bits rebuilt from the flagged rank words -- window rounded up to 8 slots, the end mark set by the reader, the
//       flags of earlier rows in front of the tile's first row dropped -- equal the low byte of wave_tile_meta's descriptor,
//       lane by lane;
//   (b) the sign of every folded value is label x the value's sign, its magnitude the value's; the rank under the flag is the
//       rank; a flag sits on the first slot of every row and nowhere else.
// The flagged words are held in a vector of exactly the stream's slots: a read behind them is an error here (the device
// buffers carry padding, the reference reader must not need it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dsgd_layout_host.hpp"

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                           \
    }                                                                     \
  } while (0)

struct Row {
  int hot, cold;   // entries below / from the split rank on (hot > WS_MAXNNZ or cold > WS_MAXNNZ: a long row)
};

struct Seen {   // what a case exercised, so that the driver can insist that every edge was met somewhere
  bool slots_mult8 = false, lead = false, lead_flags = false, over64 = false, cap254 = false, end_of_stream_mult8 = false;
  bool gap_between = false, gap_at_end = false, general = false, last_word_flag_dropped = false;
};

static unsigned int bits_of(float f) {
  unsigned int u;
  std::memcpy(&u, &f, 4);
  return u;
}

static void check_tiles(const std::vector<WTile>& wt, const std::vector<unsigned short>& meta, const std::vector<long long>& hrp,
                        const std::vector<unsigned short>& colf, Seen& seen) {
  for (size_t t = 0; t < wt.size(); ++t) {
    const WTile& T = wt[t];
    const int nrows = (int)(short)(T.info & 0xffff);
    const int n = (int)((unsigned int)T.info >> 16);
    unsigned int bits[64];
    packed_lane_bits(T, colf.data(), (long long)colf.size(), bits);
    int flagged_lanes_over1 = 0;
    for (int l = 0; l < 64; ++l) {
      const unsigned int want = nrows < 0 ? 0u : (meta[t * 64 + (size_t)l] & 255u);
      if (bits[l] != want)
        std::fprintf(stderr, "tile %zu (r0 %d, rows %d, slots %d, pos0 %lld) lane %d: %02x, descriptor %02x\n", t, T.r0, nrows, n,
                     T.pos0, l, bits[l], want);
      CHECK(bits[l] == want);
      if (bits[l] & (bits[l] - 1u)) ++flagged_lanes_over1;
    }
    if (nrows < 0) continue;
    const long long first = hrp[(size_t)T.r0] - T.pos0;
    if (n % 8 == 0) seen.slots_mult8 = true;
    if (n % 8 == 0 && T.pos0 + n == (long long)colf.size()) seen.end_of_stream_mult8 = true;
    if (first > 0) seen.lead = true;
    for (long long e = T.pos0; e < T.pos0 + first; ++e)
      if (colf[(size_t)e] & 0x8000u) seen.lead_flags = true;
    if (nrows > 64) seen.over64 = true;
    if (nrows == WS_MAXROWS) seen.cap254 = true;
    if (flagged_lanes_over1) seen.general = true;
    // a flag behind the end mark inside the rounded window (the row after the next one's first slot)
    for (long long e = T.pos0 + n + 1; e < T.pos0 + ((n + 7) & ~7) && e < (long long)colf.size(); ++e)
      if (colf[(size_t)e] & 0x8000u) seen.last_word_flag_dropped = true;
  }
}

static void run_case(const char* name, const std::vector<Row>& rows, int label_mode, Seen& seen) {
  const long long n_rows = (long long)rows.size();
  std::vector<long long> rp((size_t)n_rows + 1, 0);
  std::vector<int> cold_cnt((size_t)n_rows);
  std::vector<signed char> label((size_t)n_rows);
  for (long long i = 0; i < n_rows; ++i) {
    rp[(size_t)i + 1] = rp[(size_t)i] + rows[(size_t)i].hot + rows[(size_t)i].cold;
    cold_cnt[(size_t)i] = rows[(size_t)i].cold;
    label[(size_t)i] = (signed char)(label_mode < 0 ? -1 : (label_mode > 0 ? 1 : ((i * 7 + i / 3) % 3 == 0 ? -1 : 1)));
  }
  std::vector<long long> hrp, ctp, crp, long_rows, long_weight;
  split_offsets(rp, cold_cnt, true, hrp, ctp, crp, long_rows, long_weight);
  for (size_t k = 0; k < long_rows.size(); ++k) {
    const long long i = long_rows[k];
    if (i + 1 < n_rows) seen.gap_between = true;
    if (i + 1 == n_rows) seen.gap_at_end = true;
  }
  // the streams: ranks below 2^15 (the largest on purpose), values of both signs, zeros of both signs
  const size_t nh = (size_t)hrp[(size_t)n_rows], nc = (size_t)ctp[(size_t)n_rows];
  std::vector<unsigned short> hcol(nh), hcolf(nh, (unsigned short)0xdead);
  std::vector<float> hval(nh), hvaly(nh, 123.0f), cval(nc), cvaly(nc, 123.0f);
  for (size_t e = 0; e < nh; ++e) {
    hcol[e] = (unsigned short)(e % 5 == 0 ? 32767 : (e * 2654435761u) % 32768u);
    hval[e] = e % 11 == 0 ? 0.0f : (e % 13 == 0 ? -0.0f : ((e % 2) ? 1.0f : -1.0f) * (0.125f + (float)(e % 97)));
  }
  for (size_t e = 0; e < nc; ++e) cval[e] = e % 7 == 0 ? -0.0f : ((e % 3) ? -1.0f : 1.0f) * (0.5f + (float)(e % 31));
  packed_streams_ref(hrp.data(), n_rows, label.data(), hcol.data(), hval.data(), hcolf.data(), hvaly.data());
  packed_streams_ref(ctp.data(), n_rows, label.data(), nullptr, cval.data(), nullptr, cvaly.data());
  // (b) slot by slot
  {
    std::vector<int> owner(nh, -1), cowner(nc, -1);
    for (long long i = 0; i < n_rows; ++i) {
      for (long long e = hrp[(size_t)i]; e < hrp[(size_t)i + 1]; ++e) owner[(size_t)e] = (int)i;
      for (long long e = ctp[(size_t)i]; e < ctp[(size_t)i + 1]; ++e) cowner[(size_t)e] = (int)i;
    }
    for (size_t e = 0; e < nh; ++e) {
      CHECK(owner[e] >= 0);
      const int i = owner[e];
      CHECK((hcolf[e] & 0x7fffu) == hcol[e]);
      CHECK(((hcolf[e] & 0x8000u) != 0) == ((long long)e == hrp[(size_t)i]));
      const bool neg = std::signbit(hval[e]) != (label[(size_t)i] < 0);
      CHECK(std::signbit(hvaly[e]) == neg);
      CHECK((bits_of(hvaly[e]) & 0x7fffffffu) == (bits_of(hval[e]) & 0x7fffffffu));
    }
    for (size_t e = 0; e < nc; ++e) {
      CHECK(cowner[e] >= 0);
      const int i = cowner[e];
      CHECK(std::signbit(cvaly[e]) == (std::signbit(cval[e]) != (label[(size_t)i] < 0)));
      CHECK((bits_of(cvaly[e]) & 0x7fffffffu) == (bits_of(cval[e]) & 0x7fffffffu));
    }
  }
  // (a) the whole-stream tile table, at both row caps the builders use
  const int before = g_fail;
  for (int max_rows : {WS_MAXROWS, CT_MAXROWS}) {
    HostTiles ht;
    build_wave_tiles(hrp.data(), n_rows, label.data(), ht, max_rows);
    check_tiles(ht.wt, ht.meta16, hrp, hcolf, seen);
  }
  // ... and the chunked tables: one worker, three unequal ranges
  auto chunked = [&](const std::vector<StreamSeg>& segs, int n_wg) {
    ChunkTables T;
    cut_row_chunks(segs, n_wg, std::vector<double>(), hrp, ctp, long_rows, long_weight, label.data(), T);
    check_tiles(T.wt, T.meta, hrp, hcolf, seen);
  };
  auto seg = [](long long a, long long b) {
    StreamSeg s{};
    s.row_begin = a;
    s.row_end = b;
    return s;
  };
  chunked({seg(0, n_rows)}, 1);
  chunked({seg(0, n_rows)}, 3);
  if (n_rows >= 6) chunked({seg(0, n_rows / 6), seg(n_rows / 6, n_rows / 2 + 1), seg(n_rows / 2 + 1, n_rows)}, 2);
  if (n_rows >= 3) chunked({seg(1, n_rows - 1)}, 5);
  if (g_fail != before) std::fprintf(stderr, "case %s failed\n", name);
}

int main() {
  Seen seen;
  auto rep = [](std::vector<Row>& v, int n, Row r) {
    for (int i = 0; i < n; ++i) v.push_back(r);
  };
  const Row LONG_HOT{WS_MAXNNZ + 1, 2}, LONG_COLD{3, WS_MAXNNZ + 1};
  for (int label_mode : {0, -1, 1}) {
    {   // the row lengths of the issue, in both orders, with explicit-zero rows (hot = 0 -> one slot)
      std::vector<Row> v = {{1, 1}, {7, 0}, {8, 2}, {9, 1}, {503, 3}, {504, 1}, {504, 0}, {503, 1}, {9, 9}, {8, 0}, {7, 7}, {1, 0}, {0, 4}};
      run_case("lengths", v, label_mode, seen);
    }
    {   // slot counts that are multiples of 8, closed by a long row and by the end of the stream
      std::vector<Row> v = {{8, 1}, {8, 1}, {16, 1}, LONG_HOT, {24, 1}, {8, 0}, LONG_COLD, {504, 1}, {8, 1}, {8, 1}, {496, 1}, {16, 2}, {16, 2}};
      run_case("multiples of 8", v, label_mode, seen);
    }
    {   // windows that start in front of their first row, with the starts of short rows in those slots
      std::vector<Row> v = {{3, 1}, {504, 1}, {1, 1}, {1, 1}, {1, 1}, {504, 1}, {2, 0}, {2, 0}, {3, 0}, {500, 1}, {5, 1}, {504, 2}, {7, 1}, {504, 1}, {6, 1}, {1, 1}};
      run_case("leads", v, label_mode, seen);
    }
    {   // emptied / long rows between tiled rows, several in a row, first and last
      std::vector<Row> v = {LONG_HOT, {5, 1}, {9, 2}, LONG_COLD, LONG_HOT, {12, 0}, {3, 3}, LONG_HOT, {1, 1}, LONG_COLD};
      run_case("gaps", v, label_mode, seen);
      v.push_back({4, 4});
      run_case("gaps, tiled last", v, label_mode, seen);
    }
    {   // more than 64 rows in a tile; the 254-row cap (one-slot rows: the next tile's window opens on six of their starts)
      std::vector<Row> v;
      rep(v, 100, {2, 1});
      rep(v, 3, {40, 1});
      rep(v, 700, {1, 0});
      rep(v, 90, {3, 2});
      v.push_back(LONG_HOT);
      rep(v, 300, {0, 1});
      run_case("short rows", v, label_mode, seen);
    }
    {   // rows like the benchmark's (~70 hot slots), enough of them for several chunks
      std::vector<Row> v;
      for (int i = 0; i < 400; ++i) v.push_back({40 + (i * 37) % 61, 1 + i % 9});
      run_case("plain", v, label_mode, seen);
    }
  }
  CHECK(seen.slots_mult8);
  CHECK(seen.end_of_stream_mult8);
  CHECK(seen.lead);
  CHECK(seen.lead_flags);
  CHECK(seen.over64);
  CHECK(seen.cap254);
  CHECK(seen.gap_between);
  CHECK(seen.gap_at_end);
  CHECK(seen.general);
  CHECK(seen.last_word_flag_dropped);
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all checks passed\n");
  return 0;
}
