// The witness of the packed form's edge matrices (tests/packed_edge_data.py): which tile shapes do the project's own builders
// cut from them?  Built with AddressSanitizer and UBSan and run by tests/test_packed_edges.py, one matrix file per run.
//
// The program reads a matrix and its (DSGD_FSTEP_ROWS, row ranges) configurations, splits the rows by the hot set the file
// names (split_offsets), sizes the launch as the library does (fstep_grid, csrc/dsgd_route.hpp), cuts the chunks
// (cut_row_chunks) and flags the hot stream (packed_streams_ref).  For every hot tile of every configuration
//   (a) packed_lane_bits -- the host's copy of the lines in w_tile_q<..., true> -- equals the low byte of the lane descriptors,
//       and a PADDING tile (what a wave holds when its chunk has fewer tiles than waves: the chunk's last record, rows = -1)
//       gives no bits at all;
//   (b) the tile is counted into the edge classes below, printed per configuration and as totals ("TOTAL name count");
//   (c) deliberately wrong readers are run beside the right one and counted where they differ from the descriptors
//       ("MUTANT name tiles"): a matrix on which a mutant never differs does not reach that edge.
// Rules of the builders that decide what can be reached are printed as "RULE ..." lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "dsgd_layout_host.hpp"
#include "dsgd_route.hpp"

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                           \
    }                                                                     \
  } while (0)

// ---- the readers -------------------------------------------------------------------------------------------------------
enum Reader { RIGHT, NO_EXTRA_DROP, MASK_EM_MINUS_1, MASK_ONE_SLOT_WIDE, NO_MASK, KEEP_255_ON_PADDING, N_READERS };
static const char* const READER_NAME[N_READERS] = {"right", "no_extra_drop", "mask_em_minus_1", "mask_one_slot_wide", "no_mask",
                                                   "keep_255_on_padding"};
// packed_lane_bits with one line changed (csrc/dsgd_layout_host.hpp; the right reader is checked against it below)
static void read_bits(Reader how, const WTile& T, const unsigned short* colf, long long n_words, unsigned int (&bits)[64]) {
  const int nrows = (int)(short)(T.info & 0xffff);
  const int n = (int)((unsigned int)T.info >> 16);
  const int window = (n + 7) & ~7;
  int total = 0;
  for (int l = 0; l < 64; ++l) {
    unsigned int b = 0;
    for (int k = 0; k < 8; ++k) {
      const int slot = 8 * l + k;
      const long long e = T.pos0 + slot;
      if (slot < window && e >= 0 && e < n_words && (colf[e] & 0x8000u)) b |= 1u << k;
    }
    if (nrows < 0 && how != KEEP_255_ON_PADDING) b = 0;
    const unsigned int em = nrows < 0 ? 0u : 1u << (n & 7);
    if (l == (n >> 3)) {
      unsigned int mask = em - 1u + em;
      if (how == MASK_EM_MINUS_1) mask = em - 1u;
      if (how == MASK_ONE_SLOT_WIDE) mask = 4u * em - 1u;
      if (how == NO_MASK) mask = ~0u;
      b = (b & mask) | em;
    }
    bits[l] = b;
    for (unsigned int x = b; x; x &= x - 1u) ++total;
  }
  if (how != NO_EXTRA_DROP)
    for (int extra = total - nrows - 1; extra > 0; --extra) bits[0] &= bits[0] - 1u;
}

// ---- the matrix file ---------------------------------------------------------------------------------------------------
struct Cfg {
  long long fstep_rows;
  std::vector<StreamSeg> segs;
};
struct Case {
  long long n_rows = 0, nnz = 0, dp = 0, hot_n = 0;
  std::vector<long long> rp;
  std::vector<int> col;
  std::vector<signed char> label;
  std::vector<unsigned char> hot;
  std::vector<Cfg> cfgs;
};
template <class T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
static bool read_case(const char* path, Case& c) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::vector<long long> h;
  bool ok = read_vec(f, h, 5) && h[0] > 0 && h[0] <= 8192 && h[1] >= 0 && h[1] < (1LL << 24) && h[2] > 0 && h[2] < 65536 && h[4] >= 0 && h[4] < 64;
  if (ok) {
    c.n_rows = h[0], c.nnz = h[1], c.dp = h[2], c.hot_n = h[3];
    ok = read_vec(f, c.rp, (size_t)c.n_rows + 1) && read_vec(f, c.col, (size_t)c.nnz) && read_vec(f, c.label, (size_t)c.n_rows) &&
         read_vec(f, c.hot, (size_t)c.dp);
    for (long long k = 0; ok && k < h[4]; ++k) {
      std::vector<long long> a, r;
      ok = read_vec(f, a, 2) && a[1] > 0 && a[1] <= 64 && read_vec(f, r, (size_t)(2 * a[1]));
      if (!ok) break;
      Cfg g;
      g.fstep_rows = a[0];
      for (long long j = 0; j < a[1]; ++j) {
        StreamSeg s{};
        s.row_begin = r[(size_t)(2 * j)];
        s.row_end = r[(size_t)(2 * j + 1)];
        ok = ok && 0 <= s.row_begin && s.row_begin < s.row_end && s.row_end <= c.n_rows;
        g.segs.push_back(s);
      }
      c.cfgs.push_back(g);
    }
  }
  std::fclose(f);
  if (ok) {
    ok = c.rp[0] == 0 && c.rp[(size_t)c.n_rows] == c.nnz;
    for (long long i = 0; ok && i < c.n_rows; ++i) ok = c.rp[(size_t)i] <= c.rp[(size_t)i + 1];
    for (long long e = 0; ok && e < c.nnz; ++e) ok = c.col[(size_t)e] >= 0 && c.col[(size_t)e] < c.dp;
  }
  return ok;
}

// ---- counting ----------------------------------------------------------------------------------------------------------
typedef std::map<std::string, long long> Counts;
static const char* const CLASSES[] = {
    "tiles", "end_mark_on_8_below_cap", "largest_tile_511", "extra_1", "extra_2", "extra_3", "extra_4", "extra_5", "extra_6", "extra_7",
    "tiny_tile_with_extra", "rows_over_64", "rows_at_cap_254", "last_tile_stream_mult8", "last_tile_stream_not_mult8",
    "chunk_under_16_tiles", "chunk_without_tiles", "first_chunk_without_tiles", "row_start_in_slot_7", "row_over_8_lanes",
    "general_path_tiles", "flag_right_behind_end_mark", "padding_tiles_checked"};

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: packed_edges_test <matrix file>\n");
    return 2;
  }
  Case c;
  if (!read_case(argv[1], c)) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  // the split by the file's hot set
  std::vector<int> cold_cnt((size_t)c.n_rows, 0);
  for (long long i = 0; i < c.n_rows; ++i)
    for (long long e = c.rp[(size_t)i]; e < c.rp[(size_t)i + 1]; ++e) cold_cnt[(size_t)i] += c.hot[(size_t)c.col[(size_t)e]] ? 0 : 1;
  std::vector<long long> hrp, ctp, crp, long_rows, long_weight;
  split_offsets(c.rp, cold_cnt, true, hrp, ctp, crp, long_rows, long_weight);
  const size_t nh = (size_t)hrp[(size_t)c.n_rows];
  // the flagged rank words: exactly the stream's slots (a read behind them is an error here)
  std::vector<unsigned short> hcol(nh), hcolf(nh, (unsigned short)0xdead);
  std::vector<float> hval(nh, 1.0f), hvaly(nh);
  for (size_t e = 0; e < nh; ++e) hcol[e] = (unsigned short)((e * 2654435761u) % (unsigned int)c.hot_n);
  packed_streams_ref(hrp.data(), c.n_rows, c.label.data(), hcol.data(), hval.data(), hcolf.data(), hvaly.data());

  std::printf("RULE largest tile: append_wave_tiles closes a tile when row_ptr[i + 1] - pos0 > WS_SLOTS - 1 = %d -- a tile holds at most %d "
              "slots, the end mark of the largest sits in lane 63, bit 7 (n >> 3 always names a lane)\n", WS_SLOTS - 1, WS_SLOTS - 1);
  std::printf("RULE rows without hot entries: split_offsets gives every tiled row max(hot, 1) slots -- an empty row and a row with cold "
              "entries only own one explicit-zero slot and one tile row\n");
  // the rows themselves (what no cut changes)
  Counts rows_seen;
  auto is_long = [&](long long i) { return hrp[(size_t)i + 1] == hrp[(size_t)i]; };
  auto hot_of = [&](long long i) { return (c.rp[(size_t)i + 1] - c.rp[(size_t)i]) - cold_cnt[(size_t)i]; };
  for (long long i = 1; i + 1 < c.n_rows; ++i) {
    const bool between = !is_long(i - 1) && !is_long(i + 1) && hot_of(i - 1) > 0 && hot_of(i + 1) > 0;
    if (is_long(i) && !is_long(i + 1)) ++rows_seen["long_row_before_a_tiled_row"];
    if (is_long(i) && !is_long(i - 1)) ++rows_seen["long_row_after_a_tiled_row"];
    if (c.rp[(size_t)i + 1] == c.rp[(size_t)i] && between) ++rows_seen["empty_row_between_hot_rows"];
    if (!is_long(i) && hot_of(i) == 0 && cold_cnt[(size_t)i] > 0 && between) ++rows_seen["cold_only_row_between_hot_rows"];
  }

  Counts total;
  long long mutant[N_READERS] = {0};
  int max_slots = 0;
  for (const Cfg& g : c.cfgs) {
    Knobs k;
    k.fstep_min = 1;
    k.fstep_rows = g.fstep_rows;
    RouteFacts f;
    f.dp = (int)c.dp;
    f.n_rows = c.n_rows;
    f.n_cu = 256;
    f.hsplit = (int)c.hot_n;
    f.cold_col16 = true;
    f.coldm_nnz = ctp[(size_t)c.n_rows];
    long long tot = 0, smallest = c.n_rows;
    for (const StreamSeg& s : g.segs) {
      tot += s.row_end - s.row_begin;
      smallest = std::min(smallest, s.row_end - s.row_begin);
    }
    const int n_wg = fstep_grid(k, f, (int)g.segs.size(), tot, 0, smallest);
    CHECK(n_wg > 0);
    if (n_wg <= 0) continue;
    ChunkTables T;
    cut_row_chunks(g.segs, n_wg, std::vector<double>(), hrp, ctp, long_rows, long_weight, c.label.data(), T);
    Counts seen;
    for (size_t ci = 0; ci < T.chunks.size(); ++ci) {
      const FChunk& ch = T.chunks[ci];
      const int nt = ch.tile_end - ch.tile_begin;
      if (nt > 0 && nt < 16) ++seen["chunk_under_16_tiles"];
      if (nt == 0) ++seen["chunk_without_tiles"];
      if (nt == 0 && ci == 0) ++seen["first_chunk_without_tiles"];
      if (nt > 0 && nt < 16) {   // the waves from nt on hold the chunk's last record as a padding tile
        WTile P = T.wt[(size_t)ch.tile_end - 1];
        P.info |= 0xffff;
        unsigned int bits[64], wrong[64];
        packed_lane_bits(P, hcolf.data(), (long long)hcolf.size(), bits);
        read_bits(KEEP_255_ON_PADDING, P, hcolf.data(), (long long)hcolf.size(), wrong);
        bool differs = false;
        for (int l = 0; l < 64; ++l) {
          CHECK(bits[l] == 0u);
          differs = differs || wrong[l] != 0u;
        }
        ++seen["padding_tiles_checked"];
        mutant[KEEP_255_ON_PADDING] += differs;
      }
    }
    for (size_t t = 0; t < T.wt.size(); ++t) {
      const WTile& W = T.wt[t];
      const int nrows = (int)(short)(W.info & 0xffff);
      const int n = (int)((unsigned int)W.info >> 16);
      if (nrows < 0) continue;   // (the stand-in of an empty table)
      unsigned int bits[64], got[64];
      packed_lane_bits(W, hcolf.data(), (long long)hcolf.size(), bits);
      bool general = false;
      for (int l = 0; l < 64; ++l) {
        const unsigned int want = T.meta[t * 64 + (size_t)l] & 255u;
        if (bits[l] != want)
          std::fprintf(stderr, "tile %zu (r0 %d, rows %d, slots %d, pos0 %lld) lane %d: %02x, descriptor %02x\n", t, W.r0, nrows, n, W.pos0, l,
                       bits[l], want);
        CHECK(bits[l] == want);
        general = general || (want & (want - 1u));
      }
      for (int r = 0; r < N_READERS; ++r) {
        if (r == KEEP_255_ON_PADDING) continue;
        read_bits((Reader)r, W, hcolf.data(), (long long)hcolf.size(), got);
        bool differs = false;
        for (int l = 0; l < 64; ++l) differs = differs || got[l] != (T.meta[t * 64 + (size_t)l] & 255u);
        if (r == RIGHT) CHECK(!differs);   // (the local copy is packed_lane_bits)
        mutant[r] += differs;
      }
      // ---- the classes
      ++seen["tiles"];
      max_slots = std::max(max_slots, n);
      const long long first = hrp[(size_t)W.r0] - W.pos0;
      int extra = 0;
      for (long long e = W.pos0; e < W.pos0 + first; ++e) extra += (hcolf[(size_t)e] & 0x8000u) ? 1 : 0;
      CHECK(first >= 0 && first < 8 && extra <= 7);
      if (n % 8 == 0 && n < WS_SLOTS - 1) ++seen["end_mark_on_8_below_cap"];
      if (n == WS_SLOTS - 1) ++seen["largest_tile_511"];
      if (extra > 0) ++seen["extra_" + std::to_string(extra)];
      if (n < 8 && extra > 0) ++seen["tiny_tile_with_extra"];
      if (nrows > 64) ++seen["rows_over_64"];
      if (nrows == WS_MAXROWS) ++seen["rows_at_cap_254"];
      if (W.pos0 + n == (long long)nh) ++seen[nh % 8 == 0 ? "last_tile_stream_mult8" : "last_tile_stream_not_mult8"];
      if (general) ++seen["general_path_tiles"];
      if ((n & 7) < 7 && W.pos0 + n + 1 < (long long)nh && (hcolf[(size_t)(W.pos0 + n + 1)] & 0x8000u)) ++seen["flag_right_behind_end_mark"];
      bool slot7 = false, wide = false;
      for (int r = 0; r < nrows; ++r) {
        const long long a = hrp[(size_t)W.r0 + (size_t)r] - W.pos0, b = hrp[(size_t)W.r0 + (size_t)r + 1] - W.pos0;
        if (b == a) continue;   // (a row of the long list inside the tile's row span owns no slot -- and closes the tile: never here)
        slot7 = slot7 || (a & 7) == 7;
        wide = wide || ((b - 1) >> 3) - (a >> 3) + 1 > 8;
      }
      if (slot7) ++seen["row_start_in_slot_7"];
      if (wide) ++seen["row_over_8_lanes"];
    }
    std::printf("CONFIG fstep_rows %lld, %zu range(s), %d workgroup(s) per worker:", g.fstep_rows, g.segs.size(), n_wg);
    for (const char* name : CLASSES) {
      std::printf(" %s %lld", name, seen[name]);
      total[name] += seen[name];
    }
    std::printf("\n");
  }
  // the end-mark mask em - 1 in place of em - 1 + em is NO mutant: the reader sets bit em itself right after the mask, so the two
  // give the same byte for every flag byte and every end slot -- shown here for all of them, and counted above all the same
  for (unsigned int b = 0; b < 256; ++b)
    for (unsigned int s = 0; s < 8; ++s) {
      const unsigned int em = 1u << s;
      CHECK(((b & (em - 1u + em)) | em) == ((b & (em - 1u)) | em));
    }
  std::printf("RULE end-mark mask: (b & (em - 1)) | em == (b & (em - 1 + em)) | em for all 256 flag bytes and 8 end slots (checked): "
              "mask_em_minus_1 is the same reader; the masks that ARE wrong -- one slot wide, none -- are counted beside it\n");
  for (const char* name : CLASSES) std::printf("TOTAL %s %lld\n", name, total[name]);
  for (const char* name : {"long_row_before_a_tiled_row", "long_row_after_a_tiled_row", "empty_row_between_hot_rows", "cold_only_row_between_hot_rows"})
    std::printf("TOTAL %s %lld\n", name, rows_seen[name]);
  std::printf("TOTAL max_slots %d\n", max_slots);
  std::printf("TOTAL hot_nnz_mod_8 %d\n", (int)(nh % 8));
  for (int r = 0; r < N_READERS; ++r) std::printf("MUTANT %s %lld\n", READER_NAME[r], mutant[r]);
  CHECK(mutant[RIGHT] == 0);
  CHECK(mutant[MASK_EM_MINUS_1] == 0);
  CHECK(max_slots <= WS_SLOTS - 1);
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
