// The host's arithmetic behind every table the gradient kernels read: wave tiles and their lane descriptors, the slot
// offsets of the hot and cold streams, each worker's tile ranges, the row chunks, the virtual tiles of resident plans, and
// the fixed-point shift of a launch.  csrc/dsgd_hip.hip allocates, uploads and launches; what it uploads is computed here.
//
// Pure host arithmetic -- no device type, no library call but <vector>, <algorithm> and <cmath> -- so that the library and
// a host test compile the same lines (tests/test_layout_host.py runs them under AddressSanitizer and UBSan, decodes every
// table with a decoder of its own and holds the tables' bytes to recorded digests).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "dsgd_layout_types.hpp"

// ---- fixed-point shifts ----------------------------------------------------------------------------------------------
// the smallest bits with 2^bits >= rows: a workgroup that meets `rows` rows, one contribution of at most 2^shift per row
// and column, keeps its 32-bit sums below 2^30 at shift = 30 - bits (every caller clamps that in its own way)
inline int rows_bits(long long rows) {
  int bits = 0;
  while ((1LL << bits) < rows) ++bits;
  return bits;
}
// data-dependent refinement of a launch's shift: amax is the largest column sum measured at shift0 (the bound kernels);
// every further step doubles it, and it has to stay within 2^30 less one unit of rounding per row
inline int refine_shift(int shift0, int max_shift, unsigned int amax, long long worst_rows) {
  int s2 = shift0;
  const double room = (double)(1LL << 30) - (double)worst_rows;
  while (s2 < max_shift && std::ldexp((double)amax, s2 + 1 - shift0) <= room) ++s2;
  return s2;
}
// The cold words' scale.  A word is emptied by whoever sees it at 2^28; until then sixteen waves can each add the rest of
// a tile, at most 2 A at shift 21 (dsgd_cold_bound_kernel).  The finest s <= 21 with
// 2^28 + 2^s + 32 * (2^(s - 21) A + 256) < 2^30 keeps every word below the band the kernels refuse (+ 256: half a unit
// of rounding for each of a tile's 512 slots).  RCV1-like data has A of a few values: s = 21.
inline int cold_shift_for(unsigned int amax) {
  int s = FIX_SHIFT;
  while (s > 1 && (double)(1LL << 28) + std::ldexp(1.0, s) + 32.0 * (std::ldexp((double)amax, s - FIX_SHIFT) + 256.0) >= (double)(1LL << 30)) --s;
  return s;
}

// ---- wave tiles ------------------------------------------------------------------------------------------
// Tiles of WHOLE rows of the hot stream with <= WS_MAXNNZ non-zeros and <= WS_MAXROWS rows.  Lane l owns the 8
// contiguous slots [8l, 8l+8) of the 512-slot window at pos0 (a multiple of 8 slots: one 16-byte load of eight 16-bit
// column ranks per lane).  Lane descriptor (16 bits): row-start bits | label sign of the row ENDING at each start << 8
// (the kernel derives each lane's first row with a wave prefix sum over the start bits).  Rows of length 0 in
// `row_ptr` are skipped: the caller emptied them and put them on the long-row list.
struct HostTiles {
  std::vector<WTile> wt;
  std::vector<int> r0;              // first row of every tile + sentinel n_rows
  std::vector<unsigned short> meta16;   // n_tiles x 64
};
// wave tiles of WHOLE rows over the rows [rb, re) of a stream given by its slot offsets (a window of <= WS_SLOTS slots that
// starts at a multiple of 8; rows without a slot or longer than a tile close the open tile and stay out), appended to wt
inline void append_wave_tiles(const long long* row_ptr, long long rb, long long re, std::vector<WTile>& wt, int max_rows) {
  const long long amask = ~7LL;
  long long start = -1;  // first row of the open tile
  auto close = [&](long long end_row) {
    if (start < 0) return;
    WTile t;
    t.pos0 = row_ptr[start] & amask;
    t.r0 = (int)start;
    t.info = (int)(((end_row - start) & 0xffff) | ((row_ptr[end_row] - t.pos0) << 16));
    wt.push_back(t);
    start = -1;
  };
  for (long long i = rb; i < re; ++i) {
    const long long len = row_ptr[i + 1] - row_ptr[i];
    if (len > WS_MAXNNZ || len == 0) {
      close(i);
      continue;
    }
    if (start >= 0 && (row_ptr[i + 1] - (row_ptr[start] & amask) > WS_SLOTS - 1 || i - start >= max_rows)) close(i);
    if (start < 0) start = i;
  }
  close(re);
}
// the 64 lane descriptors of every tile: row-start bits of the lane's eight slots | label signs of the rows ending there << 8
inline void wave_tile_meta(const long long* row_ptr, const signed char* label, const std::vector<WTile>& wt,
                           std::vector<unsigned short>& meta16) {
  const long long n_tiles = (long long)wt.size();
  meta16.assign((size_t)std::max<long long>(n_tiles, 1) * 64, (unsigned short)0);
  for (long long t = 0; t < n_tiles; ++t) {
    const WTile& T = wt[(size_t)t];
    const int t_nrows = (int)(short)(T.info & 0xffff);
    int cur_row = 0, next = 0;
    for (int l = 0; l < 64; ++l) {  // lane l owns slots [8l, 8l+8)
      unsigned int bits = 0, ys = 0;
      for (int k = 0; k < 8; ++k) {
        const long long slot = 8LL * l + k;
        bool st = false;
        if (next < t_nrows && row_ptr[T.r0 + next] - T.pos0 == slot) st = true;
        else if (next == t_nrows && row_ptr[T.r0 + t_nrows] - T.pos0 == slot) st = true;  // end mark
        if (st) {
          bits |= 1u << k;
          // the row that ends here is local row cur_row (1-based); row 0 = leading padding
          if (cur_row >= 1 && label[T.r0 + cur_row - 1] > 0) ys |= 1u << k;
          ++cur_row;
          ++next;
        }
      }
      meta16[(size_t)t * 64 + l] = (unsigned short)(bits | (ys << 8));
    }
  }
}
inline WTile unused_wave_tile() {   // (a tile table is never empty: a clamped record read must stay inside it)
  WTile t;
  t.pos0 = 0;
  t.r0 = 0;
  t.info = 0xffff;   // -1 rows, 0 slots
  return t;
}
inline void build_wave_tiles(const long long* row_ptr, long long n_rows, const signed char* label, HostTiles& out,
                             int max_rows = WS_MAXROWS) {
  std::vector<WTile>& wt = out.wt;
  std::vector<int>& wr0 = out.r0;
  wt.clear();
  wr0.clear();
  append_wave_tiles(row_ptr, 0, n_rows, wt, max_rows);
  for (const WTile& t : wt) wr0.push_back(t.r0);
  wr0.push_back((int)n_rows);
  wave_tile_meta(row_ptr, label, wt, out.meta16);
  if (wt.empty()) wt.push_back(unused_wave_tile());
}

// ---- the split streams' offsets --------------------------------------------------------------------------------------
// hrp / ctp: slot offsets of the two streams (a tiled row owns at least one slot in each: an explicit zero when it
// has no entry there); crp: the cold ENTRIES before each row (what dsgd_range_nnz reports).  A row whose hot or cold part
// exceeds a wave tile goes on the long-row list and gets no slot in either stream.
// rp: n_rows + 1 row offsets of the ranked CSR; cold_cnt: n_rows cold entries per row.
inline void split_offsets(const std::vector<long long>& rp, const std::vector<int>& cold_cnt, bool has_cold,
                          std::vector<long long>& hrp, std::vector<long long>& ctp, std::vector<long long>& crp,
                          std::vector<long long>& long_rows, std::vector<long long>& long_weight) {
  const long long n_rows = (long long)cold_cnt.size();
  hrp.assign((size_t)n_rows + 1, 0);
  ctp.assign((size_t)n_rows + 1, 0);
  crp.assign((size_t)n_rows + 1, 0);
  long_rows.clear();
  for (long long i = 0; i < n_rows; ++i) {
    const long long len = rp[(size_t)i + 1] - rp[(size_t)i], cold = cold_cnt[(size_t)i], hot = len - cold;
    if (hot > WS_MAXNNZ || cold > WS_MAXNNZ) {   // served whole from the ranked CSR, one wave per row
      long_rows.push_back(i);
      hrp[(size_t)i + 1] = hrp[(size_t)i];
      ctp[(size_t)i + 1] = ctp[(size_t)i];
      crp[(size_t)i + 1] = crp[(size_t)i];
    } else {
      hrp[(size_t)i + 1] = hrp[(size_t)i] + std::max<long long>(hot, 1);
      ctp[(size_t)i + 1] = ctp[(size_t)i] + (has_cold ? std::max<long long>(cold, 1) : 0);
      crp[(size_t)i + 1] = crp[(size_t)i] + cold;
    }
  }
  // (what a long row weighs when row chunks are cut: its own non-zeros plus ~1,300 slots' worth of its wave's waiting --
  //  0.7 us per long row measured against 75 us for a chunk of ~200 K slots, profiles/r06_fstep_wg_times.txt)
  long_weight.assign(long_rows.size() + 1, 0);
  for (size_t k = 0; k < long_rows.size(); ++k) {
    const long long i = long_rows[k];
    long_weight[k + 1] = long_weight[k] + (rp[(size_t)i + 1] - rp[(size_t)i]) + 1300;
  }
}

// ---- nnz-streaming launches (contiguous row ranges) ----------------------------------------------------
// tile and long-row ranges of every worker's row range.  wr0 / cr0: the first row of every hot / cold wave tile + the
// sentinel n_rows (cr0 may be empty: no cold stream); long_rows: the sorted long-row list.
inline void locate_segs(const std::vector<int>& wr0, const std::vector<int>& cr0, const std::vector<long long>& long_rows,
                        std::vector<StreamSeg>& segs, long long* max_tiles, long long* max_long, long long* max_ctiles = nullptr) {
  *max_tiles = 1;
  *max_long = 0;
  if (max_ctiles) *max_ctiles = 0;
  for (StreamSeg& s : segs) {
    // first tile whose rows reach row_begin: the last tile with r0 <= row_begin (it may end before row_begin when a
    // long row sits in between -- then all its rows are masked) ... one past the last tile with r0 < row_end
    long long tb = (std::upper_bound(wr0.begin(), wr0.end() - 1, (int)s.row_begin) - wr0.begin()) - 1;
    if (tb < 0) tb = 0;
    long long te = std::lower_bound(wr0.begin(), wr0.end() - 1, (int)s.row_end) - wr0.begin();
    if (te < tb) te = tb;
    s.tile_begin = tb;
    s.tile_end = te;
    *max_tiles = std::max(*max_tiles, te - tb);
    // the rows that fit no tile: a range of the sorted long-row list, handled by the same kernel (one wave per row)
    s.long_begin = std::lower_bound(long_rows.begin(), long_rows.end(), s.row_begin) - long_rows.begin();
    s.long_end = std::lower_bound(long_rows.begin(), long_rows.end(), s.row_end) - long_rows.begin();
    *max_long = std::max(*max_long, s.long_end - s.long_begin);
    // the cold stream's tiles of the range, located the same way
    s.ctile_begin = s.ctile_end = 0;
    if (cr0.size() > 1) {
      long long cb = (std::upper_bound(cr0.begin(), cr0.end() - 1, (int)s.row_begin) - cr0.begin()) - 1;
      if (cb < 0) cb = 0;
      long long ce = std::lower_bound(cr0.begin(), cr0.end() - 1, (int)s.row_end) - cr0.begin();
      if (ce < cb) ce = cb;
      s.ctile_begin = cb;
      s.ctile_end = ce;
    }
    if (max_ctiles) *max_ctiles = std::max(*max_ctiles, s.ctile_end - s.ctile_begin);
  }
}
// The most rows ONE workgroup of the streaming launch can meet: workgroup b of a worker owns the 16-tile groups b,
// b + grid_x, ... of its tile range plus its share of the long rows.  (Rows between the first rows of two tiles bound the
// rows of a tile from above.)
inline long long stream_worst_rows(const std::vector<StreamSeg>& segs, const std::vector<int>& wr0, long long grid_x) {
  long long worst = 1;
  std::vector<long long> rows_of((size_t)grid_x);
  for (const StreamSeg& sg : segs) {
    std::fill(rows_of.begin(), rows_of.end(), 0);
    long long g = 0;
    for (long long t = sg.tile_begin; t < sg.tile_end; t += 16, ++g) {
      const long long t1 = std::min<long long>(t + 16, sg.tile_end);
      rows_of[(size_t)(g % grid_x)] += (long long)wr0[(size_t)t1] - (long long)wr0[(size_t)t];
    }
    const long long n_long = sg.long_end - sg.long_begin;
    const long long long_share = (n_long + 16LL * grid_x - 1) / (16LL * grid_x) * 16;
    for (long long v : rows_of) worst = std::max(worst, v + long_share);
  }
  return worst;
}

// ---- row chunks (csrc/dsgd_fstep.hpp) --------------------------------------------------------------------------------
struct ChunkTables {
  std::vector<FChunk> chunks;              // n_workers x n_wg
  std::vector<WTile> wt, ct;               // hot / cold tiles cut at the chunks' boundaries (never empty)
  std::vector<unsigned short> meta, cmeta; // their lane descriptors
  long long worst_rows = 1;                // rows of the largest chunk
};
// Cut every worker's rows [row_begin, row_end) into n_wg chunks of equal weight (share: the chunks' shares of their
// worker's weight, n_workers x n_wg, or empty for equal shares) and lay out both streams' tiles chunk by chunk.
inline void cut_row_chunks(const std::vector<StreamSeg>& row_segs, int n_wg, const std::vector<double>& share,
                           const std::vector<long long>& hrp, const std::vector<long long>& ctp,
                           const std::vector<long long>& long_rows, const std::vector<long long>& long_weight,
                           const signed char* label, ChunkTables& out) {
  const int n_workers = (int)row_segs.size();
  std::vector<WTile>&wt = out.wt, &ct = out.ct;
  wt.clear();
  ct.clear();
  out.chunks.assign((size_t)n_workers * (size_t)n_wg, FChunk());
  long long worst = 1;
  for (int k = 0; k < n_workers; ++k) {
    const long long rb = row_segs[(size_t)k].row_begin, re = row_segs[(size_t)k].row_end;
    // a row's weight: its slots in the two streams (6 bytes each) plus what every row costs (descriptor share, dcold, coef8);
    // a LONG row (in neither stream) its own non-zeros plus what its wave waits for it: ~10 us, five tiles' worth (round 6:
    // the chunks with the most long rows were the launch's last, 0.7-0.9 us per long row)
    auto W = [&](long long i) {
      const size_t nl = (size_t)(std::lower_bound(long_rows.begin(), long_rows.end(), i) - long_rows.begin());
      return hrp[(size_t)i] + ctp[(size_t)i] + 2 * i + long_weight[nl];
    };
    const long long w0 = W(rb), wtot = W(re) - w0;
    long long cut = rb;
    double share_total = 0.0, share_run = 0.0;
    const bool shares = share.size() == (size_t)n_workers * (size_t)n_wg;
    for (int b = 0; b < n_wg; ++b) share_total += shares ? share[(size_t)k * (size_t)n_wg + (size_t)b] : 1.0;
    for (int b = 0; b < n_wg; ++b) {
      long long nxt = re;
      share_run += shares ? share[(size_t)k * (size_t)n_wg + (size_t)b] : 1.0;
      if (b + 1 < n_wg) {
        const long long target = w0 + (long long)((double)wtot * share_run / share_total);
        long long lo = cut, hi = re;   // first row i in [cut, re] with W(i) >= target
        while (lo < hi) {
          const long long mid = (lo + hi) >> 1;
          if (W(mid) >= target) hi = mid;
          else lo = mid + 1;
        }
        nxt = lo;
      }
      FChunk& ch = out.chunks[(size_t)k * (size_t)n_wg + (size_t)b];
      ch.row_begin = (int)cut;
      ch.row_end = (int)nxt;
      ch.tile_begin = (int)wt.size();
      append_wave_tiles(hrp.data(), cut, nxt, wt, WS_MAXROWS);
      ch.tile_end = (int)wt.size();
      ch.ctile_begin = (int)ct.size();
      append_wave_tiles(ctp.data(), cut, nxt, ct, CT_MAXROWS);
      {
        // The chunk's cold tiles are walked twice by 16 waves with a stride of 16: 29-35 tiles of ~90 rows left some waves
        // three tiles and most two (phases A and C: 11 of a workgroup's 70 us).  Smaller tiles in a number just below a
        // multiple of 16 give every wave the same count (round 6).
        const size_t c0 = (size_t)ch.ctile_begin;
        auto waste = [](size_t n) { return n == 0 ? 1.0 : (double)((n + 15) / 16 * 16) / (double)n; };
        size_t n_best = ct.size() - c0;
        if (n_best % 16 != 0 && nxt > cut) {
          int mr_best = CT_MAXROWS;
          const long long target = (long long)((n_best + 15) / 16 * 16);
          int mr = (int)std::min<long long>(CT_MAXROWS, std::max<long long>(8, (nxt - cut + target - 1) / target));
          std::vector<WTile> tmp;
          for (int tries = 0; tries < 6 && mr >= 8 && waste(n_best) > 1.04; ++tries, --mr) {
            tmp.clear();
            append_wave_tiles(ctp.data(), cut, nxt, tmp, mr);
            if (waste(tmp.size()) < waste(n_best) && tmp.size() <= 3 * (size_t)target) {
              n_best = tmp.size();
              mr_best = mr;
            }
          }
          if (mr_best != CT_MAXROWS) {
            ct.resize(c0);
            append_wave_tiles(ctp.data(), cut, nxt, ct, mr_best);
          }
        }
      }
      ch.ctile_end = (int)ct.size();
      ch.long_begin = (int)(std::lower_bound(long_rows.begin(), long_rows.end(), cut) - long_rows.begin());
      ch.long_end = (int)(std::lower_bound(long_rows.begin(), long_rows.end(), nxt) - long_rows.begin());
      worst = std::max(worst, nxt - cut);
      cut = nxt;
    }
  }
  wave_tile_meta(hrp.data(), label, wt, out.meta);
  wave_tile_meta(ctp.data(), label, ct, out.cmeta);
  if (wt.empty()) wt.push_back(unused_wave_tile());
  if (ct.empty()) ct.push_back(unused_wave_tile());
  out.worst_rows = worst;
}

// ---- virtual tiles (dsgd_vt_grad_kernel) ---------------------------------------------------------------------
// Lay the lists of a plan out over the split streams: a row gets max(ceil(hot slots / 8), cold entries, 1) consecutive
// lanes of a 64-lane tile (whole rows per tile, every list starts a tile); a row that sits on the long-row list or holds
// more than 64 cold entries becomes a record of its own (one wave per row, whole CSR).
struct VtTables {
  std::vector<VtLane> lanes;        // 64 per tile
  std::vector<int> tile_rows;       // rows of every tile
  std::vector<MbRec> long_rows;     // the rows outside the tiles, list by list
  std::vector<long long> vt_off;    // n_lists + 1 tile offsets
  std::vector<WorkSeg> segs;        // n_lists tile ranges, then n_lists ranges of long_rows
  std::vector<int> grid, gxt, shift;   // per step: workgroups per worker, those of them that walk tiles, shift
};
// The streams as the host holds them.  hrp / ctp / crp / row_ptr: n_rows + 1 offsets; label: n_rows; ccol: the cold
// stream's 16-bit ranks, ctp[n_rows] of them.
struct VtStreams {
  long long n_rows;
  const long long *hrp, *ctp, *crp, *row_ptr;
  const signed char* label;
  const unsigned short* ccol;
};
// idx / offsets: the plan's lists, step-major (offsets: n_steps * n_workers + 1).  false: an index lies outside the rows
// (the row-wise kernel reports it).
inline bool vt_tables(const int* idx, const long long* offsets, long long n_steps, int n_workers, int n_cu, int vt_tpw,
                      const VtStreams& m, VtTables& out) {
  const long long n_lists = n_steps * n_workers;
  std::vector<VtLane>& lanes = out.lanes;
  lanes.clear();
  lanes.reserve((size_t)offsets[n_lists] * 10);
  std::vector<int>& tile_rows = out.tile_rows;
  tile_rows.clear();
  std::vector<MbRec>& long_rows = out.long_rows;
  long_rows.clear();
  std::vector<long long> long_off((size_t)n_lists + 1, 0);
  out.vt_off.assign((size_t)n_lists + 1, 0);
  const VtLane empty{0u, 0u, 0u, 0u};
  for (long long li = 0; li < n_lists; ++li) {
    int used = 0, rows = 0;   // lanes and rows of the open tile
    for (long long t = offsets[li]; t < offsets[li + 1]; ++t) {
      const long long r = idx[t];
      if (r < 0 || r >= m.n_rows) return false;
      const long long hot = m.hrp[r + 1] - m.hrp[r], cold = m.crp[r + 1] - m.crp[r];
      if (hot <= 0 || cold > 64) {   // long-row list / too many cold entries for a tile: one wave per row, whole CSR
        MbRec lr;
        lr.st = m.row_ptr[r];
        lr.len = (int)(m.row_ptr[r + 1] - m.row_ptr[r]);
        lr.y = (float)m.label[r];
        long_rows.push_back(lr);
        continue;
      }
      const int nl = (int)std::max<long long>(std::max<long long>((hot + 7) / 8, cold), 1);
      if (used + nl > 64) {                               // close the tile
        lanes.resize(lanes.size() + (size_t)(64 - used), empty);
        tile_rows.push_back(rows);
        used = 0;
        rows = 0;
      }
      const unsigned int ypos = m.label[r] > 0 ? VT_YPOS : 0u;
      for (int j = 0; j < nl; ++j) {
        VtLane L;
        const long long left = hot - 8LL * j;
        const unsigned int cnt = (unsigned int)std::max<long long>(0, std::min<long long>(8, left));
        L.hp = cnt ? (unsigned int)(m.hrp[r] + 8LL * j) : 0u;
        L.info = cnt | (j == 0 ? VT_START : 0u) | (j == nl - 1 ? VT_LAST : 0u) | ypos | (j < cold ? VT_COLD : 0u) |
                 ((unsigned int)rows << 16);
        L.cp = j < cold ? (unsigned int)(m.ctp[r] + j) : 0u;
        L.crank = j < cold ? (unsigned int)m.ccol[m.ctp[r] + j] : 0u;
        lanes.push_back(L);
      }
      used += nl;
      ++rows;
    }
    lanes.resize(lanes.size() + (size_t)(64 - used), empty);   // (a list is never empty: its last tile is open)
    tile_rows.push_back(rows);
    out.vt_off[(size_t)li + 1] = (long long)tile_rows.size();
    long_off[(size_t)li + 1] = (long long)long_rows.size();
  }
  // per step: the grid (workgroups per worker) and the fixed-point shift from the rows ONE workgroup can meet
  out.grid.assign((size_t)n_steps, 1);
  out.gxt.assign((size_t)n_steps, 1);
  out.shift.assign((size_t)n_steps, 21);
  const long long per_worker = std::max<long long>(1, n_cu / n_workers);
  std::vector<WorkSeg>& segs = out.segs;
  segs.assign((size_t)n_lists * 2, WorkSeg());
  for (long long li = 0; li < n_lists; ++li) {
    segs[(size_t)(n_lists + li)].begin = long_off[(size_t)li];
    segs[(size_t)(n_lists + li)].end = long_off[(size_t)li + 1];
  }
  for (long long s = 0; s < n_steps; ++s) {
    long long max_t = 1;
    for (int k = 0; k < n_workers; ++k) {
      const long long li = s * n_workers + k;
      segs[(size_t)li].begin = out.vt_off[(size_t)li];
      segs[(size_t)li].end = out.vt_off[(size_t)li + 1];
      max_t = std::max(max_t, segs[(size_t)li].end - segs[(size_t)li].begin);
    }
    long long max_long = 0;
    for (int k = 0; k < n_workers; ++k)
      max_long = std::max(max_long, long_off[(size_t)(s * n_workers + k) + 1] - long_off[(size_t)(s * n_workers + k)]);
    // workgroups of their own for the rows outside the tiled streams (one wave per row), beside the tile workgroups
    const long long gl = max_long ? std::max<long long>(1, std::min<long long>((max_long + 15) / 16, std::max<long long>(1, per_worker / 8))) : 0;
    const long long gx = std::max<long long>(1, std::min(per_worker - gl, (max_t + 16LL * vt_tpw - 1) / (16LL * vt_tpw)));
    long long worst = 1;
    std::vector<long long> rows_of((size_t)gx);
    for (int k = 0; k < n_workers; ++k) {
      const WorkSeg& sg = segs[(size_t)(s * n_workers + k)];
      std::fill(rows_of.begin(), rows_of.end(), 0);
      for (long long t = sg.begin; t < sg.end; ++t) rows_of[(size_t)(((t - sg.begin) / 16) % gx)] += tile_rows[(size_t)t];
      for (long long v : rows_of) worst = std::max(worst, v);
    }
    if (gl) worst = std::max(worst, (max_long + 16 * gl - 1) / (16 * gl) * 16);   // rows one long-row workgroup can meet
    out.gxt[(size_t)s] = (int)gx;
    out.grid[(size_t)s] = (int)(gx + gl);
    out.shift[(size_t)s] = std::min(21, 30 - rows_bits(worst));   // (<= 21: the fixed-point conversion is one fma against 1.5 * 2^23)
  }
  return true;
}

// ---- the packed copies of the split streams (the row-chunk kernel's PACKED form, csrc/dsgd_fstep.hpp) ------------------
// What dsgd_pack_streams_kernel builds on the device, stated on the host: for the slots [row_ptr[i], row_ptr[i + 1]) of every
// row, colf = the 16-bit rank with bit 15 set on the row's FIRST slot (col = nullptr: no ranks, the cold stream) and valy =
// label[i] > 0 ? x : -x.  A pure function of the slot: whichever tile table addresses the stream reads the same words.
inline void packed_streams_ref(const long long* row_ptr, long long n_rows, const signed char* label, const unsigned short* col,
                               const float* val, unsigned short* colf, float* valy) {
  for (long long i = 0; i < n_rows; ++i)
    for (long long e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      if (col) colf[e] = (unsigned short)(col[e] | (e == row_ptr[i] ? 0x8000u : 0u));
      valy[e] = label[i] > 0 ? val[e] : -val[e];
    }
}
// The start bits of a tile's 64 lanes as the PACKED kernel derives them (w_tile_q, csrc/dsgd_kernels.hpp -- the same steps in
// the same order): the flags of the window's slots, a window of the tile's slots rounded up to 8 (a lane beyond it reads
// zeros); in lane n >> 3 the flags behind slot n dropped and the end mark set at n; and, where the wave then counts more
// starts than the tile's rows + 1, that many of lane 0's lowest flags dropped (rows that start in the up to 7 slots between
// pos0 and the tile's first row).  colf: the flagged ranks, n_words of them (the stream and its padding).
inline void packed_lane_bits(const WTile& T, const unsigned short* colf, long long n_words, unsigned int (&bits)[64]) {
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
    if (nrows < 0) b = 0;
    const unsigned int em = nrows < 0 ? 0u : 1u << (n & 7);
    if (l == (n >> 3)) b = (b & (em - 1u + em)) | em;
    bits[l] = b;
    for (unsigned int x = b; x; x &= x - 1u) ++total;
  }
  for (int extra = total - nrows - 1; extra > 0; --extra) bits[0] &= bits[0] - 1u;
}
