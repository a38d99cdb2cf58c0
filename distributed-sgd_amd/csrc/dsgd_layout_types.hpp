// The plain records and constants that the host writes into device tables and the kernels read: work ranges, wave tiles,
// row chunks, virtual-tile lanes.  No HIP type and no library call, so that the kernel headers, the host's table arithmetic
// (csrc/dsgd_layout_host.hpp) and a host test (tests/test_layout_host.py) compile the same layouts.
#pragma once

// one unit of gradient work: worker k processes items [begin, end) -- positions in the resident
// index list (idx != nullptr) or CSR row numbers themselves (contiguous range)
struct WorkSeg {
  long long begin;
  long long end;
};
static_assert(sizeof(WorkSeg) == 16, "read with one scalar load");

// Fixed-point gradient accumulation.  Measured on MI355X (tools/microbench3.hip): ds_add_f32 retires
// 0.31 lanes/clk/CU (188 Gnnz/s chip-wide) while ds_add_u32 runs at the HBM streaming rate
// (671 Gnnz/s).  The scatter therefore accumulates round(y*x * 2^21 / vmax2) as 32-bit integers in
// LDS (vmax2 = max|x| rounded up to a power of two, so the scaling is exact; overflow control of the
// 32-bit accumulators: see w_scatter).  Integer addition is
// associative: the gradient of a whole-shard batch is bit-reproducible run to run, and exact up to
// the 2^-22 * vmax2 rounding of each contribution (fp32 atomics round at the ulp of the RUNNING sum).
constexpr int FIX_SHIFT = 21;

struct StreamSeg {
  long long row_begin, row_end;    // rows of this worker's batch
  long long tile_begin, tile_end;  // tiles intersecting [row_begin, row_end)
  long long long_begin, long_end;  // wave-tile mode: range of the long-row list (rows that fit no tile)
  long long ctile_begin, ctile_end;  // cold-stream tiles intersecting [row_begin, row_end)
};
static_assert(sizeof(StreamSeg) == 64, "eight 64-bit fields, read with scalar loads");

// wave tiles (dsgd_wseg_kernel, csrc/dsgd_kernels.hpp)
constexpr int WS_SLOTS = 512;
constexpr int WS_MAXNNZ = WS_SLOTS - 8;
constexpr int WS_MAXROWS = 254;
constexpr int WS_PAD = WS_SLOTS + 8;   // padding elements behind col/val
constexpr int WS_SPILL_AT = 1 << 28;   // cold-stream accumulators (shift 21, returning atomics): spill / panic bands
constexpr int WS_PANIC_AT = 1 << 30;
constexpr int WS_COEF_STRIDE = 256;

struct WTile {       // 16 bytes, read with one scalar load
  long long pos0;    // first slot of the window (multiple of 4)
  int r0;            // global row of local row 1
  int info;          // rows in the tile (low 16 bits, signed; -1: unused entry) | slots holding its non-zeros << 16
};
static_assert(sizeof(WTile) == 16, "read with one scalar load");

// Cold tiles: WTile records and 16-bit lane descriptors exactly as the hot stream's (build_wave_tiles on the cold row
// offsets), at most CT_MAXROWS rows per tile: cold rows hold ~6 entries, a 512-slot tile ~90 rows, and the gradient
// kernel keeps a tile's gate coefficients as two bytes per lane.
constexpr int CT_MAXROWS = 128;

struct FChunk {          // 32 bytes, read with scalar loads
  int row_begin, row_end;      // the chunk's rows
  int tile_begin, tile_end;    // its hot tiles (of the chunked tile table)
  int ctile_begin, ctile_end;  // its cold tiles
  int long_begin, long_end;    // its range of the long-row list
};
static_assert(sizeof(FChunk) == 32, "read with scalar loads");

struct __attribute__((aligned(16))) MbRec {   // one row of a wave's batch, as the passes need it
  long long st;    // first non-zero
  int len;
  float y;         // label (+1 / -1)
};
static_assert(sizeof(MbRec) == 16, "one 16-byte record per row");

struct VtLane {          // 16 bytes, one per lane of a virtual tile (written by the host: vt_build)
  unsigned int hp;       // first of the lane's <= 8 slots in the hot stream
  unsigned int info;     // valid slots (bits 0-3) | first lane of its row (4) | last lane (5) | label > 0 (6) |
                         // has a cold entry (8) | local row of the tile (bits 16-21)
  unsigned int cp;       // the lane's cold entry in the cold stream
  unsigned int crank;    // ... and its rank - hsplit (the host keeps a copy of the cold ranks: no load depends on a load)
};
constexpr unsigned int VT_START = 1u << 4, VT_LAST = 1u << 5, VT_YPOS = 1u << 6, VT_COLD = 1u << 8;
static_assert(sizeof(VtLane) == 16, "one 16-byte descriptor per lane");
