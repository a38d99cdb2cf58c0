// libdsgd_hip -- MI355X (gfx950 / CDNA4) engine behind include/dsgd.h.
//
// Hot path of zifeo/distributed-sgd re-designed for one MI355X per process:
//   * the CSR shard, w, g and dimSparsity stay resident in HBM (288 GB/GPU); w/g/ds are
//     3 x 189 KB and live in the XCD L2s, so the only HBM stream is the CSR itself
//     (8 B per non-zero + 12 B per row -- SURVEY.md 8(d));
//   * gradient kernels: whole row ranges stream the matrix split by column rank (hot tiles with weights and gradient
//     in LDS, a row-ordered cold stream); index-list batches run the mini-batch engine (dsgd_batch.hpp); every sum is
//     accumulated in fixed point (exact, order-independent) and rounded once;
//   * exact reduce + regularise + aggregate + update are one fused kernel over D+1 columns;
//   * the synchronous master's Vec.mean over workers is one ncclAllReduce on the same stream.
// Citations "ref:" are relative to /root/reference/src/main/scala/epfl/distributed/.
//
// This file is written for gfx950 only: wave64, no CUDA paths, no compatibility layers.

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <chrono>
#include <vector>

#include "../../include/dsgd.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e__ = (expr);                                                                  \
    if (e__ != hipSuccess) return fail(DSGD_EHIP, "%s: %s", #expr, hipGetErrorString(e__));   \
  } while (0)

#define DSGD_TRY(expr)        \
  do {                        \
    int rc__ = (expr);        \
    if (rc__ != DSGD_OK) return rc__; \
  } while (0)

// ------------------------------------------------------------------------------------------------
// RCCL, resolved lazily so that single-GPU users never map the (very large) library
// ------------------------------------------------------------------------------------------------
namespace rccl {
typedef struct ncclComm* comm_t;
typedef struct {
  char internal[DSGD_UNIQUE_ID_BYTES];
} unique_id_t;
enum { kFloat32 = 7, kInt64 = 4, kUint32 = 3, kSum = 0 };
static int (*GetUniqueId)(unique_id_t*) = nullptr;
static int (*CommInitRank)(comm_t*, int, unique_id_t, int) = nullptr;
static int (*CommDestroy)(comm_t) = nullptr;
static int (*CommAbort)(comm_t) = nullptr;   // optional: only used to give up a group that not every rank joined
static int (*AllReduce)(const void*, void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
static int (*GroupStart)() = nullptr;
static int (*GroupEnd)() = nullptr;
static const char* (*GetErrorString)(int) = nullptr;
static std::once_flag once;
static bool ok = false;

static void load() {
  void* h = nullptr;
#ifdef DSGD_TEST_COLLECTIVE_SEAM
  // TEST BUILDS ONLY (tests/rccl_stub/build_seam.py compiles this file a second time with -DDSGD_TEST_COLLECTIVE_SEAM into
  // tests/rccl_stub/libdsgd_hip_seam.so): DSGD_RCCL_LIB=<path> names the library that serves the collectives -- a
  // host-staged shim that lets several ranks share ONE device, which RCCL refuses (the world = 2 arithmetic on a one-GPU
  // box).  The product library (distributed-sgd_amd/lib/libdsgd_hip.so) is compiled without this block: no environment
  // variable can put anything in RCCL's place there.
  if (const char* forced = getenv("DSGD_RCCL_LIB")) {
    h = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
  }
#endif
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);  // reuse a copy the process already has
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) return;
  GetUniqueId = (decltype(GetUniqueId))dlsym(h, "ncclGetUniqueId");
  CommInitRank = (decltype(CommInitRank))dlsym(h, "ncclCommInitRank");
  CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
  CommAbort = (decltype(CommAbort))dlsym(h, "ncclCommAbort");
  AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
  GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart");
  GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
  GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
  ok = GetUniqueId && CommInitRank && CommDestroy && AllReduce && GroupStart && GroupEnd && GetErrorString;
}
static bool available() {
  std::call_once(once, load);
  return ok;
}
}  // namespace rccl

#define RCCL_TRY(expr)                                                                          \
  do {                                                                                          \
    int r__ = (expr);                                                                           \
    if (r__ != 0) return fail(DSGD_ERCCL, "%s: %s", #expr, rccl::GetErrorString(r__));          \
  } while (0)

#include "dsgd_buf.hpp"      // (host only: the owners of device and pinned memory)
#include "dsgd_layout_cache.hpp"   // (host only: the few device layouts a gradient family keeps per row-range configuration)
#include "dsgd_plan_cache.hpp"   // (host only: the device blocks plans take and hand back, and a plan's hold on one)
#include "dsgd_plan_check.hpp"   // (host only: a plan's lists against the rows loaded now)
#include "dsgd_layout_host.hpp"  // (host only: the arithmetic behind every table the gradient kernels read)
#include "dsgd_route.hpp"        // (host only: the switches, and which kernel family serves a call)
#include "dsgd_kernels.hpp"
#include "dsgd_logistic.hpp"   // (the logistic model beside the SVM: its own gradient, finish, evaluation and probabilities)
#include "dsgd_lg_topics.hpp"  // (... over several topics: one-vs-rest label planes on the same rows, one launch pair per step)
#include "dsgd_lg_eval.hpp"    // (... evaluated as Master evaluates: classes and tallies of K row ranges, the rows of a list)
#include "dsgd_lg_eval_job.hpp"   // (... and the job's evaluation on every rank: the gather record, its fold, the kernel that fills it)
#include "dsgd_batch.hpp"
#include "dsgd_cs.hpp"
#include "dsgd_lg_cs.hpp"   // (the logistic model on column slices: the cell layout and the exchange above, logistic arithmetic)
#include "dsgd_lg_cs_async.hpp"   // (its asynchronous iterations of a one-worker plan: a sibling body, the kernel above untouched)
#include "dsgd_dense.hpp"
#include "dsgd_fstep.hpp"
#include "dsgd_tcol.hpp"
#include "dsgd_lg_cols.hpp"   // (the logistic model's whole-split steps by column lists: coefficients, column-wise gradient)
#include "dsgd_shuffle.hpp"
#include "dsgd_cs64.hpp"   // (last: the fp64 mode)
#include "dsgd_rp64.hpp"   // (... and its row-parallel gradient family, on float and on Double feature values)
#include "dsgd_sparse.hpp" // (the Sparse form at the boundary: compaction and scatter-in)
#include "dsgd_predict.hpp" // (distributed evaluation: predictions and per-split tallies of K row ranges in one launch)
#include "dsgd_eval_list.hpp" // (sampled evaluation: the tallies of the rows a device-resident list names in one launch)
#include "dsgd_snapshot.hpp" // (the consistent loss check beside the lock-free engine: one snapshot of w, its scalars, its window)

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct dsgd_plan {
  // (the blocks from the context's cache -- d_idx, d_segs, d_cs_*, the record -- go back to it with the plan, in this order)
  CacheBuf<int> d_idx;
  std::vector<long long> offsets;  // n_steps * n_workers + 1
  CacheBuf<WorkSeg> d_segs;        // n_steps * n_workers
  long long n_steps = 0;
  int n_workers = 0;
  long long max_items = 0;  // largest single list
  long long max_step_rows = 0;  // largest step (all workers together)
  bool fits = false;            // every list fits the staged sub-batch of dsgd_plan_kernel (rows and work items)
  long long fits_rows = -1;     // ... of the data set with this many rows (the one loaded at plan creation)
  // virtual tiles (dsgd_vt_grad_kernel): the lists laid out over the split streams, built at the first run that needs them
  std::vector<int> h_idx;       // host copy of the lists (a plan drawn on the device fetches it only if a host builder asks: plan_host_idx)
  bool idx_trusted = false;     // the lists were drawn by the library inside the caller's row ranges: nothing to validate
                                //   (ranges of the data loaded THEN: cleared by plan_revalidate after a load)
  bool drawn = false;           // ... drawn by the library at all (such plans never take the one-workgroup kernel: fits stays false)
  long long checked_load = -1;  // the context's load_gen the lists were last checked against (plan_revalidate)
  DevBuf<VtLane> d_vt_lanes; // 64 descriptors per tile
  DevBuf<WorkSeg> d_vt_segs; // tile range of every list, then (n_lists further entries) its range of d_vt_long
  DevBuf<MbRec> d_vt_long;   // rows of the lists that sit in no tile (long-row list, more than 64 cold entries)
  DevBuf<uint4> d_vt_packed; // plans up to vt_pack_mb: the tiles' own copy of the rows they touch (4 KiB per tile)
  std::vector<long long> vt_off;       // n_lists + 1 tile offsets
  std::vector<int> vt_grid, vt_gxt, vt_shift;  // per step: workgroups per worker, those of them that walk tiles, shift
  long long vt_layout = -1;     // the layout generation the tiles were built for (-1: not built)
  bool vt_ok = false;           // every row of every list sits in the tiled streams
  // column slices (dsgd_cs_step_kernel): the lists laid out per (slice, step), built at the first run that can use them
  CacheBuf<CsHdr> d_cs_hdr;     // the six layout arrays: from the cache (device-built) or the plan's own (host-built)
  CacheBuf<unsigned int> d_cs_meta;
  CacheBuf<unsigned short> d_cs_rf;
  CacheBuf<uint4> d_cs_col;
  CacheBuf<float4> d_cs_val;
  CacheBuf<unsigned short> d_cs_cl;
  int cs_G = 0, cs_spl = 0, cs_nt = 0, cs_slot_stride = 0, cs_row_stride = 0, cs_cl_stride = 0;
  std::vector<int> cs_shift;    // per step
  long long cs_layout = -1;     // the layout generation (column ranking) the slices were built for
  bool cs_ok = false;
  bool cs_device_built = false; // laid out by dsgd_cs_layout_kernel (false: by the host, DSGD_CS_HOST_LAYOUT=1)
  // what the plan's set-up enqueued on the context's BUILD stream (lists uploaded, cells laid out) ends with this event;
  // the first run makes the launch stream wait for it
  Event built_ev;
  bool built_pending = false;
  // dsgd_plan_record: gate decisions and regulariser scalars of the steps run (column-slice plans)
  CacheBuf<unsigned int> d_gate_rec;
  CacheBuf<float> d_s_rec;
  int gate_words = 0;
  // a row-parallel fp64 plan (dsgd_plan_create_rp64_n and its kin): the lists and their ranges only, no layout -- its steps are
  // the two launches of dsgd_sync_step_f64 over d_idx / d_segs, on whichever value type is loaded at the run (plan_run_rp64)
  bool rp64 = false;
  // a logistic plan (dsgd_plan_create_lg_n, dsgd_plan_create_from_seed_lg): likewise the lists and their ranges only -- its steps
  // are the two launches of dsgd_lg_sync_step over d_idx / d_segs (plan_run_lg, csrc/dsgd_lg_calls.hpp)
  bool lg = false;
  // ... that additionally asked for its column slices (dsgd_plan_create_lg_cs_n, dsgd_plan_create_from_seed_lg_cs): laid out at
  // creation by dsgd_cs_layout_kernel into d_cs_* (LG_CS_G slices); while they are current its steps are ONE launch of
  // dsgd_lg_cs_step_kernel (plan_run_lg_cs), else plan_run_lg's two per step
  bool lg_cs = false;
  void cs_free() {
    d_cs_hdr.reset(), d_cs_meta.reset(), d_cs_rf.reset(), d_cs_col.reset(), d_cs_val.reset(), d_cs_cl.reset();
    cs_ok = false;
  }
  ~dsgd_plan() {   // (members go in reverse order: the hand-backs are spelled out to keep theirs)
    d_idx.reset(), d_segs.reset();
    cs_free();
    d_gate_rec.reset(), d_s_rec.reset();
  }
};

struct FusedArgs {
  int hg, n_wg, hc, nc, n_wgc;
  double inv_scale, inv_scale_cold;
};

struct dsgd_ctx {
  dsgd_config cfg{};
  Knobs k;     // every DSGD_* switch, read once by dsgd_create (csrc/dsgd_route.hpp)
  int dp = 0;  // D + 1
  std::mutex mu;
  hipStream_t stream = nullptr;
  // data
  long long n_rows = 0, nnz = 0;
  DevBuf<long long> d_row_ptr;
  DevBuf<int> d_col;
  DevBuf<float> d_val;
  DevBuf<signed char> d_label;
  int group = 16;  // lanes per row of the row-wise prediction / evaluation kernels, from the mean row length
  // column layout: external keys <-> internal frequency ranks (identity until prepare_layout)
  DevBuf<int> d_perm;   // key  -> rank
  bool layout_ready = false;
  int hw_eval = DSGD_LDS_FLOATS;
  // nnz-streaming kernels (contiguous row ranges)
  DevBuf<StreamSeg> d_ssegs;
  std::vector<StreamSeg> ssegs_last;
  // The matrix is SPLIT by column rank into a hot stream (rank < hsplit: wave tiles, weights and gradient in LDS, no
  // gathers) and a cold stream (col - hsplit, val, row) handled by two small kernels whose LDS holds the cold weights /
  // the cold gradient.
  std::vector<long long> h_row_ptr;     // host copy of the internal row_ptr (tile building at layout time)
  std::vector<long long> h_crow_ptr;    // cold ENTRIES before each row
  std::vector<long long> h_hrp, h_ctp;  // slot offsets of the hot / cold stream (virtual tiles are built from them)
  std::vector<unsigned short> h_ccol;   // host copy of the 16-bit cold ranks (a virtual tile's descriptor carries its cold rank)
  long long layout_gen = 0;             // bumped whenever the split streams are rebuilt, and by every load (what a plan or a
                                        //   column-list layout stamped is stale from the load on, not from the next ranking on)
  long long load_gen = 0;               // bumped by every successful dsgd_load_csr / _f64 (plan_revalidate)
  bool layout_seen_by_build = false;    // the build stream is ordered behind the kernels that wrote the current split streams
  unsigned int cs_tag0 = 0;             // column-slice steps launched so far (the exchange granules' tags run on)
  DevBuf<float> d_cs_w;              // the weights slice-major while cs_w_G != 0: then d_w is STALE -- every entry point that
  DevBuf<float> d_cs_ds;             //   is not a column-slice launch converts back first (bind); dimSparsity likewise (a copy)
  int cs_w_G = 0;                       // slices of the slice-major state (0: the weights are in d_w, rank order)
  DevBuf<unsigned long long> d_cs_x; // exchange buffer of dsgd_cs_step_kernel: [2][CS_MAX_G][CS_XSTRIDE] granules
  DevBuf<unsigned int> d_cs_sync;    // its arrival counter and abort word
  DevBuf<unsigned int> d_cs_max;     // the layout kernels' maxima and flags (4 words) ...
  HostBuf<unsigned int> h_cs_max;     // ... and where pass 1's come back to (pinned)
  hipStream_t build_stream = nullptr;   // a plan's set-up (uploads, layout kernels) runs here, beside the launch stream
  PlanCache plan_cache;                 // device blocks that plans hand back (dsgd_plan_destroy) and take again (dsgd_plan_create)
  std::vector<dsgd_plan*> plans;        // the plans alive: what dsgd_plan_destroy did not see, dsgd_destroy gives back and deletes
  // scratch of dsgd_plan_create_from_seed, kept across epochs (grow-only): a hipFree per epoch would wait for the whole
  // device -- i.e. for the epoch that is running on the launch stream while the next one's lists are drawn
  DevBuf<void> seed_scratch[9];   // (bytes)
  // the one-step layout of per-request steps (dsgd_cs_request_kernel), strides at their maxima, per slice count
  struct ReqLayout {
    DevBuf<CsHdr> hdr;
    DevBuf<unsigned int> meta;
    DevBuf<unsigned short> rf, col;
    DevBuf<float> val;
    DevBuf<unsigned short> cl;
    int G = 0;
  } req_layout;
  std::vector<signed char> h_label;
  // wave tiles over d_hcol/d_hval
  DevBuf<WTile> d_wtiles;
  DevBuf<unsigned short> d_wmeta;
  long long n_wtiles = 0;
  std::vector<int> h_wtile_r0;          // first row of every wave tile (+ sentinel n_rows)
  std::vector<long long> wlong_rows;    // rows that fit no wave tile (sorted): one wave per row, from the whole CSR
  std::vector<long long> wlong_weight;  // prefix sums of their weights in the row chunks' balance (slots; fstep_layout)
  DevBuf<int> d_wlong_rows;          // the same list on the device
  DevBuf<int> d_part;                // per-workgroup partial sums of the wseg gradient kernel: part_wgs x part_stride
  long long part_wgs = 0;
  int part_stride = 0;
  int hsplit = HSPLIT_MAX;              // hot ranks: 2 * hsplit words of LDS (DSGD_HSPLIT, clamped and aligned by dsgd_create)
  DevBuf<unsigned short> d_hcol;     // hot stream (16-bit ranks < hsplit), WS_PAD elements of padding
  DevBuf<float> d_hval;
  DevBuf<long long> d_hrow_ptr;      // n_rows + 1 (rows of the long list: empty)
  long long hot_nnz = 0;
  DevBuf<void> d_ccol;               // cold stream in row order: rank - hsplit (16-bit words, or 32-bit when there
  DevBuf<float> d_cval;              // are more than 65536 cold columns), value; WS_PAD elements of padding
  bool cold_col16 = false;
  DevBuf<long long> d_ctp;           // n_rows + 1: slot offsets of the cold stream (a tiled row owns >= 1 slot)
  long long coldm_nnz = 0;              // slots of the cold stream
  DevBuf<WTile> d_ctiles;            // wave tiles over d_ccol/d_cval (same records and lane descriptors as the hot ones)
  DevBuf<unsigned short> d_cmeta;
  long long n_ctiles = 0;
  std::vector<int> h_ctile_r0;          // first row of every cold tile (+ sentinel n_rows)
  DevBuf<float> d_dcold;             // n_rows: cold part of x.w (rows without cold entries stay 0)
  DevBuf<int> d_partc;               // per-workgroup cold gradient partials: partc_wgs x partc_stride
  long long partc_wgs = 0;
  int partc_stride = 0;
  DevBuf<signed char> d_coef8;  // n_rows: gate coefficient y * [y (x . w) >= 0] of the last whole-range step
  const char* last_grad_kernel = "";
  // vectors
  DevBuf<float> d_w;
  DevBuf<float> d_ds;
  DevBuf<float> d_g;  // workers x dp
  DevBuf<long long> d_g64;  // workers x dp fixed-point accumulators of the streaming kernel (zero between steps)
  float fix_scale = 4194304.0f;  // 2^cold_shift / vmax2
  int cold_shift = FIX_SHIFT;    // shift of the cold columns' words: FIX_SHIFT unless the data's cold tiles need less (build_split)
  int vexp = 0;                  // vmax2 = 2^vexp >= max |value|
  int last_shift = FIX_SHIFT;    // shift of the last gradient launch (streaming kernels or index-list kernel)
  std::vector<StreamSeg> bound_segs;   // split layout: the (ranges, grid) configuration bound_shift was measured for
  unsigned bound_grid = 0;
  int bound_shift = 0;
  DevBuf<unsigned int> d_bound;
  // Row chunks (csrc/dsgd_fstep.hpp): the whole gradient of a row range in ONE launch.  Per (row ranges, workgroups per
  // worker) configuration the host cuts the ranges into chunks balanced by stream bytes and lays out wave tiles of both
  // streams that end at the chunk boundaries; a few configurations stay cached (a fit alternates train steps only; the
  // tests and the bench's legs bring their own).
  struct FstepLayout {
    int n_wg = 0;                    // workgroups (chunks) per worker
    DevBuf<WTile> d_tiles;
    DevBuf<unsigned short> d_meta;
    DevBuf<WTile> d_ctiles;
    DevBuf<unsigned short> d_cmeta;
    DevBuf<FChunk> d_chunks;
    long long worst_rows = 1;        // rows of the largest chunk
    int shift = -1;                  // the measured fixed-point shift of the hot accumulators (-1: not measured yet)
    // measured balance (round 6): the workgroups' own durations, summed by the kernel over `launches` launches, re-cut the
    // chunks once or twice per configuration (a chunk's share of the weight follows its workgroup's measured rate)
    DevBuf<unsigned long long> d_times;
    HostBuf<unsigned long long> h_times;   // pinned
    Event times_ev;
    std::vector<double> share;       // per chunk: its share of its worker's weight (empty: equal shares)
    int launches = 0, rebalances = 0;
    bool times_pending = false;
  };
  LayoutCache<FstepLayout> fstep_cache;   // (keyed by the ranges and n_wg)
  int last_fstep_rebalances = 0;     // how often the configuration of the last chunked launch has been re-cut (dsgd_tuning_info)
  // The chunked launch's PACKED form (csrc/dsgd_fstep.hpp): copies of the split streams, slot for slot -- hot ranks with the
  // row starts in bit 15, y * x of both streams -- built on the device by the first chunked launch of a split that may use
  // them (csrc/dsgd_fstep_host.hpp: fstep_packed_streams) and dropped with the streams they copy (packed_drop)
  DevBuf<unsigned short> d_hcolf;    // hot_nnz + WS_PAD
  DevBuf<float> d_hvaly;             // hot_nnz + WS_PAD
  DevBuf<float> d_cvaly;             // coldm_nnz + WS_PAD
  int packed_state = 0;              // 0: not asked for since the split was built, 1: built, -1: no memory for them (the plain form runs)
  bool last_fstep_packed = false;    // the last chunked launch ran the PACKED form (dsgd_tuning_info slot [0]: 5 instead of 4)
  // Column lists (csrc/dsgd_tcol.hpp): whole-split steps of 10^3 .. 10^5 rows as dot + column-wise gradient + reduce, no
  // partials.  Per (row ranges) configuration the device sorts the ranges' entries by (worker, column) once; a few
  // configurations stay cached.
  struct TcolLayout {
    long long n_ent = 0;             // entries of the ranges' rows
    int share = 0, n_wg = 0;         // entries per workgroup of the gradient kernel, its workgroups
    int bm_words = 0;                // words of the step's bitmap (every worker's range padded to 64 rows; a multiple of 4)
    DevBuf<unsigned int> d_ent_pk;
    DevBuf<float> d_ent_val;
    DevBuf<TcShare> d_shares;
    DevBuf<int> d_key_of_cid;
    DevBuf<int> d_bit_base;       // [workers]
    DevBuf<unsigned int> d_bitmap;   // the gate's decisions of the last step over these ranges
  };
  LayoutCache<TcolLayout> tcol_cache;
  TcolGate tcol_gate;                // their back-off from callers that never repeat a configuration
  bool fused_apply_pending = false;
  FusedArgs fused_args{};
  DevBuf<float> d_redpart;    // per-block partial sums of w.ds and |w|^2 of the fused reduce + apply kernel
  int redpart_cap = 0;
  // Pinned staging of the per-request entry points (Slave.gradient / Slave.forward hand over w and the sample indices
  // and get a dense vector back): a copy between pageable memory and the device is staged by the runtime, blocks the
  // calling thread and cannot overlap the kernels around it (151 us for a batch-size-100 dsgd_gradient, of which the
  // kernels are ~35: profiles/r02_boundary_latency.json).
  struct Pinned {
    HostBuf<void> p;           // (bytes)
    Event ev;                  // the last copy FROM this buffer to the device
    bool armed = false;
  };
  Pinned pin_w, pin_idx, pin_segs, pin_out, pin_upd;
  // dsgd_update_grad: persistent device staging (keys, values) -- no allocation per call, nothing that synchronises the
  // device while the persistent engine is resident
  DevBuf<int> d_upd_key;
  DevBuf<float> d_upd_dv;
  hipStream_t upd_stream = nullptr;
  DevBuf<float> d_pred;     // dsgd_forward's predictions (grown on demand)
  DevBuf<signed char> d_pred8;          // dsgd_predict_ranges' predictions (grown on demand) ...
  DevBuf<long long> d_pred_tab;         // ... its range table (off[K + 1], begin[K]) followed by the tallies [K][3], K at its maximum
  DevBuf<float> d_gsum;  // dp (all-reduce buffer / sum over hosted workers)
  DevBuf<float> d_tmp;   // dp scratch (ranked order)
  DevBuf<float> d_io;    // dp staging for vectors crossing the API in key order
  DevBuf<DevScalars> d_sc;
  HostBuf<DevScalars> h_sc;  // pinned
  // per-request steps: {n_active, err} written by the request's last kernel into host-mapped memory (no copy back);
  // n_active is read as a DIFFERENCE against the value the host last saw, so the request needs no memset either
  HostBuf<int> h_req;                   // host-mapped index lists of a per-request step (REQ_MAPPED_ITEMS entries; the kernels read .dev())
  const int* cur_idx = nullptr;           // where stage_lists put the lists of the request in flight
  HostBuf<unsigned long long> h_mail;   // host-mapped: {n_active, err, sequence number of the request that wrote them, -}
  unsigned long long mail_seq = 0;        // requests answered through the mailbox so far
  bool ctr_known = false;                 // the host knows the device's n_active (ctr_last) and that err is clear
  unsigned long long ctr_last = 0;
  bool s_dirty = true;
  bool s_lazy = false;      // s and |w|^2 of the resident w are still per-block pairs in d_redpart[red_par] (fra_scalars)
  int red_par = 0;          // the half of d_redpart the last scalar-writing kernel wrote
  bool nsq_dirty = false;   // |w|^2 stale although s is current (after dsgd_plan_kernel)
  bool have_ds = false;
  // staging for host-provided index lists
  DevBuf<int> d_idx;
  DevBuf<WorkSeg> d_segs;
  std::vector<WorkSeg> segs_last;  // what d_segs currently holds
  long long pending_samples = 0;   // rows enqueued by *_async calls since the last dsgd_synchronize
  bool job_pending = false;        // ... and row-parallel fp64 plan runs under a communicator among them: the JOB's rows run on in d_sc->n_samples
                                   // (until dsgd_synchronize or the next call that resets the counters: reset_counters)
  // persistent Hogwild engine
  hipStream_t async_stream = nullptr;
  hipStream_t query_stream = nullptr;
  DevBuf<HogState> d_hog;
  HostBuf<HogState> h_hog;   // pinned
  DevBuf<float> d_gcold;
  DevBuf<long long> d_asg;  // begin[n], end[n]
  DevBuf<unsigned long long> d_hog_it;   // per worker: iterations done (continues across exchange rounds)
  DevBuf<unsigned int> d_trace;          // dsgd_async_set_trace: one record per update of the next engine runs
  long long trace_cap = 0;                  // records asked for
  int trace_mw = 0;                         // mask words per record of the last traced run ((batch + 31) / 32)
  int trace_batch = 0;                      // ... and its batch size (a record carries one x . w per sampled row)
  DevBuf<float> d_tdot;                  // traced runs: n_workers x batch, the x . w of every worker's mini-batch in flight
  HostBuf<int> h_one;        // pinned constant 1: source of the stop-flag copy
  // small-batch plan kernel (one persistent workgroup): cold strip and the multi-worker sum buffer
  DevBuf<unsigned long long> d_tprof;   // DSGD_PLAN_PROF=1: phase cycle counters of dsgd_plan_kernel (tuning runs)
  DevBuf<float> d_plan_gcold;
  int hog_hl = HOG_HL, hog_wl = HOG_WL;   // LDS-resident ranks of the Hogwild engine (accumulators / weight copy)
  int hog_workers = 0;      // capacity of the per-worker buffers
  int hog_n = 0, hog_batch = 0, hog_bug = 0;   // the running configuration
  float hog_lr = 0.0f;
  unsigned long long hog_seed = 0;
  long long exchange_every = 0;   // dsgd_async_set_exchange: cross-GPU exchange period in local updates (0 = none)
  DevBuf<float> d_wprev;       // weights at the last exchange
  DevBuf<float> d_wdelta;      // 2 x dp: all-reduced updates, this replica's own part
  // dsgd_async_check (csrc/dsgd_snapshot.hpp): two snapshots of w in rank order, allocated at the first check -- the last
  // check's and the best one's (dsgd_async_check_keep makes the last one the best one: the two handles change places, the
  // next check writes into the other buffer); -1: holds nothing.  reset_layout drops both (the rank order goes).
  DevBuf<float> d_snap[2];
  int snap_last = -1, snap_best = -1;
  DevBuf<unsigned long long> d_snap_win;   // {max ~before, max after} of the last snapshot's update counts
  HostBuf<unsigned long long> h_snap_win;   // pinned
  bool async_running = false;
  bool join_in_progress = false;            // one thread blocks on the engine (without the mutex); the others wait for it
  std::condition_variable join_cv;
  int join_rc = DSGD_OK;                    // what that thread's join returned: every waiter reports it
  std::string join_err;
  // exchange mode: the rounds (engine launch, delta, all-reduce, apply) are enqueued by a helper thread so that
  // dsgd_async_start returns at once and dsgd_async_updates / dsgd_async_stop stay responsive
  std::thread exch_thread;
  std::atomic<bool> exch_done{true};
  int exch_rc = DSGD_OK;
  std::string exch_err;
  // comm
  rccl::comm_t comm = nullptr;
  bool comm_broken = false;   // a grouped collective failed half way: the communicator was aborted
  bool comm_broken_ok = false;   // (set only inside dsgd_comm_destroy: the one call a broken context accepts)
  int world = 1, rank = 0;
  // profiling of the gradient kernel
  bool prof = false;
  bool prof_main_only = false;
  std::vector<std::pair<Event, Event>> prof_ev;
  size_t prof_used = 0;
  std::vector<int> prof_kind;
  double prof_kms[3] = {0.0, 0.0, 0.0};
  long long prof_kn[3] = {0, 0, 0};
  int n_cu = 256;
  // the fp64 mode (DSGD_F_FP64, csrc/dsgd_cs64.hpp): the weights and dimSparsity in fp64, rank order like d_w / d_ds; while
  // cs_w_G != 0 the weights are slice-major in d_cs_w64 (bind converts back, as for fp32)
  bool fp64 = false;
  DevBuf<double> d_w64;
  DevBuf<double> d_ds64;
  DevBuf<double> d_io64;               // dp staging (key order) / scratch
  DevBuf<double> d_cs_w64;
  DevBuf<double> d_cs_ds64;
  DevBuf<double> d_nsq64;              // |w|^2 of the loss
  DevBuf<unsigned long long> d_cs64_x; // exchange buffer of dsgd_cs64_step_kernel: [2][CS64_G][2 * CS_XSTRIDE] granules
  unsigned int cs64_tag0 = 0;
  DevBuf<double> d_cs_dl64;            // dsgd_async_step_f64: the update of the listed columns, slice-major [CS64_G][Sp]
  DevBuf<int> d_upd64_key;             // dsgd_update_grad_f64: the keys and values of a peer's update (grow-only)
  DevBuf<double> d_upd64_dv;
  // the row-parallel fp64 family (csrc/dsgd_rp64.hpp): [rp64_k][rp64_stride] fixed-point column sums, zero between calls
  // (grow-only), s of the call, the gradient in key order
  DevBuf<unsigned long long> d_rp64_acc;
  long long rp64_stride = 0;
  int rp64_k = 0;
  DevBuf<double> d_rp64_s;
  DevBuf<double> d_rp64_g;
  // ... across ranks (dsgd_comm_init_f64, dsgd_comm_init_f64v): the gather buffer ([world, padded][rp64_gk][rp64_gwords]
  // [rp64_gstride], zero between calls; csrc/dsgd_rp64_gather.hpp), the list ranges its header kernel writes for the finish,
  // the pinned words the ranks' worker counts and value types are read into, and whether the communicator was attached
  // through dsgd_comm_init_f64v (Double data accepted)
  DevBuf<unsigned long long> d_rp64_gath;
  long long rp64_gstride = 0;
  int rp64_gk = 0;
  int rp64_gwords = 0;
  bool comm_v64 = false;
  DevBuf<WorkSeg> d_rp64_gsegs;
  HostBuf<unsigned long long> h_rp64_ranks;
  // Double feature values (dsgd_load_csr_f64; csrc/dsgd_rp64.hpp): the values parallel to d_col / d_val (which holds them
  // rounded), and the low words of the two-word column sums ([rp64v_k][rp64_stride], zero between calls; the high words
  // are d_rp64_acc)
  DevBuf<double> d_val64;
  DevBuf<unsigned long long> d_rp64v_lo;
  int rp64v_k = 0;
  long long rp64v_stride = 0;
  // an epoch's steps in one call (dsgd_sync_steps_f64): the call's list ranges ([n_steps][K]) and per-step running active
  // counts, the fused step's arrival counter, whose bit 62 says that a launch gave up (a 16-byte block of its own: word 0), with
  // the pinned copy the host reads it into, the target the last fused launch was given, the bound of a workgroup's wait in ticks of the device's wall
  // clock, and how many workgroups of each fused kernel a compute unit holds (0: not asked yet)
  DevBuf<WorkSeg> d_rp64_ssegs;
  DevBuf<unsigned long long> d_rp64_cum;
  DevBuf<unsigned long long> d_rp64_sync;
  HostBuf<unsigned long long> h_rp64_sync;
  unsigned long long rp64_target = 0;
  unsigned long long rp64_wait_ticks = 0;
  int rp64_occ[2] = {0, 0};               // [0] dsgd_rp64_step_kernel, [1] dsgd_rp64v_step_kernel
  bool rp64_occ_known[2] = {false, false};
  // Sparse values at the boundary (csrc/dsgd_sparse.hpp): the compaction's output in host-mapped memory the kernel writes in
  // place ([2 words: count, gave up][dp keys][dp values of 8 bytes]), its scan state, and the staged pairs of a sparse setter
  HostBuf<unsigned long long> h_sp_out;
  DevBuf<unsigned long long> d_sp_state;
  unsigned long long sp_launches = 0;
  unsigned int sp_epoch = 0;
  Pinned pin_sp;
  DevBuf<char> d_sp_in;                  // [dp keys][dp values of 8 bytes]
  std::vector<unsigned int> sp_seen;        // key -> the stamp of the call that saw it last (the repeated-key check)
  unsigned int sp_stamp = 0;
  std::vector<int32_t> row_len;             // the loaded rows' lengths (the bound on an asynchronous step's delta)
  // The logistic model (csrc/dsgd_logistic.hpp): [lg_k][lg_stride] fixed-point column sums of its own, zero between calls
  // (grow-only; nothing is shared with the SVM's accumulators), the gradient in key order, the per-workgroup sums of |w|^2
  // (lg_finish_blocks words) followed by the evaluation's per-workgroup loss sums (n_cu words), an epoch's list ranges, the
  // probabilities.  bind_count numbers the entry points' binds: the |w|^2 words describe the resident weights while no other
  // entry point has bound since the logistic call that left them (lg_nsq_stamp: that call's number).
  // Across ranks (dsgd_comm_init_lg sets comm_lg; csrc/dsgd_lg_gather.hpp): d_lg_acc also holds, in front of the lg_k slots, the
  // agreement record of lg_world ranks and one header word per slot; h_lg_rec is the pinned copy of the record.
  DevBuf<unsigned long long> d_lg_acc;
  long long lg_stride = 0;
  int lg_k = 0;
  int lg_world = 1;
  bool comm_lg = false;
  HostBuf<long long> h_lg_rec;
  DevBuf<float> d_lg_g;
  DevBuf<double> d_lg_part;
  DevBuf<unsigned long long> d_lg_tally;   // dsgd_lg_loss_acc_ranges: [LG_MAX_RANGES][LG_TALLY_WORDS] class tallies, one set per range
  long long lg_pending_active = 0;         // rows of logistic plan runs since the last dsgd_synchronize (every row contributes)
  DevBuf<WorkSeg> d_lg_ssegs;
  DevBuf<float> d_lg_p;
  // Its asynchronous iteration (dsgd_lg_async_step, dsgd_lg_update_grad), grown on demand: the delta in rank order and, behind
  // it, in key order ([2][dp]); the keys and values of a peer's update
  DevBuf<double> d_lg_delta;
  DevBuf<int> d_lg_upd_key;
  DevBuf<double> d_lg_upd_dv;
  // Its distributed evaluation (csrc/dsgd_lg_eval.hpp: dsgd_lg_predict_ranges), grown on demand: the table's three arrays at
  // LG_PRED_MAX_RANGES ranges, the tallies [LG_PRED_MAX_RANGES][LG_TALLY_WORDS], one loss word per workgroup, the class bytes
  // (the probabilities go through d_lg_p; the |w|^2 words stay where dsgd_lg_loss_acc keeps them, in d_lg_part)
  DevBuf<long long> d_lg_pred_tab;
  DevBuf<unsigned long long> d_lg_pred_tally;
  DevBuf<double> d_lg_pred_part;
  DevBuf<signed char> d_lg_cls;
  // The job's evaluation across ranks (csrc/dsgd_lg_eval_job.hpp: dsgd_lg_eval_job): the gather record at LG_PRED_MAX_RANGES
  // positions, a buffer of its own (dropped after a collective that failed half way)
  DevBuf<unsigned long long> d_lge_rec;
  // Its column lists (csrc/dsgd_lg_cols.hpp): whole-split steps as coefficients + column-wise gradient + finish.  Per (row
  // ranges) configuration the device sorts the ranges' entries by (worker, column) once; at most eight configurations stay
  // cached (the least recently used one makes room), all dropped by a load.
  struct LgColsLayout {
    long long n_ent = 0;             // entries of the ranges' rows
    int share = 0, n_wg = 0;         // entries per workgroup of the gradient kernel, its workgroups
    DevBuf<uint2> d_ent;             // [n_wg * share] {x, position | first-of-column flag}
    DevBuf<TcShare> d_shares;
    DevBuf<int> d_slot_of_cid;       // compact id of a (worker, column) -> its word of d_lg_acc
    DevBuf<int> d_pos_base;          // [workers] where each worker's rows start in d_cq
    DevBuf<double> d_cq;             // the coefficients of the last step over these ranges, one per row
  };
  LayoutCache<LgColsLayout> lgc_cache;
  // Several topics (csrc/dsgd_lg_topics.hpp; dsgd_lg_topics_set): lgt_T label planes [T][n_rows] beside d_label, the topics'
  // weights [T][lgt_w_stride] in rank order beside d_w, their column sums [T][lgt_k][lgt_acc_stride] (zero between calls), the
  // |w_t|^2 and loss words (lgt_part_words), the tallies [T][LG_TALLY_WORDS], an epoch's list ranges, the probabilities.
  // lgt_gen: the layout the weights' rank order belongs to; lgt_nsq_stale: the |w_t|^2 words do not describe the weights.
  int lgt_T = 0, lgt_k = 0;
  long long lgt_gen = -1;
  bool lgt_nsq_stale = true;
  DevBuf<signed char> d_lgt_planes;
  DevBuf<float> d_lgt_w;
  DevBuf<unsigned long long> d_lgt_acc;
  DevBuf<double> d_lgt_part;
  DevBuf<unsigned long long> d_lgt_tally;
  DevBuf<WorkSeg> d_lgt_ssegs;
  DevBuf<float> d_lgt_p;
  unsigned long long bind_count = 0;
  unsigned long long lg_nsq_stamp = ~0ull - 1;
};

// what the route functions of csrc/dsgd_route.hpp need from the context
static RouteFacts route_facts(const dsgd_ctx* c) {
  RouteFacts f;
  f.dp = c->dp;
  f.n_rows = c->n_rows;
  f.n_cu = c->n_cu;
  f.hsplit = c->hsplit;
  f.cold_col16 = c->cold_col16;
  f.coldm_nnz = c->coldm_nnz;
  f.comm = c->comm != nullptr;
  f.prof = c->prof;
  f.fp64 = c->fp64;
  f.val64 = (bool)c->d_val64;
  f.async_running = c->async_running;
  return f;
}
static int check_ctx(dsgd_ctx* c) {
  if (!c) return fail(DSGD_EINVAL, "null context");
  return DSGD_OK;
}
static int cs_sp(int dp, int G) { return (((dp + G - 1) / G) + 4) & ~3; }   // padded columns per slice (as the kernel computes it)
// Consecutive column-slice launches keep the weights slice-major (a launch then loads and stores ONE contiguous piece per
// workgroup); whatever else touches w first gets them back in rank order.  Every entry point binds, under the context
// mutex: the one place.
static int cs_unslice(dsgd_ctx* c) {
  if (!c->cs_w_G) return DSGD_OK;
  if (c->fp64) {
    hipLaunchKernelGGL(dsgd_cs64_unslice_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, c->d_cs_w64, c->d_w64, c->dp,
                       cs64_sp(c->dp));
    HIP_TRY(hipGetLastError());
    c->cs_w_G = 0;
    return DSGD_OK;
  }
  hipLaunchKernelGGL(dsgd_cs_unslice_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, c->d_cs_w, c->d_w, c->dp, c->cs_w_G,
                     cs_sp(c->dp, c->cs_w_G));
  HIP_TRY(hipGetLastError());
  c->cs_w_G = 0;
  return DSGD_OK;
}
static int bind(dsgd_ctx* c, bool keep_sliced = false) {  // host threads migrate (JVM pool): bind the device on every call
  HIP_TRY(hipSetDevice(c->cfg.device));
  ++c->bind_count;   // (whatever binds may change w: the logistic model's cached |w|^2 is good for its own calls only)
  if (c->comm_broken && !c->comm_broken_ok)
    return fail(DSGD_ERCCL, "the context's communicator was aborted after a collective that not every rank joined: "
                            "dsgd_comm_destroy, then attach a new one (without it the replicas would silently diverge)");
  if (c->cs_w_G && !keep_sliced) return cs_unslice(c);
  return DSGD_OK;
}
template <typename V>
static CsrViewT<V> view_of(dsgd_ctx* c, const V* val) {
  CsrViewT<V> v;
  v.n_rows = c->n_rows;
  v.row_ptr = c->d_row_ptr;
  v.col = c->d_col;
  v.val = val;
  v.label = c->d_label;
  return v;
}
static CsrView view(dsgd_ctx* c) { return view_of(c, c->d_val.get()); }
static CsrView64 view64(dsgd_ctx* c) { return view_of(c, c->d_val64.get()); }   // (Double data loaded: dsgd_load_csr_f64)

// host -> device through a pinned buffer of the context: wait until the previous copy out of it has executed, then the
// caller fills it and enqueues the copy (pin_sent); device -> host: enqueue into pin_out, synchronise, copy out.
static int pin_acquire(dsgd_ctx::Pinned& b, size_t bytes) {
  if (b.armed) {
    HIP_TRY(hipEventSynchronize(b.ev));
    b.armed = false;
  }
  DSGD_TRY(b.p.reserve(std::max<size_t>(bytes, 4096)));
  if (!b.ev) HIP_TRY(hipEventCreateWithFlags(&b.ev.e, hipEventDisableTiming));
  return DSGD_OK;
}
static int pin_sent(dsgd_ctx::Pinned& b, hipStream_t on) {   // (owners other than a context: the dense object)
  HIP_TRY(hipEventRecord(b.ev, on));
  b.armed = true;
  return DSGD_OK;
}
static int pin_sent(dsgd_ctx* c, dsgd_ctx::Pinned& b, hipStream_t on = nullptr) { return pin_sent(b, on ? on : c->stream); }

static int ensure_g(dsgd_ctx* c, int n_workers) {
  const size_t n = (size_t)n_workers * c->dp;
  if (n <= c->d_g.cap() && n <= c->d_g64.cap()) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->d_g.reset();
  c->d_g64.reset();
  DSGD_TRY(c->d_g.alloc(n));
  DSGD_TRY(c->d_g64.alloc(n));
  HIP_TRY(hipMemsetAsync(c->d_g, 0, sizeof(float) * (size_t)n_workers * c->dp, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_g64, 0, sizeof(long long) * (size_t)n_workers * c->dp, c->stream));
  return DSGD_OK;
}
static int ensure_idx(dsgd_ctx* c, long long n) {
  if ((size_t)n <= c->d_idx.cap()) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return c->d_idx.reserve((size_t)n, Grow::twice);
}
// one int list through pin_idx into d_idx (ensure_idx came first; the caller says where cur_idx points)
static int send_idx(dsgd_ctx* c, const int32_t* idx, long long n) {
  DSGD_TRY(pin_acquire(c->pin_idx, sizeof(int) * (size_t)n));
  memcpy(c->pin_idx.p, idx, sizeof(int) * (size_t)n);
  HIP_TRY(hipMemcpyAsync(c->d_idx, c->pin_idx.p, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  return pin_sent(c, c->pin_idx);
}
static int ensure_segs(dsgd_ctx* c, int n) {
  if ((size_t)n <= c->d_segs.cap()) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->segs_last.clear();
  return c->d_segs.reserve((size_t)n);
}

// upload work segments; identical consecutive uploads (timed loops over the same ranges) are skipped
static int upload_segs(dsgd_ctx* c, const std::vector<WorkSeg>& segs) {
  const int n = (int)segs.size();
  DSGD_TRY(ensure_segs(c, n));
  if ((int)c->segs_last.size() == n && memcmp(c->segs_last.data(), segs.data(), sizeof(WorkSeg) * n) == 0) return DSGD_OK;
  // (ordered on the stream behind the launches that still read d_segs)
  DSGD_TRY(pin_acquire(c->pin_segs, sizeof(WorkSeg) * (size_t)n));
  memcpy(c->pin_segs.p, segs.data(), sizeof(WorkSeg) * (size_t)n);
  HIP_TRY(hipMemcpyAsync(c->d_segs, c->pin_segs.p, sizeof(WorkSeg) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_segs));
  c->segs_last = segs;
  return DSGD_OK;
}

// The cached layouts of the three gradient families (csrc/dsgd_layout_cache.hpp) go behind an idle launch stream: its
// kernels may still read them.  layout_room: before a family builds another one.  layouts_drop_all: THE place where they go
// when the rows or their ranking change (dsgd_load_csr, build_split), with the column lists' back-off, which counted misses
// over what went; dsgd_destroy leaves them to the members' destructors, every stream idle.
static auto stream_idle(dsgd_ctx* c) {
  return [c] { return hipStreamSynchronize(c->stream) == hipSuccess; };
}
template <class L>
static int layout_room(dsgd_ctx* c, LayoutCache<L>& cache) {
  if (cache.make_room(c->layout_gen, stream_idle(c))) return DSGD_OK;
  return fail(DSGD_EHIP, "hipStreamSynchronize(c->stream): %s", hipGetErrorString(hipGetLastError()));
}
// the packed copies of the split streams go where the streams go (build_split, reset_layout); the callers' stream is idle or
// about to be synchronised by layouts_drop_all
static void packed_drop(dsgd_ctx* c) {
  c->d_hcolf.reset(), c->d_hvaly.reset(), c->d_cvaly.reset();
  c->packed_state = 0;
  c->last_fstep_packed = false;
}
static void layouts_drop_all(dsgd_ctx* c) {
  c->fstep_cache.clear(stream_idle(c));
  c->tcol_cache.clear(stream_idle(c));
  c->lgc_cache.clear(stream_idle(c));
  c->tcol_gate.reset();
}

// per-block partial sums of w.ds and |w|^2 (fra_scalars): one pair per FRA_COLS columns
static int ensure_redpart(dsgd_ctx* c) {
  const int blocks = (c->dp + FRA_COLS - 1) / FRA_COLS;
  if (blocks <= c->redpart_cap) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->redpart_cap = 0;
  DSGD_TRY(c->d_redpart.alloc(4 * (size_t)blocks));   // two halves: see red_out
  c->redpart_cap = blocks;
  return DSGD_OK;
}

// The per-block pairs (w . ds, |w|^2) live in one of two halves of d_redpart: a kernel that writes new pairs takes
// the half the previous one did not (a lazy consumer may still be reading the old pairs in the same launch).
static float* red_cur(dsgd_ctx* c) { return c->d_redpart + (size_t)c->red_par * 2 * (size_t)c->redpart_cap; }
static float* red_out(dsgd_ctx* c) { return c->d_redpart + (size_t)(1 - c->red_par) * 2 * (size_t)c->redpart_cap; }

// s = 2*lambda*(w.ds) must match the resident w.  allow_lazy: the caller goes on to the fused reduce + update, which
// adds the pairs itself; everybody else gets the scalars finalised in DevScalars.
static int ensure_s(dsgd_ctx* c, bool allow_lazy = false) {
  const int blocks = (c->dp + FRA_COLS - 1) / FRA_COLS;
  if (c->s_dirty) {
    c->nsq_dirty = false;
    DSGD_TRY(ensure_redpart(c));
    // (the summation order of the fused step: equal weights give bit-equal s whichever kernel left it)
    hipLaunchKernelGGL(dsgd_wstats_cols_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_w, c->d_ds, c->dp,
                       (float)c->cfg.lambda, c->d_sc, red_out(c));
    HIP_TRY(hipGetLastError());
    c->red_par ^= 1;
    c->s_dirty = false;
    c->s_lazy = false;
    return DSGD_OK;
  }
  if (c->s_lazy && !allow_lazy) {
    hipLaunchKernelGGL(dsgd_scalars_finalize_kernel, dim3(1), dim3(64), 0, c->stream, red_cur(c), (unsigned int)blocks,
                       (float)c->cfg.lambda, c->d_sc);
    HIP_TRY(hipGetLastError());
    c->s_lazy = false;
  }
  return DSGD_OK;
}

static int read_scalars(dsgd_ctx* c) {
  HIP_TRY(hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DSGD_OK;
}
static int reset_counters(dsgd_ctx* c) {
  // err .. counts: everything after s_reg / wnorm2
  HIP_TRY(hipMemsetAsync((char*)c->d_sc.get() + offsetof(DevScalars, err), 0, sizeof(DevScalars) - offsetof(DevScalars, err),
                         c->stream));
  c->ctr_known = true;   // (until the next gradient launch)
  c->ctr_last = 0;
  c->job_pending = false;   // (n_samples is zero again: the rows of plan runs under a communicator no longer run on in it)
  return DSGD_OK;
}
static int check_err_flag(dsgd_ctx* c) {
  const int err = c->h_sc->err;
  if (err) {
    HIP_TRY(hipMemsetAsync(&c->d_sc->err, 0, sizeof(int), c->stream));
    // the abort word FIRST, whatever else is set: left raised it would end every later column-slice launch at its first poll
    if ((err & (8 | 16)) && c->d_cs_sync) HIP_TRY(hipMemsetAsync(c->d_cs_sync, 0, sizeof(unsigned int) * 2, c->stream));
    if (err & 2)
      return fail(DSGD_ESTATE, "fixed-point gradient accumulator left its safe band; the step is invalid");
    if (err & 16) return 1;   // (a per-request step beyond the one-step layout: nothing was applied -- its peers' 8 comes with it)
    if (err & 8)
      return fail(DSGD_ESTATE, "the column-slice kernel's exchange between its workgroups timed out; the run is invalid "
                               "(DSGD_CS=0 selects the row-parallel kernels)");
    if (err & 4)
      return fail(DSGD_ESTATE, "a small-batch plan was created for other data than is loaded now (its lists no longer fit "
                               "the staged sub-batch): create the plan again");
    return fail(DSGD_ERANGE, "sample index / key outside the loaded data");
  }
  return DSGD_OK;
}

static int grid_for(dsgd_ctx* c, long long items, int group) {
  const long long groups_per_block = 256 / group;
  long long blocks = (items + groups_per_block - 1) / groups_per_block;
  const long long cap = (long long)c->n_cu * 8;  // memory-bound: ~8 blocks of 256 per CU, grid-stride the rest
  return (int)std::max<long long>(1, std::min(blocks, cap));
}

// kind 0: the main gradient kernel, 1 / 2: the cold stream's dot / gradient pass (dsgd_cold_kernel)
static int prof_begin(dsgd_ctx* c, size_t* slot, int kind = 0) {
  if (!c->prof || (kind != 0 && c->prof_main_only)) {   // (a skipped bracket: prof_end ignores the slot)
    *slot = (size_t)-1;
    return DSGD_OK;
  }
  if (c->prof_used == c->prof_ev.size()) {
    Event a, b;
    HIP_TRY(hipEventCreate(&a.e));
    HIP_TRY(hipEventCreate(&b.e));
    c->prof_ev.emplace_back(std::move(a), std::move(b));
    c->prof_kind.push_back(0);
  }
  *slot = c->prof_used++;
  c->prof_kind[*slot] = kind;
  HIP_TRY(hipEventRecord(c->prof_ev[*slot].first, c->stream));
  return DSGD_OK;
}
static int prof_end(dsgd_ctx* c, size_t slot) {
  if (!c->prof || slot == (size_t)-1) return DSGD_OK;
  HIP_TRY(hipEventRecord(c->prof_ev[slot].second, c->stream));
  return DSGD_OK;
}
static int prof_collect(dsgd_ctx* c) {  // stream must be idle
  for (size_t i = 0; i < c->prof_used; ++i) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->prof_ev[i].first, c->prof_ev[i].second));
    const int k = c->prof_kind[i];
    c->prof_kms[k] += ms;
    c->prof_kn[k]++;
  }
  c->prof_used = 0;
  return DSGD_OK;
}

static int ensure_part(dsgd_ctx* c, DevBuf<int>& buf, long long* wgs, int* stride, long long need_wgs, int need_cols);

// Index-list batches spread over workgroups (dsgd_mb_grad_kernel): per-workgroup fixed-point partials, then the exact
// finish of the streaming path.  `allow_fused`: the caller goes on to launch_finish_sync (one hosted worker without
// peers then gets regulariser + update fused into the reduction); otherwise the sums land in d_g.
static int launch_grad_mb(dsgd_ctx* c, const int* d_idx, const WorkSeg* d_segs, int n_workers, long long max_items,
                          bool allow_fused) {
  const int hl = std::min(c->dp, MB_HL);
  const long long per_worker = std::max<long long>(1, c->n_cu / n_workers);
  long long rows_per_wg = std::max<long long>(64, (max_items + per_worker - 1) / per_worker);
  const long long wgs = std::max<long long>(1, (max_items + rows_per_wg - 1) / rows_per_wg);
  DSGD_TRY(ensure_part(c, c->d_part, &c->part_wgs, &c->part_stride, wgs * n_workers, hl));
  const int shift = 30 - rows_bits(rows_per_wg);   // at most one contribution per row and column: a workgroup's sums stay below 2^30
  c->last_shift = shift;
  MbArgs a;
  a.m = view(c);
  a.w = c->d_w;
  a.idx = d_idx;
  a.segs = d_segs;
  a.part = c->d_part;
  a.g64_base = c->d_g64;
  a.g_stride = c->dp;
  a.sc = c->d_sc;
  a.qscale = std::ldexp(1.0f, shift - c->vexp);
  a.part_stride = c->part_stride;
  a.rows_per_wg = (int)rows_per_wg;
  a.hl = hl;
  a.wl = std::min(MB_WL, c->dp) & ~255;   // whole 1 KiB pieces
  a.dp = c->dp;
  a.tprof = c->d_tprof;
  const size_t lds = sizeof(float) * (size_t)mb_lds_words(hl, a.wl);
  size_t slot = 0;
  DSGD_TRY(prof_begin(c, &slot));
  c->ctr_known = false;
  hipLaunchKernelGGL(dsgd_mb_grad_kernel, dim3((unsigned)wgs, n_workers), dim3(MB_THREADS), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  DSGD_TRY(prof_end(c, slot));
  c->last_grad_kernel = "dsgd_mb_grad_kernel";
  const double inv = 1.0 / (double)a.qscale;
  c->fused_apply_pending = false;
  if (allow_fused) {
    DSGD_TRY(ensure_redpart(c));
    // (no cold partials here: nc = 0, and hc only has to lie at or beyond D + 1 -- a multiple of 4 keeps the reduce on
    //  its 16-byte loads; with hc = D + 1 = 47,237 it fell back to 4-byte loads: 21.5 us for 25 MB of partials)
    c->fused_args = {hl, (int)wgs, (c->dp + 3) & ~3, 0, 0, inv, inv};
    c->fused_apply_pending = true;   // launched by launch_finish_sync, which knows lr
    return DSGD_OK;
  }
  hipLaunchKernelGGL(dsgd_fix_reduce_kernel, dim3((c->dp + 63) / 64, n_workers), dim3(1024), 0, c->stream, c->d_g64, c->d_g,
                     (long long)c->dp, c->dp, hl, c->d_part, c->part_stride, (int)wgs, c->dp, 0, (const int*)nullptr, 0, 0, inv, inv);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// ---- virtual tiles (dsgd_vt_grad_kernel) ---------------------------------------------------------------------
// Lay the lists of a plan out over the split streams: a row gets max(ceil(hot slots / 8), cold entries, 1) consecutive
// lanes of a 64-lane tile (whole rows per tile, every list starts a tile).  Not possible (vt_ok = false, the plan keeps
// using dsgd_mb_grad_kernel) when a row sits on the long-row list, holds more than 64 cold entries, or the streams are
// not in their 16-bit / 32-bit-addressable form.
// (returns 1 for a SOFT failure -- host or device memory for the layout could not be had: vt_build frees what was
//  allocated and the plan runs from dsgd_mb_grad_kernel, exactly as for lists the layout cannot hold)
#define VT_SOFT(expr)                 \
  do {                                \
    if ((expr) != hipSuccess) {       \
      (void)hipGetLastError();        \
      return 1;                       \
    }                                 \
  } while (0)
static int plan_host_idx(dsgd_ctx* c, dsgd_plan* p);
static void vt_drop(dsgd_plan* p) {
  p->d_vt_lanes.reset();
  p->d_vt_segs.reset();
  p->d_vt_long.reset();
  p->d_vt_packed.reset();
}
static int vt_build_impl(dsgd_ctx* c, dsgd_plan* p) {
  p->vt_layout = c->layout_gen;
  p->vt_ok = false;
  vt_drop(p);
  const int H = std::min(c->hsplit, c->dp);
  const long long n_lists = (long long)p->n_steps * p->n_workers;
  if (!c->cold_col16 || c->dp <= H || c->hot_nnz + WS_PAD >= (1LL << 32) || c->coldm_nnz + WS_PAD >= (1LL << 32)) return DSGD_OK;
  DSGD_TRY(plan_host_idx(c, p));
  if (c->h_hrp.size() != (size_t)c->n_rows + 1 || (long long)p->h_idx.size() != p->offsets[n_lists]) return DSGD_OK;
  if ((long long)c->h_ccol.size() != c->coldm_nnz) return DSGD_OK;
  const VtStreams m{c->n_rows, c->h_hrp.data(), c->h_ctp.data(), c->h_crow_ptr.data(), c->h_row_ptr.data(), c->h_label.data(), c->h_ccol.data()};
  VtTables T;
  const bool inside = vt_tables(p->h_idx.data(), p->offsets.data(), p->n_steps, p->n_workers, c->n_cu, c->k.vt_tpw, m, T);
  p->vt_off.swap(T.vt_off);
  if (!inside) return DSGD_OK;   // (the mb kernel reports the bad index)
  p->vt_grid.swap(T.grid);
  p->vt_gxt.swap(T.gxt);
  p->vt_shift.swap(T.shift);
  const std::vector<VtLane>& lanes = T.lanes;
  const std::vector<WorkSeg>& segs = T.segs;
  const std::vector<MbRec>& long_rows = T.long_rows;
  VT_SOFT(p->d_vt_lanes.try_alloc(std::max<size_t>(lanes.size(), 64)));
  VT_SOFT(p->d_vt_segs.try_alloc(segs.size()));
  VT_SOFT(p->d_vt_long.try_alloc(std::max<size_t>(long_rows.size(), 1)));
  HIP_TRY(hipMemcpy(p->d_vt_lanes, lanes.data(), sizeof(VtLane) * lanes.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_vt_segs, segs.data(), sizeof(WorkSeg) * segs.size(), hipMemcpyHostToDevice));
  if (!long_rows.empty())
    HIP_TRY(hipMemcpy(p->d_vt_long, long_rows.data(), sizeof(MbRec) * long_rows.size(), hipMemcpyHostToDevice));
  // small and mid-size plans get their own copy of the rows they touch, in tile order (dsgd_vt_pack_kernel): one
  // coalesced round trip per step instead of descriptors -> scattered rows
  const long long n_tiles = (long long)T.tile_rows.size();
  // (bounded by DSGD_VT_PACK_MB and by a quarter of the device memory that is free right now: a plan's copy must not be
  //  what makes the next allocation of the data path fail)
  size_t mem_free = 0, mem_total = 0;
  if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) {
    (void)hipGetLastError();
    mem_free = 0;
  }
  if (n_tiles > 0 && n_tiles * 4096 <= ((long long)c->k.vt_pack_mb << 20) && (size_t)n_tiles * 4096 <= mem_free / 4 &&
      p->d_vt_packed.try_alloc((size_t)n_tiles * (4096 / sizeof(uint4))) != hipSuccess)
    (void)hipGetLastError();      // (no room for the copy: the plan runs from its descriptors)
  if (p->d_vt_packed) {
    VtArgs a{};
    a.hcol = c->d_hcol;
    a.hval = c->d_hval;
    a.ccol = reinterpret_cast<const unsigned short*>(c->d_ccol.get());
    a.cval = c->d_cval;
    a.w = c->d_w;
    a.lanes = p->d_vt_lanes;
    a.hsplit = H;
    const long long blocks = (n_tiles + 3) / 4;   // four tiles (waves) per block
    hipLaunchKernelGGL(dsgd_vt_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, a, n_tiles, p->d_vt_packed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  p->vt_ok = true;
  return DSGD_OK;
}
#undef VT_SOFT
static int vt_build(dsgd_ctx* c, dsgd_plan* p) {
  int rc;
  try {
    rc = vt_build_impl(c, p);
  } catch (const std::bad_alloc&) {   // (160 bytes of host memory per listed row; nothing may unwind across the C ABI)
    rc = 1;
  }
  if (rc == 1) {
    vt_drop(p);
    p->vt_ok = false;   // (vt_layout is stamped: the plan keeps the row-wise kernel until the layout changes)
    return DSGD_OK;
  }
  return rc;
}

static int launch_grad_vt(dsgd_ctx* c, dsgd_plan* p, long long step) {
  const int H = std::min(c->hsplit, c->dp);
  const int gx = p->vt_grid[(size_t)step], shift = p->vt_shift[(size_t)step];
  DSGD_TRY(ensure_part(c, c->d_part, &c->part_wgs, &c->part_stride, (long long)gx * p->n_workers, H));
  c->last_shift = std::min(shift, c->cold_shift);   // (the cold lanes add at the cold scale)
  VtArgs a;
  a.hcol = c->d_hcol;
  a.hval = c->d_hval;
  a.ccol = reinterpret_cast<const unsigned short*>(c->d_ccol.get());
  a.cval = c->d_cval;
  a.w = c->d_w;
  a.lanes = p->d_vt_lanes;
  a.packed = p->d_vt_packed;
  a.tsegs = p->d_vt_segs + step * p->n_workers;
  a.lsegs = p->d_vt_segs + ((long long)p->n_steps + step) * p->n_workers;
  a.long_recs = p->d_vt_long;
  a.mfull = view(c);
  a.part = c->d_part;
  a.g64_base = c->d_g64;
  a.g_stride = c->dp;
  a.sc = c->d_sc;
  a.qscale = std::ldexp(1.0f, shift - c->vexp);
  a.cold_scale = c->fix_scale;
  a.part_stride = c->part_stride;
  a.hsplit = H;
  a.gx_tiles = p->vt_gxt[(size_t)step];
  const size_t lds = sizeof(float) * (size_t)(((H + 4) & ~3) + 16 * 64 + H + 64);
  size_t slot = 0;
  DSGD_TRY(prof_begin(c, &slot));
  c->ctr_known = false;
  if (a.packed) hipLaunchKernelGGL(dsgd_vt_grad_kernel<true>, dim3((unsigned)gx, p->n_workers), dim3(1024), lds, c->stream, a);
  else hipLaunchKernelGGL(dsgd_vt_grad_kernel<false>, dim3((unsigned)gx, p->n_workers), dim3(1024), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  DSGD_TRY(prof_end(c, slot));
  c->last_grad_kernel = "dsgd_vt_grad_kernel";
  DSGD_TRY(ensure_redpart(c));
  // hot ranks: the workgroups' partials at this launch's scale; cold ranks: the 64-bit accumulators at the cold scale
  c->fused_args = {H, gx, H, 0, 0, 1.0 / (double)a.qscale, 1.0 / (double)c->fix_scale};
  c->fused_apply_pending = true;
  return DSGD_OK;
}

// ---- column slices (dsgd_cs_step_kernel) ---------------------------------------------------------------------
// Lay the lists of a plan out per (slice, step): slice b holds the entries whose rank is b (mod G), a row's entries
// inside a slice in slots of <= CS_L.  Not possible (cs_ok = false, the plan keeps the row-parallel kernels) beyond
// CS_MAX_K hosted workers, for steps of more than CS_MAX_SLOTS rows or slots, when the slices do not fit LDS, or when the
// layout would exceed DSGD_CS_MAX_MB.  Returns 1 for a soft failure (memory): the caller frees and falls back.
#define CS_SOFT(expr)                 \
  do {                                \
    if ((expr) != hipSuccess) {       \
      (void)hipGetLastError();        \
      return 1;                       \
    }                                 \
  } while (0)
// the end of every plan: its cache blocks go back to the context behind whatever the launch stream still holds (an event per
// block), its virtual tiles with the object (the caller has idled the launch stream if it holds any).  (built_ev may still be
// pending on the build stream: destroying a recorded event is allowed, its resources go when it completes)
static void plan_release(dsgd_ctx* c, dsgd_plan* p) {
  c->plans.erase(std::remove(c->plans.begin(), c->plans.end(), p), c->plans.end());
  delete p;
}
// the host copy of a plan's lists: plans drawn on the device (dsgd_plan_create_from_seed) have none until a HOST builder
// (virtual tiles, DSGD_CS_HOST_LAYOUT=1) needs it
static int plan_host_idx(dsgd_ctx* c, dsgd_plan* p) {
  const long long n_lists = (long long)p->n_steps * p->n_workers;
  const long long n = p->offsets.empty() ? 0 : p->offsets[(size_t)n_lists];
  if ((long long)p->h_idx.size() == n || !p->d_idx) return DSGD_OK;
  if (p->built_pending && p->built_ev) HIP_TRY(hipEventSynchronize(p->built_ev));
  p->h_idx.resize((size_t)n);
  HIP_TRY(hipMemcpy(p->h_idx.data(), p->d_idx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  return DSGD_OK;
}
static int ensure_build_stream(dsgd_ctx* c) {
  if (!c->build_stream) HIP_TRY(hipStreamCreateWithFlags(&c->build_stream, hipStreamNonBlocking));
  return DSGD_OK;
}
// the arrays every column-slice launch shares: the exchange buffer and its abort word (each for itself: a failure between
// the two must not leave the first behind alone)
static int ensure_cs_exchange(dsgd_ctx* c) {
  if (!c->d_cs_x) {
    DevBuf<unsigned long long> x;
    const size_t n = (size_t)2 * CS_MAX_G * CS_XSTRIDE;
    if (x.try_alloc(n) != hipSuccess || hipMemset(x, 0, sizeof(unsigned long long) * n) != hipSuccess) {
      (void)hipGetLastError();
      return 1;
    }
    c->d_cs_x = std::move(x);
  }
  if (!c->d_cs_sync) {
    DevBuf<unsigned int> y;
    if (y.try_alloc(2) != hipSuccess || hipMemset(y, 0, sizeof(unsigned int) * 2) != hipSuccess) {
      (void)hipGetLastError();
      return 1;
    }
    c->d_cs_sync = std::move(y);
  }
  return DSGD_OK;
}
static int ensure_cs_max(dsgd_ctx* c) {
  DSGD_TRY(c->d_cs_max.reserve(4));
  DSGD_TRY(c->h_cs_max.reserve(4));
  return DSGD_OK;
}

// A plan's column slices laid out by the device (csrc/dsgd_cs.hpp: dsgd_cs_layout_kernel), on the build stream: pass 1
// counts (one read-back of four words: the strides), pass 2 fills.  Returns 1 for a soft failure (memory).
static int cs_build_device_impl(dsgd_ctx* c, dsgd_plan* p) {
  if (!c->layout_seen_by_build) {   // (once per column layout: the layout kernels read the ranked CSR the launch stream wrote)
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->layout_seen_by_build = true;
  }
  p->cs_free();
  p->cs_layout = c->layout_gen;
  p->cs_device_built = true;
  const int K = p->n_workers;
  const long long n_steps = p->n_steps, n_lists = n_steps * K;
  if (K > CS_MAX_K || p->max_step_rows > CS_MAX_SLOTS) return DSGD_OK;
  // (fp64: always CS64_G slices, the fp64 kernel's own LDS budget)
  // (a logistic plan: its own LDS budget, csrc/dsgd_lg_cs_host.hpp)
  const int G = p->lg ? lg_cs_pick_G(c->dp, K)
                      : c->fp64 ? ((K <= CS64_MAX_K && cs64_lds_bytes(c->dp, K) <= CS64_LDS_MAX && c->dp >= 4 * CS64_G) ? CS64_G : 0)
                                : cs_pick_G(c->k, route_facts(c), K, false);
  if (!G) return DSGD_OK;
  if (n_steps * (long long)G > 0x7fffffffLL) return DSGD_OK;
  if (!p->idx_trusted) {
    if ((long long)p->h_idx.size() != p->offsets[(size_t)n_lists]) return DSGD_OK;
    for (long long r : p->h_idx)
      if (r < 0 || r >= c->n_rows) return DSGD_OK;   // (the row-wise kernel reports the bad index)
  }
  p->cs_shift.assign((size_t)n_steps, 21);
  for (long long st = 0; st < n_steps; ++st) {
    long long worst_list = 1;
    for (int k = 0; k < K; ++k) worst_list = std::max(worst_list, p->offsets[(size_t)(st * K + k) + 1] - p->offsets[(size_t)(st * K + k)]);
    p->cs_shift[(size_t)st] = 30 - rows_bits(worst_list);   // at most one contribution per row and column: a worker's sums stay below 2^30
  }
  DSGD_TRY(ensure_build_stream(c));
  DSGD_TRY(ensure_cs_max(c));
  if (int rc = ensure_cs_exchange(c)) return rc;
  hipStream_t bs = c->build_stream;
  CsBuildArgs ba{};
  ba.m = view(c);
  ba.idx = p->d_idx;
  ba.segs = p->d_segs;
  ba.maxima = c->d_cs_max;
  ba.n_steps_plan = n_steps;
  ba.dp = c->dp;
  ba.G = G;
  ba.K = K;
  HIP_TRY(hipMemsetAsync(c->d_cs_max, 0, sizeof(unsigned int) * 4, bs));
  hipLaunchKernelGGL(dsgd_cs_layout_kernel<false>, dim3((unsigned)(n_steps * G)), dim3(CS_THREADS), 0, bs, ba);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->h_cs_max, c->d_cs_max, sizeof(unsigned int) * 4, hipMemcpyDeviceToHost, bs));
  HIP_TRY(hipStreamSynchronize(bs));
  const long long max_slots = std::max<long long>(1, c->h_cs_max[0]), max_cols = std::max<long long>(1, c->h_cs_max[1]);
  const long long max_rows = std::max<long long>(1, p->max_step_rows);
  if (c->h_cs_max[2] & 1u) return DSGD_OK;
  if (max_slots > CS_MAX_SLOTS || max_rows > CS_MAX_SLOTS || max_cols > (long long)CS_MAX_CLT * CS_THREADS) return DSGD_OK;
  const long long big = std::max(max_slots, max_rows);
  const bool one_fits = big <= CS_THREADS && max_cols <= 4 * CS_THREADS;                  // one slot per lane
  const bool narrow_fits = big <= 2 * CS_THREADS_NARROW && max_cols <= 8 * CS_THREADS_NARROW;
  const int slot_stride = (int)((max_slots + 63) / 64 * 64), row_stride = (int)((max_rows + 1 + 63) / 64 * 64);
  const int cl_stride = (int)((max_cols + CS_THREADS - 1) / CS_THREADS * CS_THREADS);
  const long long cells = (long long)G * n_steps;
  const long long bytes = cells * ((long long)slot_stride * (4 + CS_L * 2 + CS_L * 4) + (long long)row_stride * 2 + (long long)cl_stride * 2 + 8);
  if (bytes > ((long long)c->k.cs_max_mb << 20)) return DSGD_OK;
  // (a slot's CS_L columns are 16-bit, CS_L / 8 uint4; its values CS_L / 4 float4.  After a failure the blocks taken so
  // far stay with the plan: cs_build's cs_free hands them back)
  PlanCache& pc = c->plan_cache;
  DSGD_TRY(p->d_cs_hdr.take(pc, (size_t)cells));
  DSGD_TRY(p->d_cs_meta.take(pc, (size_t)(cells * slot_stride)));
  DSGD_TRY(p->d_cs_rf.take(pc, (size_t)(cells * row_stride)));
  DSGD_TRY(p->d_cs_col.take(pc, (size_t)(cells * slot_stride * (CS_L / 8))));
  DSGD_TRY(p->d_cs_val.take(pc, (size_t)(cells * slot_stride * (CS_L / 4))));
  DSGD_TRY(p->d_cs_cl.take(pc, (size_t)(cells * cl_stride)));
  ba.hdr = p->d_cs_hdr;
  ba.slot_meta = p->d_cs_meta;
  ba.row_first = p->d_cs_rf;
  ba.col = reinterpret_cast<unsigned short*>(p->d_cs_col.get());
  ba.val = reinterpret_cast<float*>(p->d_cs_val.get());
  ba.clist = p->d_cs_cl;
  ba.slot_stride = slot_stride;
  ba.row_stride = row_stride;
  ba.cl_stride = cl_stride;
  hipLaunchKernelGGL(dsgd_cs_layout_kernel<true>, dim3((unsigned)(n_steps * G)), dim3(CS_THREADS), 0, bs, ba);
  HIP_TRY(hipGetLastError());
  p->cs_G = G;
  p->cs_nt = (c->k.cs_nt == CS_THREADS_NARROW && narrow_fits && !c->fp64 && !p->lg) ? CS_THREADS_NARROW : CS_THREADS;
  p->cs_spl = (p->cs_nt == CS_THREADS && (p->lg ? big <= CS_THREADS : one_fits)) ? 1 : 2;   // (the logistic kernel reads no column list)
  p->cs_slot_stride = slot_stride;
  p->cs_row_stride = row_stride;
  p->cs_cl_stride = cl_stride;
  p->cs_ok = true;
  return DSGD_OK;
}
static int cs_build_impl(dsgd_ctx* c, dsgd_plan* p) {
  p->cs_free();
  p->cs_layout = c->layout_gen;
  p->cs_device_built = false;
  // (the lists were uploaded on the build stream: the gather below runs on the launch stream)
  if (p->built_pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  const int K = p->n_workers;
  const long long n_steps = p->n_steps, n_lists = n_steps * K;
  if (K > CS_MAX_K || p->max_step_rows > CS_MAX_SLOTS) return DSGD_OK;
  const int G = cs_pick_G(c->k, route_facts(c), K, false);   // (a wide model: narrower slices)
  if (!G) return DSGD_OK;
  DSGD_TRY(plan_host_idx(c, p));
  if (c->h_row_ptr.size() != (size_t)c->n_rows + 1 || (long long)p->h_idx.size() != p->offsets[n_lists]) return DSGD_OK;
  const long long N = p->offsets[n_lists];
  std::vector<long long> pre((size_t)N + 1);
  pre[0] = 0;
  for (long long t = 0; t < N; ++t) {
    const long long r = p->h_idx[(size_t)t];
    if (r < 0 || r >= c->n_rows) return DSGD_OK;   // (the row-wise kernel reports the bad index)
    pre[(size_t)t + 1] = pre[(size_t)t] + (c->h_row_ptr[(size_t)r + 1] - c->h_row_ptr[(size_t)r]);
  }
  const long long E = pre[(size_t)N];
  if (E > (64LL << 20)) return DSGD_OK;   // (the rows' entries pass through host memory once: 8 bytes each)
  // the listed rows' (rank, value) pairs: the ranked CSR lives on the device only
  std::vector<int> ecol((size_t)std::max<long long>(E, 1));
  std::vector<float> eval((size_t)std::max<long long>(E, 1));
  {
    DevBuf<long long> d_pre;   // (released at the end of this block, behind the synchronise)
    DevBuf<int> d_ecol;
    DevBuf<float> d_eval;
    hipError_t e = d_pre.try_alloc(pre.size());
    if (e == hipSuccess) e = d_ecol.try_alloc(ecol.size());
    if (e == hipSuccess) e = d_eval.try_alloc(eval.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_pre, pre.data(), sizeof(long long) * pre.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
      const int blocks = (int)std::max<long long>(1, std::min<long long>((N + 3) / 4, (long long)c->n_cu * 8));
      hipLaunchKernelGGL(dsgd_rows_gather_kernel, dim3(blocks), dim3(256), 0, c->stream, view(c), p->d_idx, N, d_pre, d_ecol, d_eval);
      e = hipGetLastError();
    }
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(ecol.data(), d_ecol, sizeof(int) * (size_t)E, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(eval.data(), d_eval, sizeof(float) * (size_t)E, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return 1;
    }
  }
  // pass 1: slots and distinct columns per (slice, step) -> the strides of the layout
  long long max_slots = 1, max_rows = 1, max_cols = 1;
  p->cs_shift.assign((size_t)n_steps, 21);
  {
    std::vector<int> cnt((size_t)G);
    std::vector<long long> seen((size_t)c->dp, -1);   // the last step that touched the rank
    for (long long s = 0; s < n_steps; ++s) {
      std::vector<long long> slots((size_t)G, 0), cols((size_t)G, 0);
      long long worst_list = 1;
      for (int k = 0; k < K; ++k) worst_list = std::max(worst_list, p->offsets[(size_t)(s * K + k) + 1] - p->offsets[(size_t)(s * K + k)]);
      for (long long t = p->offsets[(size_t)(s * K)]; t < p->offsets[(size_t)((s + 1) * K)]; ++t) {
        std::fill(cnt.begin(), cnt.end(), 0);
        for (long long e = pre[(size_t)t]; e < pre[(size_t)t + 1]; ++e) {
          const int rank = ecol[(size_t)e];
          ++cnt[(size_t)(rank % G)];
          if (seen[(size_t)rank] != s) {
            seen[(size_t)rank] = s;
            ++cols[(size_t)(rank % G)];
          }
        }
        for (int b = 0; b < G; ++b) slots[(size_t)b] += (cnt[(size_t)b] + CS_L - 1) / CS_L;
      }
      for (int b = 0; b < G; ++b) {
        max_slots = std::max(max_slots, slots[(size_t)b]);
        max_cols = std::max(max_cols, cols[(size_t)b]);
      }
      max_rows = std::max(max_rows, p->offsets[(size_t)((s + 1) * K)] - p->offsets[(size_t)(s * K)]);
      p->cs_shift[(size_t)s] = 30 - rows_bits(worst_list);   // at most one contribution per row and column: a worker's sums stay below 2^30
    }
  }
  if (max_slots > CS_MAX_SLOTS || max_rows > CS_MAX_SLOTS || max_cols > (long long)CS_MAX_CLT * CS_THREADS) return DSGD_OK;
  const long long big = std::max(max_slots, max_rows);
  const bool one_fits = big <= CS_THREADS && max_cols <= 4 * CS_THREADS;                  // one slot per lane
  const bool narrow_fits = big <= 2 * CS_THREADS_NARROW && max_cols <= 8 * CS_THREADS_NARROW;
  const int slot_stride = (int)((max_slots + 63) / 64 * 64), row_stride = (int)((max_rows + 1 + 63) / 64 * 64);
  const int cl_stride = (int)((max_cols + CS_THREADS - 1) / CS_THREADS * CS_THREADS);
  const long long cells = (long long)G * n_steps;
  const long long bytes = cells * ((long long)slot_stride * (4 + CS_L * 2 + CS_L * 4) + (long long)row_stride * 2 + (long long)cl_stride * 2 + 8);
  if (bytes > ((long long)c->k.cs_max_mb << 20)) return DSGD_OK;
  // pass 2: the layout
  std::vector<CsHdr> hdr((size_t)cells);
  std::vector<unsigned int> meta((size_t)(cells * slot_stride), 0u);
  std::vector<unsigned short> rf((size_t)(cells * row_stride), (unsigned short)0);
  std::vector<unsigned short> col((size_t)(cells * slot_stride * CS_L), (unsigned short)0);   // [cell][2 pieces][slot][8]
  std::vector<float> val((size_t)(cells * slot_stride * CS_L), 0.0f);                         // [cell][4 pieces][slot][4]
  std::vector<unsigned short> clist((size_t)(cells * cl_stride), (unsigned short)0xffffu);
  {
    std::vector<std::vector<std::pair<unsigned short, float>>> bucket((size_t)G);
    std::vector<std::vector<unsigned short>> touched((size_t)G);
    std::vector<long long> seen((size_t)c->dp, -1);
    for (long long s = 0; s < n_steps; ++s) {
      std::vector<int> cur((size_t)G, 0);
      for (auto& v : touched) v.clear();
      int r = 0;
      for (int k = 0; k < K; ++k) {
        for (long long t = p->offsets[(size_t)(s * K + k)]; t < p->offsets[(size_t)(s * K + k) + 1]; ++t, ++r) {
          for (auto& v : bucket) v.clear();
          for (long long e = pre[(size_t)t]; e < pre[(size_t)t + 1]; ++e) {
            const int rank = ecol[(size_t)e];
            bucket[(size_t)(rank % G)].emplace_back((unsigned short)(rank / G), eval[(size_t)e]);
            if (seen[(size_t)rank] != s) {
              seen[(size_t)rank] = s;
              touched[(size_t)(rank % G)].push_back((unsigned short)(rank / G));
            }
          }
          const unsigned short ypos = c->h_label[(size_t)p->h_idx[(size_t)t]] > 0 ? (unsigned short)0x8000u : (unsigned short)0;
          for (int b = 0; b < G; ++b) {
            const long long cell = (long long)b * n_steps + s;
            rf[(size_t)(cell * row_stride + r)] = (unsigned short)(cur[(size_t)b] | ypos);
            const auto& bk = bucket[(size_t)b];
            for (size_t j0 = 0; j0 < bk.size(); j0 += CS_L) {
              const long long slot = cell * slot_stride + cur[(size_t)b];
              meta[(size_t)slot] = (unsigned int)r | ((unsigned int)k << 16);
              const long long sl = cur[(size_t)b];
              for (size_t j = j0; j < std::min(bk.size(), j0 + CS_L); ++j) {
                const long long q = (long long)(j - j0);   // entry q of the slot: piece q / 8 of its columns, q / 4 of its values
                col[(size_t)((((cell * 2 + q / 8) * slot_stride) + sl) * 8 + q % 8)] = bk[j].first;
                val[(size_t)((((cell * 4 + q / 4) * slot_stride) + sl) * 4 + q % 4)] = bk[j].second;
              }
              ++cur[(size_t)b];
            }
          }
        }
      }
      for (int b = 0; b < G; ++b) {
        const long long cell = (long long)b * n_steps + s;
        rf[(size_t)(cell * row_stride + r)] = (unsigned short)cur[(size_t)b];   // the sentinel: one past the last row's slots
        hdr[(size_t)cell].counts = (unsigned int)cur[(size_t)b] | ((unsigned int)r << 16);
        hdr[(size_t)cell].shift = p->cs_shift[(size_t)s] | (int)((unsigned int)touched[(size_t)b].size() << 16);
        std::sort(touched[(size_t)b].begin(), touched[(size_t)b].end());
        std::copy(touched[(size_t)b].begin(), touched[(size_t)b].end(), clist.begin() + (size_t)(cell * cl_stride));
      }
    }
  }
  // (outside the cache: the synchronous copies below are not ordered behind a cached block's last reader)
  PlanCache& pc = c->plan_cache;
  CS_SOFT(p->d_cs_hdr.alloc_uncached(pc, hdr.size()));
  CS_SOFT(p->d_cs_meta.alloc_uncached(pc, meta.size()));
  CS_SOFT(p->d_cs_rf.alloc_uncached(pc, rf.size()));
  CS_SOFT(p->d_cs_col.alloc_uncached(pc, col.size() / 8));   // (uint4: eight 16-bit columns)
  CS_SOFT(p->d_cs_val.alloc_uncached(pc, val.size() / 4));   // (float4)
  CS_SOFT(p->d_cs_cl.alloc_uncached(pc, clist.size()));
  CS_SOFT(hipMemcpy(p->d_cs_cl, clist.data(), sizeof(unsigned short) * clist.size(), hipMemcpyHostToDevice));
  CS_SOFT(hipMemcpy(p->d_cs_hdr, hdr.data(), sizeof(CsHdr) * hdr.size(), hipMemcpyHostToDevice));
  CS_SOFT(hipMemcpy(p->d_cs_meta, meta.data(), sizeof(unsigned int) * meta.size(), hipMemcpyHostToDevice));
  CS_SOFT(hipMemcpy(p->d_cs_rf, rf.data(), sizeof(unsigned short) * rf.size(), hipMemcpyHostToDevice));
  CS_SOFT(hipMemcpy(p->d_cs_col, col.data(), sizeof(unsigned short) * col.size(), hipMemcpyHostToDevice));
  CS_SOFT(hipMemcpy(p->d_cs_val, val.data(), sizeof(float) * val.size(), hipMemcpyHostToDevice));
  if (ensure_cs_exchange(c)) return 1;
  p->cs_G = G;
  p->cs_nt = (c->k.cs_nt == CS_THREADS_NARROW && narrow_fits) ? CS_THREADS_NARROW : CS_THREADS;
  p->cs_spl = (p->cs_nt == CS_THREADS && one_fits) ? 1 : 2;
  p->cs_slot_stride = slot_stride;
  p->cs_row_stride = row_stride;
  p->cs_cl_stride = cl_stride;
  p->cs_ok = true;
  return DSGD_OK;
}
#undef CS_SOFT
static int cs_build(dsgd_ctx* c, dsgd_plan* p) {
  int rc;
  try {
    rc = (c->k.cs_host_layout && !c->fp64 && !p->lg) ? cs_build_impl(c, p) : cs_build_device_impl(c, p);
  } catch (const std::bad_alloc&) {   // (nothing may unwind across the C ABI)
    rc = 1;
  }
  if (rc != DSGD_OK) p->cs_free();   // (whatever the builder had taken when it gave up)
  return rc == 1 ? DSGD_OK : rc;    // (soft: cs_layout is stamped, the plan keeps the row-parallel kernels until the layout changes)
}

// the weights slice-major for G slices (they stay so until something else touches w: bind)
static int cs_ensure_sliced(dsgd_ctx* c, int G) {
  if (c->cs_w_G == G) return DSGD_OK;
  DSGD_TRY(cs_unslice(c));
  const int Sp = cs_sp(c->dp, G), n = G * Sp;
  const size_t cap = (size_t)(c->dp + (CS_MAX_G + 1) * 8);
  DSGD_TRY(c->d_cs_w.reserve(cap));
  DSGD_TRY(c->d_cs_ds.reserve(cap));
  hipLaunchKernelGGL(dsgd_cs_slice_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_w, c->d_cs_w, c->dp, G, Sp);
  hipLaunchKernelGGL(dsgd_cs_slice_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_ds, c->d_cs_ds, c->dp, G, Sp);
  HIP_TRY(hipGetLastError());
  c->cs_w_G = G;   // (dimSparsity can only change through an entry point that converts back first)
  return DSGD_OK;
}
// a step's granules carry the count of column-slice steps the context has launched: nothing to clear between launches
// (until the 32-bit count would wrap)
static int cs_take_tags(dsgd_ctx* c, unsigned long long n_launch, unsigned int* tag0) {
  if ((unsigned long long)c->cs_tag0 + n_launch + 1ull >= (1ull << 32)) {
    HIP_TRY(hipMemsetAsync(c->d_cs_x, 0, sizeof(unsigned long long) * 2 * CS_MAX_G * CS_XSTRIDE, c->stream));
    c->cs_tag0 = 0;
  }
  *tag0 = c->cs_tag0;
  c->cs_tag0 += (unsigned int)n_launch;
  return DSGD_OK;
}
static void cs_common_args(dsgd_ctx* c, CsArgs& a, int G, int K, float lr) {
  a.w = c->d_cs_w;
  a.ds = c->d_cs_ds;
  a.xbuf = c->d_cs_x;
  a.sync = c->d_cs_sync;
  a.sc = c->d_sc;
  a.tprof = c->d_tprof;
  a.lr = lr;
  a.lambda = (float)c->cfg.lambda;
  a.vexp = c->vexp;
  a.dp = c->dp;
  a.G = G;
  a.K = K;
  a.mail = nullptr;
  a.mail_seq = 0ull;
  a.gate_rec = nullptr;
  a.s_rec = nullptr;
  a.gate_words = 0;
  a.test_skip_publish = c->k.cs_test_skip;
}
static void cs_after_launch(dsgd_ctx* c, int shift) {
  c->last_grad_kernel = "dsgd_cs_step_kernel";
  c->last_shift = shift;
  c->fused_apply_pending = false;
  c->s_dirty = true;    // the kernel carries s = 2 lambda (w . ds) itself; whoever needs it next recomputes it from the weights
  c->s_lazy = false;
  c->nsq_dirty = false;
}

// the steps [step_begin, step_end) of a plan with column slices: ONE launch
static int launch_cs(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, float lr) {
  CsArgs a;
  a.hdr = p->d_cs_hdr;
  a.slot_meta = p->d_cs_meta;
  a.row_first = p->d_cs_rf;
  a.col = p->d_cs_col;
  a.val = p->d_cs_val;
  a.clist = p->d_cs_cl;
  a.cl_stride = p->cs_cl_stride;
  DSGD_TRY(cs_ensure_sliced(c, p->cs_G));
  cs_common_args(c, a, p->cs_G, p->n_workers, lr);
  a.n_steps_plan = p->n_steps;
  a.step_begin = step_begin;
  a.step_end = step_end;
  a.slot_stride = p->cs_slot_stride;
  a.row_stride = p->cs_row_stride;
  a.gate_rec = p->d_gate_rec;
  a.s_rec = p->d_s_rec;
  a.gate_words = p->gate_words;
  const size_t lds = sizeof(float) * (size_t)cs_lds_words(c->dp, a.G, a.K);
  DSGD_TRY(cs_take_tags(c, (unsigned long long)(step_end - step_begin), &a.tag0));
  size_t slot = 0;
  DSGD_TRY(prof_begin(c, &slot));
  c->ctr_known = false;
  if (p->cs_nt == CS_THREADS_NARROW)
    hipLaunchKernelGGL((dsgd_cs_step_kernel<CS_THREADS_NARROW, 2, 8>), dim3((unsigned)a.G), dim3(CS_THREADS_NARROW), lds, c->stream, a);
  else if (p->cs_spl == 1)
    hipLaunchKernelGGL((dsgd_cs_step_kernel<CS_THREADS, 1, 4>), dim3((unsigned)a.G), dim3(CS_THREADS), lds, c->stream, a);
  else
    hipLaunchKernelGGL((dsgd_cs_step_kernel<CS_THREADS, 2, 8>), dim3((unsigned)a.G), dim3(CS_THREADS), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  DSGD_TRY(prof_end(c, slot));
  cs_after_launch(c, p->cs_shift[(size_t)(step_end - 1)]);
  return DSGD_OK;
}

// A per-request step of the reference's sizes (<= CS_MAX_K hosted workers, <= CS_MAX_SLOTS rows; route_request): the lists staged
// by stage_lists (c->cur_idx, c->d_segs) go through dsgd_cs_request_kernel -- every slice lays its cell out and runs the step,
// ONE launch.
static int launch_cs_request(dsgd_ctx* c, int G, int K, long long worst_list, float lr) {
  dsgd_ctx::ReqLayout& L = c->req_layout;
  constexpr int SLOT_STRIDE = CS_MAX_SLOTS, ROW_STRIDE = CS_MAX_SLOTS + 64, CL_STRIDE = CS_MAX_CLT * CS_THREADS;
  if (L.G < G) {   // (grown once: 8 -> 16 slices)
    HIP_TRY(hipStreamSynchronize(c->stream));
    L = dsgd_ctx::ReqLayout();
    DSGD_TRY(L.hdr.alloc((size_t)G));
    DSGD_TRY(L.meta.alloc((size_t)G * SLOT_STRIDE));
    DSGD_TRY(L.rf.alloc((size_t)G * ROW_STRIDE));
    DSGD_TRY(L.col.alloc((size_t)G * SLOT_STRIDE * CS_L));
    DSGD_TRY(L.val.alloc((size_t)G * SLOT_STRIDE * CS_L));
    DSGD_TRY(L.cl.alloc((size_t)G * CL_STRIDE));
    L.G = G;
  }
  if (ensure_cs_exchange(c)) return fail(DSGD_ENOMEM, "out of device memory (column-slice exchange buffer)");
  DSGD_TRY(ensure_cs_max(c));
  DSGD_TRY(cs_ensure_sliced(c, G));
  CsArgs a;
  a.hdr = L.hdr;
  a.slot_meta = L.meta;
  a.row_first = L.rf;
  a.col = reinterpret_cast<const uint4*>(L.col.get());
  a.val = reinterpret_cast<const float4*>(L.val.get());
  a.clist = L.cl;
  a.cl_stride = CL_STRIDE;
  cs_common_args(c, a, G, K, lr);
  a.n_steps_plan = 1;
  a.step_begin = 0;
  a.step_end = 1;
  a.slot_stride = SLOT_STRIDE;
  a.row_stride = ROW_STRIDE;
  a.mail = c->h_mail.dev();
  a.mail_seq = ++c->mail_seq;
  CsBuildArgs ba{};
  ba.m = view(c);
  ba.idx = c->cur_idx;
  ba.segs = c->d_segs;
  ba.hdr = L.hdr;
  ba.slot_meta = L.meta;
  ba.row_first = L.rf;
  ba.col = L.col;
  ba.val = L.val;
  ba.clist = L.cl;
  ba.maxima = c->d_cs_max;   // (a request only ever raises flags here; nobody reads the maxima)
  ba.n_steps_plan = 1;
  ba.slot_stride = SLOT_STRIDE;
  ba.row_stride = ROW_STRIDE;
  ba.cl_stride = CL_STRIDE;
  ba.dp = c->dp;
  ba.G = G;
  ba.K = K;
  const size_t lds = sizeof(float) * (size_t)cs_req_lds_words(c->dp, G, K);
  DSGD_TRY(cs_take_tags(c, 1ull, &a.tag0));
  c->ctr_known = false;
  hipLaunchKernelGGL(dsgd_cs_request_kernel, dim3((unsigned)G), dim3(CS_THREADS), lds, c->stream, a, ba);
  HIP_TRY(hipGetLastError());
  cs_after_launch(c, 30 - rows_bits(worst_list));
  c->last_grad_kernel = "dsgd_cs_request_kernel";
  return DSGD_OK;
}

// gradient of n_workers index lists (or row ranges too small for the streaming kernels) living at d_segs (device);
// max_items = largest list
static int launch_grad(dsgd_ctx* c, const int* d_idx, const WorkSeg* d_segs, int n_workers, long long max_items,
                       bool allow_fused = false) {
  return launch_grad_mb(c, d_idx, d_segs, n_workers, max_items, allow_fused);
}

// regularise each hosted worker's sum, aggregate (locally and across ranks), update w -- in three parts, so that ONE host
// thread can drive several contexts (dsgd_sync_step_devices): every context's kernels in front of the collective are
// enqueued first, then all the all-reduces inside one ncclGroup, then the updates behind them.
//   finish_pre         without peers: the whole fused reduce + regularise + mean + update (nothing else follows);
//                      with peers: exact column sums + regulariser + sum over the hosted workers -> d_gsum
//   finish_collective  the synchronous master's Future.sequence + Vec.mean (ref: core/Master.scala:190-194) as ONE all-reduce
//                      of D+1 floats over xGMI, ordered on the same stream as the kernels around it
//   finish_post        w <- w - lr * sum / (workers x world), the next regulariser scalar
static int finish_pre(dsgd_ctx* c, int n_workers, float lr, bool mail) {
  const int dp = c->dp;
  const int cblocks = (dp + FRA_COLS - 1) / FRA_COLS;
  if (!c->fused_apply_pending) return fail(DSGD_ESTATE, "internal: no gradient partials pending");
  c->fused_apply_pending = false;
  const FusedArgs& f = c->fused_args;
  if (c->s_dirty) return fail(DSGD_ESTATE, "internal: regulariser scalar not prepared");
  if (!c->comm) {
    hipLaunchKernelGGL(dsgd_fix_reduce_apply_kernel<true>, dim3(cblocks), dim3(1024), 0, c->stream, c->d_g64, (long long)dp,
                       n_workers, c->d_w, c->d_ds, dp, f.hg, c->d_part, c->part_stride, f.n_wg, f.hc, f.nc, c->d_partc, c->partc_stride, f.n_wgc,
                       f.inv_scale, f.inv_scale_cold, lr, (float)c->cfg.lambda, c->d_sc, red_out(c), (float*)nullptr,
                       (const float*)red_cur(c), c->s_lazy ? 1 : 0, mail ? c->h_mail.dev() : (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    c->red_par ^= 1;
    c->s_lazy = true;   // the new pairs stay in d_redpart: the next step adds them itself, anyone else asks ensure_s
    c->s_dirty = false;
    return DSGD_OK;
  }
  hipLaunchKernelGGL(dsgd_fix_reduce_apply_kernel<false>, dim3(cblocks), dim3(1024), 0, c->stream, c->d_g64, (long long)dp,
                     n_workers, c->d_w, c->d_ds, dp, f.hg, c->d_part, c->part_stride, f.n_wg, f.hc, f.nc, c->d_partc, c->partc_stride, f.n_wgc,
                     f.inv_scale, f.inv_scale_cold, lr, (float)c->cfg.lambda, c->d_sc, red_out(c), c->d_gsum,
                     (const float*)red_cur(c), c->s_lazy ? 1 : 0, (unsigned long long*)nullptr);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
static int finish_collective(dsgd_ctx* c) {
  if (!c->comm) return DSGD_OK;
  RCCL_TRY(rccl::AllReduce(c->d_gsum, c->d_gsum, (size_t)c->dp, rccl::kFloat32, rccl::kSum, c->comm, c->stream));
  return DSGD_OK;
}
static int finish_post(dsgd_ctx* c, int n_workers, float lr) {
  if (!c->comm) return DSGD_OK;
  const int cblocks = (c->dp + FRA_COLS - 1) / FRA_COLS;
  const float k_total = (float)n_workers * (float)c->world;
  hipLaunchKernelGGL(dsgd_apply_cols_kernel, dim3(cblocks), dim3(256), 0, c->stream, c->d_w, c->d_gsum, c->d_ds, c->dp, k_total, lr,
                     (float)c->cfg.lambda, c->d_sc, red_out(c), 0);
  HIP_TRY(hipGetLastError());
  c->red_par ^= 1;
  c->s_lazy = true;
  c->s_dirty = false;
  return DSGD_OK;
}
static int launch_finish_sync(dsgd_ctx* c, int n_workers, float lr, bool mail = false) {
  DSGD_TRY(finish_pre(c, n_workers, lr, mail));
  DSGD_TRY(finish_collective(c));
  return finish_post(c, n_workers, lr);
}

// ---- column layout -------------------------------------------------------------------------------------
static int launch_permute_in(dsgd_ctx* c, const float* d_in, float* d_out) {
  hipLaunchKernelGGL(dsgd_permute_in_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_in, d_out, c->d_perm,
                     c->dp);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
static int launch_permute_out(dsgd_ctx* c, const float* d_in, float* d_out) {
  hipLaunchKernelGGL(dsgd_permute_out_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_in, d_out, c->d_perm,
                     c->dp);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
static int launch_promote64_in(dsgd_ctx* c, const float* d_in, double* d_out) {
  hipLaunchKernelGGL(dsgd_promote64_in_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_in, d_out, c->d_perm, c->dp);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
static int launch_round64_out(dsgd_ctx* c, const double* d_in, float* d_out) {
  hipLaunchKernelGGL(dsgd_round64_out_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_in, d_out, c->d_perm, c->dp);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
static int set_identity_perm(dsgd_ctx* c) {
  std::vector<int> id(c->dp);
  for (int j = 0; j < c->dp; ++j) id[j] = j;
  HIP_TRY(hipMemcpy(c->d_perm, id.data(), sizeof(int) * c->dp, hipMemcpyHostToDevice));
  return DSGD_OK;
}
// the fp64 weights and dimSparsity into ranked order (in = true) or back to key order, d_io64 as scratch
static int permute64_resident(dsgd_ctx* c, bool in) {
  double* v[2] = {c->d_w64, c->d_ds64};
  for (double* x : v) {
    if (in)
      hipLaunchKernelGGL(dsgd_permute64_in_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, x, c->d_io64, c->d_perm, c->dp);
    else
      hipLaunchKernelGGL(dsgd_permute64_out_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, x, c->d_io64, c->d_perm, c->dp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(x, c->d_io64, sizeof(double) * c->dp, hipMemcpyDeviceToDevice, c->stream));
  }
  return DSGD_OK;
}
static int count_columns(dsgd_ctx* c, long long nnz, unsigned int* d_cnt, bool features = false) {
  HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned int) * c->dp, c->stream));
  if (nnz > 0) {
    const int hcnt = std::min(c->dp, DSGD_LDS_FLOATS);
    const int blocks = (int)std::max<long long>(1, std::min<long long>((nnz + 4095) / 4096, c->n_cu));
    const size_t lds = sizeof(unsigned int) * hcnt;
    if (features && c->d_val64)   // dimSparsity's feature counts: abs(v) > 1e-20 on the Double (the ranking needs no more than the floats)
      hipLaunchKernelGGL(dsgd_colcount64v_kernel, dim3(blocks), dim3(1024), lds, c->stream, c->d_col, c->d_val64, nnz, d_cnt, c->dp, hcnt, c->d_sc);
    else
      hipLaunchKernelGGL(dsgd_colcount_kernel, dim3(blocks), dim3(1024), lds, c->stream, c->d_col, c->d_val, nnz, d_cnt, c->dp, hcnt, c->d_sc);
    HIP_TRY(hipGetLastError());
  }
  return DSGD_OK;
}

// ---- wave tiles (laid out by csrc/dsgd_layout_host.hpp: build_wave_tiles) ----------------------------------------
static int upload_wave_tiles(dsgd_ctx* c, HostTiles& ht) {
  c->d_wtiles.reset();
  c->d_wmeta.reset();
  c->d_wlong_rows.reset();
  c->n_wtiles = (long long)ht.r0.size() - 1;
  c->h_wtile_r0.swap(ht.r0);
  DSGD_TRY(c->d_wtiles.alloc(ht.wt.size()));
  const size_t meta_bytes = sizeof(unsigned short) * ht.meta16.size();
  DSGD_TRY(c->d_wmeta.alloc(ht.meta16.size()));
  HIP_TRY(hipMemcpy(c->d_wtiles, ht.wt.data(), sizeof(WTile) * ht.wt.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_wmeta, ht.meta16.data(), meta_bytes, hipMemcpyHostToDevice));
  c->bound_segs.clear();
  std::vector<int> lr(c->wlong_rows.begin(), c->wlong_rows.end());
  lr.push_back(0);
  DSGD_TRY(c->d_wlong_rows.alloc(lr.size()));
  HIP_TRY(hipMemcpy(c->d_wlong_rows, lr.data(), sizeof(int) * lr.size(), hipMemcpyHostToDevice));
  c->ssegs_last.clear();
  return DSGD_OK;
}

// split the ranked CSR into the hot stream (rank < hsplit) and the cold stream (rank - hsplit), both in row order with
// wave tiles of whole rows; rows whose hot or cold part exceeds a wave tile stay on the long-row list and in neither.
static int build_split(dsgd_ctx* c) {
  layouts_drop_all(c);   // (the chunked tile tables index the streams built here; the column lists are sorted by the ranks about to change)
  c->d_hcol.reset(), c->d_hval.reset(), c->d_hrow_ptr.reset();
  c->d_ccol.reset(), c->d_cval.reset(), c->d_ctp.reset(), c->d_ctiles.reset(), c->d_cmeta.reset();
  c->d_dcold.reset(), c->d_coef8.reset();
  packed_drop(c);
  const long long n_rows = c->n_rows;
  const int H = std::min(c->hsplit, c->dp);
  DSGD_TRY(c->d_coef8.alloc((size_t)std::max<long long>(n_rows, 1)));
  HIP_TRY(hipMemset(c->d_coef8, 0, (size_t)std::max<long long>(n_rows, 1)));
  DSGD_TRY(c->d_dcold.alloc((size_t)std::max<long long>(n_rows, 1)));
  HIP_TRY(hipMemset(c->d_dcold, 0, sizeof(float) * (size_t)std::max<long long>(n_rows, 1)));
  // cold entries per row
  DevBuf<int> d_cnt;
  DSGD_TRY(d_cnt.alloc((size_t)std::max<long long>(n_rows, 1)));
  CsrView m = view(c);
  {
    const int blocks = (int)std::max<long long>(1, std::min<long long>((n_rows + 15) / 16, (long long)c->n_cu * 16));
    hipLaunchKernelGGL(dsgd_split_count_kernel<16>, dim3(blocks), dim3(256), 0, c->stream, m, H, d_cnt);
  }
  std::vector<int> cnt((size_t)n_rows);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * (size_t)n_rows, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  d_cnt.reset();
  if (e != hipSuccess) return fail(DSGD_EHIP, "split counts: %s", hipGetErrorString(e));
  std::vector<long long>&hrp = c->h_hrp, &ctp = c->h_ctp;
  ++c->layout_gen;
  c->layout_seen_by_build = false;
  split_offsets(c->h_row_ptr, cnt, c->dp > H, hrp, ctp, c->h_crow_ptr, c->wlong_rows, c->wlong_weight);
  c->hot_nnz = hrp[n_rows];
  c->coldm_nnz = ctp[n_rows];
  DSGD_TRY(c->d_hcol.alloc((size_t)(c->hot_nnz + WS_PAD)));
  DSGD_TRY(c->d_hval.alloc((size_t)(c->hot_nnz + WS_PAD)));
  HIP_TRY(hipMemset(c->d_hcol + c->hot_nnz, 0, sizeof(unsigned short) * WS_PAD));
  HIP_TRY(hipMemset(c->d_hval + c->hot_nnz, 0, sizeof(float) * WS_PAD));
  DSGD_TRY(c->d_hrow_ptr.alloc(hrp.size()));
  HIP_TRY(hipMemcpy(c->d_hrow_ptr, hrp.data(), sizeof(long long) * hrp.size(), hipMemcpyHostToDevice));
  // 16-bit cold ids whenever there are at most 65536 cold columns (DSGD_COLD_UNPACKED=1 forces the 32-bit form: tests)
  c->cold_col16 = c->dp - H <= 65536 && !getenv("DSGD_COLD_UNPACKED");
  const size_t csz = c->cold_col16 ? sizeof(unsigned short) : sizeof(unsigned int);
  DSGD_TRY(c->d_ccol.alloc(csz * (size_t)(c->coldm_nnz + WS_PAD)));
  DSGD_TRY(c->d_cval.alloc((size_t)(c->coldm_nnz + WS_PAD)));
  HIP_TRY(hipMemset((char*)c->d_ccol.get() + csz * (size_t)c->coldm_nnz, 0, csz * WS_PAD));
  HIP_TRY(hipMemset(c->d_cval + c->coldm_nnz, 0, sizeof(float) * WS_PAD));
  DSGD_TRY(c->d_ctp.alloc(ctp.size()));
  HIP_TRY(hipMemcpy(c->d_ctp, ctp.data(), sizeof(long long) * ctp.size(), hipMemcpyHostToDevice));
  {
    const int blocks = (int)std::max<long long>(1, std::min<long long>((n_rows + 3) / 4, (long long)c->n_cu * 16));
    if (c->cold_col16)
      hipLaunchKernelGGL(dsgd_split_fill_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, m, H, c->d_hrow_ptr, c->d_ctp,
                         c->d_hcol, c->d_hval, c->d_ccol, c->d_cval);
    else
      hipLaunchKernelGGL(dsgd_split_fill_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, m, H, c->d_hrow_ptr, c->d_ctp,
                         c->d_hcol, c->d_hval, c->d_ccol, c->d_cval);
    HIP_TRY(hipGetLastError());
  }
  c->h_ccol.clear();
  if (c->cold_col16 && c->k.vt_enable && c->coldm_nnz > 0) {   // (75 MB for the 8.4 M-row shard)
    c->h_ccol.resize((size_t)c->coldm_nnz);
    HIP_TRY(hipMemcpyAsync(c->h_ccol.data(), c->d_ccol, sizeof(unsigned short) * (size_t)c->coldm_nnz, hipMemcpyDeviceToHost, c->stream));
  }
  HostTiles ht;
  build_wave_tiles(hrp.data(), n_rows, c->h_label.data(), ht);
  DSGD_TRY(upload_wave_tiles(c, ht));
  // the cold stream's own tiles (label signs unused there)
  HostTiles hc;
  build_wave_tiles(ctp.data(), n_rows, c->h_label.data(), hc, CT_MAXROWS);
  c->n_ctiles = (long long)hc.r0.size() - 1;
  c->h_ctile_r0.swap(hc.r0);
  DSGD_TRY(c->d_ctiles.alloc(hc.wt.size()));
  DSGD_TRY(c->d_cmeta.alloc(hc.meta16.size()));
  HIP_TRY(hipMemcpy(c->d_ctiles, hc.wt.data(), sizeof(WTile) * hc.wt.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_cmeta, hc.meta16.data(), sizeof(unsigned short) * hc.meta16.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the cold words' scale: the finest that keeps every word below the band the kernels refuse (cold_shift_for)
  c->cold_shift = FIX_SHIFT;
  if (c->n_ctiles > 0 && c->coldm_nnz > 0) {
    DSGD_TRY(c->d_bound.reserve(1));
    HIP_TRY(hipMemsetAsync(c->d_bound, 0, sizeof(unsigned int), c->stream));
    const int blocks = (int)std::max<long long>(1, std::min<long long>((c->n_ctiles + 3) / 4, (long long)c->n_cu * 32));
    hipLaunchKernelGGL(dsgd_cold_bound_kernel, dim3(blocks), dim3(CB_THREADS), 0, c->stream, c->d_ctiles, c->n_ctiles,
                       (const void*)c->d_ccol, c->cold_col16 ? 1 : 0, c->d_cval, c->coldm_nnz + WS_PAD,
                       std::ldexp(1.0f, FIX_SHIFT - c->vexp), c->d_bound);
    HIP_TRY(hipGetLastError());
    unsigned int amax = 0;
    HIP_TRY(hipMemcpyAsync(&amax, c->d_bound, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->cold_shift = cold_shift_for(amax);
  }
  c->fix_scale = std::ldexp(1.0f, c->cold_shift - c->vexp);
  return DSGD_OK;
}

// Rank the columns by how often they occur in the loaded rows (summed over ranks when a
// communicator is attached, so every replica uses the same order) and relabel the CSR columns.
// Runs once, lazily, at the first compute call after dsgd_load_csr.
// (in three parts -- the counts, their all-reduce, the ranking and the split -- so that one host thread can prepare several
//  contexts: dsgd_build_dim_sparsity_devices)
static int layout_begin(dsgd_ctx* c, DevBuf<unsigned int>& d_cnt) {   // (d_cnt stays empty when there is nothing to do)
  d_cnt.reset();
  if (c->layout_ready) return DSGD_OK;
  DSGD_TRY(d_cnt.alloc((size_t)c->dp));
  const int rc = count_columns(c, c->nnz, d_cnt);
  if (rc) d_cnt.reset();
  return rc;
}
static int layout_collective(dsgd_ctx* c, unsigned int* d_cnt) {
  if (!d_cnt || !c->comm) return DSGD_OK;
  int r = rccl::AllReduce(d_cnt, d_cnt, (size_t)c->dp, rccl::kUint32, rccl::kSum, c->comm, c->stream);
  if (r) return fail(DSGD_ERCCL, "ncclAllReduce(column counts): %s", rccl::GetErrorString(r));
  return DSGD_OK;
}
static int layout_finish(dsgd_ctx* c, DevBuf<unsigned int>& d_cnt) {   // (releases d_cnt)
  if (!d_cnt) return DSGD_OK;
  std::vector<unsigned int> cnt(c->dp);
  int rc = DSGD_OK;
  {
    hipError_t e = hipMemcpyAsync(cnt.data(), d_cnt, sizeof(unsigned int) * c->dp, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(DSGD_EHIP, "column counts: %s", hipGetErrorString(e));
  }
  d_cnt.reset();
  DSGD_TRY(rc);
  std::vector<int> order(c->dp);
  for (int j = 0; j < c->dp; ++j) order[j] = j;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cnt[a] > cnt[b]; });  // ties: ascending key
  std::vector<int> perm(c->dp);
  for (int r = 0; r < c->dp; ++r) perm[order[r]] = r;
  // bring the resident vectors (identity layout so far) into ranked order
  HIP_TRY(hipMemcpy(c->d_perm, perm.data(), sizeof(int) * c->dp, hipMemcpyHostToDevice));
  DSGD_TRY(launch_permute_in(c, c->d_w, c->d_tmp));
  HIP_TRY(hipMemcpyAsync(c->d_w, c->d_tmp, sizeof(float) * c->dp, hipMemcpyDeviceToDevice, c->stream));
  DSGD_TRY(launch_permute_in(c, c->d_ds, c->d_tmp));
  HIP_TRY(hipMemcpyAsync(c->d_ds, c->d_tmp, sizeof(float) * c->dp, hipMemcpyDeviceToDevice, c->stream));
  if (c->fp64) DSGD_TRY(permute64_resident(c, true));
  if (c->nnz > 0) {
    const int blocks = (int)std::min<long long>((c->nnz + 255) / 256, (long long)c->n_cu * 8);
    hipLaunchKernelGGL(dsgd_remap_cols_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_col, c->nnz, c->d_perm);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  DSGD_TRY(build_split(c));
  c->layout_ready = true;
  c->s_dirty = true;
  return DSGD_OK;
}
// fp64 across ranks: ONE vexp, the largest over the ranks' data (the fixed-point grid of every worker's sums and the
// finish that reads them).  ncclSum is the one reduction used anywhere here: a [world] vector with the own slot filled,
// summed, the maximum taken locally.  (The value stays when the communicator goes; dsgd_load_csr sets the data's own.)
static int vexp_collective(dsgd_ctx* c) {
  if (!c->comm || !c->fp64) return DSGD_OK;
  std::vector<long long> v((size_t)c->world, 0);
  v[(size_t)c->rank] = c->vexp;
  DevBuf<long long> d_v;
  DSGD_TRY(d_v.alloc(v.size()));
  hipError_t e = hipMemcpyAsync(d_v, v.data(), sizeof(long long) * v.size(), hipMemcpyHostToDevice, c->stream);
  int r = 0;
  if (e == hipSuccess) r = rccl::AllReduce(d_v, d_v, v.size(), rccl::kInt64, rccl::kSum, c->comm, c->stream);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(v.data(), d_v, sizeof(long long) * v.size(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && !r) e = hipStreamSynchronize(c->stream);
  d_v.reset();
  if (r) return fail(DSGD_ERCCL, "ncclAllReduce(vexp): %s", rccl::GetErrorString(r));
  if (e != hipSuccess) return fail(DSGD_EHIP, "vexp: %s", hipGetErrorString(e));
  c->vexp = (int)*std::max_element(v.begin(), v.end());
  c->fix_scale = std::ldexp(1.0f, c->cold_shift - c->vexp);
  return DSGD_OK;
}
static int prepare_layout(dsgd_ctx* c) {
  if (c->layout_ready) return DSGD_OK;
  DevBuf<unsigned int> d_cnt;
  DSGD_TRY(layout_begin(c, d_cnt));
  int rc = layout_collective(c, d_cnt);
  if (!rc) rc = vexp_collective(c);
  if (rc) return rc;
  return layout_finish(c, d_cnt);
}
// back to the identity layout (before new data is loaded): resident vectors return to key order
static int reset_layout(dsgd_ctx* c) {
  // (the snapshots of dsgd_async_check are in the rank order that goes; no engine runs here and the callers have
  //  synchronised the stream)
  c->d_snap[0].reset(), c->d_snap[1].reset();
  c->snap_last = c->snap_best = -1;
  packed_drop(c);   // (2.9 GB at 8.4 M rows: not kept while the next data is loaded)
  if (c->layout_ready) {
    DSGD_TRY(launch_permute_out(c, c->d_w, c->d_tmp));
    HIP_TRY(hipMemcpyAsync(c->d_w, c->d_tmp, sizeof(float) * c->dp, hipMemcpyDeviceToDevice, c->stream));
    DSGD_TRY(launch_permute_out(c, c->d_ds, c->d_tmp));
    HIP_TRY(hipMemcpyAsync(c->d_ds, c->d_tmp, sizeof(float) * c->dp, hipMemcpyDeviceToDevice, c->stream));
    if (c->fp64) DSGD_TRY(permute64_resident(c, false));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  DSGD_TRY(set_identity_perm(c));
  c->layout_ready = false;
  c->s_dirty = true;
  return DSGD_OK;
}

// ---- nnz-streaming launches (contiguous row ranges) ----------------------------------------------------
static int upload_ssegs(dsgd_ctx* c, const std::vector<StreamSeg>& segs) {
  const int n = (int)segs.size();
  if ((size_t)n > c->d_ssegs.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ssegs_last.clear();
    DSGD_TRY(c->d_ssegs.reserve((size_t)n));
  }
  if ((int)c->ssegs_last.size() == n && memcmp(c->ssegs_last.data(), segs.data(), sizeof(StreamSeg) * n) == 0) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(c->d_ssegs, segs.data(), sizeof(StreamSeg) * n, hipMemcpyHostToDevice));
  c->ssegs_last = segs;
  return DSGD_OK;
}
static StreamSeg make_sseg(long long rb, long long re) {
  StreamSeg s{};
  s.row_begin = rb;
  s.row_end = re;
  return s;
}
static int ensure_part(dsgd_ctx* c, DevBuf<int>& buf, long long* wgs, int* stride, long long need_wgs, int need_cols) {
  if (need_wgs <= *wgs && need_cols <= *stride) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  *wgs = std::max<long long>(need_wgs, c->n_cu);
  *stride = std::max(*stride, (need_cols + 63) / 64 * 64);
  return buf.alloc((size_t)*wgs * (size_t)*stride);
}

// whole row ranges: hot stream in wave tiles, cold stream before (x.w) and after (gradient) it
template <bool SCATTER>
static int launch_stream(dsgd_ctx* c, const std::vector<StreamSeg>& row_segs) {
  const int n_workers = (int)row_segs.size();
  std::vector<StreamSeg> segs(row_segs);
  long long max_tiles, max_long, max_ctiles;
  locate_segs(c->h_wtile_r0, c->h_ctile_r0, c->wlong_rows, segs, &max_tiles, &max_long, &max_ctiles);
  DSGD_TRY(upload_ssegs(c, segs));
  const int H = std::min(c->hsplit, c->dp);
  const int nc = c->dp - H;                                     // cold columns
  // ... of which in the LDS tile of the cold kernels (next to 16 strips and the gradient kernel's 64 dummy words)
  const int nc_lds = std::min(nc, DSGD_LDS_FLOATS - 16 * CT_STRIP - 64 - 4);
  const long long per_worker = std::max<long long>(1, c->n_cu / n_workers);
  dim3 gridc((unsigned)std::max<long long>(1, std::min(per_worker, (max_ctiles + 15) / 16)), n_workers);
  const bool cold = nc > 0 && max_ctiles > 0;
  const bool wide = nc > nc_lds;
  const size_t lds_cdot = sizeof(float) * (size_t)(((nc_lds + 3) & ~3) + 16 * CT_STRIP);
  const size_t lds_cgrad = sizeof(float) * (size_t)(((nc_lds + 64 + 3) & ~3) + 16 * CT_STRIP);
  if (cold) {
    size_t slot_c = 0;
    DSGD_TRY(prof_begin(c, &slot_c, 1));
#define DSGD_COLD_LAUNCH(C16, GR, WD, LDS)                                                                               \
  hipLaunchKernelGGL((dsgd_cold_kernel<C16, GR, WD>), gridc, dim3(1024), LDS, c->stream, c->d_ctiles, c->d_cmeta,      \
                     c->d_ccol, c->d_cval, c->d_ssegs, c->d_w, c->d_dcold, c->d_coef8, c->d_g64, (long long)c->dp, c->d_sc, \
                     H, nc_lds, c->fix_scale, c->d_partc, c->partc_stride)
#define DSGD_COLD_DISPATCH(GR, LDS)                                       \
  do {                                                                    \
    if (c->cold_col16 && !wide) DSGD_COLD_LAUNCH(true, GR, false, LDS);   \
    else if (c->cold_col16) DSGD_COLD_LAUNCH(true, GR, true, LDS);        \
    else if (!wide) DSGD_COLD_LAUNCH(false, GR, false, LDS);              \
    else DSGD_COLD_LAUNCH(false, GR, true, LDS);                          \
  } while (0)
    DSGD_COLD_DISPATCH(false, lds_cdot);
    HIP_TRY(hipGetLastError());
    DSGD_TRY(prof_end(c, slot_c));
  }
  long long bx = std::min(per_worker, std::max((max_tiles + 15) / 16, (max_long + 15) / 16));
  dim3 grid((unsigned)std::max<long long>(1, bx), n_workers);
  const int hw = H, hg = SCATTER ? H : 0;
  const size_t lds = sizeof(float) * (size_t)(16 * WS_COEF_STRIDE + hw + hg + (SCATTER ? 64 : 0) + 4);
  if (SCATTER) {
    DSGD_TRY(ensure_part(c, c->d_part, &c->part_wgs, &c->part_stride, (long long)grid.x * grid.y, hg));
    if (cold) DSGD_TRY(ensure_part(c, c->d_partc, &c->partc_wgs, &c->partc_stride, (long long)gridc.x * gridc.y, nc_lds));
  }
  // Fixed-point scale of THIS launch: a column receives at most one contribution per row, |contribution| <= 2^shift:
  // with rows(b) <= 2^bits for every workgroup b (stream_worst_rows), shift = 30 - bits keeps every 32-bit LDS sum below 2^30.
  float main_scale = c->fix_scale;
  if (SCATTER) {
    const long long worst = stream_worst_rows(segs, c->h_wtile_r0, grid.x);
    const int bits = rows_bits(worst);
    const int shift0 = std::max(1, std::min(c->k.max_shift, 30 - bits));   // safe for ANY data: rows x largest value
    int shift = shift0;
    if (c->k.fix_bound && shift0 < c->k.max_shift) {
      // data-dependent refinement (dsgd_wseg_bound_kernel): measured once per (ranges, grid) configuration
      const bool hit = c->bound_grid == grid.x && c->bound_segs.size() == segs.size() &&
                       memcmp(c->bound_segs.data(), segs.data(), sizeof(StreamSeg) * segs.size()) == 0;
      if (!hit) {
        DSGD_TRY(c->d_bound.reserve(1));
        HIP_TRY(hipMemsetAsync(c->d_bound, 0, sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(dsgd_wseg_bound_kernel, grid, dim3(1024), sizeof(unsigned int) * (size_t)(hg + 16), c->stream,
                           c->d_hrow_ptr, c->d_hcol, c->d_hval, c->d_wtiles, c->n_wtiles, c->n_rows, view(c),
                           c->d_wlong_rows, c->d_ssegs, hg, std::ldexp(1.0f, shift0 - c->vexp), c->d_bound);
        HIP_TRY(hipGetLastError());
        unsigned int amax = 0;
        HIP_TRY(hipMemcpyAsync(&amax, c->d_bound, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->bound_segs = segs;
        c->bound_grid = grid.x;
        c->bound_shift = refine_shift(shift0, c->k.max_shift, amax, worst);
      }
      shift = c->bound_shift;
    }
    main_scale = std::ldexp(1.0f, shift - c->vexp);
    c->last_shift = cold ? std::min(shift, c->cold_shift) : shift;   // (the coarser of the two grids of this launch)
  }
  CsrView mh = view(c);
  mh.row_ptr = c->d_hrow_ptr;
  mh.col = reinterpret_cast<const int*>(c->d_hcol.get());   // 16-bit ranks; the kernel reinterprets the pointer
  mh.val = c->d_hval;
  CsrView mf = view(c);
  size_t slot = 0;
  if (SCATTER) DSGD_TRY(prof_begin(c, &slot));
  c->ctr_known = false;
  hipLaunchKernelGGL(dsgd_wseg_kernel<SCATTER>, grid, dim3(1024), lds, c->stream, mh, mf, c->d_wtiles, c->d_wmeta, c->d_w,
                     c->d_g64, (long long)c->dp, c->d_ssegs, c->d_sc, hw, hg, main_scale, c->d_coef8, c->d_wlong_rows,
                     SCATTER ? c->d_part : nullptr, c->part_stride, c->d_dcold, c->fix_scale);
  HIP_TRY(hipGetLastError());
  if (SCATTER) DSGD_TRY(prof_end(c, slot));
  if (!SCATTER) return DSGD_OK;
  c->last_grad_kernel = "dsgd_wseg_kernel<true>";
  if (cold) {
    size_t slot_g = 0;
    DSGD_TRY(prof_begin(c, &slot_g, 2));
    DSGD_COLD_DISPATCH(true, lds_cgrad);
    HIP_TRY(hipGetLastError());
    DSGD_TRY(prof_end(c, slot_g));
  }
  // the exact column sums of every hosted worker go straight into regularise + sum (+ mean + update + next s when
  // there are no peers): g itself is never materialised
  DSGD_TRY(ensure_redpart(c));
  c->fused_args = {hg, (int)grid.x, H, cold ? nc_lds : 0, (int)gridc.x, 1.0 / (double)main_scale, 1.0 / (double)c->fix_scale};
  c->fused_apply_pending = true;   // launched by launch_finish_sync, which knows lr
  return DSGD_OK;
}

#include "dsgd_fstep_host.hpp"   // (the row chunks: fstep_layout, launch_fstep)
#include "dsgd_tcol_host.hpp"    // (the column lists: the (worker, column) sort, tcol_layout, launch_tcol)

static int hog_raise_stop(dsgd_ctx* c);

// small-batch steps as ONE persistent workgroup (dsgd_plan_kernel): eligible when no collective sits between the
// gradient and the update and a step is small enough for one CU
// does the list fit the staged sub-batch of dsgd_plan_kernel (at most PLAN_CAP rows and PLAN_CAP work items of 128
// non-zeros)?  Row lengths from the host copy of the internal row pointers.
static_assert(PLAN_STAGE_CAP == PLAN_CAP && PLAN_STAGE_CH == BT_CH, "csrc/dsgd_plan_check.hpp restates the staged sub-batch");
static const long long* host_row_ptr(const dsgd_ctx* c) {   // (NULL: no host copy of these rows)
  return c->h_row_ptr.size() == (size_t)c->n_rows + 1 ? c->h_row_ptr.data() : nullptr;
}
static bool list_fits_staged(const dsgd_ctx* c, const int32_t* idx, long long n) {
  return plan_list_fits_staged(host_row_ptr(c), c->n_rows, idx, n);
}
// A plan that outlived a load (include/dsgd.h, dsgd_load_csr): its lists are judged against the rows loaded NOW before they
// reach a kernel or a layout builder.  An index outside them: DSGD_ERANGE, nothing enqueued, the plan as it was (asked again
// at its next use, so a later load under which the lists fit lets it run).  Inside: the one-workgroup kernel's "fits" from
// the new row lengths, and the lists are no longer trusted unseen -- dsgd_cs_layout_kernel reads row_ptr[r] unchecked.
static int plan_revalidate(dsgd_ctx* c, dsgd_plan* p) {
  if (p->checked_load == c->load_gen) return DSGD_OK;
  const long long n_lists = (long long)p->n_steps * p->n_workers;
  DSGD_TRY(plan_host_idx(c, p));
  if ((long long)p->h_idx.size() != p->offsets[(size_t)n_lists]) return fail(DSGD_ESTATE, "internal: the plan's lists are not on the host");
  const PlanCheck v = plan_check_lists(p->h_idx.data(), p->offsets.data(), n_lists, host_row_ptr(c), c->n_rows);
  if (v.bad_at >= 0)
    return fail(DSGD_ERANGE, "the plan holds sample index %d (position %lld), outside the %lld rows loaded since it was made; nothing ran, "
                             "the plan runs again under data that holds its rows", p->h_idx[(size_t)v.bad_at], v.bad_at, c->n_rows);
  p->fits = v.fits && !p->drawn;
  p->fits_rows = c->n_rows;
  p->idx_trusted = false;
  p->checked_load = c->load_gen;
  return DSGD_OK;
}
static int launch_plan_kernel(dsgd_ctx* c, const int* d_idx, const WorkSeg* d_segs, long long step_begin,
                              long long step_end, float lr, bool mail = false) {
  if (!c->d_plan_gcold) {
    const size_t strip = (size_t)std::max(1, c->dp - plan_hl(c->dp));
    DSGD_TRY(c->d_plan_gcold.alloc(strip));
    HIP_TRY(hipMemsetAsync(c->d_plan_gcold, 0, sizeof(float) * strip, c->stream));
  }
  PlanArgs a;
  a.m = view(c);
  a.w = c->d_w;
  a.ds = c->d_ds;
  a.gcold = c->d_plan_gcold;
  a.idx = d_idx;
  a.segs = d_segs;
  a.sc = c->d_sc;
  a.step_begin = step_begin;
  a.step_end = step_end;
  a.lr = lr;
  a.lambda = (float)c->cfg.lambda;
  a.tprof = c->d_tprof;
  a.mail = mail ? c->h_mail.dev() : nullptr;
  a.mail_seq = mail ? ++c->mail_seq : 0ull;
  a.vexp = c->vexp;
  a.dp = c->dp;
  const size_t lds = sizeof(float) * (size_t)plan_lds_words(c->dp);
  size_t slot = 0;
  DSGD_TRY(prof_begin(c, &slot));
  // (every list fits the staged sub-batch: the callers checked the row lengths)
  c->ctr_known = false;
  hipLaunchKernelGGL(dsgd_plan_kernel, dim3(1), dim3(PLAN_THREADS), lds, c->stream, a);
  c->last_grad_kernel = "dsgd_plan_kernel";
  HIP_TRY(hipGetLastError());
  DSGD_TRY(prof_end(c, slot));
  c->s_lazy = false;
  c->s_dirty = false;     // the kernel leaves s = 2*lambda*(w . ds) of the weights it ends with ...
  c->nsq_dirty = true;    // ... but not |w|^2 (needed only by dsgd_loss_acc)
  return DSGD_OK;
}

static int require_data(dsgd_ctx* c) {
  if (!c->d_row_ptr) return fail(DSGD_ESTATE, "no data loaded (dsgd_load_csr)");
  return DSGD_OK;
}
// the synchronous entry points own w; they are refused while the lock-free engine is updating it
static int require_sync_mode(dsgd_ctx* c) {
  if (c->async_running) return fail(DSGD_ESTATE, "async computation running (dsgd_async_stop / dsgd_async_wait first)");
  return DSGD_OK;
}
static int require_ds(dsgd_ctx* c) {
  if (!c->have_ds) return fail(DSGD_ESTATE, "dimSparsity not set (dsgd_set_dim_sparsity / dsgd_build_dim_sparsity)");
  return DSGD_OK;
}

// the fp64 mode (DSGD_F_FP64) runs plans of column-slice steps, dsgd_sync_step, dsgd_forward and dsgd_loss_acc; every other
// entry point that would run an fp32 training kernel refuses an fp64 context and leaves its state as it is
static int refuse_fp64(dsgd_ctx* c, const char* what) {
  if (c && c->fp64)
    return fail(DSGD_EUNSUPPORTED, "%s is not available in an fp64 context (DSGD_F_FP64: plans of <= %d workers and <= %d rows per "
                                   "step, dsgd_sync_step, dsgd_forward, dsgd_loss_acc)", what, CS64_MAX_K, CS_MAX_SLOTS);
  return DSGD_OK;
}
static int refuse_fp64_all(dsgd_ctx* const* ctxs, int n, const char* what) {
  for (int i = 0; i < n; ++i) DSGD_TRY(refuse_fp64(ctxs[i], what));
  return DSGD_OK;
}

// ---- Sparse values at the boundary (csrc/dsgd_sparse.hpp; include/dsgd.h "SPARSE VALUES") ----
static size_t sp_vals_off(dsgd_ctx* c) { return 16 + ((sizeof(int) * (size_t)c->dp + 7) & ~(size_t)7); }
static int sp_tiles(dsgd_ctx* c) { return (c->dp + SP_TILE - 1) / SP_TILE; }
static int sp_reset_state(dsgd_ctx* c) {
  HIP_TRY(hipMemsetAsync(c->d_sp_state, 0, sizeof(unsigned long long) * (size_t)(SP_STATE_HEAD + sp_tiles(c)), c->stream));
  c->sp_launches = 0;
  c->sp_epoch = 0;
  c->h_sp_out[0] = 0;
  c->h_sp_out[1] = 0;
  return DSGD_OK;
}
static int sp_ensure(dsgd_ctx* c) {
  if (c->h_sp_out) return DSGD_OK;
  const size_t words = (sp_vals_off(c) + sizeof(double) * (size_t)c->dp + 7) / 8;
  DSGD_TRY(c->h_sp_out.alloc(words, hipHostMallocMapped));
  if (c->d_sp_state.try_alloc((size_t)(SP_STATE_HEAD + sp_tiles(c))) != hipSuccess) {
    c->h_sp_out.reset();   // (neither without the other: sp_ensure starts from h_sp_out)
    return fail(DSGD_ENOMEM, "out of memory (the sparse boundary's buffers)");
  }
  return sp_reset_state(c);
}
// enqueue the compaction of `in` (dp slots; perm == nullptr: already in key order) into the mapped buffer
template <typename TIn, typename TOut, bool REG>
static int sp_compact(dsgd_ctx* c, const TIn* in, const int* perm) {
  DSGD_TRY(sp_ensure(c));
  const int tiles = sp_tiles(c);
  if (++c->sp_epoch == 0) c->sp_epoch = 1;
  char* out = reinterpret_cast<char*>(c->h_sp_out.dev());
  hipLaunchKernelGGL((dsgd_sparse_compact_kernel<TIn, TOut, REG>), dim3(tiles), dim3(SP_THREADS), 0, c->stream, const_cast<TIn*>(in), perm, c->dp,
                     c->d_sc, c->d_sp_state, c->sp_launches * (unsigned long long)tiles, c->sp_epoch, reinterpret_cast<int*>(out + 16),
                     reinterpret_cast<TOut*>(out + sp_vals_off(c)), c->h_sp_out.dev());
  HIP_TRY(hipGetLastError());
  ++c->sp_launches;
  return DSGD_OK;
}
// behind the call's synchronisation: the count, and the pairs if they fit (otherwise the outputs stay as they are)
template <typename T>
static int sp_deliver(dsgd_ctx* c, int32_t* key_out, T* val_out, int64_t cap, int64_t* nnz_out) {
  if (c->h_sp_out[1]) {
    (void)sp_reset_state(c);
    (void)hipStreamSynchronize(c->stream);
    return fail(DSGD_ESTATE, "the compaction's scan across its workgroups timed out; nothing was delivered");
  }
  const int64_t nnz = (int64_t)c->h_sp_out[0];
  *nnz_out = nnz;
  if (nnz > cap) return fail(DSGD_EINVAL, "the Sparse value holds %lld entries, the output arrays %lld", (long long)nnz, (long long)cap);
  const char* out = reinterpret_cast<const char*>(c->h_sp_out.get());
  if (nnz > 0) {
    memcpy(key_out, out + 16, sizeof(int32_t) * (size_t)nnz);
    memcpy(val_out, out + sp_vals_off(c), sizeof(T) * (size_t)nnz);
  }
  return DSGD_OK;
}
static int sp_check_out(const void* key_out, const void* val_out, int64_t cap, const int64_t* nnz_out) {
  if (!nnz_out || cap < 0 || (cap > 0 && (!key_out || !val_out))) return fail(DSGD_EINVAL, "null output arrays / negative cap");
  return DSGD_OK;
}
// the keys of a Sparse value are host data: checked before anything moves (math/Sparse.scala:61-68 accepts 0..size; a map
// holds a key once).  nnz < 0 ("the resident weights") passes.
static int sp_check_keys(dsgd_ctx* c, const int32_t* key, const void* val, int64_t nnz) {
  if (nnz <= 0) return DSGD_OK;
  if (!key || !val) return fail(DSGD_EINVAL, "null key / value arrays");
  for (int64_t i = 0; i < nnz; ++i)
    if (key[i] < 0 || key[i] >= c->dp) return fail(DSGD_ERANGE, "key %d at position %lld outside [0, %d]", key[i], (long long)i, c->dp - 1);
  if (nnz > c->dp) return fail(DSGD_EINVAL, "%lld keys for %d slots: a Sparse value has unique keys", (long long)nnz, c->dp);
  if (c->sp_seen.size() != (size_t)c->dp) c->sp_seen.assign((size_t)c->dp, 0u);
  if (++c->sp_stamp == 0) {
    std::fill(c->sp_seen.begin(), c->sp_seen.end(), 0u);
    c->sp_stamp = 1;
  }
  for (int64_t i = 0; i < nnz; ++i) {
    if (c->sp_seen[(size_t)key[i]] == c->sp_stamp)
      return fail(DSGD_EINVAL, "key %d repeated at position %lld: a Sparse value has unique keys", key[i], (long long)i);
    c->sp_seen[(size_t)key[i]] = c->sp_stamp;
  }
  return DSGD_OK;
}
// w (rank order, dp slots) <- the checked pairs, 0 elsewhere; the caller may reuse its arrays when this returns
template <typename TIn, typename TW>
static int sp_scatter(dsgd_ctx* c, const int32_t* key, const TIn* val, int64_t nnz, TW* w) {
  const size_t voff = (sizeof(int) * (size_t)c->dp + 7) & ~(size_t)7;
  DSGD_TRY(c->d_sp_in.reserve(voff + sizeof(double) * (size_t)c->dp));
  if (nnz > 0) {
    const size_t vo = (sizeof(int) * (size_t)nnz + 7) & ~(size_t)7;
    DSGD_TRY(pin_acquire(c->pin_sp, vo + sizeof(TIn) * (size_t)nnz));
    char* p = static_cast<char*>(c->pin_sp.p.get());
    memcpy(p, key, sizeof(int) * (size_t)nnz);
    memcpy(p + vo, val, sizeof(TIn) * (size_t)nnz);
    HIP_TRY(hipMemcpyAsync(c->d_sp_in, p, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_sp_in + voff, p + vo, sizeof(TIn) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
    DSGD_TRY(pin_sent(c, c->pin_sp));
  }
  const int blocks = std::max(1, std::min(SP_SCATTER_BLOCKS, (c->dp + SP_TILE - 1) / SP_TILE));
  hipLaunchKernelGGL((dsgd_sparse_scatter_kernel<TIn, TW>), dim3(blocks), dim3(SP_THREADS), 0, c->stream, reinterpret_cast<const int*>(c->d_sp_in.get()),
                     reinterpret_cast<const TIn*>(c->d_sp_in + voff), (int)std::max<int64_t>(nnz, 0), c->d_perm, w, c->dp);
  HIP_TRY(hipGetLastError());
  c->s_dirty = true;
  return DSGD_OK;
}
// An asynchronous step changes the weights, so its delta must fit BEFORE it runs.  The delta's support lies inside the
// union of the listed rows' columns (the regulariser is support-only, math/Vec.scala:65-75): at most
// min(D + 1, the listed rows' lengths summed) entries.  The rows are host data: one outside the loaded rows is DSGD_ERANGE here.
static int sp_async_cap(dsgd_ctx* c, const int32_t* idx, int64_t n, int64_t cap) {
  long long bound = 0;
  for (int64_t t = 0; t < n; ++t) {
    if (idx[t] < 0 || idx[t] >= c->n_rows) return fail(DSGD_ERANGE, "sample index %d outside the %lld loaded rows", idx[t], c->n_rows);
    if (bound < c->dp) bound += c->row_len[(size_t)idx[t]];
  }
  bound = std::min<long long>(bound, c->dp);
  if (cap < bound)
    return fail(DSGD_EINVAL, "cap = %lld is below the bound on this step's delta, min(D + 1, the listed rows' lengths summed) = %lld: "
                             "nothing ran", (long long)cap, bound);
  return DSGD_OK;
}

extern "C" {

int dsgd_abi_version(void) { return DSGD_ABI_VERSION; }
const char* dsgd_last_error(void) { return g_err; }

int dsgd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
  }
  return ok;
}

int dsgd_create(const dsgd_config* cfg, dsgd_ctx** out) {
  if (!cfg || !out) return fail(DSGD_EINVAL, "null argument");
  if (cfg->n_features < 1) return fail(DSGD_EINVAL, "n_features must be >= 1");
  if (!(cfg->lambda == cfg->lambda)) return fail(DSGD_EINVAL, "lambda is NaN");
  if (cfg->flags & ~DSGD_F_FP64) return fail(DSGD_EINVAL, "unknown flags 0x%x (only DSGD_F_FP64 is defined)", cfg->flags);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(DSGD_EUNSUPPORTED, "no HIP device visible: libdsgd_hip has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= n) return fail(DSGD_EINVAL, "device %d out of range (%d devices)", cfg->device, n);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(DSGD_EUNSUPPORTED, "device %d is %s; this library is built for gfx950 only", cfg->device, prop.gcnArchName);
  dsgd_ctx* c = new (std::nothrow) dsgd_ctx();
  if (!c) return fail(DSGD_ENOMEM, "out of host memory");
  c->plan_cache.launch = &c->stream;
  c->plan_cache.build = &c->build_stream;
  c->cfg = *cfg;
  c->dp = cfg->n_features + 1;
  c->n_cu = prop.multiProcessorCount;
  c->fp64 = (cfg->flags & DSGD_F_FP64) != 0;
  auto bail = [&](int rc) {
    dsgd_destroy(c);
    return rc;
  };
#define HIP_TRY_B(expr)                                                                               \
  do {                                                                                                \
    hipError_t e__ = (expr);                                                                          \
    if (e__ != hipSuccess) return bail(fail(DSGD_EHIP, "%s: %s", #expr, hipGetErrorString(e__)));     \
  } while (0)
#define DSGD_TRY_B(expr)              \
  do {                                \
    const int rc__ = (expr);          \
    if (rc__ != DSGD_OK) return bail(rc__); \
  } while (0)
  HIP_TRY_B(hipSetDevice(cfg->device));
  HIP_TRY_B(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  DSGD_TRY_B(c->d_w.alloc((size_t)c->dp + 1));  // + the zero slot w[dp] of the wseg kernels
  HIP_TRY_B(hipMemsetAsync(c->d_w + c->dp, 0, sizeof(float), c->stream));
  DSGD_TRY_B(c->d_ds.alloc((size_t)c->dp));
  DSGD_TRY_B(c->d_gsum.alloc((size_t)c->dp));
  DSGD_TRY_B(c->d_tmp.alloc((size_t)c->dp));
  DSGD_TRY_B(c->d_io.alloc((size_t)c->dp));
  DSGD_TRY_B(c->d_perm.alloc((size_t)c->dp));
  DSGD_TRY_B(c->d_sc.alloc(1));
  DSGD_TRY_B(c->h_sc.alloc(1));
  DSGD_TRY_B(c->h_mail.alloc(4, hipHostMallocMapped));
  c->h_mail[0] = c->h_mail[1] = c->h_mail[2] = c->h_mail[3] = 0;
  HIP_TRY_B(hipMemsetAsync(c->d_w, 0, sizeof(float) * c->dp, c->stream));
  HIP_TRY_B(hipMemsetAsync(c->d_ds, 0, sizeof(float) * c->dp, c->stream));
  HIP_TRY_B(hipMemsetAsync(c->d_gsum, 0, sizeof(float) * c->dp, c->stream));
  HIP_TRY_B(hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), c->stream));
  DSGD_TRY_B(ensure_g(c, 1));
  DSGD_TRY_B(set_identity_perm(c));
  c->hw_eval = std::min(c->dp, DSGD_LDS_FLOATS);
  knobs_read(c->k, getenv);   // every switch, once (csrc/dsgd_route.hpp: the table)
  c->plan_cache.cache_cap = (size_t)c->k.cache_mb << 20;
  {   // the fused step's wait is bounded in wall-clock time: 2 s of the device's constant-rate clock (kHz; 100 MHz where unknown)
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, cfg->device) != hipSuccess || khz <= 0) khz = 100000;
    c->rp64_wait_ticks = (unsigned long long)khz * 2000ull;
  }
  if (c->k.plan_prof) {
    // (16 counters + four words per workgroup of the chunked launch's LAST run: start, end, cycles in the hot tiles, XCC id)
    DSGD_TRY_B(c->d_tprof.alloc(16 + 4 * 1024));
    HIP_TRY_B(hipMemsetAsync(c->d_tprof, 0, sizeof(unsigned long long) * (16 + 4 * 1024), c->stream));
  }
  c->hsplit = std::max(1, std::min(c->k.hsplit, HSPLIT_MAX));   // (< 65536: 16-bit ranks)
  if (c->hsplit >= 8) c->hsplit &= ~3;   // 16-byte aligned tile boundaries: the LDS tiles are staged / written back in 16-byte pieces
  const int lds_max = DSGD_LDS_FLOATS * (int)sizeof(float);
#define DSGD_ATTR(fn) HIP_TRY_B(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max))
  DSGD_ATTR(dsgd_eval_kernel<64>);
  DSGD_ATTR(dsgd_eval_kernel<32>);
  DSGD_ATTR(dsgd_eval_kernel<16>);
  DSGD_ATTR(dsgd_eval_kernel<8>);
  DSGD_ATTR(dsgd_predict_kernel<64>);
  DSGD_ATTR(dsgd_predict_kernel<32>);
  DSGD_ATTR(dsgd_predict_kernel<16>);
  DSGD_ATTR(dsgd_predict_kernel<8>);
  DSGD_ATTR(dsgd_eval_list_kernel<64>);
  DSGD_ATTR(dsgd_eval_list_kernel<32>);
  DSGD_ATTR(dsgd_eval_list_kernel<16>);
  DSGD_ATTR(dsgd_eval_list_kernel<8>);
  DSGD_ATTR(dsgd_lg_predict_ranges_kernel);
  DSGD_ATTR(dsgd_lg_eval_list_kernel);
  DSGD_ATTR(dsgd_lg_topics_eval_kernel);
  DSGD_ATTR(dsgd_colcount_kernel);
  DSGD_ATTR((dsgd_hogwild_kernel<false, false>));
  DSGD_ATTR((dsgd_hogwild_kernel<true, false>));
  DSGD_ATTR((dsgd_hogwild_kernel<false, true>));
  DSGD_ATTR((dsgd_hogwild_kernel<true, true>));
  DSGD_ATTR(dsgd_mb_grad_kernel);
  DSGD_ATTR(dsgd_vt_grad_kernel<true>);
  DSGD_ATTR(dsgd_vt_grad_kernel<false>);
  DSGD_ATTR(dsgd_plan_kernel);
  DSGD_ATTR((dsgd_cs_step_kernel<CS_THREADS, 1, 4>));
  DSGD_ATTR((dsgd_cs_step_kernel<CS_THREADS, 2, 8>));
  DSGD_ATTR((dsgd_cs_step_kernel<CS_THREADS_NARROW, 2, 8>));
  DSGD_ATTR((dsgd_lg_cs_step_kernel<1>));
  DSGD_ATTR((dsgd_lg_cs_step_kernel<2>));
  DSGD_ATTR(dsgd_wseg_kernel<true>);
  DSGD_ATTR(dsgd_wseg_kernel<false>);
  DSGD_ATTR(dsgd_wseg_bound_kernel);
  DSGD_ATTR(dsgd_fstep_kernel<false>);
  DSGD_ATTR(dsgd_fstep_kernel<true>);
  DSGD_ATTR(dsgd_fstep_bound_kernel);
  if (c->fp64) {   // the fp64 state (csrc/dsgd_cs64.hpp)
    DSGD_TRY_B(c->d_w64.alloc((size_t)c->dp));
    DSGD_TRY_B(c->d_ds64.alloc((size_t)c->dp));
    DSGD_TRY_B(c->d_io64.alloc((size_t)c->dp));
    DSGD_TRY_B(c->d_nsq64.alloc(1));
    HIP_TRY_B(hipMemsetAsync(c->d_w64, 0, sizeof(double) * c->dp, c->stream));
    HIP_TRY_B(hipMemsetAsync(c->d_ds64, 0, sizeof(double) * c->dp, c->stream));
    DSGD_ATTR((dsgd_cs64_step_kernel<CS_THREADS, 1, 4>));
    DSGD_ATTR((dsgd_cs64_step_kernel<CS_THREADS, 2, 8>));
    DSGD_ATTR((dsgd_cs64_async_kernel<CS_THREADS, 1, 4>));
    DSGD_ATTR((dsgd_cs64_async_kernel<CS_THREADS, 2, 8>));
    DSGD_ATTR(dsgd_colcount64v_kernel);
  }
  {   // the column lists' gradient kernel: its table, the bitmap, 16 words
    const int tc_lds = (int)(sizeof(long long) * TC_MAX_SHARE + TC_MAX_BITS / 8 + 64);
#define DSGD_ATTR_TC(fn) HIP_TRY_B(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, tc_lds))
    DSGD_ATTR_TC(dsgd_tc_grad_kernel<1>);
    DSGD_ATTR_TC(dsgd_tc_grad_kernel<2>);
#undef DSGD_ATTR_TC
  }
  DSGD_ATTR((dsgd_cold_kernel<true, false, false>));
  DSGD_ATTR((dsgd_cold_kernel<true, false, true>));
  DSGD_ATTR((dsgd_cold_kernel<false, false, false>));
  DSGD_ATTR((dsgd_cold_kernel<false, false, true>));
  DSGD_ATTR((dsgd_cold_kernel<true, true, false>));
  DSGD_ATTR((dsgd_cold_kernel<true, true, true>));
  DSGD_ATTR((dsgd_cold_kernel<false, true, false>));
  DSGD_ATTR((dsgd_cold_kernel<false, true, true>));
#undef DSGD_ATTR
  HIP_TRY_B(hipStreamSynchronize(c->stream));
#undef HIP_TRY_B
#undef DSGD_TRY_B
  *out = c;
  return DSGD_OK;
}

int dsgd_destroy(dsgd_ctx* c) {
  if (!c) return DSGD_OK;
  std::unique_lock<std::mutex> lk(c->mu);   // a call still running on another thread finishes first
  (void)hipSetDevice(c->cfg.device);
  // The persistent Hogwild kernel only exits on its stop flag: raise it and wait BEFORE any hipFree (hipFree
  // synchronises the device -- it would wait forever on that kernel, or free memory the kernel still reads).
  if (c->async_stream) {
    (void)hog_raise_stop(c);
    // a thread inside dsgd_async_wait / dsgd_async_stop blocks on the engine WITHOUT the mutex (async_wait_released) and
    // comes back for it: it is the one thread that joins exch_thread, and it still uses the context afterwards -- wait
    // until it has left (the stop flag above lets it finish)
    c->join_cv.wait(lk, [c] { return !c->join_in_progress; });
    if (c->exch_thread.joinable()) c->exch_thread.join();
    (void)hipStreamSynchronize(c->async_stream);
    c->async_running = false;
  }
  // every stream idle before anything is released: the members release themselves (delete c), in no particular order
  if (c->upd_stream) (void)hipStreamSynchronize(c->upd_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->build_stream) (void)hipStreamSynchronize(c->build_stream);
  if (c->comm && rccl::available()) rccl::CommDestroy(c->comm);
  // plans still alive: their blocks come back through the cache, which then lets go of everything -- in this order, and both
  // before the members go
  while (!c->plans.empty()) plan_release(c, c->plans.back());
  c->plan_cache.drop_all();
  const hipStream_t streams[] = {c->upd_stream, c->async_stream, c->query_stream, c->build_stream, c->stream};
  lk.unlock();
  delete c;
  for (hipStream_t s : streams)
    if (s) (void)hipStreamDestroy(s);
  return DSGD_OK;
}

// dsgd_load_csr (val64_in == nullptr) and dsgd_load_csr_f64 (val_in: the same values rounded to float, val64_in: as given)
static void lgt_drop(dsgd_ctx* c);   // (csrc/dsgd_lg_topics_calls.hpp)
static int load_csr_impl(dsgd_ctx* c, int64_t n_rows, const int64_t* row_ptr_in, const int32_t* col_in, const float* val_in,
                         const double* val64_in, const int8_t* label) {
  if (n_rows < 1 || !row_ptr_in || !label) return fail(DSGD_EINVAL, "n_rows must be >= 1 and arrays non-null");
  if (row_ptr_in[0] != 0) return fail(DSGD_EINVAL, "row_ptr[0] must be 0");
  const int64_t* row_ptr = row_ptr_in;
  const int32_t* col = col_in;
  const float* val = val_in;
  const double* val64 = val64_in;
  int64_t nnz = row_ptr[n_rows];
  if (nnz < 0 || (nnz > 0 && (!col || !val))) return fail(DSGD_EINVAL, "bad nnz / null col,val");
  for (int64_t i = 0; i < n_rows; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) return fail(DSGD_EINVAL, "row_ptr not monotone at row %lld", (long long)i);
  // keys must be valid Sparse keys for a vector of size D (ref: math/Sparse.scala:61-68 accepts 0..size)
  float vmax = 0.0f;
  double vmax64 = 0.0;   // (Double values: the largest |v| as a double)
  for (int64_t p = 0; p < nnz; ++p) {
    if (col[p] < 0 || col[p] > c->cfg.n_features)
      return fail(DSGD_ERANGE, "column id %d at nnz %lld outside [0, %d]", col[p], (long long)p, c->cfg.n_features);
    const float a = std::fabs(val[p]);
    if (!(a <= 3.0e38f)) return fail(DSGD_EINVAL, "non-finite value at nnz %lld", (long long)p);  // Vec.scala:14 NaN guard
    vmax = std::max(vmax, a);
    if (val64) {
      const double a64 = std::fabs(val64[p]);
      if (!(a64 <= 3.0e38)) return fail(DSGD_EINVAL, "non-finite value at nnz %lld", (long long)p);
      vmax64 = std::max(vmax64, a64);
    }
  }
  for (int64_t i = 0; i < n_rows; ++i)
    if (label[i] != 1 && label[i] != -1) return fail(DSGD_EINVAL, "label[%lld] = %d, expected +1/-1", (long long)i, label[i]);
  // A row is a Map[Int, Number] in the reference (math/Sparse.scala:11): a key occurs once.  The fixed-point bound of
  // the streaming kernels ("one contribution per row and column") relies on it, so duplicates are rejected here
  // (ascending rows -- the RCV1 files -- take the cheap path).
  {
    std::vector<int32_t> keys;
    for (int64_t i = 0; i < n_rows; ++i) {
      const int64_t b = row_ptr[i], e = row_ptr[i + 1];
      bool ascending = true;
      for (int64_t p = b + 1; p < e && ascending; ++p) ascending = col[p] > col[p - 1];
      if (ascending) continue;
      keys.assign(col + b, col + e);
      std::sort(keys.begin(), keys.end());
      if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
        return fail(DSGD_EINVAL, "row %lld holds a key twice (a Sparse vector is a map: one value per key)", (long long)i);
    }
  }
  // Internal CSR: an empty row (Sparse.zeros) gets ONE explicit zero on key 0.  x.w, the gate and the
  // gradient are unchanged (the product and y*x are 0 and every counting kernel skips abs(v) <= 1e-20),
  // and the streaming kernels can rely on "every row owns at least one slot".
  std::vector<int64_t> prow;
  std::vector<int32_t> pcol;
  std::vector<float> pval;
  std::vector<double> pval64;
  {
    int64_t n_empty = 0;
    for (int64_t i = 0; i < n_rows; ++i) n_empty += row_ptr[i + 1] == row_ptr[i];
    if (n_empty > 0) {
      prow.resize((size_t)n_rows + 1);
      pcol.reserve((size_t)(nnz + n_empty));
      pval.reserve((size_t)(nnz + n_empty));
      if (val64) pval64.reserve((size_t)(nnz + n_empty));
      prow[0] = 0;
      for (int64_t i = 0; i < n_rows; ++i) {
        if (row_ptr[i + 1] == row_ptr[i]) {
          pcol.push_back(0);
          pval.push_back(0.0f);
          if (val64) pval64.push_back(0.0);
        } else {
          pcol.insert(pcol.end(), col + row_ptr[i], col + row_ptr[i + 1]);
          pval.insert(pval.end(), val + row_ptr[i], val + row_ptr[i + 1]);
          if (val64) pval64.insert(pval64.end(), val64 + row_ptr[i], val64 + row_ptr[i + 1]);
        }
        prow[i + 1] = (int64_t)pcol.size();
      }
      row_ptr = prow.data();
      col = pcol.data();
      val = pval.data();
      if (val64) val64 = pval64.data();
      nnz = row_ptr[n_rows];
    }
  }
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));   // the persistent engine reads the matrix that would be freed here
  if (val64 && c->comm && !c->comm_v64)
    return fail(DSGD_EUNSUPPORTED, "dsgd_load_csr_f64 is not available while a communicator is attached (the gather's slots hold one "
                                   "word per column; the data and the weights are unchanged)");
  HIP_TRY(hipStreamSynchronize(c->stream));
  lgt_drop(c);   // (the topics' planes label the rows that go)
  DSGD_TRY(reset_layout(c));
  c->d_row_ptr.reset();
  c->d_col.reset();
  c->d_val.reset();
  c->d_label.reset();
  c->d_val64.reset();   // (float values again unless this load brings doubles)
  DSGD_TRY(c->d_row_ptr.alloc((size_t)(n_rows + 1)));
  if (n_rows >= (int64_t)1 << 31) return fail(DSGD_EUNSUPPORTED, "more than 2^31-1 rows per context");
  // padding: the streaming kernels read whole windows (up to 512 slots) without clamping
  DSGD_TRY(c->d_col.alloc((size_t)(nnz + WS_PAD)));
  DSGD_TRY(c->d_val.alloc((size_t)(nnz + WS_PAD)));
  HIP_TRY(hipMemset(c->d_col + nnz, 0, sizeof(int) * WS_PAD));
  HIP_TRY(hipMemset(c->d_val + nnz, 0, sizeof(float) * WS_PAD));
  DSGD_TRY(c->d_label.alloc((size_t)n_rows));
  HIP_TRY(hipMemcpy(c->d_row_ptr, row_ptr, sizeof(long long) * (size_t)(n_rows + 1), hipMemcpyHostToDevice));
  if (nnz) {
    HIP_TRY(hipMemcpy(c->d_col, col, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_val, val, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(c->d_label, label, (size_t)n_rows, hipMemcpyHostToDevice));
  if (val64) {   // 8 bytes per non-zero, parallel to d_col / d_val (the ranking relabels d_col in place: the entries stay where they are)
    DSGD_TRY(c->d_val64.alloc((size_t)(nnz + 1)));
    if (nnz) HIP_TRY(hipMemcpy(c->d_val64, val64, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  c->n_rows = n_rows;
  c->row_len.resize((size_t)n_rows);
  for (int64_t i = 0; i < n_rows; ++i) c->row_len[(size_t)i] = (int32_t)std::min<int64_t>(row_ptr_in[i + 1] - row_ptr_in[i], c->dp);
  c->nnz = nnz;
  {
    int e = 0;
    std::frexp(vmax > 0.0f ? vmax : 1.0f, &e);  // vmax = f * 2^e, f in [0.5, 1)  ->  vmax2 = 2^e >= vmax
    if (vmax > 0.0f && std::ldexp(1.0f, e - 1) == vmax) e -= 1;  // vmax itself a power of two
    c->vexp = e;   // vmax2 = 2^e
    c->cold_shift = FIX_SHIFT;   // (until the layout of this data is built)
    c->fix_scale = std::ldexp(1.0f, FIX_SHIFT - e);
  }
  if (val64) {   // vexp from the largest |v| as a double (the same rule)
    int e = 0;
    std::frexp(vmax64 > 0.0 ? vmax64 : 1.0, &e);
    if (vmax64 > 0.0 && std::ldexp(1.0, e - 1) == vmax64) e -= 1;
    c->vexp = e;
    c->fix_scale = std::ldexp(1.0f, FIX_SHIFT - e);
  }
  c->h_row_ptr.assign(row_ptr, row_ptr + n_rows + 1);
  c->h_label.assign(label, label + n_rows);
  c->ssegs_last.clear();
  // everything stamped with the old data is stale from here on, not only from the next ranking on (build_split bumps
  // layout_gen again): plans' slices and tiles, column-list layouts; the plans' lists are checked at their next use
  ++c->layout_gen;
  ++c->load_gen;
  c->bound_segs.clear();
  layouts_drop_all(c);   // (they hold the old rows' entries)
  c->last_grad_kernel = "";  // (dsgd_grad_kernel_name / dsgd_tuning_info report launches over THIS data: calls that record none --
  c->last_shift = FIX_SHIFT; //  the row-parallel fp64 requests -- would go on reporting the old data's)
  // (the wave tiles cover the hot stream and are built with the layout, at the first compute call)
  c->group = eval_group(nnz, n_rows);
  return DSGD_OK;
}

int dsgd_load_csr(dsgd_ctx* c, int64_t n_rows, const int64_t* row_ptr, const int32_t* col, const float* val, const int8_t* label) {
  DSGD_TRY(check_ctx(c));
  return load_csr_impl(c, n_rows, row_ptr, col, val, nullptr, label);
}

int dsgd_value_bits(dsgd_ctx* c, int32_t* bits_out) {
  DSGD_TRY(check_ctx(c));
  if (!bits_out) return fail(DSGD_EINVAL, "null bits_out");
  std::lock_guard<std::mutex> lk(c->mu);
  *bits_out = c->d_val64 ? 64 : 32;
  return DSGD_OK;
}

int dsgd_n_rows(dsgd_ctx* c, int64_t* n_rows, int64_t* nnz) {
  DSGD_TRY(check_ctx(c));
  if (n_rows) *n_rows = c->n_rows;
  if (nnz) *nnz = c->nnz;
  return DSGD_OK;
}

int dsgd_set_dim_sparsity(dsgd_ctx* c, const float* ds) {
  DSGD_TRY(check_ctx(c));
  if (!ds) return fail(DSGD_EINVAL, "null ds");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));
  HIP_TRY(hipMemcpyAsync(c->d_io, ds, sizeof(float) * c->dp, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(launch_permute_in(c, c->d_io, c->d_ds));
  if (c->fp64) DSGD_TRY(launch_promote64_in(c, c->d_io, c->d_ds64));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->have_ds = true;
  c->s_dirty = true;
  return DSGD_OK;
}

// dimSparsity in three parts around its all-reduce (one host thread, several contexts: dsgd_build_dim_sparsity_devices)
static int ds_begin(dsgd_ctx* c, long long n_train, DevBuf<unsigned int>& d_cnt) {   // (layout ready)
  d_cnt.reset();
  long long nnz_train = 0;
  HIP_TRY(hipMemcpy(&nnz_train, c->d_row_ptr + n_train, sizeof(long long), hipMemcpyDeviceToHost));
  DSGD_TRY(d_cnt.alloc((size_t)c->dp));
  int rc = reset_counters(c);
  if (!rc) rc = count_columns(c, nnz_train, d_cnt, true);
  if (rc) d_cnt.reset();
  return rc;
}
static int ds_collective(dsgd_ctx* c, unsigned int* d_cnt) {
  if (!c->comm) return DSGD_OK;
  // the reference counts over the WHOLE train set (Main.scala:57-60); shards sum their counts
  int r = rccl::AllReduce(d_cnt, d_cnt, (size_t)c->dp, rccl::kUint32, rccl::kSum, c->comm, c->stream);
  if (r) return fail(DSGD_ERCCL, "ncclAllReduce(feature counts): %s", rccl::GetErrorString(r));
  return DSGD_OK;
}
static int ds_finish(dsgd_ctx* c, DevBuf<unsigned int>& d_cnt, float* ds_out) {   // (releases d_cnt)
  int rc = DSGD_OK;
  unsigned int cnt_key0 = 0;
  {
    // Main.scala:60 does buff(idx - 1): a feature id 0 in a train row would index buff(-1)
    int rank0 = 0;
    hipError_t e = hipMemcpyAsync(&rank0, c->d_perm, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(&cnt_key0, d_cnt + rank0, sizeof(unsigned int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(DSGD_EHIP, "dimSparsity: %s", hipGetErrorString(e));
  }
  if (!rc) {
    hipLaunchKernelGGL(dsgd_ds_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_cnt, c->d_perm, c->d_ds, c->dp);
    if (c->fp64)
      hipLaunchKernelGGL(dsgd_ds64_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_cnt, c->d_perm, c->d_ds64, c->dp);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) rc = fail(DSGD_EHIP, "dimSparsity kernels: %s", hipGetErrorString(le));
  }
  if (!rc) rc = read_scalars(c);
  d_cnt.reset();
  DSGD_TRY(rc);
  DSGD_TRY(check_err_flag(c));
  if (cnt_key0) return fail(DSGD_ERANGE, "feature id 0 cannot be counted by Main.scala:60 (buff(idx - 1))");
  c->have_ds = true;
  c->s_dirty = true;
  if (ds_out) {
    if (c->fp64)   // (the fp64 values rounded)
      DSGD_TRY(launch_round64_out(c, c->d_ds64, c->d_io));
    else
      DSGD_TRY(launch_permute_out(c, c->d_ds, c->d_io));
    HIP_TRY(hipMemcpyAsync(ds_out, c->d_io, sizeof(float) * c->dp, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return DSGD_OK;
}
static int ds_checks(dsgd_ctx* c, long long n_train) {
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_sync_mode(c));
  if (n_train < 1 || n_train > c->n_rows) return fail(DSGD_EINVAL, "n_train %lld outside [1, %lld]", n_train, c->n_rows);
  return DSGD_OK;
}

int dsgd_build_dim_sparsity(dsgd_ctx* c, int64_t n_train, float* ds_out) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(ds_checks(c, n_train));
  DSGD_TRY(prepare_layout(c));
  DevBuf<unsigned int> d_cnt;
  DSGD_TRY(ds_begin(c, n_train, d_cnt));
  DSGD_TRY(ds_collective(c, d_cnt));
  return ds_finish(c, d_cnt, ds_out);
}

static int set_weights_locked(dsgd_ctx* c, const float* w) {
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_w, bytes));
  memcpy(c->pin_w.p, w, bytes);   // the caller may reuse w as soon as this returns
  HIP_TRY(hipMemcpyAsync(c->d_io, c->pin_w.p, bytes, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_w));
  if (c->fp64)   // (promoted)
    DSGD_TRY(launch_promote64_in(c, c->d_io, c->d_w64));
  else
    DSGD_TRY(launch_permute_in(c, c->d_io, c->d_w));
  c->s_dirty = true;
  return DSGD_OK;
}

int dsgd_set_weights(dsgd_ctx* c, const float* w) {
  DSGD_TRY(check_ctx(c));
  if (!w) return fail(DSGD_EINVAL, "null w");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));
  return set_weights_locked(c, w);
}

int dsgd_get_weights(dsgd_ctx* c, float* w_out) {
  DSGD_TRY(check_ctx(c));
  if (!w_out) return fail(DSGD_EINVAL, "null w_out");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_out, bytes));
  if (c->fp64)   // (the fp64 weights rounded)
    DSGD_TRY(launch_round64_out(c, c->d_w64, c->d_io));
  else
    DSGD_TRY(launch_permute_out(c, c->d_w, c->d_io));
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_io, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(w_out, c->pin_out.p, bytes);
  return DSGD_OK;
}

// stage host index lists for n_workers workers; returns the largest list length
constexpr long long REQ_MAPPED_ITEMS = 16384;   // index entries of one request read in place from host memory (64 KiB)
static int stage_lists(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers,
                       long long* max_items, long long* total) {
  long long tot = 0, mx = 0;
  for (int k = 0; k < n_workers; ++k) {
    if (n_per_worker[k] <= 0)
      return fail(DSGD_EINVAL, "worker %d has an empty sample list: Vec.sum requires a non-empty list", k);
    if (!idx_per_worker[k]) return fail(DSGD_EINVAL, "null index list for worker %d", k);
    tot += n_per_worker[k];
    mx = std::max<long long>(mx, n_per_worker[k]);
  }
  std::vector<WorkSeg> segs(n_workers);
  long long off = 0;
  if (c->k.req_mapped && tot <= REQ_MAPPED_ITEMS) {
    // the reference's batch sizes: the lists go into a host-mapped buffer the kernels read in place -- no copy on the
    // stream in front of the launch (every per-request entry point returns behind its kernels: the buffer is free again)
    if (!c->h_req) DSGD_TRY(c->h_req.alloc((size_t)REQ_MAPPED_ITEMS, hipHostMallocMapped));
    for (int k = 0; k < n_workers; ++k) {
      memcpy(c->h_req + off, idx_per_worker[k], sizeof(int) * (size_t)n_per_worker[k]);
      segs[k].begin = off;
      segs[k].end = off + n_per_worker[k];
      off += n_per_worker[k];
    }
    c->cur_idx = c->h_req.dev();
  } else {
    DSGD_TRY(ensure_idx(c, tot));
    // one copy for all lists, on the stream (behind the previous step's kernels, which may still be reading d_idx)
    DSGD_TRY(pin_acquire(c->pin_idx, sizeof(int) * (size_t)tot));
    for (int k = 0; k < n_workers; ++k) {
      memcpy(static_cast<int*>(c->pin_idx.p.get()) + off, idx_per_worker[k], sizeof(int) * (size_t)n_per_worker[k]);
      segs[k].begin = off;
      segs[k].end = off + n_per_worker[k];
      off += n_per_worker[k];
    }
    HIP_TRY(hipMemcpyAsync(c->d_idx, c->pin_idx.p, sizeof(int) * (size_t)tot, hipMemcpyHostToDevice, c->stream));
    DSGD_TRY(pin_sent(c, c->pin_idx));
    c->cur_idx = c->d_idx;
  }
  DSGD_TRY(upload_segs(c, segs));
  *max_items = mx;
  *total = tot;
  return DSGD_OK;
}

int dsgd_gradient(dsgd_ctx* c, const float* w, const int32_t* idx, int64_t n, float* g_out, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_gradient"));
  if (!g_out) return fail(DSGD_EINVAL, "null g_out");
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");  // ref: math/Vec.scala:129
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));   // g accumulators, s and (with w != NULL) the weights belong to the running engine
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(ensure_s(c));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  const int64_t nn = n;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, 1, mx));
  hipLaunchKernelGGL(dsgd_regularize_kernel, dim3((c->dp + 1023) / 1024, 1), dim3(1024), 0, c->stream, c->d_g,
                     (long long)c->dp, c->dp, c->d_sc);
  HIP_TRY(hipGetLastError());
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_out, bytes));
  DSGD_TRY(launch_permute_out(c, c->d_g, c->d_io));
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_io, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_g, 0, bytes, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  memcpy(g_out, c->pin_out.p, bytes);
  DSGD_TRY(prof_collect(c));
  DSGD_TRY(check_err_flag(c));
  if (stats) {
    stats->n_samples = n;
    stats->n_active = (int64_t)c->h_sc->n_active;
  }
  return DSGD_OK;
}

int dsgd_apply(dsgd_ctx* c, const float* g_mean, float lr) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_apply"));
  if (!g_mean) return fail(DSGD_EINVAL, "null g_mean");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  HIP_TRY(hipMemcpyAsync(c->d_io, g_mean, sizeof(float) * c->dp, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(launch_permute_in(c, c->d_io, c->d_gsum));
  DSGD_TRY(ensure_redpart(c));
  hipLaunchKernelGGL(dsgd_apply_cols_kernel, dim3((c->dp + FRA_COLS - 1) / FRA_COLS), dim3(256), 0, c->stream, c->d_w,
                     c->d_gsum, c->d_ds, c->dp, 1.0f, lr, (float)c->cfg.lambda, c->d_sc, red_out(c), 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->red_par ^= 1;
  c->s_lazy = false;
  c->s_dirty = false;
  return DSGD_OK;
}

static int finish_stats(dsgd_ctx* c, dsgd_batch_stats* stats, long long total) {
  DSGD_TRY(read_scalars(c));
  DSGD_TRY(prof_collect(c));
  DSGD_TRY(check_err_flag(c));
  if (stats) {
    stats->n_samples = total;
    stats->n_active = (int64_t)c->h_sc->n_active;
  }
  return DSGD_OK;
}

// the statistics of a per-request step from the host-mapped mailbox its last kernel wrote: n_active as the difference
// against the value the host last saw (no memset in front of the request), the error flags as they are
static int finish_mail(dsgd_ctx* c, dsgd_batch_stats* stats, long long total, unsigned long long before, bool seq = false) {
  // (seq: the request's ONE workgroup wrote its sequence number behind the two words, with release order, as its last
  //  act -- the host polls the mapped word instead of waiting for the stream's completion signal; what the request
  //  enqueues next is ordered behind the kernel by the stream as always)
  bool seen = false;
  if (seq) {
    const volatile unsigned long long* m = c->h_mail;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned int spin = 0; !seen; ++spin) {
      seen = __atomic_load_n(&m[2], __ATOMIC_ACQUIRE) == c->mail_seq;
      if (!seen && (spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(500)) break;
    }
  }
  if (!seen) HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned long long now = c->h_mail[0];
  const int err = (int)c->h_mail[1];
  c->ctr_last = now;
  c->ctr_known = err == 0;
  if (err) {   // (rare: the flags are cleared for the next request, as check_err_flag does)
    c->h_sc->err = err;
    return check_err_flag(c);
  }
  if (stats) {
    stats->n_samples = total;
    stats->n_active = (int64_t)(now - before);
  }
  return DSGD_OK;
}

// (finish = false: stop behind the gradient kernels -- the caller splits the finish around a grouped collective)
static int ranges_enqueue(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int n_workers, float lr,
                          long long* total, bool finish = true) {
  if (n_workers < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "need at least one worker");
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  std::vector<WorkSeg> segs(n_workers);
  long long mx = 0, tot = 0, smallest = LLONG_MAX;
  for (int k = 0; k < n_workers; ++k) {
    if (row_end[k] <= row_begin[k])
      return fail(DSGD_EINVAL, "worker %d has an empty row range: Vec.sum requires a non-empty list", k);
    if (row_begin[k] < 0 || row_end[k] > c->n_rows)
      return fail(DSGD_ERANGE, "worker %d range [%lld, %lld) outside the %lld loaded rows", k, (long long)row_begin[k],
                  (long long)row_end[k], c->n_rows);
    segs[k].begin = row_begin[k];
    segs[k].end = row_end[k];
    mx = std::max<long long>(mx, row_end[k] - row_begin[k]);
    smallest = std::min<long long>(smallest, row_end[k] - row_begin[k]);
    tot += row_end[k] - row_begin[k];
  }
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(ensure_g(c, n_workers));
  DSGD_TRY(ensure_s(c, true));
  std::vector<StreamSeg> ssegs(n_workers);
  for (int k = 0; k < n_workers; ++k) ssegs[k] = make_sseg(row_begin[k], row_end[k]);
  long long ent = tot * 75;   // non-zeros of the ranges (the host's copy of the row offsets; else RCV1's mean row)
  if (c->h_row_ptr.size() == (size_t)c->n_rows + 1) {
    ent = 0;
    for (int k = 0; k < n_workers; ++k) ent += c->h_row_ptr[(size_t)row_end[k]] - c->h_row_ptr[(size_t)row_begin[k]];
  }
  const RangesRoute r = route_ranges(c->k, route_facts(c), n_workers, tot, ent, smallest);
  int trc = 1;   // (1: the column lists were not tried, or declined softly -- no memory, the back-off: the ranges' other family)
  if (r.try_tcol) {
    // 10^3 .. 10^5 rows: column lists (csrc/dsgd_tcol.hpp) -- dot, column-wise gradient, reduce: no partials
    DSGD_TRY(upload_segs(c, segs));
    trc = launch_tcol(c, segs, mx);
    if (trc != DSGD_OK && trc != 1) return trc;
  }
  if (trc == 1) switch (r.then) {
    case RANGES_FSTEP:   // shards of 10^4 .. 2 * 10^6 rows: row chunks, the three passes of the split streams in ONE launch (csrc/dsgd_fstep.hpp)
      DSGD_TRY(launch_fstep(c, ssegs, r.fstep_wg));
      break;
    case RANGES_STREAM:   // whole contiguous ranges: the nnz-streaming kernel (coalesced 16-byte loads, no per-row latency chain)
      DSGD_TRY(launch_stream<true>(c, ssegs));  // (the profiling events bracket the main kernel only)
      break;
    case RANGES_ROWWISE:
      DSGD_TRY(upload_segs(c, segs));
      DSGD_TRY(launch_grad(c, nullptr, c->d_segs, n_workers, mx, true));
      break;
  }
  if (finish) DSGD_TRY(launch_finish_sync(c, n_workers, lr));
  *total = tot;
  return DSGD_OK;
}

int dsgd_sync_step_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, float lr,
                          dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_sync_step_ranges"));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(reset_counters(c));
  long long tot = 0;
  DSGD_TRY(ranges_enqueue(c, row_begin, row_end, n_workers, lr, &tot));
  return finish_stats(c, stats, tot);
}

int dsgd_sync_step_ranges_async(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers,
                                float lr) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_sync_step_ranges_async"));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  long long tot = 0;
  DSGD_TRY(ranges_enqueue(c, row_begin, row_end, n_workers, lr, &tot));
  c->pending_samples += tot;
  return DSGD_OK;
}

int dsgd_synchronize(dsgd_ctx* c, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  DSGD_TRY(read_scalars(c));
  DSGD_TRY(prof_collect(c));
  // (a logistic plan's rows: all of them active -- across ranks they are the job's, counted by the device in n_samples)
  const long long act = (long long)c->h_sc->n_active + c->lg_pending_active + (c->job_pending && !c->fp64 ? (long long)c->h_sc->n_samples : 0);
  const int err = c->h_sc->err;
  const long long pending = c->pending_samples + (c->job_pending ? (long long)c->h_sc->n_samples : 0);
  c->pending_samples = 0;   // (whatever the outcome: the rows of a rejected run are not carried into the next report)
  c->lg_pending_active = 0;
  c->job_pending = false;
  DSGD_TRY(reset_counters(c));
  if ((err & (8 | 16)) && c->d_cs_sync) HIP_TRY(hipMemsetAsync(c->d_cs_sync, 0, sizeof(unsigned int) * 2, c->stream));   // the abort word, first
  if (err & 2)
    return fail(DSGD_ESTATE, "fixed-point gradient accumulator left its safe band; the steps since the last "
                             "synchronize are invalid");
  if (err & 8)
    return fail(DSGD_ESTATE, "the column-slice kernel's exchange between its workgroups timed out; the steps since the last "
                             "synchronize are invalid (DSGD_CS=0 selects the row-parallel kernels)");
  if (err) return fail(DSGD_ERANGE, "sample index / key outside the loaded data");
  if (stats) {
    stats->n_active = act;
    stats->n_samples = pending;
  }
  return DSGD_OK;
}

int dsgd_cache_trim(dsgd_ctx* c, int64_t keep_bytes, int64_t* held_out) {
  DSGD_TRY(check_ctx(c));
  if (keep_bytes < 0) return fail(DSGD_EINVAL, "negative keep_bytes");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  c->plan_cache.trim((size_t)keep_bytes, false);
  if (held_out) *held_out = (int64_t)c->plan_cache.cache_bytes;
  return DSGD_OK;
}

int dsgd_plan_create_n(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps,
                       int32_t n_workers, dsgd_plan** out) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || !out || n_steps < 1 || n_workers < 1 || n_idx < 0) return fail(DSGD_EINVAL, "bad plan arguments");
  if (n_steps > INT64_MAX / n_workers) return fail(DSGD_EINVAL, "n_steps * n_workers overflows");
  if (offsets[n_steps * n_workers] != n_idx)
    return fail(DSGD_EINVAL, "offsets end at %lld but idx holds %lld entries", (long long)offsets[n_steps * n_workers], (long long)n_idx);
  return dsgd_plan_create(c, idx, offsets, n_steps, n_workers, out);
}

static void plan_abandon(dsgd_ctx* c, dsgd_plan* p) {
  (void)hipStreamSynchronize(c->build_stream);
  plan_release(c, p);
}
// A plan's frame: offsets checked, the two device blocks taken from the cache, the list ranges uploaded (build stream).
// The caller fills p->d_idx on the build stream and calls plan_finish; on failure everything is given back.
static int plan_frame(dsgd_ctx* c, const int64_t* offsets, int64_t n_steps, int32_t n_workers, dsgd_plan** out, bool rp64 = false, bool lg = false) {
  const int64_t n_lists = n_steps * n_workers;
  if (offsets[0] != 0) return fail(DSGD_EINVAL, "offsets[0] must be 0");
  long long mx = 0;
  for (int64_t i = 0; i < n_lists; ++i) {
    if (offsets[i + 1] <= offsets[i])
      return fail(DSGD_EINVAL, "list %lld is empty: Vec.sum requires a non-empty list", (long long)i);
    mx = std::max<long long>(mx, offsets[i + 1] - offsets[i]);
  }
  if (c->fp64 && !rp64) {   // what dsgd_cs64_step_kernel can hold, refused here rather than at the first run
    long long rows = 0;
    for (int64_t st = 0; st < n_steps; ++st) rows = std::max<long long>(rows, offsets[(st + 1) * n_workers] - offsets[st * n_workers]);
    if (n_workers > CS64_MAX_K)
      return fail(DSGD_EUNSUPPORTED, "fp64 plans host at most %d workers per step (this plan has %d)", CS64_MAX_K, n_workers);
    if (rows > CS_MAX_SLOTS)
      return fail(DSGD_EUNSUPPORTED, "fp64 plans take at most %d rows per step (this plan has a step of %lld)", CS_MAX_SLOTS, rows);
    if (cs64_lds_bytes(c->dp, n_workers) > CS64_LDS_MAX || c->dp < 4 * CS64_G)
      return fail(DSGD_EUNSUPPORTED, "fp64 plans: a model of %d features needs %lld bytes of LDS per slice at %d workers (at most %lld; "
                                     "at least %d features)", c->cfg.n_features, cs64_lds_bytes(c->dp, n_workers), n_workers, CS64_LDS_MAX,
                  4 * CS64_G - 1);
  }
  dsgd_plan* p = new (std::nothrow) dsgd_plan();
  if (!p) return fail(DSGD_ENOMEM, "out of host memory");
  c->plans.push_back(p);
  p->rp64 = rp64;
  p->lg = lg;
  p->n_steps = n_steps;
  p->n_workers = n_workers;
  p->max_items = mx;
  p->offsets.assign(offsets, offsets + n_lists + 1);
  for (int64_t st = 0; st < n_steps; ++st)
    p->max_step_rows = std::max<long long>(p->max_step_rows, offsets[(st + 1) * n_workers] - offsets[st * n_workers]);
  p->fits_rows = c->n_rows;
  p->checked_load = c->load_gen;   // (what the creators establish -- fits, lists drawn inside the rows -- is about this load)
  std::vector<WorkSeg> segs((size_t)n_lists);
  for (int64_t i = 0; i < n_lists; ++i) {
    segs[i].begin = offsets[i];
    segs[i].end = offsets[i + 1];
  }
  // the lists go up on the context's BUILD stream (beside whatever the launch stream is running: the next epoch's plan
  // can be set up while this epoch's steps run), into blocks earlier plans handed back
  int rc = ensure_build_stream(c);
  if (rc == DSGD_OK && (p->d_idx.take(c->plan_cache, (size_t)offsets[n_lists]) || p->d_segs.take(c->plan_cache, (size_t)n_lists)))
    rc = fail(DSGD_ENOMEM, "out of device memory (plan of %lld index entries)", (long long)offsets[n_lists]);
  if (rc == DSGD_OK && hipEventCreateWithFlags(&p->built_ev.e, hipEventDisableTiming) != hipSuccess) rc = fail(DSGD_EHIP, "hipEventCreate");
  hipError_t e = hipSuccess;
  if (rc == DSGD_OK) e = hipMemcpyAsync(p->d_segs, segs.data(), sizeof(WorkSeg) * segs.size(), hipMemcpyHostToDevice, c->build_stream);
  if (rc == DSGD_OK && e == hipSuccess) e = hipStreamSynchronize(c->build_stream);   // (segs is a local: staged before it goes)
  if (rc == DSGD_OK && e != hipSuccess) rc = fail(DSGD_EHIP, "plan upload: %s", hipGetErrorString(e));
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    plan_abandon(c, p);
    return fail(rc, "%s", msg);
  }
  *out = p;
  return DSGD_OK;
}
// what route_plan needs from a plan; dsgd_plan_run, plan_run64 and dsgd_plan_info ask the same question
static PlanRoute plan_route(const dsgd_ctx* c, const dsgd_plan* p) {
  PlanFacts f;
  f.rp64 = p->rp64;
  f.lg = p->lg;
  f.cs_current = p->cs_ok && p->cs_layout == c->layout_gen;
  f.lg_cs_current = p->lg && p->lg_cs && f.cs_current;
  f.fits_here = p->fits && p->fits_rows == c->n_rows;
  f.vt_current = p->vt_ok && p->vt_layout == c->layout_gen;
  f.max_step_rows = p->max_step_rows;
  f.n_workers = p->n_workers;
  return route_plan(c->k, route_facts(c), f);
}
static int cs64_refused(dsgd_ctx* c);   // (dsgd_fp64_host.hpp, which in turn needs plan_finish: the one declaration ahead)
// (csrc/dsgd_lg_calls.hpp, behind the plans' entry points that dispatch into it: a logistic plan's refusals and its run)
// What a logistic call is to a communicator attached with dsgd_comm_init_lg (include/dsgd.h "ACROSS RANKS"): a step that spans
// the ranks (collective), a call that stays on the shard, or one that is refused.  Under any other communicator: all refused.
enum LgScope { LG_SPANS, LG_STAYS_LOCAL, LG_ONE_PROCESS };
static int lg_refuse(dsgd_ctx* c, const char* what, LgScope scope);
static int plan_run_lg(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, float lr);
// the lists are in p->d_idx (enqueued on the build stream): lay the plan out for the device, close its set-up
static int plan_finish(dsgd_ctx* c, dsgd_plan* p, dsgd_plan** out) {
  int rc = DSGD_OK;
  // the column slices of the reference's own step sizes are laid out NOW (by the device, on the build stream), not inside
  // the first dsgd_plan_run -- a call its callers time; without a column layout yet (no data / no dimSparsity) at the first run
  if (plan_lays_out_at_creation(c->k, route_facts(c), p->rp64 || p->lg, (bool)c->d_row_ptr, c->have_ds)) {   // (a row-parallel or logistic plan has no layout)
    rc = prepare_layout(c);
    if (rc == DSGD_OK) rc = cs_build(c, p);
    if (rc == DSGD_OK && c->fp64 && !p->cs_ok) rc = cs64_refused(c);
  }
  if (rc == DSGD_OK && hipEventRecord(p->built_ev, c->build_stream) != hipSuccess) rc = fail(DSGD_EHIP, "hipEventRecord");
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    plan_abandon(c, p);
    return fail(rc, "%s", msg);
  }
  p->built_pending = true;
  *out = p;
  return DSGD_OK;
}

// the fp64 mode's plan step-range check is shared with dsgd_plan_run: a null plan, or steps outside it
static int plan_steps_check(const dsgd_plan* p, int64_t step_begin, int64_t step_end) {
  if (!p) return fail(DSGD_EINVAL, "null plan");
  if (step_begin < 0 || step_end > p->n_steps || step_end < step_begin)
    return fail(DSGD_EINVAL, "steps [%lld, %lld) outside the plan's %lld steps", (long long)step_begin, (long long)step_end,
                p->n_steps);
  return DSGD_OK;
}

}  // extern "C" (the entry points below are declared with C linkage in include/dsgd.h and keep it)
// ---- the fp64 mode (DSGD_F_FP64): ALL of its host code, top to bottom; what follows here may call into it ----
#include "dsgd_fp64_host.hpp"
extern "C" {

// (below the fp64 mode's host code: they dispatch into it)

// Double feature values (include/dsgd.h "THE FP64 MODE", csrc/dsgd_rp64.hpp): dsgd_load_csr's validation and refusals; the
// context keeps the doubles beside the values rounded to float (the ranking, the layout code: unchanged)
int dsgd_load_csr_f64(dsgd_ctx* c, int64_t n_rows, const int64_t* row_ptr, const int32_t* col, const double* val, const int8_t* label) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(require_fp64(c, "dsgd_load_csr_f64"));
  if (n_rows < 1 || !row_ptr || !label) return fail(DSGD_EINVAL, "n_rows must be >= 1 and arrays non-null");
  if (row_ptr[0] != 0) return fail(DSGD_EINVAL, "row_ptr[0] must be 0");
  const int64_t nnz = row_ptr[n_rows];
  if (nnz < 0 || (nnz > 0 && (!col || !val))) return fail(DSGD_EINVAL, "bad nnz / null col,val");
  std::vector<float> vf((size_t)nnz);
  for (int64_t p = 0; p < nnz; ++p) vf[(size_t)p] = (float)val[p];   // (NaN stays NaN, beyond the float range: inf -- refused below, in order)
  static const double zero64 = 0.0;
  return load_csr_impl(c, n_rows, row_ptr, col, vf.data(), nnz ? val : &zero64, label);
}

int dsgd_sync_step(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers,
                   float lr, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !idx_per_worker || !n_per_worker) return fail(DSGD_EINVAL, "need at least one worker");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  long long rows = 0;
  for (int k = 0; k < n_workers; ++k) rows += std::max<long long>(0, n_per_worker[k]);
  const RequestRoute r = route_request(
      c->k, route_facts(c), n_workers, rows,
      [&] {
        for (int k = 0; k < n_workers; ++k)
          if (!idx_per_worker[k] || !list_fits_staged(c, idx_per_worker[k], n_per_worker[k])) return false;
        return true;
      },
      [&] {   // (what is wrong with a list, stage_lists and the row-wise kernel report)
        for (int k = 0; k < n_workers; ++k) {
          if (n_per_worker[k] <= 0 || !idx_per_worker[k]) return false;
          for (int64_t t = 0; t < n_per_worker[k]; ++t)
            if (idx_per_worker[k][t] < 0 || idx_per_worker[k][t] >= c->n_rows) return false;
        }
        return true;
      });
  long long mx = 0, tot = 0;
  switch (r.first) {
    case REQ_F64_RANKS: return sync_step64_ranks(c, idx_per_worker, n_per_worker, n_workers, (double)lr, stats);
    case REQ_F64_ROWS:   // Double data: the row-parallel pair, inside the limits of the one-step plan this call is on float data
      DSGD_TRY(cs64_step_limits(c, n_workers, rows));
      return sync_step64_rows(c, idx_per_worker, n_per_worker, n_workers, (double)lr, stats);
    case REQ_F64_CS: return sync_step64(c, idx_per_worker, n_per_worker, n_workers, (double)lr, stats);
    case REQ_ONE_WG_READBACK:   // the reference's batch sizes: one persistent workgroup does the whole closure
      DSGD_TRY(reset_counters(c));
      DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
      DSGD_TRY(launch_plan_kernel(c, c->cur_idx, c->d_segs, 0, 1, lr));
      return finish_stats(c, stats, tot);
    case REQ_ONE_WG_MAIL: {   // ... its statistics through the host-mapped mailbox (see below)
      if (!c->ctr_known) DSGD_TRY(reset_counters(c));
      const unsigned long long before = c->ctr_last;
      DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
      DSGD_TRY(launch_plan_kernel(c, c->cur_idx, c->d_segs, 0, 1, lr, true));
      return finish_mail(c, stats, tot, before, c->k.req_spin);
    }
    case REQ_CS: {   // the reference's own sizes (application.conf:15,27): the step laid out and run by the column-slice kernel, one launch
      if (!c->ctr_known) DSGD_TRY(reset_counters(c));
      const unsigned long long before = c->ctr_last;
      DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
      DSGD_TRY(launch_cs_request(c, r.G, n_workers, mx, lr));
      const int rc = finish_mail(c, stats, tot, before, c->k.req_spin);
      if (rc != 1) return rc;
      // (the step does not fit the one-step layout -- more than CS_MAX_SLOTS slots or 4,096 columns in one slice: nothing
      //  was applied; the row-parallel kernels below take it.  They work on the rank-ordered vector: the slice-major
      //  copy the request made is dropped -- left "live" it would overwrite their update at the next bind)
      DSGD_TRY(cs_unslice(c));
      break;
    }
    case REQ_ROWWISE_READBACK:
    case REQ_ROWWISE_MAIL: break;
  }
  DSGD_TRY(ensure_g(c, n_workers));
  DSGD_TRY(ensure_s(c, true));
  if (r.rowwise == REQ_ROWWISE_READBACK) {   // (the collective path / profiling brackets: the plain read-back)
    DSGD_TRY(reset_counters(c));
    DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
    DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, n_workers, mx, true));
    DSGD_TRY(launch_finish_sync(c, n_workers, lr));
    return finish_stats(c, stats, tot);
  }
  // the request's statistics come back through the host-mapped mailbox the fused reduce writes (no memset in front, no
  // copy behind: two calls and ~7 us of GPU time per request)
  if (!c->ctr_known) DSGD_TRY(reset_counters(c));
  const unsigned long long before = c->ctr_last;
  DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
  DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, n_workers, mx, true));
  DSGD_TRY(launch_finish_sync(c, n_workers, lr, true));
  return finish_mail(c, stats, tot, before);
}

int dsgd_plan_create(dsgd_ctx* c, const int32_t* idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                     dsgd_plan** out) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || !out || n_steps < 1 || n_workers < 1) return fail(DSGD_EINVAL, "bad plan arguments");
  const int64_t n_lists = n_steps * n_workers;
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(refuse_fp64_comm(c, "dsgd_plan_create"));
  DSGD_TRY(refuse_val64(c, "dsgd_plan_create"));
  DSGD_TRY(bind(c, true));   // (nothing here touches w: slice-major weights stay as they are)
  dsgd_plan* p = nullptr;
  DSGD_TRY(plan_frame(c, offsets, n_steps, n_workers, &p));
  p->h_idx.assign(idx, idx + offsets[n_lists]);
  p->fits = true;
  for (int64_t i = 0; i < n_lists && p->fits; ++i) p->fits = list_fits_staged(c, idx + offsets[i], offsets[i + 1] - offsets[i]);
  // (pageable sources: the runtime stages them and returns when they are staged; ordered on the build stream)
  hipError_t e = hipMemcpyAsync(p->d_idx, idx, sizeof(int) * (size_t)offsets[n_lists], hipMemcpyHostToDevice, c->build_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->build_stream);
  if (e != hipSuccess) {
    plan_abandon(c, p);
    return fail(DSGD_EHIP, "plan upload: %s", hipGetErrorString(e));
  }
  return plan_finish(c, p, out);
}

// ---- an epoch's lists drawn on the device (seed_scratch, the scan, the walk's call, the draw; the four entry points) ----
#include "dsgd_seed_host.hpp"

// the lists of a plan as the device holds them (tests: the device-drawn lists against csrc/jrand.c's)
int dsgd_plan_read_lists(dsgd_ctx* c, dsgd_plan* p, int32_t* idx_out, int64_t n, int64_t* offsets_out, int64_t n_offsets) {
  DSGD_TRY(check_ctx(c));
  if (!p || n < 0 || n_offsets < 0 || (n > 0 && !idx_out) || (n_offsets > 0 && !offsets_out)) return fail(DSGD_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  const long long n_lists = (long long)p->n_steps * p->n_workers;
  if (n > p->offsets[(size_t)n_lists] || n_offsets > n_lists + 1) return fail(DSGD_EINVAL, "more entries asked for than the plan holds");
  if (p->built_pending && p->built_ev) HIP_TRY(hipEventSynchronize(p->built_ev));
  if (n) HIP_TRY(hipMemcpy(idx_out, p->d_idx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n_offsets; ++i) offsets_out[i] = p->offsets[(size_t)i];
  return DSGD_OK;
}

// gate decisions and regulariser scalars of a column-slice plan's steps on record (include/dsgd.h)
int dsgd_plan_record(dsgd_ctx* c, dsgd_plan* p, int32_t on) {
  DSGD_TRY(check_ctx(c));
  if (!p) return fail(DSGD_EINVAL, "null plan");
  if (p->lg) return fail(DSGD_EUNSUPPORTED, "dsgd_plan_record: a logistic plan keeps no record (there is no gate)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  HIP_TRY(hipStreamSynchronize(c->stream));
  p->d_gate_rec.reset();
  p->d_s_rec.reset();
  p->gate_words = 0;
  if (!on) return DSGD_OK;
  const int words = (int)((std::max<long long>(p->max_step_rows, 1) + 31) / 32);
  if (p->d_gate_rec.take(c->plan_cache, (size_t)p->n_steps * words) || p->d_s_rec.take(c->plan_cache, (size_t)p->n_steps)) {
    p->d_gate_rec.reset();
    return fail(DSGD_ENOMEM, "out of device memory (plan record)");
  }
  p->gate_words = words;
  // (blocks from the cache were ordered against the BUILD stream: order them against the launch stream, which clears them)
  HIP_TRY(hipStreamSynchronize(c->build_stream ? c->build_stream : c->stream));
  HIP_TRY(hipMemsetAsync(p->d_gate_rec, 0, sizeof(unsigned int) * (size_t)p->n_steps * words, c->stream));
  HIP_TRY(hipMemsetAsync(p->d_s_rec, 0, sizeof(float) * (size_t)p->n_steps, c->stream));
  return DSGD_OK;
}

int dsgd_plan_read_record(dsgd_ctx* c, dsgd_plan* p, int64_t step_begin, int64_t step_end, uint32_t* gate_mask, float* s_used,
                          int32_t* mask_words_out) {
  DSGD_TRY(check_ctx(c));
  if (!p) return fail(DSGD_EINVAL, "null plan");
  if (p->lg) return fail(DSGD_EUNSUPPORTED, "dsgd_plan_read_record: a logistic plan keeps no record (there is no gate)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  if (mask_words_out) *mask_words_out = p->gate_words;
  if (!gate_mask && !s_used) return DSGD_OK;
  if (!p->d_gate_rec) return fail(DSGD_ESTATE, "the plan keeps no record (dsgd_plan_record)");
  if (!p->rp64 && !(p->cs_ok && p->cs_layout == c->layout_gen))
    return fail(DSGD_EUNSUPPORTED, "only plans that run on column slices and row-parallel fp64 plans keep a record (see dsgd_plan_info)");
  if (step_begin < 0 || step_end > p->n_steps || step_end < step_begin) return fail(DSGD_EINVAL, "steps outside the plan");
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t n = (size_t)(step_end - step_begin);
  if (gate_mask && n)
    HIP_TRY(hipMemcpy(gate_mask, p->d_gate_rec + (size_t)step_begin * p->gate_words, sizeof(unsigned int) * n * (size_t)p->gate_words,
                      hipMemcpyDeviceToHost));
  if (s_used && n) HIP_TRY(hipMemcpy(s_used, p->d_s_rec + step_begin, sizeof(float) * n, hipMemcpyDeviceToHost));
  return DSGD_OK;
}

#ifdef DSGD_TEST_COLLECTIVE_SEAM
// TEST BUILDS ONLY (tests/rccl_stub/libdsgd_hip_seam.so; the product library has no such symbol): from step `from_step`
// (1-based, counted inside each launch) on, slice 1 of every column-slice launch withholds its granules; 0 = off.
extern "C" int dsgd_test_cs_skip_publish(dsgd_ctx* c, int32_t from_step) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  c->k.cs_test_skip = from_step < 0 ? 0 : from_step;
  return DSGD_OK;
}
// ... and the bytes the library holds right now, counted where it allocates (csrc/dsgd_buf.hpp): the whole process', every
// context and dense engine together.  What a context took, dsgd_destroy gives back (tests/test_gpu_ctx_lifetime.py).
extern "C" void dsgd_test_live_bytes(int64_t* device_bytes, int64_t* pinned_bytes) {
  std::lock_guard<std::mutex> ld(g_live_dev.mu), lp(g_live_pin.mu);
  if (device_bytes) *device_bytes = g_live_dev.bytes;
  if (pinned_bytes) *pinned_bytes = g_live_pin.bytes;
}
#endif

int dsgd_plan_info(dsgd_ctx* c, dsgd_plan* p, int32_t* vals, int32_t n) {
  DSGD_TRY(check_ctx(c));
  if (!p || !vals || n < 0 || n > 9) return fail(DSGD_EINVAL, "bad plan_info arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  if (p->checked_load != c->load_gen) {   // (data loaded since: how the plan will run is a question about the new rows)
    DSGD_TRY(bind(c, true));
    DSGD_TRY(plan_revalidate(c, p));
  }
  const PlanRoute r = plan_route(c, p);
  const bool cs = r == PLAN_CS || r == PLAN_CS64 || r == PLAN_LG_CS;
  const int32_t all[9] = {plan_info_code(r, p->cs_layout == c->layout_gen || p->vt_layout == c->layout_gen),
                          cs ? p->cs_G : 0, cs ? p->cs_slot_stride : 0, cs ? p->cs_row_stride : 0, cs ? p->cs_cl_stride : 0,
                          cs ? p->cs_spl : 0, (cs && p->cs_device_built) ? 1 : 0, p->gate_words, cs ? p->cs_nt : 0};
  for (int i = 0; i < n; ++i) vals[i] = all[i];
  return DSGD_OK;
}

int dsgd_plan_destroy(dsgd_ctx* c, dsgd_plan* p) {
  DSGD_TRY(check_ctx(c));
  if (!p) return DSGD_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  c->comm_broken_ok = true;   // (a context whose communicator was given up can still let go of its plans)
  const int brc = bind(c, true);
  c->comm_broken_ok = false;
  DSGD_TRY(brc);
  // the plan's blocks go back to the context's cache behind everything the launch stream still holds (an event per block:
  // no hipFree, no device synchronisation -- an epoch of the reference is one plan); a set-up that never ran is ordered
  // in front of that first
  if (p->built_pending) HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
  // (the larger steps' tiles are allocated per plan and go with it: not before their last reader)
  if (p->d_vt_lanes || p->d_vt_segs || p->d_vt_long || p->d_vt_packed) HIP_TRY(hipStreamSynchronize(c->stream));
  plan_release(c, p);
  return DSGD_OK;
}

int dsgd_plan_run(dsgd_ctx* c, dsgd_plan* p, int64_t step_begin, int64_t step_end, float lr) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(plan_steps_check(p, step_begin, step_end));
  std::lock_guard<std::mutex> lk(c->mu);
  if (p->lg) return plan_run_lg(c, p, step_begin, step_end, lr);   // (its own refusals; dimSparsity plays no part)
  if (!p->rp64) DSGD_TRY(refuse_fp64_comm(c, "dsgd_plan_run"));   // (a row-parallel plan spans the ranks: plan_run_rp64_ranks)
  DSGD_TRY(bind(c, true));
  if (c->fp64) return plan_run64(c, p, step_begin, step_end, (double)lr);
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(plan_revalidate(c, p));   // (a plan from before the last load: DSGD_ERANGE here, before anything is enqueued)
  DSGD_TRY(prepare_layout(c));
  // the reference's own batch sizes: column slices, the whole range of steps in ONE launch (csrc/dsgd_cs.hpp)
  if (c->k.cs_enable && !c->comm) {
    if (p->cs_layout != c->layout_gen) {   // (created before the column layout existed, or the layout changed since)
      DSGD_TRY(cs_build(c, p));
      if (p->cs_device_built && c->build_stream) {
        HIP_TRY(hipEventRecord(p->built_ev, c->build_stream));
        p->built_pending = true;
      }
    }
  }
  if (p->built_pending) {   // the plan's set-up ran beside the launch stream: wait for it, once
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  PlanRoute r = plan_route(c, p);
  if (r == PLAN_CS) {
    if (step_end > step_begin) DSGD_TRY(launch_cs(c, p, step_begin, step_end, lr));
    c->pending_samples += p->offsets[step_end * p->n_workers] - p->offsets[step_begin * p->n_workers];
    return DSGD_OK;
  }
  DSGD_TRY(cs_unslice(c));   // (bound with the slice-major weights kept: the row-parallel kernels below read d_w)
  if (r == PLAN_ONE_WG) {
    if (step_end > step_begin) DSGD_TRY(launch_plan_kernel(c, p->d_idx, p->d_segs, step_begin, step_end, lr));
    c->pending_samples += p->offsets[step_end * p->n_workers] - p->offsets[step_begin * p->n_workers];
    return DSGD_OK;
  }
  DSGD_TRY(ensure_g(c, p->n_workers));
  DSGD_TRY(ensure_s(c, true));
  if (c->k.vt_enable && p->vt_layout != c->layout_gen) {   // (the tiles are laid out at the first run that needs them)
    DSGD_TRY(vt_build(c, p));
    r = plan_route(c, p);
  }
  const bool vt = r == PLAN_VT;
  for (int64_t s = step_begin; s < step_end; ++s) {
    if (vt) {   // the lists as virtual tiles over the split streams
      DSGD_TRY(launch_grad_vt(c, p, s));
      DSGD_TRY(launch_finish_sync(c, p->n_workers, lr));
      c->pending_samples += p->offsets[(s + 1) * p->n_workers] - p->offsets[s * p->n_workers];
      continue;
    }
    const WorkSeg* segs = p->d_segs + s * p->n_workers;
    long long mx = 0;
    for (int k = 0; k < p->n_workers; ++k)
      mx = std::max<long long>(mx, p->offsets[s * p->n_workers + k + 1] - p->offsets[s * p->n_workers + k]);
    DSGD_TRY(launch_grad(c, p->d_idx, segs, p->n_workers, mx, true));
    DSGD_TRY(launch_finish_sync(c, p->n_workers, lr));
    c->pending_samples += p->offsets[(s + 1) * p->n_workers] - p->offsets[s * p->n_workers];
  }
  return DSGD_OK;
}

// (rp64: dsgd_async_plan_create_rp64 -- the same lists into a row-parallel plan; lg: dsgd_async_plan_create_lg -- into a one-worker
//  LOGISTIC plan of an fp32 context, csrc/dsgd_lg_calls.hpp)
static int async_plan_impl(dsgd_ctx* c, const char* what, bool rp64, bool lg, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers,
                           int32_t batch, uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out) {
  DSGD_TRY(check_ctx(c));
  if (!assigned_begin || !assigned_end || !out || n_workers < 1 || batch < 1 || first_update < 0 || n_updates < 1)
    return fail(DSGD_EINVAL, "bad async plan arguments");
  {   // (refused with *out as it was)
    std::lock_guard<std::mutex> lk0(c->mu);
    if (lg) {
      DSGD_TRY(lg_refuse(c, what, LG_ONE_PROCESS));
    } else if (rp64) {
      DSGD_TRY(require_fp64(c, what));
      DSGD_TRY(refuse_fp64_comm(c, what));
    } else {
      DSGD_TRY(refuse_val64(c, what));
    }
  }
  *out = nullptr;
  for (int k = 0; k < n_workers; ++k) {
    const long long len = assigned_end[k] - assigned_begin[k];
    if (assigned_begin[k] < 0 || len < 1 || len > 0x7fffffffLL) return fail(DSGD_EINVAL, "worker %d has no rows", k);
  }
  if (n_updates > 0x7fffffffLL) return fail(DSGD_EINVAL, "at most 2^31 - 1 updates per plan");
  std::lock_guard<std::mutex> lk(c->mu);
  if (lg) {
    DSGD_TRY(lg_refuse(c, what, LG_ONE_PROCESS));
  } else {
    DSGD_TRY(require_fp64(c, what));
    DSGD_TRY(refuse_fp64_comm(c, what));
    if (!rp64) DSGD_TRY(refuse_val64(c, what));
  }
  DSGD_TRY(bind(c, true));   // (nothing here touches w)
  if (lg) DSGD_TRY(require_data(c));
  for (int k = 0; k < n_workers; ++k)
    if (assigned_end[k] > c->n_rows)
      return fail(DSGD_ERANGE, "worker %d's rows [%lld, %lld) outside the %lld loaded", k, (long long)assigned_begin[k],
                  (long long)assigned_end[k], c->n_rows);
  std::vector<int64_t> offsets((size_t)n_updates + 1);
  for (int64_t u = 0; u <= n_updates; ++u) offsets[(size_t)u] = u * batch;
  dsgd_plan* p = nullptr;
  DSGD_TRY(plan_frame(c, offsets.data(), n_updates, 1, &p, rp64, lg));
  p->idx_trusted = true;   // (drawn here inside the callers' row ranges)
  p->drawn = true;
  p->fits = false;
  std::vector<long long> sb2(2 * (size_t)n_workers);
  for (int k = 0; k < n_workers; ++k) {
    sb2[(size_t)k] = assigned_begin[k];
    sb2[(size_t)n_workers + (size_t)k] = assigned_end[k];
  }
  long long* d_sb = nullptr;
  hipError_t e = seed_scratch(c, 7, sizeof(long long) * sb2.size(), (void**)&d_sb);
  if (e == hipSuccess) e = hipMemcpyAsync(d_sb, sb2.data(), sizeof(long long) * sb2.size(), hipMemcpyHostToDevice, c->build_stream);
  if (e == hipSuccess) {
    AsyncListArgs a;
    a.asg_begin = d_sb;
    a.asg_end = d_sb + n_workers;
    a.K = n_workers;
    a.batch = batch;
    a.positional_bug = positional_bug ? 1 : 0;
    a.seed = seed;
    a.first = first_update;
    a.idx_out = p->d_idx;
    hipLaunchKernelGGL(dsgd_async_lists_kernel, dim3((unsigned)n_updates), dim3(256), 0, c->build_stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->build_stream);   // (sb2 and the scratch: done with before they go)
  if (e != hipSuccess) {
    plan_abandon(c, p);
    return fail(DSGD_EHIP, "drawing the async lists: %s", hipGetErrorString(e));
  }
  return plan_finish(c, p, out);
}
int dsgd_async_plan_create(dsgd_ctx* c, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                           uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out) {
  return async_plan_impl(c, "dsgd_async_plan_create", false, false, assigned_begin, assigned_end, n_workers, batch, seed, positional_bug, first_update,
                         n_updates, out);
}
int dsgd_async_plan_create_rp64(dsgd_ctx* c, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                                uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out) {
  return async_plan_impl(c, "dsgd_async_plan_create_rp64", true, false, assigned_begin, assigned_end, n_workers, batch, seed, positional_bug,
                         first_update, n_updates, out);
}

static int forward_run(dsgd_ctx* c, const int32_t* idx, int64_t n, float* pred_out);
int dsgd_forward(dsgd_ctx* c, const float* w, const int32_t* idx, int64_t n, float* pred_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 0 || (n > 0 && (!idx || !pred_out))) return fail(DSGD_EINVAL, "bad forward arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  if (w) DSGD_TRY(require_sync_mode(c));   // replacing the weights under the lock-free engine is refused
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  if (n == 0) return DSGD_OK;  // samplesIdx.map over an empty Seq is an empty reply (ref: core/Slave.scala:133)
  return forward_run(c, idx, n, pred_out);
}

int dsgd_forward_f64(dsgd_ctx* c, const double* w, const int32_t* idx, int64_t n, double* pred_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 0 || (n > 0 && (!idx || !pred_out))) return fail(DSGD_EINVAL, "bad forward arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_forward_f64"));
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  if (w) DSGD_TRY(require_sync_mode(c));   // replacing the weights under the lock-free engine is refused
  DSGD_TRY(prepare_layout(c));
  for (int64_t t = 0; t < n; ++t)   // (host data: checked before the weights are replaced)
    if (idx[t] < 0 || idx[t] >= c->n_rows) return fail(DSGD_ERANGE, "sample index %d outside the %lld loaded rows", idx[t], c->n_rows);
  if (w) {
    DSGD_TRY(put64(c, w, c->d_w64));   // (the Double weights as they are: no float rounding)
    c->s_dirty = true;
  }
  if (n == 0) return DSGD_OK;
  std::vector<float> pred((size_t)n);
  DSGD_TRY(forward_run(c, idx, n, pred.data()));
  for (int64_t t = 0; t < n; ++t) pred_out[t] = (double)pred[(size_t)t];   // (-1, 0 or +1: exact)
  return DSGD_OK;
}

// the predictions of n >= 1 rows from the resident weights (bound: rank order)
static int forward_run(dsgd_ctx* c, const int32_t* idx, int64_t n, float* pred_out) {
  DSGD_TRY(ensure_idx(c, n));
  DSGD_TRY(reset_counters(c));
  if ((size_t)n > c->d_pred.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_pred.reserve((size_t)std::max<long long>(n, 4096)));
  }
  float* d_pred = c->d_pred;
  DSGD_TRY(send_idx(c, idx, n));
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(float) * (size_t)n));
  const int G = c->group;
  dim3 grid(grid_for(c, n, G));
  CsrView m = view(c);
  if (c->fp64 && c->d_val64) {
    hipLaunchKernelGGL(dsgd_forward64v_kernel, dim3(grid_for(c, n, 16)), dim3(256), 0, c->stream, view64(c), c->d_w64, c->d_idx, (long long)n, d_pred, c->d_sc);
  } else if (c->fp64) {
    hipLaunchKernelGGL(dsgd_forward64_kernel, dim3(grid_for(c, n, 16)), dim3(256), 0, c->stream, m, c->d_w64, c->d_idx, (long long)n, d_pred, c->d_sc);
  } else switch (G) {
    case 64: hipLaunchKernelGGL(dsgd_forward_kernel<64>, grid, dim3(256), 0, c->stream, m, c->d_w, c->d_idx, (long long)n, d_pred, c->d_sc); break;
    case 32: hipLaunchKernelGGL(dsgd_forward_kernel<32>, grid, dim3(256), 0, c->stream, m, c->d_w, c->d_idx, (long long)n, d_pred, c->d_sc); break;
    case 16: hipLaunchKernelGGL(dsgd_forward_kernel<16>, grid, dim3(256), 0, c->stream, m, c->d_w, c->d_idx, (long long)n, d_pred, c->d_sc); break;
    default: hipLaunchKernelGGL(dsgd_forward_kernel<8>, grid, dim3(256), 0, c->stream, m, c->d_w, c->d_idx, (long long)n, d_pred, c->d_sc); break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, d_pred, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));
  memcpy(pred_out, c->pin_out.p, sizeof(float) * (size_t)n);
  return check_err_flag(c);
}

// the row-wise evaluation of rows [row_begin, row_end) on the rank-ordered weights `w` (the resident ones, or a snapshot of
// them: dsgd_async_check).  beside_engine: the shape that becomes resident next to the persistent Hogwild engine.
static int launch_eval_rows(dsgd_ctx* c, const float* w, long long row_begin, long long row_end, bool beside_engine) {
  const int G = c->group;
  // beside the persistent Hogwild engine (2 waves x 232 VGPRs per SIMD, 136 KB of LDS) only ONE more wave per SIMD
  // and 16 KB of LDS fit a CU: 256-lane blocks with a small weight tile, one per CU
  const int bs = beside_engine ? 256 : 1024;
  const long long groups_per_block = bs / G;
  const long long rows = row_end - row_begin;
  dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(c->n_cu, (rows + groups_per_block - 1) / groups_per_block)));
  // small ranges do not amortise staging 160 KiB of weights per workgroup: shrink the LDS tile
  const int hw = std::min(beside_engine ? std::min(c->hw_eval, 4096) : (rows >= 4096 ? c->hw_eval : std::min(c->hw_eval, 1024)),
                          DSGD_LDS_FLOATS - 4);
  const size_t lds = sizeof(float) * (size_t)(hw + 4);   // (+ the workgroup's three tally words)
  CsrView m = view(c);
  switch (G) {
    case 64: hipLaunchKernelGGL(dsgd_eval_kernel<64>, grid, dim3(bs), lds, c->stream, m, w, row_begin, row_end, c->d_sc, hw); break;
    case 32: hipLaunchKernelGGL(dsgd_eval_kernel<32>, grid, dim3(bs), lds, c->stream, m, w, row_begin, row_end, c->d_sc, hw); break;
    case 16: hipLaunchKernelGGL(dsgd_eval_kernel<16>, grid, dim3(bs), lds, c->stream, m, w, row_begin, row_end, c->d_sc, hw); break;
    default: hipLaunchKernelGGL(dsgd_eval_kernel<8>, grid, dim3(bs), lds, c->stream, m, w, row_begin, row_end, c->d_sc, hw); break;
  }
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// evaluation in three parts around the all-reduce of its tallies (one host thread, several contexts: dsgd_loss_acc_devices)
static int eval_enqueue(dsgd_ctx* c, const float* w, int64_t row_begin, int64_t row_end) {
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  if (row_end <= row_begin)  // samples.map(...).reduce on an empty collection throws (ref: SparseSVM.scala:21-23)
    return fail(DSGD_EINVAL, "empty row range: reduce on an empty sample list");
  if (row_begin < 0 || row_end > c->n_rows)
    return fail(DSGD_ERANGE, "rows [%lld, %lld) outside the %lld loaded rows", (long long)row_begin, (long long)row_end, c->n_rows);
  if (w) DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  // |w|^2 of the loss: cached with s while the synchronous kernels own w; while the lock-free engine runs w moves
  // under the cache, so every check recomputes it (MasterAsync's leaky loss check, core/MasterAsync.scala:96-162,
  // compares successive losses).  The engine keeps its own s (HogState), so refreshing d_sc here disturbs nothing.
  if (c->fp64) {   // fp64 tallies and |w|^2 (csrc/dsgd_cs64.hpp)
    DSGD_TRY(reset_counters(c));
    const long long rows = row_end - row_begin;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((long long)c->n_cu * 8, (rows + 15) / 16)));
    if (c->d_val64)
      hipLaunchKernelGGL(dsgd_eval64v_kernel, grid, dim3(256), 0, c->stream, view64(c), c->d_w64, (long long)row_begin, (long long)row_end, c->d_sc);
    else
      hipLaunchKernelGGL(dsgd_eval64_kernel, grid, dim3(256), 0, c->stream, view(c), c->d_w64, (long long)row_begin, (long long)row_end, c->d_sc);
    hipLaunchKernelGGL(dsgd_norm64_kernel, dim3(1), dim3(256), 0, c->stream, c->d_w64, c->dp, c->d_nsq64);
    HIP_TRY(hipGetLastError());
    return DSGD_OK;
  }
  if (c->async_running || c->nsq_dirty) c->s_dirty = true;
  DSGD_TRY(ensure_s(c));  // also refreshes |w|^2
  if (c->async_running) c->s_dirty = true;
  DSGD_TRY(reset_counters(c));
  if (!c->async_running && row_end - row_begin >= 4096) {
    std::vector<StreamSeg> ssegs(1, make_sseg(row_begin, row_end));
    DSGD_TRY(launch_stream<false>(c, ssegs));
  } else {
    DSGD_TRY(launch_eval_rows(c, c->d_w, (long long)row_begin, (long long)row_end, c->async_running));
  }
  return DSGD_OK;
}
static int eval_collective(dsgd_ctx* c) {
  if (!c->comm) return DSGD_OK;
  // shard-wise evaluation: three tallies + row count summed over ranks
  RCCL_TRY(rccl::AllReduce(c->d_sc->counts, c->d_sc->counts, 4, rccl::kInt64, rccl::kSum, c->comm, c->stream));
  return DSGD_OK;
}
static int eval_read(dsgd_ctx* c, double* loss, double* acc, int64_t* counts) {
  long long tallies[4] = {0, 0, 0, 0};
  DSGD_TRY(read_scalars(c));
  for (int i = 0; i < 4; ++i) tallies[i] = (long long)c->h_sc->counts[i];
  const double n = (double)tallies[3];
  double nsq = (double)c->h_sc->wnorm2;
  if (c->fp64) HIP_TRY(hipMemcpy(&nsq, c->d_nsq64, sizeof(double), hipMemcpyDeviceToHost));
  if (loss) *loss = c->cfg.lambda * nsq + ((double)tallies[1] + 2.0 * (double)tallies[2]) / n;
  if (acc) *acc = (double)tallies[0] / n;
  if (counts) {
    counts[0] = tallies[0];
    counts[1] = tallies[1];
    counts[2] = tallies[2];
  }
  return DSGD_OK;
}

int dsgd_loss_acc(dsgd_ctx* c, const float* w, int64_t row_begin, int64_t row_end, double* loss, double* acc,
                  int64_t* counts) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(eval_enqueue(c, w, row_begin, row_end));
  DSGD_TRY(eval_collective(c));
  return eval_read(c, loss, acc, counts);
}

#include "dsgd_lg_calls.hpp"   // (the logistic model's entry points: dsgd_lg_*)
#include "dsgd_lg_topics_calls.hpp"   // (... over several topics: dsgd_lg_topics_*)

// ---- distributed evaluation (csrc/dsgd_predict.hpp; ref: core/Master.scala:61-98) ----
// The checks of dsgd_predict_ranges / _f64 that need no device: nothing has changed when one of them fails.
static int predict_check(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges, const int8_t* pred_out,
                         long long* total_out) {
  if (n_ranges < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "bad predict arguments: no ranges");
  if (n_ranges > PRED_MAX_RANGES) return fail(DSGD_EINVAL, "%d ranges in one call (at most %d)", n_ranges, PRED_MAX_RANGES);
  if (!pred_out) return fail(DSGD_EINVAL, "null pred_out");
  long long total = 0;
  std::vector<std::pair<long long, long long>> iv;
  for (int k = 0; k < n_ranges; ++k) {
    if (row_begin[k] > row_end[k])
      return fail(DSGD_EINVAL, "range %d: begin %lld > end %lld", k, (long long)row_begin[k], (long long)row_end[k]);
    if (row_begin[k] == row_end[k]) continue;   // an empty split: an empty reply (ref: core/Slave.scala:133 over an empty Seq)
    if (row_begin[k] < 0 || row_end[k] > c->n_rows)
      return fail(DSGD_ERANGE, "rows [%lld, %lld) of range %d outside the %lld loaded rows", (long long)row_begin[k], (long long)row_end[k], k,
                  c->n_rows);
    iv.emplace_back((long long)row_begin[k], (long long)row_end[k]);
    total += row_end[k] - row_begin[k];
  }
  // preds.size is the row count only while no row repeats: .toMap collapses repeated keys (core/Master.scala:73)
  std::sort(iv.begin(), iv.end());
  for (size_t i = 1; i < iv.size(); ++i)
    if (iv[i].first < iv[i - 1].second)
      return fail(DSGD_EINVAL, "ranges overlap: [%lld, %lld) and [%lld, %lld)", iv[i - 1].first, iv[i - 1].second, iv[i].first, iv[i].second);
  if (total == 0)   // preds.map(...).reduce over an empty map throws (core/Master.scala:96)
    return fail(DSGD_EINVAL, "no rows in any range: reduce on an empty prediction map");
  *total_out = total;
  return DSGD_OK;
}

// the launch, the copies back and the fold, from the resident weights (bound; the ranges checked)
static int predict_run(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int K, long long total, int8_t* pred_out,
                       int64_t* counts_out, double* loss, double* acc) {
  const size_t tab_words = (size_t)(2 * K + 1), cnt_words = (size_t)(3 * K);
  if (!c->d_pred_tab || (size_t)total > c->d_pred8.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_pred_tab.reserve((size_t)(2 * PRED_MAX_RANGES + 1) + 3 * PRED_MAX_RANGES));
    DSGD_TRY(c->d_pred8.reserve((size_t)std::max<long long>(total, 4096), Grow::twice));
  }
  long long* d_tab = c->d_pred_tab;
  unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d_tab + (2 * PRED_MAX_RANGES + 1));
  // |w|^2 of the loss, as dsgd_loss_acc takes it (eval_enqueue)
  if (loss && c->fp64) {
    hipLaunchKernelGGL(dsgd_norm64_kernel, dim3(1), dim3(256), 0, c->stream, c->d_w64, c->dp, c->d_nsq64);
  } else if (loss) {
    if (c->nsq_dirty) c->s_dirty = true;
    DSGD_TRY(ensure_s(c));
  }
  DSGD_TRY(pin_acquire(c->pin_idx, sizeof(long long) * tab_words));
  long long* h_tab = static_cast<long long*>(c->pin_idx.p.get());
  h_tab[0] = 0;
  for (int k = 0; k < K; ++k) {
    h_tab[k + 1] = h_tab[k] + (long long)(row_end[k] - row_begin[k]);
    h_tab[K + 1 + k] = (long long)row_begin[k];
  }
  HIP_TRY(hipMemcpyAsync(d_tab, h_tab, sizeof(long long) * tab_words, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_idx));
  HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * cnt_words, c->stream));
  signed char* d_pred = c->d_pred8;
  if (c->fp64) {
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((long long)c->n_cu * 8, (total + 15) / 16)));
    const size_t lds = sizeof(float) * (size_t)pred_lds_words(K);
    if (c->d_val64)
      hipLaunchKernelGGL(dsgd_predict64v_kernel, grid, dim3(256), lds, c->stream, view64(c), c->d_w64, d_tab, K, d_pred, d_cnt);
    else
      hipLaunchKernelGGL(dsgd_predict64_kernel, grid, dim3(256), lds, c->stream, view(c), c->d_w64, d_tab, K, d_pred, d_cnt);
  } else {
    // dsgd_eval_kernel's launch: one 1024-lane workgroup per CU at most, a small weight tile for small calls
    const int G = c->group;
    const long long groups_per_block = 1024 / G;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(c->n_cu, (total + groups_per_block - 1) / groups_per_block)));
    const int hw = std::min(total >= 4096 ? c->hw_eval : std::min(c->hw_eval, 1024), (DSGD_LDS_FLOATS - pred_lds_words(K)) & ~3);
    const size_t lds = sizeof(float) * (size_t)(((hw + 3) & ~3) + pred_lds_words(K));
    CsrView m = view(c);
    switch (G) {
      case 64: hipLaunchKernelGGL(dsgd_predict_kernel<64>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_tab, K, d_pred, d_cnt, hw); break;
      case 32: hipLaunchKernelGGL(dsgd_predict_kernel<32>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_tab, K, d_pred, d_cnt, hw); break;
      case 16: hipLaunchKernelGGL(dsgd_predict_kernel<16>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_tab, K, d_pred, d_cnt, hw); break;
      default: hipLaunchKernelGGL(dsgd_predict_kernel<8>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_tab, K, d_pred, d_cnt, hw); break;
    }
  }
  HIP_TRY(hipGetLastError());
  // both replies through the pinned buffer: the tallies in front (8-byte aligned), the bytes behind them
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(unsigned long long) * cnt_words + (size_t)total));
  unsigned long long* h_cnt = static_cast<unsigned long long*>(c->pin_out.p.get());
  signed char* h_pred = reinterpret_cast<signed char*>(h_cnt + cnt_words);
  HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, sizeof(unsigned long long) * cnt_words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h_pred, d_pred, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // (synchronises; wnorm2 of the fp32 loss)
  memcpy(pred_out, h_pred, (size_t)total);
  long long t3[3] = {0, 0, 0};
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < 3; ++j) {
      t3[j] += (long long)h_cnt[3 * k + j];
      if (counts_out) counts_out[3 * k + j] = (int64_t)h_cnt[3 * k + j];
    }
  if (t3[0] + t3[1] + t3[2] != total) return fail(DSGD_ESTATE, "internal: %lld rows tallied of %lld", t3[0] + t3[1] + t3[2], total);
  const double n = (double)total;
  if (loss) {
    double nsq = (double)c->h_sc->wnorm2;
    if (c->fp64) HIP_TRY(hipMemcpy(&nsq, c->d_nsq64, sizeof(double), hipMemcpyDeviceToHost));
    *loss = c->cfg.lambda * nsq + ((double)t3[1] + 2.0 * (double)t3[2]) / n;   // (eval_read's expression)
  }
  if (acc) *acc = (double)t3[0] / n;
  return DSGD_OK;
}

int dsgd_predict_ranges(dsgd_ctx* c, const float* w, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges,
                        int8_t* pred_out, int64_t* counts_out, double* loss, double* acc) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->fp64 && w)
    return fail(DSGD_EINVAL, "dsgd_predict_ranges on an fp64 context takes w == NULL (the resident Double weights); "
                             "dsgd_predict_ranges_f64 takes a Double w");
  DSGD_TRY(require_data(c));
  long long total = 0;
  DSGD_TRY(predict_check(c, row_begin, row_end, n_ranges, pred_out, &total));
  DSGD_TRY(require_sync_mode(c));   // (the concurrent loss check of the lock-free engine is dsgd_loss_acc's)
  if (loss && !c->fp64) DSGD_TRY(require_ds(c));   // (|w|^2 comes with s, as in dsgd_loss_acc)
  DSGD_TRY(bind(c));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  return predict_run(c, row_begin, row_end, n_ranges, total, pred_out, counts_out, loss, acc);
}

int dsgd_predict_ranges_f64(dsgd_ctx* c, const double* w, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges,
                            int8_t* pred_out, int64_t* counts_out, double* loss, double* acc) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_predict_ranges_f64"));
  DSGD_TRY(require_data(c));
  long long total = 0;
  DSGD_TRY(predict_check(c, row_begin, row_end, n_ranges, pred_out, &total));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(bind(c));
  DSGD_TRY(prepare_layout(c));
  if (w) {
    DSGD_TRY(put64(c, w, c->d_w64));   // (the Double weights as they are: no float rounding)
    c->s_dirty = true;
  }
  return predict_run(c, row_begin, row_end, n_ranges, total, pred_out, counts_out, loss, acc);
}

// ---- evaluation over a list of rows, given or drawn (csrc/dsgd_eval_list.hpp; ref: core/Master.scala:109-118) ----
// |w|^2 of the loss, ONE launch over the n >= 1 rows c->d_idx names, the tallies back (bound, the weights resident, the list
// enqueued on the context's stream).  Outputs are written when everything has succeeded, idx_out (n entries) among them.
static int eval_list_run(dsgd_ctx* c, long long n, double* loss, double* acc, int64_t* counts, int32_t* idx_out) {
  // |w|^2 as dsgd_predict_ranges takes it
  if (loss && c->fp64) {
    hipLaunchKernelGGL(dsgd_norm64_kernel, dim3(1), dim3(256), 0, c->stream, c->d_w64, c->dp, c->d_nsq64);
  } else if (loss) {
    if (c->nsq_dirty) c->s_dirty = true;
    DSGD_TRY(ensure_s(c));
  }
  DSGD_TRY(reset_counters(c));
  const int* d_idx = c->d_idx;
  if (c->fp64) {
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((long long)c->n_cu * 8, (n + 15) / 16)));
    if (c->d_val64)
      hipLaunchKernelGGL(dsgd_eval_list64v_kernel, grid, dim3(256), 0, c->stream, view64(c), c->d_w64, d_idx, n, c->d_sc);
    else
      hipLaunchKernelGGL(dsgd_eval_list64_kernel, grid, dim3(256), 0, c->stream, view(c), c->d_w64, d_idx, n, c->d_sc);
  } else {
    // dsgd_predict_ranges' launch: one 1024-lane workgroup per CU at most, a small weight tile for small calls
    const int G = c->group;
    const long long groups_per_block = 1024 / G;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(c->n_cu, (n + groups_per_block - 1) / groups_per_block)));
    const int hw = std::min(n >= 4096 ? c->hw_eval : std::min(c->hw_eval, 1024), DSGD_LDS_FLOATS - 4);
    const size_t lds = sizeof(float) * (size_t)(hw + 4);   // (+ the workgroup's tally words)
    CsrView m = view(c);
    switch (G) {
      case 64: hipLaunchKernelGGL(dsgd_eval_list_kernel<64>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_idx, n, c->d_sc, hw); break;
      case 32: hipLaunchKernelGGL(dsgd_eval_list_kernel<32>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_idx, n, c->d_sc, hw); break;
      case 16: hipLaunchKernelGGL(dsgd_eval_list_kernel<16>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_idx, n, c->d_sc, hw); break;
      default: hipLaunchKernelGGL(dsgd_eval_list_kernel<8>, grid, dim3(1024), lds, c->stream, m, c->d_w, d_idx, n, c->d_sc, hw); break;
    }
  }
  HIP_TRY(hipGetLastError());
  if (idx_out) {
    DSGD_TRY(pin_acquire(c->pin_out, sizeof(int) * (size_t)n));
    HIP_TRY(hipMemcpyAsync(c->pin_out.p, d_idx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  }
  DSGD_TRY(read_scalars(c));   // (synchronises; wnorm2 of the fp32 loss)
  DSGD_TRY(check_err_flag(c));
  long long t3[3];
  for (int j = 0; j < 3; ++j) t3[j] = (long long)c->h_sc->counts[j];
  if (t3[0] + t3[1] + t3[2] != n) return fail(DSGD_ESTATE, "internal: %lld rows tallied of %lld", t3[0] + t3[1] + t3[2], n);
  double nsq = (double)c->h_sc->wnorm2;
  if (loss && c->fp64) HIP_TRY(hipMemcpy(&nsq, c->d_nsq64, sizeof(double), hipMemcpyDeviceToHost));
  if (loss) *loss = c->cfg.lambda * nsq + ((double)t3[1] + 2.0 * (double)t3[2]) / (double)n;   // (eval_read's expression)
  if (acc) *acc = (double)t3[0] / (double)n;
  for (int j = 0; counts && j < 3; ++j) counts[j] = (int64_t)t3[j];
  if (idx_out) memcpy(idx_out, c->pin_out.p, sizeof(int) * (size_t)n);
  return DSGD_OK;
}

// what the float and the Double form of a call share up to the layout: dsgd_predict_ranges' / _f64's rules for w and the mode
static int eval_list_mode(dsgd_ctx* c, const char* what, bool f64, bool have_w) {
  if (f64) DSGD_TRY(require_fp64(c, what));
  else if (c->fp64 && have_w)
    return fail(DSGD_EINVAL, "%s on an fp64 context takes w == NULL (the resident Double weights); %s_f64 takes a Double w", what, what);
  DSGD_TRY(require_data(c));
  return DSGD_OK;
}
// the weights of a call replace the resident ones (bound, the layout prepared)
static int eval_list_weights(dsgd_ctx* c, const float* w, const double* w64) {
  if (w) DSGD_TRY(set_weights_locked(c, w));
  if (w64) {
    DSGD_TRY(put64(c, w64, c->d_w64));   // (the Double weights as they are: no float rounding)
    c->s_dirty = true;
  }
  return DSGD_OK;
}

static int loss_acc_list_impl(dsgd_ctx* c, const char* what, bool f64, const float* w, const double* w64, const int32_t* idx, int64_t n,
                              double* loss, double* acc, int64_t* counts) {
  DSGD_TRY(check_ctx(c));
  if (!idx || n < 1)   // samples.map(...).reduce on an empty collection throws (ref: SparseSVM.scala:21-23)
    return fail(DSGD_EINVAL, "%s: no list, or an empty one (reduce on an empty sample list)", what);
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(eval_list_mode(c, what, f64, w != nullptr));
  DSGD_TRY(require_sync_mode(c));
  if (loss && !c->fp64) DSGD_TRY(require_ds(c));   // (|w|^2 comes with s, as in dsgd_loss_acc)
  DSGD_TRY(bind(c));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(eval_list_weights(c, w, w64));
  DSGD_TRY(ensure_idx(c, n));
  DSGD_TRY(send_idx(c, idx, n));
  return eval_list_run(c, n, loss, acc, counts, nullptr);
}
int dsgd_loss_acc_list(dsgd_ctx* c, const float* w, const int32_t* idx, int64_t n, double* loss, double* acc, int64_t* counts) {
  return loss_acc_list_impl(c, "dsgd_loss_acc_list", false, w, nullptr, idx, n, loss, acc, counts);
}
int dsgd_loss_acc_list_f64(dsgd_ctx* c, const double* w, const int32_t* idx, int64_t n, double* loss, double* acc, int64_t* counts) {
  return loss_acc_list_impl(c, "dsgd_loss_acc_list_f64", true, nullptr, w, idx, n, loss, acc, counts);
}

// The first n entries of Random.shuffle(0 until len) as the rows row_begin + entry, drawn into c->d_idx on the context's
// stream: a one-worker, one-step job of dsgd_plan_create_from_seed_job with max_samples = batch_size = n (seed_walk and
// seed_draw of csrc/dsgd_seed_host.hpp, a scratch list in place of a plan).  Refuses before anything is enqueued.
static int sampled_draw(dsgd_ctx* c, const char* what, unsigned long long s0, int64_t row_begin, long long len, long long n, long long* draws) {
  DSGD_TRY(ensure_idx(c, n));
  *draws = 0;
  if (len == 1) {   // (a shuffle of one entry draws nothing: the row itself)
    DSGD_TRY(pin_acquire(c->pin_idx, sizeof(int)));
    *static_cast<int*>(c->pin_idx.p.get()) = (int)row_begin;
    HIP_TRY(hipMemcpyAsync(c->d_idx, c->pin_idx.p, sizeof(int), hipMemcpyHostToDevice, c->stream));
    return pin_sent(c, c->pin_idx);
  }
  const int chunks = (int)((n + JR_MAX_TAKE - 1) / JR_MAX_TAKE);
  const SeedRequest r{what, false, true, true, std::vector<long long>(1, len), 0, 1, &row_begin, (int)n, 0x7fffffff, chunks, JR_JOB_MAX_REJ, ""};
  const JrFrame f = jr_frame(r.len, 0, 1, 1, (int)n);
  DSGD_TRY(ensure_build_stream(c));
  const SeedLaps lap;
  JrWalked w;
  DSGD_TRY(seed_walk(c, r, f, s0, len, lap, &w));
  DSGD_TRY(seed_draw(c, r, f, w, s0, len, c->d_idx, c->stream, lap));
  *draws = f.nominal + w.rej_total;
  return DSGD_OK;
}

static int loss_acc_sampled_impl(dsgd_ctx* c, const char* what, bool f64, const float* w, const double* w64, uint64_t* jstate, int64_t row_begin,
                                 int64_t row_end, int64_t samples_count, double* loss, double* acc, int64_t* counts, int32_t* idx_out,
                                 int64_t* n_out, int64_t* draws_out) {
  DSGD_TRY(check_ctx(c));
  if (!jstate) return fail(DSGD_EINVAL, "%s: null jstate", what);
  if (samples_count < 1 || row_begin >= row_end)   // (the JVM would have spent the shuffle's draws before .reduce throws; not here)
    return fail(DSGD_EINVAL, "%s: an empty sample (samples_count %lld of rows [%lld, %lld)): reduce on an empty sample list", what,
                (long long)samples_count, (long long)row_begin, (long long)row_end);
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(eval_list_mode(c, what, f64, w != nullptr));
  if (row_begin < 0 || row_end > c->n_rows)
    return fail(DSGD_ERANGE, "rows [%lld, %lld) outside the %lld loaded rows", (long long)row_begin, (long long)row_end, c->n_rows);
  DSGD_TRY(require_sync_mode(c));
  if (loss && !c->fp64) DSGD_TRY(require_ds(c));
  const long long len = row_end - row_begin, n = std::min<long long>(samples_count, len);   // (the reference's `take`)
  if (len > JR_MAX_LEN) return fail(DSGD_EUNSUPPORTED, "%s draws windows up to %d rows (dsgd_jrand_shuffle, then %s)", what, JR_MAX_LEN,
                                    f64 ? "dsgd_loss_acc_list_f64" : "dsgd_loss_acc_list");
  DSGD_TRY(bind(c));
  DSGD_TRY(prepare_layout(c));
  const unsigned long long s0 = *jstate & JR_MASK;
  long long draws = 0;
  DSGD_TRY(sampled_draw(c, what, s0, row_begin, len, n, &draws));   // (a refusal leaves the weights as they were)
  DSGD_TRY(eval_list_weights(c, w, w64));
  DSGD_TRY(eval_list_run(c, n, loss, acc, counts, idx_out));
  *jstate = jr_jump_dev(s0, (unsigned long long)draws);
  if (n_out) *n_out = n;
  if (draws_out) *draws_out = draws;
  return DSGD_OK;
}
int dsgd_loss_acc_sampled(dsgd_ctx* c, const float* w, uint64_t* jstate, int64_t row_begin, int64_t row_end, int64_t samples_count, double* loss,
                          double* acc, int64_t* counts, int32_t* idx_out, int64_t* n_out, int64_t* draws_out) {
  return loss_acc_sampled_impl(c, "dsgd_loss_acc_sampled", false, w, nullptr, jstate, row_begin, row_end, samples_count, loss, acc, counts, idx_out,
                               n_out, draws_out);
}
int dsgd_loss_acc_sampled_f64(dsgd_ctx* c, const double* w, uint64_t* jstate, int64_t row_begin, int64_t row_end, int64_t samples_count,
                              double* loss, double* acc, int64_t* counts, int32_t* idx_out, int64_t* n_out, int64_t* draws_out) {
  return loss_acc_sampled_impl(c, "dsgd_loss_acc_sampled_f64", true, nullptr, w, jstate, row_begin, row_end, samples_count, loss, acc, counts,
                               idx_out, n_out, draws_out);
}

int dsgd_async_step(dsgd_ctx* c, const int32_t* idx, int64_t n, float lr, float* delta_out, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_async_step"));
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(ensure_s(c));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  const int64_t nn = n;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, 1, mx));
  hipLaunchKernelGGL(dsgd_async_finish_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_w, c->d_g, c->dp, c->d_ds, (float)n,
                     lr, (float)c->cfg.lambda, delta_out ? c->d_tmp : (float*)nullptr, c->d_sc);
  HIP_TRY(hipGetLastError());
  c->s_dirty = false;
  if (delta_out) {
    DSGD_TRY(launch_permute_out(c, c->d_tmp, c->d_io));
    HIP_TRY(hipMemcpyAsync(delta_out, c->d_io, sizeof(float) * c->dp, hipMemcpyDeviceToHost, c->stream));
  }
  return finish_stats(c, stats, tot);
}

int dsgd_update_grad(dsgd_ctx* c, const int32_t* key, const float* dv, int64_t nnz) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_update_grad"));
  if (nnz < 0 || (nnz > 0 && (!key || !dv))) return fail(DSGD_EINVAL, "bad update arguments");
  if (nnz == 0) return DSGD_OK;
  for (int64_t i = 0; i < nnz; ++i)   // the keys are host data: validated here, no device-side error flag to wait for
    if (key[i] < 0 || key[i] >= c->dp) return fail(DSGD_ERANGE, "key %d at position %lld outside [0, %d]", key[i], (long long)i, c->dp - 1);
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  // The reference applies a peer's update while its own asyncTask runs (core/Slave.scala:177-185 is an RPC handler on
  // another pool thread).  Here: pinned staging + a persistent device buffer (hipMalloc / hipFree per call -- hipFree
  // synchronises the DEVICE, i.e. waits for the persistent engine to reach its update budget), the copy and the kernel
  // on a side stream while the engine is resident, atomic adds to w, and the engine's incremental regulariser scalar
  // told about the foreign update.
  if (!c->upd_stream) HIP_TRY(hipStreamCreateWithFlags(&c->upd_stream, hipStreamNonBlocking));
  const long long upd_cap = std::max<long long>(c->dp, 4096);   // a Sparse delta holds at most D + 1 entries; longer inputs go in pieces
  DSGD_TRY(c->d_upd_key.reserve((size_t)upd_cap));
  DSGD_TRY(c->d_upd_dv.reserve((size_t)upd_cap));
  // (an engine that has reached its budget but has not been joined yet is not live: its kernel has exited, nothing adds
  //  to w any more and nobody reads HogState::s_reg -- the update takes the plain path with the Sparse filter pass)
  const bool live = c->async_running && !(c->exch_done.load() && hipStreamQuery(c->async_stream) == hipSuccess);
  hipStream_t st = live ? c->upd_stream : c->stream;
  for (int64_t o = 0; o < nnz; o += upd_cap) {
    const long long n = std::min<long long>(upd_cap, nnz - o);
    DSGD_TRY(pin_acquire(c->pin_upd, (sizeof(int) + sizeof(float)) * (size_t)n));
    int* pk = static_cast<int*>(c->pin_upd.p.get());
    float* pv = reinterpret_cast<float*>(pk + n);
    memcpy(pk, key + o, sizeof(int) * (size_t)n);
    memcpy(pv, dv + o, sizeof(float) * (size_t)n);
    HIP_TRY(hipMemcpyAsync(c->d_upd_key, pk, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->d_upd_dv, pv, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st));
    DSGD_TRY(pin_sent(c, c->pin_upd, st));
    const int blocks = (int)std::min<long long>((n + 255) / 256, 64);
    hipLaunchKernelGGL(dsgd_update_grad_kernel, dim3(blocks), dim3(256), 0, st, c->d_w, c->d_perm, c->d_ds, c->d_upd_key,
                       c->d_upd_dv, n, (float)c->cfg.lambda, live ? &c->d_hog->s_reg : (float*)nullptr);
    HIP_TRY(hipGetLastError());
  }
  if (!live) {
    // the Sparse filter pass rewrites every w[j] non-atomically: only while no engine is adding to w
    hipLaunchKernelGGL(dsgd_filter_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, st, c->d_w, c->dp);
    HIP_TRY(hipGetLastError());
  }
  c->s_dirty = true;
  HIP_TRY(hipStreamSynchronize(st));   // the update is applied when the call returns (the RPC's Ack, proto.proto:40)
  return DSGD_OK;
}

// The logistic model's peer update (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS; the state rules are lg_enter's,
// csrc/dsgd_lg_calls.hpp): Double values, w_k = (float)((double)w_k - dv_k), no filter pass and no running engine beside it.
int dsgd_lg_update_grad(dsgd_ctx* c, const int32_t* key, const double* dv, int64_t nnz) {
  DSGD_TRY(check_ctx(c));
  if (nnz < 0 || (nnz > 0 && (!key || !dv))) return fail(DSGD_EINVAL, "dsgd_lg_update_grad: bad update arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lg_refuse(c, "dsgd_lg_update_grad", LG_ONE_PROCESS));
  if (nnz == 0) return DSGD_OK;
  {   // the keys are host data: validated here, before anything moves (a delta holds each key once)
    std::vector<unsigned char> seen((size_t)c->dp, 0);
    for (int64_t i = 0; i < nnz; ++i)
      if (key[i] < 0 || key[i] >= c->dp)
        return fail(DSGD_ERANGE, "dsgd_lg_update_grad: key %d at position %lld outside [0, %d]", key[i], (long long)i, c->dp - 1);
    for (int64_t i = 0; i < nnz; ++i) {
      if (seen[(size_t)key[i]])
        return fail(DSGD_EINVAL, "dsgd_lg_update_grad: key %d repeated at position %lld: a delta has unique keys", key[i], (long long)i);
      seen[(size_t)key[i]] = 1;
    }
  }
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_update_grad", LG_ONE_PROCESS, &fresh));
  if (c->d_lg_upd_key.cap() < (size_t)nnz || c->d_lg_upd_dv.cap() < (size_t)nnz) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lg_upd_key.reserve((size_t)std::max<long long>(nnz, c->dp)));
    DSGD_TRY(c->d_lg_upd_dv.reserve((size_t)std::max<long long>(nnz, c->dp)));
  }
  HIP_TRY(hipMemcpyAsync(c->d_lg_upd_key, key, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_lg_upd_dv, dv, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
  const long long blocks = std::max<long long>(1, std::min<long long>((nnz + LG_THREADS - 1) / LG_THREADS, (long long)c->n_cu * 8));
  hipLaunchKernelGGL(dsgd_lg_update_kernel, dim3((unsigned)blocks), dim3(LG_THREADS), 0, c->stream, c->d_lg_upd_key.get(), c->d_lg_upd_dv.get(),
                     (long long)nnz, c->d_perm.get(), c->d_w.get(), c->dp);
  HIP_TRY(hipGetLastError());
  c->s_dirty = true;                 // weights that came another way: the SVM's s and every |w|^2 word are stale
  c->lg_nsq_stamp = ~0ull - 1;
  HIP_TRY(hipStreamSynchronize(c->stream));   // (key and dv are the caller's: done with before the call returns)
  return DSGD_OK;
}


// ---- the Sparse forms (include/dsgd.h "SPARSE VALUES"): the dense twins' kernels, state rules and errors ----
int dsgd_set_weights_sparse(dsgd_ctx* c, const int32_t* key, const float* val, int64_t nnz) {
  DSGD_TRY(check_ctx(c));
  if (nnz < 0 || (nnz > 0 && (!key || !val))) return fail(DSGD_EINVAL, "null key / value arrays or negative nnz");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(sp_check_keys(c, key, val, nnz));
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));
  if (c->fp64) return sp_scatter<float, double>(c, key, val, nnz, c->d_w64);   // (promoted, as dsgd_set_weights)
  return sp_scatter<float, float>(c, key, val, nnz, c->d_w);
}

int dsgd_set_weights_sparse_f64(dsgd_ctx* c, const int32_t* key, const double* val, int64_t nnz) {
  DSGD_TRY(check_ctx(c));
  if (nnz < 0 || (nnz > 0 && (!key || !val))) return fail(DSGD_EINVAL, "null key / value arrays or negative nnz");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_set_weights_sparse_f64"));
  DSGD_TRY(sp_check_keys(c, key, val, nnz));
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));
  return sp_scatter<double, double>(c, key, val, nnz, c->d_w64);
}

int dsgd_get_weights_sparse(dsgd_ctx* c, int32_t* key_out, float* val_out, int64_t cap, int64_t* nnz_out) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(sp_check_out(key_out, val_out, cap, nnz_out));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (c->fp64)   // (the fp64 weights rounded, as dsgd_get_weights)
    DSGD_TRY((sp_compact<double, float, false>(c, c->d_w64, c->d_perm)));
  else
    DSGD_TRY((sp_compact<float, float, false>(c, c->d_w, c->d_perm)));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return sp_deliver<float>(c, key_out, val_out, cap, nnz_out);
}

int dsgd_get_weights_sparse_f64(dsgd_ctx* c, int32_t* key_out, double* val_out, int64_t cap, int64_t* nnz_out) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(sp_check_out(key_out, val_out, cap, nnz_out));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_get_weights_sparse_f64"));
  DSGD_TRY(bind(c));
  DSGD_TRY((sp_compact<double, double, false>(c, c->d_w64, c->d_perm)));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return sp_deliver<double>(c, key_out, val_out, cap, nnz_out);
}

int dsgd_gradient_sparse(dsgd_ctx* c, const int32_t* w_key, const float* w_val, int64_t w_nnz, const int32_t* idx, int64_t n, int32_t* g_key,
                         float* g_val, int64_t cap, int64_t* g_nnz, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_gradient_sparse"));
  DSGD_TRY(sp_check_out(g_key, g_val, cap, g_nnz));
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");  // ref: math/Vec.scala:129
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(sp_check_keys(c, w_key, w_val, w_nnz));
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(sp_ensure(c));
  if (w_nnz >= 0) DSGD_TRY((sp_scatter<float, float>(c, w_key, w_val, w_nnz, c->d_w)));
  DSGD_TRY(ensure_s(c));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  const int64_t nn = n;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, 1, mx));
  // ONE launch in place of dsgd_regularize_kernel + permute-out + memset: the support-only regulariser on the way, d_g cleared
  DSGD_TRY((sp_compact<float, float, true>(c, c->d_g, c->d_perm)));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(prof_collect(c));
  DSGD_TRY(check_err_flag(c));
  DSGD_TRY(sp_deliver<float>(c, g_key, g_val, cap, g_nnz));
  if (stats) {
    stats->n_samples = n;
    stats->n_active = (int64_t)c->h_sc->n_active;
  }
  return DSGD_OK;
}

int dsgd_gradient_sparse_f64(dsgd_ctx* c, const int32_t* w_key, const double* w_val, int64_t w_nnz, const int32_t* idx, int64_t n,
                             int32_t* g_key, double* g_val, int64_t cap, int64_t* g_nnz, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(sp_check_out(g_key, g_val, cap, g_nnz));
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");  // ref: math/Vec.scala:129
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_gradient_sparse_f64"));
  DSGD_TRY(sp_check_keys(c, w_key, w_val, w_nnz));
  DSGD_TRY(bind(c, w_nnz < 0));   // (the request's weights replace the resident ones: rank order then)
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  const int64_t nn = n;
  DSGD_TRY(rp64_check_lists(c, &idx, &nn, 1));
  DSGD_TRY(sp_ensure(c));
  if (w_nnz >= 0) DSGD_TRY((sp_scatter<double, double>(c, w_key, w_val, w_nnz, c->d_w64)));
  DSGD_TRY(rp64_ensure(c, 1));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(rp64_launch(c, 1, mx, RP64_GRADIENT, 0.0));
  DSGD_TRY((sp_compact<double, double, false>(c, c->d_rp64_g, nullptr)));   // (the finish leaves the gradient in key order)
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  DSGD_TRY(sp_deliver<double>(c, g_key, g_val, cap, g_nnz));
  if (stats) {
    stats->n_samples = n;
    stats->n_active = (int64_t)c->h_sc->n_active;
  }
  return DSGD_OK;
}

int dsgd_async_step_sparse(dsgd_ctx* c, const int32_t* idx, int64_t n, float lr, int32_t* d_key, float* d_val, int64_t cap, int64_t* d_nnz,
                           dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_async_step_sparse"));
  DSGD_TRY(sp_check_out(d_key, d_val, cap, d_nnz));
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(sp_async_cap(c, idx, n, cap));   // (before anything runs: a delta is never lost)
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(sp_ensure(c));
  DSGD_TRY(ensure_s(c));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  const int64_t nn = n;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, 1, mx));
  hipLaunchKernelGGL(dsgd_async_finish_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_w, c->d_g, c->dp, c->d_ds, (float)n, lr,
                     (float)c->cfg.lambda, c->d_tmp, c->d_sc);
  HIP_TRY(hipGetLastError());
  c->s_dirty = false;
  DSGD_TRY((sp_compact<float, float, false>(c, c->d_tmp, c->d_perm)));
  DSGD_TRY(finish_stats(c, stats, tot));
  return sp_deliver<float>(c, d_key, d_val, cap, d_nnz);
}

// ---- Hogwild persistent engine -------------------------------------------------------------------------
static int async_refresh(dsgd_ctx* c) {  // copy the engine's counters to the host without touching its stream
  HIP_TRY(hipMemcpyAsync(c->h_hog, c->d_hog, sizeof(HogState), hipMemcpyDeviceToHost, c->query_stream));
  HIP_TRY(hipStreamSynchronize(c->query_stream));
  return DSGD_OK;
}

// the master's loss check must become resident beside the engine: its 16 KiB weight tile and the engine's LDS share a CU
// (RCV1: D + 1 = 47,237)
static_assert(sizeof(float) * ((size_t)hog_lds_words(HOG_HL, HOG_WL, 47237) + 4096 + 64) <= 160 * 1024, "Hogwild + eval LDS");
// one launch of the persistent kernel on async_stream: workers run until the TOTAL update count reaches max_updates
static int hog_launch(dsgd_ctx* c, long long max_updates) {
  HogArgs a;
  a.m = view(c);
  a.w = c->d_w;
  a.ds = c->d_ds;
  a.gcold = c->d_gcold;
  a.asg_begin = c->d_asg;
  a.asg_end = c->d_asg + c->hog_n;
  a.it = c->d_hog_it;
  a.st = c->d_hog;
  a.max_updates = max_updates;
  a.seed = c->hog_seed;
  a.lr = c->hog_lr;
  a.lambda = (float)c->cfg.lambda;
  int bits = 0;
  while ((1 << bits) < c->hog_batch) ++bits;
  const int shift = 30 - bits;   // at most one contribution per row and column: sums stay below 2^30
  a.qscale = std::ldexp(1.0f, shift - c->vexp);
  a.inv_qscale = std::ldexp(1.0f, c->vexp - shift);
  a.batch = c->hog_batch;
  a.positional_bug = c->hog_bug;
  a.hl = std::min(c->dp, c->hog_hl) & ~3;   // (whole quads of ranks; the rest is cold strip)
  a.dp = c->dp;
  a.wl = std::min(c->hog_wl, c->dp) & ~255;
  a.hh = hog_hh(a.hl);
  a.direct = c->hog_n <= HOG_DIRECT_MAX ? 1 : 0;
  a.trace = c->trace_cap > 0 ? c->d_trace : nullptr;
  a.trace_cap = c->trace_cap;
  a.tdot = c->d_tdot;
  const size_t lds = sizeof(float) * (size_t)hog_lds_words(a.hl, a.wl, c->dp);
  a.tprof = c->d_tprof;
  const dim3 grid(c->hog_n), block(HOG_THREADS);
  if (a.trace) {
    if (c->d_tprof) hipLaunchKernelGGL((dsgd_hogwild_kernel<true, true>), grid, block, lds, c->async_stream, a);
    else hipLaunchKernelGGL((dsgd_hogwild_kernel<false, true>), grid, block, lds, c->async_stream, a);
  } else {
    if (c->d_tprof) hipLaunchKernelGGL((dsgd_hogwild_kernel<true, false>), grid, block, lds, c->async_stream, a);
    else hipLaunchKernelGGL((dsgd_hogwild_kernel<false, false>), grid, block, lds, c->async_stream, a);
  }
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// one round of the cross-GPU asynchronous mode on async_stream: local updates up to `upto`, then
// d_local = w_prev - w (what this replica subtracted since the last exchange); all-reduce; the peers' part
// d_sum - d_local is subtracted on top (a replica applies its own updates as it goes and its peers' updates when they
// arrive: core/Slave.scala:99-105,177-185).  With one rank the peers' part is exactly zero.
static int exchange_round(dsgd_ctx* c, long long upto) {
  const int blocks = (c->dp + 1023) / 1024;
  DSGD_TRY(hog_launch(c, upto));
  hipLaunchKernelGGL(dsgd_exchange_delta_kernel, dim3(blocks), dim3(1024), 0, c->async_stream, c->d_w, c->d_wprev,
                     c->d_wdelta, c->d_wdelta + c->dp, c->dp);
  HIP_TRY(hipGetLastError());
  RCCL_TRY(rccl::AllReduce(c->d_wdelta, c->d_wdelta, (size_t)c->dp, rccl::kFloat32, rccl::kSum, c->comm, c->async_stream));
  hipLaunchKernelGGL(dsgd_exchange_apply_kernel, dim3(1), dim3(1024), 0, c->async_stream, c->d_w, c->d_wprev,
                     c->d_wdelta, c->d_wdelta + c->dp, c->d_ds, c->dp, (float)c->cfg.lambda, c->d_hog, c->world);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

int dsgd_async_start(dsgd_ctx* c, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                     float lr, int64_t max_updates, uint64_t seed, int32_t positional_bug) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_async_start"));
  if (!assigned_begin || !assigned_end || n_workers < 1) return fail(DSGD_EINVAL, "need at least one worker");
  if (batch < 1 || batch > HOG_MAX_BATCH) return fail(DSGD_EINVAL, "batch %d outside [1, %d]", batch, HOG_MAX_BATCH);
  if (max_updates < 0) return fail(DSGD_EINVAL, "negative max_updates");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  // ref: core/Slave.scala:161 "Async computation already running, can't be initialized unless stopped first"
  if (c->async_running) return fail(DSGD_ESTATE, "async computation already running: stop it first");
  if (n_workers > c->n_cu)   // every worker is a resident workgroup (they never yield): one per CU at most
    return fail(DSGD_EINVAL, "%d workers on a device with %d compute units", n_workers, c->n_cu);
  std::vector<long long> asg(2 * (size_t)n_workers);
  for (int k = 0; k < n_workers; ++k) {
    const long long b = assigned_begin[k], e = assigned_end[k];
    if (e <= b) return fail(DSGD_EINVAL, "worker %d has no assigned samples", k);
    if (b < 0 || e > c->n_rows) return fail(DSGD_ERANGE, "worker %d range [%lld, %lld) outside the %lld loaded rows", k, b, e, c->n_rows);
    if (batch > e - b) return fail(DSGD_EINVAL, "batch %d larger than worker %d's %lld assigned samples", batch, k, e - b);
    if (positional_bug && e - b > c->n_rows) return fail(DSGD_ERANGE, "positional sampling outside the data");
    asg[k] = b;
    asg[n_workers + k] = e;
  }
  const bool exchange = c->comm && c->exchange_every > 0;
  long long n_rounds = 1;
  if (exchange) {
    // ref: core/Slave.scala:103-105 gossips every update to every peer; across GPUs the replicas exchange the SUM of
    // their updates every `exchange_every` local updates (dsgd_async_set_exchange) -- all ranks must enqueue the same
    // number of collectives, so the update budget has to be finite and identical on every rank.
    n_rounds = (max_updates + c->exchange_every - 1) / c->exchange_every;
    if (n_rounds < 1) n_rounds = 1;
    if (n_rounds > 65536)
      return fail(DSGD_EINVAL, "max_updates / exchange_every = %lld rounds: more than 65536 (give a finite update budget)", n_rounds);
  }
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(ensure_s(c));
  if (!c->async_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&c->async_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->query_stream, hipStreamNonBlocking));
    DSGD_TRY(c->d_hog.alloc(1));
    DSGD_TRY(c->h_hog.alloc(1));
    DSGD_TRY(c->h_one.alloc(1));
    *c->h_one = 1;
  }
  const int hl = std::min(c->dp, c->hog_hl) & ~3;
  const size_t strip = (size_t)std::max(1, c->dp - hl);
  if (n_workers > c->hog_workers) {
    c->hog_workers = 0;
    DSGD_TRY(c->d_gcold.alloc((size_t)n_workers * strip));
    DSGD_TRY(c->d_asg.alloc(2 * (size_t)n_workers));
    DSGD_TRY(c->d_hog_it.alloc((size_t)n_workers));
    c->hog_workers = n_workers;
  }
  if (c->trace_cap > 0) {   // traced run: records of hog_trace_words(batch) words (header, gate masks, one x . w per row)
    c->trace_mw = (batch + 31) / 32;
    c->trace_batch = batch;
    const long long need = c->trace_cap * hog_trace_words(batch);
    DSGD_TRY(c->d_trace.reserve((size_t)need));
    DSGD_TRY(c->d_tdot.reserve((size_t)n_workers * (size_t)batch));
  }
  if (exchange) {
    DSGD_TRY(c->d_wprev.reserve((size_t)c->dp));
    DSGD_TRY(c->d_wdelta.reserve(2 * (size_t)c->dp));
  }
  HIP_TRY(hipMemsetAsync(c->d_gcold, 0, sizeof(float) * (size_t)n_workers * strip, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_hog_it, 0, sizeof(unsigned long long) * (size_t)n_workers, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_asg, asg.data(), sizeof(long long) * asg.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_hog, 0, sizeof(HogState), c->stream));
  HIP_TRY(hipMemcpyAsync(&c->d_hog->s_reg, &c->d_sc->s_reg, sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  if (exchange) HIP_TRY(hipMemcpyAsync(c->d_wprev, c->d_w, sizeof(float) * c->dp, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // asg is a stack-lifetime host buffer; everything is in place before launch
  c->hog_n = n_workers;
  c->hog_batch = batch;
  c->hog_lr = lr;
  c->hog_seed = seed;
  c->hog_bug = positional_bug;
  c->exch_rc = DSGD_OK;
  c->exch_err.clear();
  if (!exchange) {
    DSGD_TRY(hog_launch(c, max_updates));
  } else {
    // The rounds are enqueued by a helper thread: a HIP queue holds a bounded number of launches (and a collective
    // may block its caller), so enqueuing thousands of rounds here would hold the context's mutex for most of the run
    // and make dsgd_async_updates / dsgd_async_stop wait behind it.
    if (c->exch_thread.joinable()) c->exch_thread.join();
    c->exch_done.store(false);
    const long long every = c->exchange_every;
    c->exch_thread = std::thread([c, n_rounds, max_updates, every]() {
      int rc = hipSetDevice(c->cfg.device) == hipSuccess ? DSGD_OK : fail(DSGD_EHIP, "hipSetDevice in the exchange thread");
      for (long long r = 0; r < n_rounds && rc == DSGD_OK; ++r) rc = exchange_round(c, std::min<long long>(max_updates, (r + 1) * every));
      if (rc != DSGD_OK) {
        c->exch_rc = rc;
        c->exch_err = g_err;   // (thread-local message of THIS thread: carried to the joining caller)
      }
      c->exch_done.store(true);
    });
  }
  c->async_running = true;
  c->s_dirty = true;
  return DSGD_OK;
}

int dsgd_async_set_exchange(dsgd_ctx* c, int64_t every_updates) {
  DSGD_TRY(check_ctx(c));
  if (every_updates < 0) return fail(DSGD_EINVAL, "negative exchange period");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->async_running) return fail(DSGD_ESTATE, "async computation running");
  c->exchange_every = every_updates;
  return DSGD_OK;
}

int dsgd_async_updates(dsgd_ctx* c, int64_t* updates, int32_t* running) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (!c->d_hog) {
    if (updates) *updates = 0;
    if (running) *running = 0;
    return DSGD_OK;
  }
  DSGD_TRY(async_refresh(c));
  if (updates) *updates = (int64_t)c->h_hog->updates;
  const bool busy = c->async_running && (!c->exch_done.load() || hipStreamQuery(c->async_stream) == hipErrorNotReady);
  if (running) *running = busy ? 1 : 0;
  return DSGD_OK;
}

// raise the engine's stop flag: a 4-byte copy on the side stream (the kernel polls device memory, not the PCIe bus)
static int hog_raise_stop(dsgd_ctx* c) {
  if (!c->d_hog || !c->h_one) return DSGD_OK;
  HIP_TRY(hipMemcpyAsync(&c->d_hog->stop, c->h_one, sizeof(int), hipMemcpyHostToDevice, c->query_stream));
  HIP_TRY(hipStreamSynchronize(c->query_stream));
  return DSGD_OK;
}

static int async_join(dsgd_ctx* c) {
  if (c->exch_thread.joinable()) c->exch_thread.join();   // (it never takes the context's mutex)
  HIP_TRY(hipStreamSynchronize(c->async_stream));
  if (c->upd_stream) HIP_TRY(hipStreamSynchronize(c->upd_stream));
  c->async_running = false;
  c->s_dirty = true;  // w moved under the scalar the synchronous kernels cache
  if (c->exch_rc != DSGD_OK) return fail(c->exch_rc, "exchange round: %s", c->exch_err.c_str());
  DSGD_TRY(async_refresh(c));
  if (c->h_hog->err) return fail(DSGD_ERANGE, "the lock-free engine sampled a row outside the loaded data");
  return DSGD_OK;
}

// Block until the engine has left the device -- WITHOUT the context's mutex: dsgd_update_grad, dsgd_loss_acc and
// dsgd_async_updates are RPC handlers of other pool threads in the reference (core/Slave.scala:177-185 runs while
// asyncTask does) and must not queue up behind a waiter for as long as the update budget lasts.  One thread does the
// blocking; a second waiter sleeps on the condition variable.
static int async_wait_released(dsgd_ctx* c, std::unique_lock<std::mutex>& lk) {
  if (c->join_in_progress) {
    c->join_cv.wait(lk, [c] { return !c->join_in_progress; });
    // the joining thread's result is every waiter's result (a failed run must not read as a success to the thread that
    // happened to come second)
    if (c->join_rc != DSGD_OK) return fail(c->join_rc, "%s", c->join_err.c_str());
    return DSGD_OK;
  }
  c->join_in_progress = true;
  hipStream_t st = c->async_stream;
  lk.unlock();
  if (c->exch_thread.joinable()) c->exch_thread.join();   // (it never takes the context's mutex)
  const hipError_t e = hipStreamSynchronize(st);
  lk.lock();
  int rc = DSGD_OK;
  if (e != hipSuccess) rc = fail(DSGD_EHIP, "hipStreamSynchronize(async stream): %s", hipGetErrorString(e));
  else if (c->async_running) rc = async_join(c);   // (its own synchronisations return at once now)
  c->join_rc = rc;
  c->join_err = rc == DSGD_OK ? "" : g_err;
  c->join_in_progress = false;   // (cleared LAST: dsgd_destroy and the other waiters go on only when the result is stored)
  c->join_cv.notify_all();
  return rc;
}

int dsgd_async_stop(dsgd_ctx* c) {  // ref: SlaveImpl.stopAsync, core/Slave.scala:187-195
  DSGD_TRY(check_ctx(c));
  std::unique_lock<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (!c->async_running) return DSGD_OK;
  DSGD_TRY(hog_raise_stop(c));
  return async_wait_released(c, lk);
}

int dsgd_async_stats(dsgd_ctx* c, int64_t* counters, double* s_engine, double* s_exact) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (!c->d_hog) return fail(DSGD_ESTATE, "the lock-free engine has never been started on this context");
  DSGD_TRY(async_refresh(c));
  if (counters) {
    counters[0] = (int64_t)c->h_hog->updates;
    counters[1] = (int64_t)c->h_hog->samples;
    counters[2] = (int64_t)c->h_hog->active;
    counters[3] = (int64_t)c->h_hog->atomics;
  }
  if (s_engine) *s_engine = (double)c->h_hog->s_reg;
  if (s_exact) {
    // the same summation the synchronous kernels use (fra_scalars), from the weights as they are now; the engine keeps
    // its own scalar (HogState), so refreshing the synchronous one disturbs nothing
    DSGD_TRY(require_ds(c));
    c->s_dirty = true;
    DSGD_TRY(ensure_s(c));
    DSGD_TRY(read_scalars(c));
    if (c->async_running) c->s_dirty = true;
    *s_exact = (double)c->h_sc->s_reg;
  }
  return DSGD_OK;
}

// ---- the consistent loss check (csrc/dsgd_snapshot.hpp; ref: core/MasterAsync.scala:109-138) ----
// Everything runs on the context's launch stream, beside the engine's: reset of the tallies and of the window, the
// snapshot kernel (copy + scalars of the copy + window), the row-wise evaluation OF THE SNAPSHOT in the shape that is
// resident beside the engine -- whether one runs or not: a check's tallies do not depend on the engine's state -- and one
// read_scalars, the call's only synchronisation.
int dsgd_async_check(dsgd_ctx* c, int64_t row_begin, int64_t row_end, double* loss, double* acc, int64_t* counts,
                     int64_t* updates_window) {
  DSGD_TRY(check_ctx(c));
  if (row_end <= row_begin)  // samples.map(...).reduce on an empty collection throws (ref: SparseSVM.scala:21-23)
    return fail(DSGD_EINVAL, "empty row range: reduce on an empty sample list");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->fp64)
    return fail(DSGD_EUNSUPPORTED, "dsgd_async_check is not available in an fp64 context: its asynchronous schedule runs no "
                                   "concurrent engine, dsgd_loss_acc between its steps is consistent already");
  if (c->comm)
    return fail(DSGD_EUNSUPPORTED, "dsgd_async_check is not available with a communicator attached: dsgd_loss_acc sums the "
                                   "tallies over the ranks");
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  if (row_begin < 0 || row_end > c->n_rows)
    return fail(DSGD_ERANGE, "rows [%lld, %lld) outside the %lld loaded rows", (long long)row_begin, (long long)row_end, c->n_rows);
  DSGD_TRY(bind(c));
  DSGD_TRY(prepare_layout(c));   // (done long ago while an engine runs: dsgd_async_start)
  // the buffer that is not the best one; everything below is ordered on the stream behind the last reader of it
  const int t = c->snap_best >= 0 ? 1 - c->snap_best : std::max(c->snap_last, 0);
  DSGD_TRY(c->d_snap[t].reserve((size_t)c->dp));
  DSGD_TRY(c->d_snap_win.reserve(2));
  DSGD_TRY(c->h_snap_win.reserve(2));
  DSGD_TRY(ensure_redpart(c));
  if (c->snap_last == t) c->snap_last = -1;   // (until the new snapshot is in: a failure below leaves no half-written "last")
  DSGD_TRY(reset_counters(c));
  HIP_TRY(hipMemsetAsync(c->d_snap_win, 0, 2 * sizeof(unsigned long long), c->stream));
  const int blocks = (c->dp + FRA_COLS - 1) / FRA_COLS;
  hipLaunchKernelGGL(dsgd_snap_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_w, c->d_ds, c->d_snap[t], c->dp,
                     (float)c->cfg.lambda, c->d_sc, red_out(c), c->d_hog.get(), c->d_snap_win);
  HIP_TRY(hipGetLastError());
  // d_sc's s / |w|^2 are the SNAPSHOT's now: dirty for everybody else, as after a check under the engine (eval_enqueue)
  c->red_par ^= 1;
  c->s_lazy = false;
  c->s_dirty = true;
  DSGD_TRY(launch_eval_rows(c, c->d_snap[t], (long long)row_begin, (long long)row_end, true));
  HIP_TRY(hipMemcpyAsync(c->h_snap_win, c->d_snap_win, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(eval_read(c, loss, acc, counts));   // (read_scalars: the one synchronisation)
  c->snap_last = t;
  if (updates_window) {
    updates_window[0] = (int64_t)~c->h_snap_win[0];
    updates_window[1] = (int64_t)c->h_snap_win[1];
  }
  return DSGD_OK;
}

int dsgd_async_check_keep(dsgd_ctx* c) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->snap_last < 0) return fail(DSGD_ESTATE, "no dsgd_async_check since the data was loaded: nothing to keep");
  c->snap_best = c->snap_last;   // (the handles change places: the next check writes into the other buffer)
  return DSGD_OK;
}

int dsgd_async_check_weights(dsgd_ctx* c, int32_t which, float* w_out) {
  DSGD_TRY(check_ctx(c));
  if (!w_out) return fail(DSGD_EINVAL, "null w_out");
  if (which != 0 && which != 1) return fail(DSGD_EINVAL, "which = %d: 0 (the last check's snapshot) or 1 (the best one)", which);
  std::lock_guard<std::mutex> lk(c->mu);
  const int t = which == 0 ? c->snap_last : c->snap_best;
  if (t < 0)
    return fail(DSGD_ESTATE, which == 0 ? "no dsgd_async_check since the data was loaded" : "no snapshot kept (dsgd_async_check_keep) since the data was loaded");
  DSGD_TRY(bind(c));
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_out, bytes));
  DSGD_TRY(launch_permute_out(c, c->d_snap[t], c->d_io));
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_io, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(w_out, c->pin_out.p, bytes);
  return DSGD_OK;
}

int dsgd_async_set_trace(dsgd_ctx* c, int64_t capacity) {
  DSGD_TRY(check_ctx(c));
  if (capacity < 0) return fail(DSGD_EINVAL, "negative trace capacity");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (c->async_running) return fail(DSGD_ESTATE, "async computation running");
  c->trace_cap = capacity;   // (the buffer is sized at dsgd_async_start: a record's length depends on the batch size)
  if (capacity == 0) {
    c->d_trace.reset();   // (no engine is resident: the release's device synchronisation returns)
    c->d_tdot.reset();
    c->trace_mw = 0;
    c->trace_batch = 0;
  }
  return DSGD_OK;
}

int dsgd_async_read_trace(dsgd_ctx* c, int32_t* worker, uint32_t* iteration, int64_t* read_at, float* s_used,
                          int32_t* n_active, uint32_t* gate_mask, int64_t n, int64_t* n_out, int32_t* mask_words_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 0 || (n > 0 && (!worker || !iteration || !read_at || !s_used || !n_active || !gate_mask)))
    return fail(DSGD_EINVAL, "bad trace arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (c->async_running) return fail(DSGD_ESTATE, "async computation running (dsgd_async_wait / dsgd_async_stop first)");
  if (!c->d_trace || !c->d_hog || c->trace_mw == 0)
    return fail(DSGD_ESTATE, "no traced run on this context (dsgd_async_set_trace, then dsgd_async_start)");
  DSGD_TRY(async_refresh(c));
  const long long have = std::min<long long>((long long)c->h_hog->updates, c->trace_cap);
  const long long m = std::min<long long>(have, n);
  const int mw = c->trace_mw, rw = (int)hog_trace_words(c->trace_batch);
  if (n_out) *n_out = have;
  if (mask_words_out) *mask_words_out = mw;
  if (m == 0) return DSGD_OK;
  std::vector<unsigned int> recs;
  try {
    recs.resize((size_t)m * (size_t)rw);
  } catch (const std::bad_alloc&) {
    return fail(DSGD_ENOMEM, "out of host memory");
  }
  HIP_TRY(hipMemcpy(recs.data(), c->d_trace, sizeof(unsigned int) * recs.size(), hipMemcpyDeviceToHost));
  for (long long i = 0; i < m; ++i) {
    const unsigned int* r = recs.data() + (size_t)i * (size_t)rw;
    worker[i] = (int32_t)r[0];
    iteration[i] = r[1];
    read_at[i] = (int64_t)(((unsigned long long)r[3] << 32) | r[2]);
    memcpy(&s_used[i], &r[4], sizeof(float));
    n_active[i] = (int32_t)r[5];
    memcpy(gate_mask + (size_t)i * (size_t)mw, r + HOG_TRACE_HDR, sizeof(unsigned int) * (size_t)mw);
  }
  return DSGD_OK;
}

int dsgd_async_read_trace_dots(dsgd_ctx* c, int64_t* seen_from, float* dots, int64_t n, int32_t* batch_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 0 || (n > 0 && (!seen_from || !dots))) return fail(DSGD_EINVAL, "bad trace arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (c->async_running) return fail(DSGD_ESTATE, "async computation running (dsgd_async_wait / dsgd_async_stop first)");
  if (!c->d_trace || !c->d_hog || c->trace_mw == 0)
    return fail(DSGD_ESTATE, "no traced run on this context (dsgd_async_set_trace, then dsgd_async_start)");
  DSGD_TRY(async_refresh(c));
  const long long have = std::min<long long>((long long)c->h_hog->updates, c->trace_cap);
  const long long m = std::min<long long>(have, n);
  const int B = c->trace_batch, mw = c->trace_mw, rw = (int)hog_trace_words(B);
  if (batch_out) *batch_out = B;
  if (m == 0) return DSGD_OK;
  std::vector<unsigned int> recs;
  try {
    recs.resize((size_t)m * (size_t)rw);
  } catch (const std::bad_alloc&) {
    return fail(DSGD_ENOMEM, "out of host memory");
  }
  HIP_TRY(hipMemcpy(recs.data(), c->d_trace, sizeof(unsigned int) * recs.size(), hipMemcpyDeviceToHost));
  for (long long i = 0; i < m; ++i) {
    const unsigned int* r = recs.data() + (size_t)i * (size_t)rw;
    const unsigned long long read_at = ((unsigned long long)r[3] << 32) | r[2];
    // the low word of seen_from, at most 2^32 - 1 updates below read_at; a launch's first iteration knows only the run's start
    seen_from[i] = (r[7] & 1u) ? 0 : (int64_t)(read_at - (unsigned long long)((unsigned int)read_at - r[6]));
    memcpy(dots + (size_t)i * (size_t)B, r + HOG_TRACE_HDR + mw, sizeof(float) * (size_t)B);
  }
  return DSGD_OK;
}

int dsgd_async_wait(dsgd_ctx* c) {
  DSGD_TRY(check_ctx(c));
  std::unique_lock<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (!c->async_running) return DSGD_OK;
  return async_wait_released(c, lk);
}

int dsgd_comm_unique_id(char* id_out) {
  if (!id_out) return fail(DSGD_EINVAL, "null id_out");
  if (!rccl::available()) return fail(DSGD_ERCCL, "librccl could not be loaded: %s", dlerror());
  rccl::unique_id_t id;
  RCCL_TRY(rccl::GetUniqueId(&id));
  memcpy(id_out, id.internal, DSGD_UNIQUE_ID_BYTES);
  return DSGD_OK;
}

int dsgd_comm_init(dsgd_ctx* c, const char* unique_id, int32_t world_size, int32_t rank) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_comm_init"));
  if (!unique_id || world_size < 1 || rank < 0 || rank >= world_size) return fail(DSGD_EINVAL, "bad communicator arguments");
  if (!rccl::available()) return fail(DSGD_ERCCL, "librccl could not be loaded");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  if (c->comm) return fail(DSGD_ESTATE, "communicator already attached");
  rccl::unique_id_t id;
  memcpy(id.internal, unique_id, DSGD_UNIQUE_ID_BYTES);
  RCCL_TRY(rccl::CommInitRank(&c->comm, world_size, id, rank));
  c->comm_broken = false;
  c->world = world_size;
  c->rank = rank;
  return DSGD_OK;
}

// The column layout of loaded data again, under the communicator that was just attached: the columns back to their keys,
// the resident vectors to key order, then the ranking from the all-reduced counts (and the ranks' common vexp).  Every
// plan's column slices belong to the layout that goes (layout_gen).
static int relayout(dsgd_ctx* c) {
  if (c->layout_ready) {
    std::vector<int> perm((size_t)c->dp), inv((size_t)c->dp);
    HIP_TRY(hipMemcpyAsync(perm.data(), c->d_perm, sizeof(int) * perm.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < c->dp; ++j) inv[(size_t)perm[(size_t)j]] = j;
    DSGD_TRY(reset_layout(c));   // (d_perm: the identity from here)
    if (c->nnz > 0) {
      DevBuf<int> d_inv;
      DSGD_TRY(d_inv.alloc(inv.size()));
      hipError_t e = hipMemcpy(d_inv, inv.data(), sizeof(int) * inv.size(), hipMemcpyHostToDevice);
      if (e == hipSuccess) {
        const int blocks = (int)std::min<long long>((c->nnz + 255) / 256, (long long)c->n_cu * 8);
        hipLaunchKernelGGL(dsgd_remap_cols_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_col, c->nnz, d_inv);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      d_inv.reset();
      if (e != hipSuccess) return fail(DSGD_EHIP, "column keys: %s", hipGetErrorString(e));
    }
  }
  return prepare_layout(c);
}

// dsgd_comm_init_f64 (v64 = false: refused on Double data) and dsgd_comm_init_f64v (Double data accepted, now and in later loads)
static int comm_init_f64_impl(dsgd_ctx* c, const char* unique_id, int32_t world_size, int32_t rank, bool v64, const char* what) {
  DSGD_TRY(check_ctx(c));
  if (!unique_id || world_size < 1 || rank < 0 || rank >= world_size) return fail(DSGD_EINVAL, "bad communicator arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, what));
  if (!v64) DSGD_TRY(refuse_val64(c, what));
  if (world_size > 64) return fail(DSGD_EUNSUPPORTED, "at most 64 ranks");
  if (!rccl::available()) return fail(DSGD_ERCCL, "librccl could not be loaded");
  const bool sliced = c->cs_w_G == CS64_G;
  DSGD_TRY(bind(c));   // (rank order: the ranking may be about to change)
  DSGD_TRY(require_sync_mode(c));
  if (c->comm) return fail(DSGD_ESTATE, "communicator already attached");
  rccl::unique_id_t id;
  memcpy(id.internal, unique_id, DSGD_UNIQUE_ID_BYTES);
  RCCL_TRY(rccl::CommInitRank(&c->comm, world_size, id, rank));
  c->comm_broken = false;
  c->world = world_size;
  c->rank = rank;
  c->comm_v64 = v64;
  // loaded data: ONE ranking and ONE vexp now, on every rank (data loaded later: at its first use, as in fp32)
  int rc = c->d_row_ptr ? relayout(c) : DSGD_OK;
  if (rc == DSGD_OK && sliced) rc = cs64_slice(c);   // (the weights back in the layout they were in)
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    (void)hipStreamSynchronize(c->stream);
    (void)rccl::CommDestroy(c->comm);
    c->comm = nullptr;
    c->comm_v64 = false;
    c->world = 1;
    c->rank = 0;
    return fail(rc, "%s", msg);
  }
  return DSGD_OK;
}
int dsgd_comm_init_f64(dsgd_ctx* c, const char* unique_id, int32_t world_size, int32_t rank) {
  return comm_init_f64_impl(c, unique_id, world_size, rank, false, "dsgd_comm_init_f64");
}
int dsgd_comm_init_f64v(dsgd_ctx* c, const char* unique_id, int32_t world_size, int32_t rank) {
  return comm_init_f64_impl(c, unique_id, world_size, rank, true, "dsgd_comm_init_f64v");
}

// The communicator the LOGISTIC model's steps span (include/dsgd.h "THE LOGISTIC MODEL -- ACROSS RANKS"): attached as
// dsgd_comm_init attaches it -- the SVM's entry points behave as under that call -- and additionally comm_lg, which lets the
// logistic steps through (lg_refuse).  Loaded data is ranked again at once, so that the ranks share ONE column ranking whatever
// the order of load and attach (data loaded later: at its first use).
int dsgd_comm_init_lg(dsgd_ctx* c, const char* unique_id, int32_t world_size, int32_t rank) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(refuse_fp64(c, "dsgd_comm_init_lg"));
  if (!unique_id || world_size < 1 || rank < 0 || rank >= world_size) return fail(DSGD_EINVAL, "bad communicator arguments");
  if (world_size > LGG_MAX_WORLD) return fail(DSGD_EUNSUPPORTED, "at most %d ranks", LGG_MAX_WORLD);
  if (!rccl::available()) return fail(DSGD_ERCCL, "librccl could not be loaded");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));   // (rank order: the ranking may be about to change)
  DSGD_TRY(require_sync_mode(c));
  if (c->comm) return fail(DSGD_ESTATE, "communicator already attached");
  rccl::unique_id_t id;
  memcpy(id.internal, unique_id, DSGD_UNIQUE_ID_BYTES);
  RCCL_TRY(rccl::CommInitRank(&c->comm, world_size, id, rank));
  c->comm_broken = false;
  c->world = world_size;
  c->rank = rank;
  c->comm_lg = true;
  const int rc = c->d_row_ptr ? relayout(c) : DSGD_OK;
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    (void)hipStreamSynchronize(c->stream);
    (void)rccl::CommDestroy(c->comm);
    c->comm = nullptr;
    c->comm_lg = false;
    c->world = 1;
    c->rank = 0;
    return fail(rc, "%s", msg);
  }
  return DSGD_OK;
}

int dsgd_comm_destroy(dsgd_ctx* c) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  c->comm_broken_ok = true;
  const int brc = bind(c);
  c->comm_broken_ok = false;
  DSGD_TRY(brc);
  c->comm_broken = false;   // (an aborted communicator is gone already: the context may attach a new one)
  if (!c->comm) {
    c->comm_v64 = false;
    c->comm_lg = false;
    c->world = 1;
    c->rank = 0;
    return DSGD_OK;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  RCCL_TRY(rccl::CommDestroy(c->comm));
  c->comm = nullptr;
  c->comm_v64 = false;
  c->comm_lg = false;
  c->world = 1;
  c->rank = 0;
  return DSGD_OK;
}

// ---- ONE host thread driving several contexts -------------------------------------------------------------------------
// The reference's dev role runs the master and every slave in ONE JVM (Main.scala:144-158): one thread of that JVM must be
// able to step all the GPUs of a node.  A collective blocks its caller until every rank has joined, so the per-context
// entry points above cannot be called one after the other from one thread; these take all the contexts at once: every
// context's kernels in front of a collective are enqueued first, then all the collectives inside one
// ncclGroupStart / ncclGroupEnd, then what follows them -- the same kernels, sums and order as N processes, one per GPU.
}  // extern "C" (the helpers below are C++)
namespace {
struct MultiLock {
  std::vector<dsgd_ctx*> held;
  int lock(dsgd_ctx* const* ctxs, int n) {
    if (!ctxs || n < 1) return fail(DSGD_EINVAL, "need at least one context");
    std::vector<dsgd_ctx*> order(ctxs, ctxs + n);
    for (dsgd_ctx* c : order)
      if (!c) return fail(DSGD_EINVAL, "null context");
    std::sort(order.begin(), order.end());   // one locking order for every caller
    if (std::adjacent_find(order.begin(), order.end()) != order.end()) return fail(DSGD_EINVAL, "a context appears twice");
    for (dsgd_ctx* c : order) {
      c->mu.lock();
      held.push_back(c);
    }
    return DSGD_OK;
  }
  ~MultiLock() {
    for (auto it = held.rbegin(); it != held.rend(); ++it) (*it)->mu.unlock();
  }
};
// every context of a grouped call joins the SAME collectives: communicators of one size, attached to all or to none
int group_shape(dsgd_ctx* const* ctxs, int n) {
  for (int i = 0; i < n; ++i) {
    if ((ctxs[i]->comm != nullptr) != (ctxs[0]->comm != nullptr) || ctxs[i]->world != ctxs[0]->world)
      return fail(DSGD_ESTATE, "the contexts of a grouped call must share one communicator shape (dsgd_comm_init_all)");
    if (ctxs[i]->layout_ready != ctxs[0]->layout_ready)
      return fail(DSGD_ESTATE, "some contexts have their column layout and some do not: load the data of all of them first");
  }
  if (n > 1 && !ctxs[0]->comm) return fail(DSGD_ESTATE, "several contexts without a communicator (dsgd_comm_init_all)");
  return DSGD_OK;
}
// phase 2 of every grouped call: fn(context) enqueues that context's collective
template <class Fn>
int grouped(dsgd_ctx* const* ctxs, int n, Fn fn) {
  if (!ctxs[0]->comm) return DSGD_OK;
  // all or nothing: whatever can be refused is refused BEFORE the group opens (a context that cannot be bound, a
  // communicator a failed group left behind) -- a collective that only some ranks joined would hang every stream
  for (int i = 0; i < n; ++i) {
    if (ctxs[i]->comm_broken)
      return fail(DSGD_ERCCL, "context %d: its communicator was abandoned after a collective that not every rank joined "
                              "(dsgd_comm_destroy + dsgd_comm_init_all)", i);
    DSGD_TRY(bind(ctxs[i]));
  }
  RCCL_TRY(rccl::GroupStart());
  int rc = DSGD_OK, joined = 0;
  for (int i = 0; i < n && rc == DSGD_OK; ++i) {
    rc = bind(ctxs[i]);
    if (rc == DSGD_OK) rc = fn(ctxs[i], i);
    if (rc == DSGD_OK) ++joined;
  }
  char first_err[sizeof(g_err)];
  snprintf(first_err, sizeof(first_err), "%s", g_err);
  const int re = rccl::GroupEnd();   // (always: a group that was started is ended)
  if (rc != DSGD_OK && joined > 0) {
    // some ranks' collectives are enqueued and the others' never will be: abort the communicators (their streams come
    // back with an error instead of hanging) and refuse further collectives on them
    for (int i = 0; i < n; ++i) {
      ctxs[i]->comm_broken = true;
      if (rccl::CommAbort && ctxs[i]->comm) {
        (void)rccl::CommAbort(ctxs[i]->comm);
        ctxs[i]->comm = nullptr;
      }
    }
    return fail(rc, "%s (the group's communicators were aborted: only %d of %d ranks had joined)", first_err, joined, n);
  }
  if (rc == DSGD_OK && re != 0) rc = fail(DSGD_ERCCL, "ncclGroupEnd: %s", rccl::GetErrorString(re));
  return rc;
}
}  // namespace
extern "C" {

int dsgd_comm_init_all(dsgd_ctx* const* ctxs, int32_t n_ctx) {
  MultiLock ml;
  DSGD_TRY(ml.lock(ctxs, n_ctx));
  DSGD_TRY(refuse_fp64_all(ctxs, n_ctx, "dsgd_comm_init_all"));
  if (!rccl::available()) return fail(DSGD_ERCCL, "librccl could not be loaded");
  for (int i = 0; i < n_ctx; ++i)
    if (ctxs[i]->comm) return fail(DSGD_ESTATE, "communicator already attached to context %d", i);
  rccl::unique_id_t id;
  RCCL_TRY(rccl::GetUniqueId(&id));
  RCCL_TRY(rccl::GroupStart());
  int rc = DSGD_OK;
  for (int i = 0; i < n_ctx && rc == DSGD_OK; ++i) {
    rc = bind(ctxs[i]);
    if (rc == DSGD_OK) {
      const int r = rccl::CommInitRank(&ctxs[i]->comm, n_ctx, id, i);
      if (r) rc = fail(DSGD_ERCCL, "ncclCommInitRank(rank %d of %d): %s", i, n_ctx, rccl::GetErrorString(r));
    }
  }
  const int re = rccl::GroupEnd();
  if (rc == DSGD_OK && re != 0) rc = fail(DSGD_ERCCL, "ncclGroupEnd: %s", rccl::GetErrorString(re));
  if (rc != DSGD_OK) {
    for (int i = 0; i < n_ctx; ++i) ctxs[i]->comm = nullptr;   // (whatever was created is abandoned: the call failed as a whole)
    return rc;
  }
  for (int i = 0; i < n_ctx; ++i) {
    ctxs[i]->world = n_ctx;
    ctxs[i]->rank = i;
  }
  return DSGD_OK;
}

int dsgd_build_dim_sparsity_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int64_t* n_train_per_ctx) {
  MultiLock ml;
  DSGD_TRY(ml.lock(ctxs, n_ctx));
  DSGD_TRY(refuse_fp64_all(ctxs, n_ctx, "dsgd_build_dim_sparsity_devices"));
  if (!n_train_per_ctx) return fail(DSGD_EINVAL, "null n_train_per_ctx");
  DSGD_TRY(group_shape(ctxs, n_ctx));
  std::vector<DevBuf<unsigned int>> cnt((size_t)n_ctx);   // (what a failure leaves is released on return)
  int rc = DSGD_OK;
  for (int i = 0; i < n_ctx && !rc; ++i) {
    rc = bind(ctxs[i]);
    if (!rc) rc = ds_checks(ctxs[i], n_train_per_ctx[i]);
  }
  // the column ranking: counts, their sum over the contexts, one order for all
  for (int i = 0; i < n_ctx && !rc; ++i) {
    rc = bind(ctxs[i]);
    if (!rc) rc = layout_begin(ctxs[i], cnt[(size_t)i]);
  }
  if (!rc) rc = grouped(ctxs, n_ctx, [&](dsgd_ctx* c, int i) { return layout_collective(c, cnt[(size_t)i]); });
  for (int i = 0; i < n_ctx && !rc; ++i) {
    rc = bind(ctxs[i]);
    if (!rc) rc = layout_finish(ctxs[i], cnt[(size_t)i]);   // (releases the buffer)
  }
  // dimSparsity: feature counts of every context's train rows, summed (Main.scala:57-60 counts the whole train set)
  for (int i = 0; i < n_ctx && !rc; ++i) {
    rc = bind(ctxs[i]);
    if (!rc) rc = ds_begin(ctxs[i], n_train_per_ctx[i], cnt[(size_t)i]);
  }
  if (!rc) rc = grouped(ctxs, n_ctx, [&](dsgd_ctx* c, int i) { return ds_collective(c, cnt[(size_t)i]); });
  for (int i = 0; i < n_ctx && !rc; ++i) {
    rc = bind(ctxs[i]);
    if (!rc) rc = ds_finish(ctxs[i], cnt[(size_t)i], nullptr);
  }
  return rc;
}

}  // extern "C"
static int devices_step_checks(dsgd_ctx* const* ctxs, int n_ctx) {
  DSGD_TRY(group_shape(ctxs, n_ctx));
  for (int i = 0; i < n_ctx; ++i) {
    dsgd_ctx* c = ctxs[i];
    DSGD_TRY(bind(c));
    DSGD_TRY(require_data(c));
    DSGD_TRY(require_ds(c));
    DSGD_TRY(require_sync_mode(c));
    if (!c->layout_ready) return fail(DSGD_ESTATE, "context %d has no column layout yet (dsgd_build_dim_sparsity_devices)", i);
  }
  return DSGD_OK;
}
static int devices_step_finish(dsgd_ctx* const* ctxs, int n_ctx, int n_workers, float lr, const std::vector<long long>& totals,
                               dsgd_batch_stats* stats) {
  DSGD_TRY(grouped(ctxs, n_ctx, [](dsgd_ctx* c, int) { return finish_collective(c); }));
  for (int i = 0; i < n_ctx; ++i) {
    DSGD_TRY(bind(ctxs[i]));
    DSGD_TRY(finish_post(ctxs[i], n_workers, lr));
  }
  dsgd_batch_stats sum{0, 0};
  for (int i = 0; i < n_ctx; ++i) {
    DSGD_TRY(bind(ctxs[i]));
    dsgd_batch_stats one{0, 0};
    DSGD_TRY(finish_stats(ctxs[i], &one, totals[(size_t)i]));
    sum.n_samples += one.n_samples;
    sum.n_active += one.n_active;
  }
  if (stats) *stats = sum;
  return DSGD_OK;
}
extern "C" {

int dsgd_sync_step_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int32_t* const* idx_per_worker,
                           const int64_t* n_per_worker, int32_t workers_per_ctx, float lr, dsgd_batch_stats* stats) {
  MultiLock ml;
  DSGD_TRY(ml.lock(ctxs, n_ctx));
  DSGD_TRY(refuse_fp64_all(ctxs, n_ctx, "dsgd_sync_step_devices"));
  if (workers_per_ctx < 1 || !idx_per_worker || !n_per_worker) return fail(DSGD_EINVAL, "need at least one worker per context");
  DSGD_TRY(devices_step_checks(ctxs, n_ctx));
  std::vector<long long> totals((size_t)n_ctx, 0);
  for (int i = 0; i < n_ctx; ++i) {   // every context's gradient kernels and its part of the finish in front of the collective
    dsgd_ctx* c = ctxs[i];
    DSGD_TRY(bind(c));
    DSGD_TRY(ensure_g(c, workers_per_ctx));
    DSGD_TRY(ensure_s(c, true));
    DSGD_TRY(reset_counters(c));
    long long mx = 0;
    DSGD_TRY(stage_lists(c, idx_per_worker + (size_t)i * workers_per_ctx, n_per_worker + (size_t)i * workers_per_ctx, workers_per_ctx,
                         &mx, &totals[(size_t)i]));
    DSGD_TRY(launch_grad(c, c->cur_idx, c->d_segs, workers_per_ctx, mx, true));
    DSGD_TRY(finish_pre(c, workers_per_ctx, lr, false));
  }
  return devices_step_finish(ctxs, n_ctx, workers_per_ctx, lr, totals, stats);
}

int dsgd_sync_step_ranges_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int64_t* row_begin, const int64_t* row_end,
                                  int32_t workers_per_ctx, float lr, dsgd_batch_stats* stats) {
  MultiLock ml;
  DSGD_TRY(ml.lock(ctxs, n_ctx));
  DSGD_TRY(refuse_fp64_all(ctxs, n_ctx, "dsgd_sync_step_ranges_devices"));
  if (workers_per_ctx < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "need at least one worker per context");
  DSGD_TRY(devices_step_checks(ctxs, n_ctx));
  std::vector<long long> totals((size_t)n_ctx, 0);
  for (int i = 0; i < n_ctx; ++i) {
    dsgd_ctx* c = ctxs[i];
    DSGD_TRY(bind(c));
    DSGD_TRY(reset_counters(c));
    DSGD_TRY(ranges_enqueue(c, row_begin + (size_t)i * workers_per_ctx, row_end + (size_t)i * workers_per_ctx, workers_per_ctx, lr,
                            &totals[(size_t)i], false));
    DSGD_TRY(finish_pre(c, workers_per_ctx, lr, false));
  }
  return devices_step_finish(ctxs, n_ctx, workers_per_ctx, lr, totals, stats);
}

int dsgd_loss_acc_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int64_t* row_begin, const int64_t* row_end, double* loss,
                          double* acc, int64_t* counts) {
  MultiLock ml;
  DSGD_TRY(ml.lock(ctxs, n_ctx));
  DSGD_TRY(refuse_fp64_all(ctxs, n_ctx, "dsgd_loss_acc_devices"));
  if (!row_begin || !row_end) return fail(DSGD_EINVAL, "null row ranges");
  DSGD_TRY(group_shape(ctxs, n_ctx));
  for (int i = 0; i < n_ctx; ++i) {
    DSGD_TRY(bind(ctxs[i]));
    if (!ctxs[i]->layout_ready) return fail(DSGD_ESTATE, "context %d has no column layout yet (dsgd_build_dim_sparsity_devices)", i);
    DSGD_TRY(eval_enqueue(ctxs[i], nullptr, row_begin[i], row_end[i]));
  }
  DSGD_TRY(grouped(ctxs, n_ctx, [](dsgd_ctx* c, int) { return eval_collective(c); }));
  for (int i = n_ctx - 1; i >= 0; --i) {   // (every replica holds the summed tallies and the same weights: context 0 answers)
    DSGD_TRY(bind(ctxs[i]));
    DSGD_TRY(eval_read(ctxs[i], i == 0 ? loss : nullptr, i == 0 ? acc : nullptr, i == 0 ? counts : nullptr));
  }
  return DSGD_OK;
}

int dsgd_prof_enable(dsgd_ctx* c, int32_t on) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  HIP_TRY(hipStreamSynchronize(c->stream));
  DSGD_TRY(prof_collect(c));
  c->prof = on != 0;
  c->prof_main_only = on == 2;   // 2: bracket only the dominant gradient kernel (two event records per step, not six)
  return DSGD_OK;
}

int dsgd_prof_read(dsgd_ctx* c, double* ms_avg, int64_t* n_launches, int32_t reset) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  HIP_TRY(hipStreamSynchronize(c->stream));
  DSGD_TRY(prof_collect(c));
  if (ms_avg) *ms_avg = c->prof_kn[0] ? c->prof_kms[0] / (double)c->prof_kn[0] : 0.0;
  if (n_launches) *n_launches = c->prof_kn[0];
  if (reset) {
    for (int k = 0; k < 3; ++k) {
      c->prof_kms[k] = 0.0;
      c->prof_kn[k] = 0;
    }
  }
  return DSGD_OK;
}

int dsgd_prof_read_kinds(dsgd_ctx* c, double* ms_avg3, int64_t* n_launches3) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  HIP_TRY(hipStreamSynchronize(c->stream));
  DSGD_TRY(prof_collect(c));
  for (int k = 0; k < 3; ++k) {
    if (ms_avg3) ms_avg3[k] = c->prof_kn[k] ? c->prof_kms[k] / (double)c->prof_kn[k] : 0.0;
    if (n_launches3) n_launches3[k] = c->prof_kn[k];
  }
  return DSGD_OK;
}

int dsgd_range_nnz(dsgd_ctx* c, int64_t row_begin, int64_t row_end, int64_t* nnz, int64_t* cold_nnz) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  DSGD_TRY(require_data(c));
  if (row_begin < 0 || row_end < row_begin || row_end > c->n_rows) return fail(DSGD_ERANGE, "row range [%lld, %lld) outside [0, %lld)", (long long)row_begin, (long long)row_end, c->n_rows);
  DSGD_TRY(prepare_layout(c));
  if (nnz) *nnz = c->h_row_ptr[(size_t)row_end] - c->h_row_ptr[(size_t)row_begin];
  if (cold_nnz) {
    const bool split = c->h_crow_ptr.size() == (size_t)c->n_rows + 1;
    *cold_nnz = split ? c->h_crow_ptr[(size_t)row_end] - c->h_crow_ptr[(size_t)row_begin] : 0;
  }
  return DSGD_OK;
}

int dsgd_debug_cycles(dsgd_ctx* c, uint64_t* out8, int32_t reset) {
  DSGD_TRY(check_ctx(c));
  if (!out8) return fail(DSGD_EINVAL, "null out8");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));
  for (int i = 0; i < 16; ++i) out8[i] = 0;
  if (!c->d_tprof) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out8, c->d_tprof, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
  if (const char* path = getenv("DSGD_FSTEP_DUMP")) {   // tuning runs: the per-workgroup words of the chunked launch's last run
    std::vector<unsigned long long> v(4 * 1024);
    HIP_TRY(hipMemcpy(v.data(), c->d_tprof + 16, sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(path, "a")) {
      fprintf(f, "# wg start end hot_tile_cycles xcc\n");
      for (int i = 0; i < 1024; ++i)
        if (v[4 * i + 1]) fprintf(f, "%d %llu %llu %llu %llu\n", i, v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
      fclose(f);
    }
  }
  if (reset) HIP_TRY(hipMemset(c->d_tprof, 0, sizeof(unsigned long long) * 16));
  return DSGD_OK;
}

int dsgd_tuning_info(dsgd_ctx* c, int32_t* vals, int32_t n) {
  DSGD_TRY(check_ctx(c));
  if (!vals || n < 0 || n > 8) return fail(DSGD_EINVAL, "bad tuning_info arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  // [0]: 4 = the split layout (the only one); 5 = ... and the last chunked launch ran its PACKED form (csrc/dsgd_fstep.hpp)
  const int32_t all[8] = {c->last_fstep_packed ? 5 : 4, std::min(c->hsplit, c->dp), c->last_shift,
                          c->cold_col16 ? 1 : 0, c->k.plan_kernel ? 1 : 0, c->k.fix_bound ? 1 : 0, c->last_fstep_rebalances,
                          c->group};
  for (int i = 0; i < n; ++i) vals[i] = all[i];
  return DSGD_OK;
}

int dsgd_column_ranks(dsgd_ctx* c, int32_t* rank_of_key) {
  DSGD_TRY(check_ctx(c));
  if (!rank_of_key) return fail(DSGD_EINVAL, "null rank_of_key");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  HIP_TRY(hipMemcpy(rank_of_key, c->d_perm, sizeof(int) * (size_t)c->dp, hipMemcpyDeviceToHost));
  return DSGD_OK;
}

const char* dsgd_grad_kernel_name(dsgd_ctx* c) {
  if (!c) return "";
  return c->last_grad_kernel;
}

int dsgd_device_ptrs(dsgd_ctx* c, void** w_dev, void** g_dev, void** stream) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  // (binding converts slice-major weights back: after a column-slice dsgd_plan_run the live weights are NOT in d_w until
  //  some entry point binds -- this one does, on the stream it hands out)
  DSGD_TRY(bind(c));
  if (w_dev) *w_dev = c->d_w;
  if (g_dev) *g_dev = c->d_gsum;
  if (stream) *stream = c->stream;
  return DSGD_OK;
}

// ---- K8: dense logistic mini-batch step (no reference counterpart; include/dsgd.h) ------------------------------
struct dsgd_dense {
  int D = 0, device = 0, n_cu = 256;
  std::mutex mu;
  hipStream_t stream = nullptr;
  long long n_rows = 0;
  DevBuf<float> d_X, d_y, d_w, d_g;
  DevBuf<float> d_gpart;      // n_wg x D
  DevBuf<double> d_lpart;     // n_wg x 2
  HostBuf<double> h_lpart;    // pinned
  int n_wg = 0;
  bool mfma = false;          // DSGD_DENSE_MFMA=1: forward product with v_mfma_f32_16x16x4_f32 (D a multiple of 256, <= 4096)
  rccl::comm_t comm = nullptr;
  int world = 1;
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t ev_used = 0;
  double ms_sum = 0.0;
  long long ms_n = 0;
  // index lists (dsgd_dense_step_list / _loss_list / _predict_list) cross in pinned memory as the per-request lists of a
  // context do (pin_acquire / pin_sent above): a second call waits for the first call's copy before it refills the buffer
  dsgd_ctx::Pinned pin_idx;
  DevBuf<int> d_idx;          // the list of the call in flight (grown on demand)
  DevBuf<float> d_p;          // dsgd_dense_predict*: probabilities (grown on demand) ...
  HostBuf<float> h_p;         // ... and their pinned landing place
  long long data_gen = 0;     // counts dsgd_dense_load / _generate: a plan checked against other data is refused at its run
  std::vector<dsgd_dense_plan*> plans;   // the plans this object still owns (dsgd_dense_destroy releases them)
};
// an epoch's lists resident on the device: step s is idx[off[s] .. off[s + 1])
struct dsgd_dense_plan {
  DevBuf<int> d_idx;
  std::vector<long long> off;   // n_steps + 1
  long long data_gen = 0;
};
static int dn_bind(dsgd_dense* d) {
  if (!d) return fail(DSGD_EINVAL, "null dense object");
  HIP_TRY(hipSetDevice(d->device));
  return DSGD_OK;
}
static int dn_collect(dsgd_dense* d) {
  for (size_t i = 0; i < d->ev_used; ++i) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, d->ev[i].first, d->ev[i].second));
    d->ms_sum += ms;
    d->ms_n++;
  }
  d->ev_used = 0;
  return DSGD_OK;
}
// One launch over positions [rb, re): rows rb .. re - 1 themselves, or -- d_list given, rb == 0 -- the rows a checked list in
// device memory names.  d_p: the forward-only probability form (grad is false).  Returns the grid, or an error code.
static int dn_launch(dsgd_dense* d, long long rb, long long re, bool grad, const int* d_list = nullptr, float* d_p = nullptr) {
  DenseListArgs l;
  DenseArgs& a = l.a;
  l.idx = d_list;
  l.p_out = d_p;
  a.X = d->d_X;
  a.y = d->d_y;
  a.w = d->d_w;
  a.gpart = grad ? d->d_gpart : nullptr;
  a.lpart = d->d_lpart;
  a.row_begin = rb;
  a.row_end = re;
  a.D = d->D;
  const int rows_per_block = d->mfma ? 16 : DN_ROWS;
  const long long n_blocks = (re - rb + rows_per_block - 1) / rows_per_block;
  const int grid = (int)std::max<long long>(1, std::min<long long>(d->mfma ? d->n_cu : d->n_wg, n_blocks));
  size_t slot = (size_t)-1;
  if (d->prof && grad) {
    if (d->ev_used == d->ev.size() && d->ev.size() >= 4096) {   // bounded pool: collect what has completed so far
      HIP_TRY(hipStreamSynchronize(d->stream));
      DSGD_TRY(dn_collect(d));
    }
    if (d->ev_used == d->ev.size()) {
      hipEvent_t x, y;
      HIP_TRY(hipEventCreate(&x));
      HIP_TRY(hipEventCreate(&y));
      d->ev.emplace_back(x, y);
    }
    slot = d->ev_used++;
    HIP_TRY(hipEventRecord(d->ev[slot].first, d->stream));
  }
  // (the variant on the matrix cores: forward product only; csrc/dsgd_dense.hpp.  DSGD_DENSE_MFMA decides for every form.)
  const dim3 lanes(d->mfma ? d->D / 4 : d->D / DN_COLS);
  const size_t lds = d->mfma ? sizeof(float) * (size_t)d->D : 0;
  if (!d_list && !d_p) {
    hipLaunchKernelGGL(d->mfma ? dsgd_dense_step_mfma_kernel : dsgd_dense_step_kernel, dim3(grid), lanes, lds, d->stream, a);
  } else {
    void (*kern)(DenseListArgs) = d_p ? (d_list ? (d->mfma ? dsgd_dense_proba_list_mfma_kernel : dsgd_dense_proba_list_kernel)
                                                : (d->mfma ? dsgd_dense_proba_mfma_kernel : dsgd_dense_proba_kernel))
                                      : (d->mfma ? dsgd_dense_step_list_mfma_kernel : dsgd_dense_step_list_kernel);
    hipLaunchKernelGGL(kern, dim3(grid), lanes, lds, d->stream, l);
  }
  HIP_TRY(hipGetLastError());
  if (slot != (size_t)-1) HIP_TRY(hipEventRecord(d->ev[slot].second, d->stream));
  return grid;
}

int dsgd_dense_create(int32_t n_features, int32_t device, dsgd_dense** out) {
  if (!out) return fail(DSGD_EINVAL, "null argument");
  if (n_features < 512 || n_features > 8192 || n_features % 512)
    return fail(DSGD_EINVAL, "n_features must be a multiple of 512 in [512, 8192] (one lane owns 8 columns)");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(DSGD_EUNSUPPORTED, "no HIP device visible: libdsgd_hip has no CPU fallback");
  if (device < 0 || device >= n) return fail(DSGD_EINVAL, "device %d out of range (%d devices)", device, n);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(DSGD_EUNSUPPORTED, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  dsgd_dense* d = new (std::nothrow) dsgd_dense();
  if (!d) return fail(DSGD_ENOMEM, "out of host memory");
  d->D = n_features;
  d->device = device;
  d->n_cu = prop.multiProcessorCount;
  d->n_wg = 2 * d->n_cu;   // two workgroups per CU: one computes while the other's loads are in flight
  if (const char* e = getenv("DSGD_DENSE_MFMA")) d->mfma = atoi(e) != 0;
  if (d->mfma && n_features > 4096) {
    delete d;
    return fail(DSGD_EUNSUPPORTED, "the MFMA variant handles at most 4096 features (one wave per 256 columns)");
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
  int rc = e == hipSuccess ? DSGD_OK : fail(DSGD_EHIP, "dense create: %s", hipGetErrorString(e));
  if (!rc) rc = d->d_w.alloc((size_t)d->D);
  if (!rc) rc = d->d_g.alloc((size_t)d->D);
  if (!rc) rc = d->d_gpart.alloc((size_t)d->n_wg * d->D);
  if (!rc) rc = d->d_lpart.alloc(2 * (size_t)d->n_wg);
  if (!rc) rc = d->h_lpart.alloc(2 * (size_t)d->n_wg);
  if (!rc && (e = hipMemset(d->d_w, 0, sizeof(float) * d->D)) != hipSuccess) rc = fail(DSGD_EHIP, "dense create: %s", hipGetErrorString(e));
  if (rc) {
    dsgd_dense_destroy(d);   // (leaves the message alone)
    return rc;
  }
  *out = d;
  return DSGD_OK;
}

int dsgd_dense_destroy(dsgd_dense* d) {
  if (!d) return DSGD_OK;
  (void)hipSetDevice(d->device);
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  if (d->comm && rccl::available()) rccl::CommDestroy(d->comm);
  for (auto& e : d->ev) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  for (dsgd_dense_plan* p : d->plans) delete p;
  const hipStream_t stream = d->stream;
  delete d;   // (the stream is idle: the members release themselves)
  if (stream) (void)hipStreamDestroy(stream);
  return DSGD_OK;
}

static int dn_alloc_rows(dsgd_dense* d, long long n_rows) {
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->d_X.reset();
  d->d_y.reset();
  d->n_rows = 0;
  d->data_gen++;   // (whatever the outcome: the plans checked against the rows that just went are stale)
  DSGD_TRY(d->d_X.alloc((size_t)n_rows * (size_t)d->D));
  DSGD_TRY(d->d_y.alloc((size_t)n_rows));
  d->n_rows = n_rows;
  return DSGD_OK;
}

int dsgd_dense_generate(dsgd_dense* d, int64_t n_rows, uint64_t seed) {
  DSGD_TRY(dn_bind(d));
  if (n_rows < 1) return fail(DSGD_EINVAL, "n_rows must be >= 1");
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_alloc_rows(d, n_rows));
  hipLaunchKernelGGL(dsgd_dense_generate_kernel, dim3((unsigned)std::min<long long>(n_rows, (long long)d->n_cu * 8)), dim3(256), 0,
                     d->stream, d->d_X, d->d_y, (long long)n_rows, d->D, (unsigned long long)seed);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(d->stream));
  return DSGD_OK;
}

int dsgd_dense_load(dsgd_dense* d, int64_t n_rows, const float* X, const float* y) {
  DSGD_TRY(dn_bind(d));
  if (n_rows < 1 || !X || !y) return fail(DSGD_EINVAL, "n_rows must be >= 1 and arrays non-null");
  for (int64_t i = 0; i < n_rows; ++i)
    if (y[i] != 0.0f && y[i] != 1.0f) return fail(DSGD_EINVAL, "label[%lld] = %g, expected 0 or 1", (long long)i, (double)y[i]);
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_alloc_rows(d, n_rows));
  HIP_TRY(hipMemcpy(d->d_X, X, sizeof(float) * (size_t)n_rows * (size_t)d->D, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d->d_y, y, sizeof(float) * (size_t)n_rows, hipMemcpyHostToDevice));
  return DSGD_OK;
}

int dsgd_dense_set_weights(dsgd_dense* d, const float* w) {
  DSGD_TRY(dn_bind(d));
  if (!w) return fail(DSGD_EINVAL, "null w");
  std::lock_guard<std::mutex> lk(d->mu);
  HIP_TRY(hipStreamSynchronize(d->stream));
  HIP_TRY(hipMemcpy(d->d_w, w, sizeof(float) * d->D, hipMemcpyHostToDevice));
  return DSGD_OK;
}
int dsgd_dense_get_weights(dsgd_dense* d, float* w_out) {
  DSGD_TRY(dn_bind(d));
  if (!w_out) return fail(DSGD_EINVAL, "null w_out");
  std::lock_guard<std::mutex> lk(d->mu);
  HIP_TRY(hipStreamSynchronize(d->stream));
  HIP_TRY(hipMemcpy(w_out, d->d_w, sizeof(float) * d->D, hipMemcpyDeviceToHost));
  return DSGD_OK;
}

static int dn_check_range(dsgd_dense* d, long long rb, long long re) {
  if (!d->d_X) return fail(DSGD_ESTATE, "no data (dsgd_dense_generate / dsgd_dense_load)");
  if (re <= rb) return fail(DSGD_EINVAL, "empty row range");
  if (rb < 0 || re > d->n_rows) return fail(DSGD_ERANGE, "rows [%lld, %lld) outside the %lld resident rows", rb, re, d->n_rows);
  return DSGD_OK;
}

// A list of the host's: n >= 1 entries, each a resident row.  Host work only -- nothing is enqueued or changed before a
// list has passed, and no kernel looks at an index again.  `base`: the position of idx[0] in what the caller was given
// (a plan's lists are checked as one).
static int dn_check_list(dsgd_dense* d, const int32_t* idx, long long n, long long base = 0) {
  if (!idx) return fail(DSGD_EINVAL, "null index list");
  if (n < 1) return fail(DSGD_EINVAL, "empty index list");
  if (!d->d_X) return fail(DSGD_ESTATE, "no data (dsgd_dense_generate / dsgd_dense_load)");
  for (long long k = 0; k < n; ++k)
    if (idx[k] < 0 || idx[k] >= d->n_rows)
      return fail(DSGD_ERANGE, "idx[%lld] = %d outside the %lld resident rows", base + k, (int)idx[k], d->n_rows);
  return DSGD_OK;
}
// a checked list into d->d_idx, behind whatever still reads the list before it (one stream)
static int dn_send_list(dsgd_dense* d, const int32_t* idx, long long n) {
  if ((size_t)n > d->d_idx.cap()) {
    HIP_TRY(hipStreamSynchronize(d->stream));
    DSGD_TRY(d->d_idx.reserve((size_t)n, Grow::twice));
  }
  DSGD_TRY(pin_acquire(d->pin_idx, sizeof(int) * (size_t)n));
  memcpy(d->pin_idx.p, idx, sizeof(int) * (size_t)n);
  HIP_TRY(hipMemcpyAsync(d->d_idx, d->pin_idx.p, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, d->stream));
  return pin_sent(d->pin_idx, d->stream);
}

// One step, enqueued: the gradient launch over positions [rb, re) (rows, or the entries of d_list), the reduce and the
// update -- under a communicator the all-reduce and the apply, every rank contributing an equal batch.  The range step,
// the list step and every step of a plan run are this.
static int dn_step(dsgd_dense* d, long long rb, long long re, const int* d_list, float lr) {
  const int grid = dn_launch(d, rb, re, true, d_list);
  if (grid < 0) return grid;
  const float scale = lr / ((float)(re - rb) * (float)d->world);
  hipLaunchKernelGGL(dsgd_dense_reduce_kernel, dim3((d->D + 63) / 64), dim3(1024), 0, d->stream, d->d_gpart, grid, d->D, d->d_g,
                     d->comm ? (float*)nullptr : d->d_w, scale);
  HIP_TRY(hipGetLastError());
  if (d->comm) {
    RCCL_TRY(rccl::AllReduce(d->d_g, d->d_g, (size_t)d->D, rccl::kFloat32, rccl::kSum, d->comm, d->stream));
    hipLaunchKernelGGL(dsgd_dense_apply_kernel, dim3((d->D + 255) / 256), dim3(256), 0, d->stream, d->d_w, d->d_g, d->D, scale);
    HIP_TRY(hipGetLastError());
  }
  return DSGD_OK;
}

int dsgd_dense_step(dsgd_dense* d, int64_t row_begin, int64_t row_end, float lr) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_range(d, row_begin, row_end));
  return dn_step(d, row_begin, row_end, nullptr, lr);
}

int dsgd_dense_step_list(dsgd_dense* d, const int32_t* idx, int64_t n, float lr) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_list(d, idx, n));
  DSGD_TRY(dn_send_list(d, idx, n));
  return dn_step(d, 0, n, d->d_idx, lr);
}

int dsgd_dense_plan_create(dsgd_dense* d, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps,
                           dsgd_dense_plan** out) {
  DSGD_TRY(dn_bind(d));
  if (!idx || !offsets || !out) return fail(DSGD_EINVAL, "null argument");
  if (n_steps < 1 || n_idx < 1) return fail(DSGD_EINVAL, "a plan needs at least one step and one entry");
  if (offsets[0] != 0 || offsets[n_steps] != n_idx)
    return fail(DSGD_EINVAL, "offsets must run from 0 to n_idx = %lld (they run from %lld to %lld)", (long long)n_idx,
                (long long)offsets[0], (long long)offsets[n_steps]);
  for (int64_t s = 0; s < n_steps; ++s) {
    if (offsets[s + 1] < offsets[s]) return fail(DSGD_EINVAL, "offsets decrease at step %lld", (long long)s);
    if (offsets[s + 1] == offsets[s]) return fail(DSGD_EINVAL, "step %lld of the plan is empty", (long long)s);
  }
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_list(d, idx, n_idx));
  dsgd_dense_plan* p = new (std::nothrow) dsgd_dense_plan();
  if (!p) return fail(DSGD_ENOMEM, "out of host memory");
  p->off.assign(offsets, offsets + n_steps + 1);
  p->data_gen = d->data_gen;
  int rc = p->d_idx.alloc((size_t)n_idx);
  hipError_t e = hipSuccess;   // (once per plan, from the caller's pageable memory: the copy has completed when the call returns)
  if (!rc && (e = hipMemcpy(p->d_idx, idx, sizeof(int) * (size_t)n_idx, hipMemcpyHostToDevice)) != hipSuccess)
    rc = fail(DSGD_EHIP, "plan upload: %s", hipGetErrorString(e));
  if (rc) {
    delete p;
    return rc;
  }
  d->plans.push_back(p);
  *out = p;
  return DSGD_OK;
}

static int dn_own_plan(dsgd_dense* d, dsgd_dense_plan* p) {
  if (!p) return fail(DSGD_EINVAL, "null plan");
  if (std::find(d->plans.begin(), d->plans.end(), p) == d->plans.end()) return fail(DSGD_EINVAL, "the plan is not this object's");
  return DSGD_OK;
}

int dsgd_dense_plan_run(dsgd_dense* d, dsgd_dense_plan* p, int64_t step_begin, int64_t step_end, float lr) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_own_plan(d, p));
  const long long n_steps = (long long)p->off.size() - 1;
  if (step_begin < 0 || step_end > n_steps || step_end < step_begin)
    return fail(DSGD_EINVAL, "steps [%lld, %lld) outside the plan's %lld steps", (long long)step_begin, (long long)step_end, n_steps);
  if (!d->d_X) return fail(DSGD_ESTATE, "no data (dsgd_dense_generate / dsgd_dense_load)");
  if (p->data_gen != d->data_gen) return fail(DSGD_ESTATE, "the plan was created before the last dsgd_dense_load / dsgd_dense_generate");
  for (long long s = step_begin; s < step_end; ++s)   // (no upload, and no host synchronisation but a full event pool's)
    DSGD_TRY(dn_step(d, 0, p->off[s + 1] - p->off[s], p->d_idx + p->off[s], lr));
  return DSGD_OK;
}

int dsgd_dense_plan_destroy(dsgd_dense* d, dsgd_dense_plan* p) {
  DSGD_TRY(dn_bind(d));
  if (!p) return DSGD_OK;
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_own_plan(d, p));
  HIP_TRY(hipStreamSynchronize(d->stream));   // (steps of it may still be enqueued)
  d->plans.erase(std::find(d->plans.begin(), d->plans.end(), p));
  delete p;
  return DSGD_OK;
}

int dsgd_dense_synchronize(dsgd_dense* d) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  HIP_TRY(hipStreamSynchronize(d->stream));
  return dn_collect(d);
}

// the evaluation launch over positions [rb, re) and its reply: the partials in one copy, one synchronisation
static int dn_loss(dsgd_dense* d, long long rb, long long re, const int* d_list, double* loss, double* acc) {
  const int grid = dn_launch(d, rb, re, false, d_list);
  if (grid < 0) return grid;
  HIP_TRY(hipMemcpyAsync(d->h_lpart, d->d_lpart, sizeof(double) * 2 * grid, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  double l = 0.0, c = 0.0;
  for (int b = 0; b < grid; ++b) {
    l += d->h_lpart[2 * b];
    c += d->h_lpart[2 * b + 1];
  }
  const double n = (double)(re - rb);
  if (loss) *loss = l / n;
  if (acc) *acc = c / n;
  return DSGD_OK;
}
int dsgd_dense_loss(dsgd_dense* d, int64_t row_begin, int64_t row_end, double* loss, double* acc) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_range(d, row_begin, row_end));
  return dn_loss(d, row_begin, row_end, nullptr, loss, acc);
}
int dsgd_dense_loss_list(dsgd_dense* d, const int32_t* idx, int64_t n, double* loss, double* acc) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_list(d, idx, n));
  DSGD_TRY(dn_send_list(d, idx, n));
  return dn_loss(d, 0, n, d->d_idx, loss, acc);
}

// sigmoid(z) of positions [rb, re) under the resident weights: the forward-only launch, then one copy, one synchronisation
static int dn_predict(dsgd_dense* d, long long rb, long long re, const int* d_list, float* p_out) {
  const size_t n = (size_t)(re - rb);
  if (n > d->d_p.cap()) {
    HIP_TRY(hipStreamSynchronize(d->stream));
    DSGD_TRY(d->d_p.reserve(n, Grow::twice));
  }
  DSGD_TRY(d->h_p.reserve(std::max<size_t>(n, 1024)));
  const int grid = dn_launch(d, rb, re, false, d_list, d->d_p);
  if (grid < 0) return grid;
  HIP_TRY(hipMemcpyAsync(d->h_p, d->d_p, sizeof(float) * n, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  memcpy(p_out, d->h_p, sizeof(float) * n);
  return DSGD_OK;
}
int dsgd_dense_predict(dsgd_dense* d, int64_t row_begin, int64_t row_end, float* p_out) {
  DSGD_TRY(dn_bind(d));
  if (!p_out) return fail(DSGD_EINVAL, "null p_out");
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_range(d, row_begin, row_end));
  return dn_predict(d, row_begin, row_end, nullptr, p_out);
}
int dsgd_dense_predict_list(dsgd_dense* d, const int32_t* idx, int64_t n, float* p_out) {
  DSGD_TRY(dn_bind(d));
  if (!p_out) return fail(DSGD_EINVAL, "null p_out");
  std::lock_guard<std::mutex> lk(d->mu);
  DSGD_TRY(dn_check_list(d, idx, n));
  DSGD_TRY(dn_send_list(d, idx, n));
  return dn_predict(d, 0, n, d->d_idx, p_out);
}

int dsgd_dense_comm_init(dsgd_dense* d, const char* unique_id, int32_t world_size, int32_t rank) {
  DSGD_TRY(dn_bind(d));
  if (!unique_id || world_size < 1 || rank < 0 || rank >= world_size) return fail(DSGD_EINVAL, "bad communicator arguments");
  if (!rccl::available()) return fail(DSGD_ERCCL, "librccl could not be loaded");
  std::lock_guard<std::mutex> lk(d->mu);
  if (d->comm) return fail(DSGD_ESTATE, "communicator already attached");
  rccl::unique_id_t id;
  memcpy(id.internal, unique_id, DSGD_UNIQUE_ID_BYTES);
  RCCL_TRY(rccl::CommInitRank(&d->comm, world_size, id, rank));
  d->world = world_size;
  return DSGD_OK;
}

int dsgd_dense_prof(dsgd_dense* d, int32_t enable, double* kernel_ms_avg, int64_t* n_launches) {
  DSGD_TRY(dn_bind(d));
  std::lock_guard<std::mutex> lk(d->mu);
  HIP_TRY(hipStreamSynchronize(d->stream));
  DSGD_TRY(dn_collect(d));
  if (kernel_ms_avg) *kernel_ms_avg = d->ms_n ? d->ms_sum / (double)d->ms_n : 0.0;
  if (n_launches) *n_launches = d->ms_n;
  d->ms_sum = 0.0;
  d->ms_n = 0;
  d->prof = enable != 0;
  return DSGD_OK;
}

}  // extern "C"
