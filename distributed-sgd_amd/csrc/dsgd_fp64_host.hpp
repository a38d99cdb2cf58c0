// Host code of libdsgd_hip's fp64 mode (DSGD_F_FP64; include/dsgd.h "THE FP64 MODE"): everything that exists only for it, to be
// read from top to bottom.  Host only, like dsgd_buf.hpp; included ONCE by dsgd_hip.hip, inside its translation unit, behind
// the context, the plans' frame (plan_frame / plan_finish / plan_release) and the helpers fp32 shares (stage_lists,
// finish_stats, the sp_* of the Sparse boundary, async_plan_impl and the from-seed plans of dsgd_seed_host.hpp further down), and in front of the
// entry points that dispatch into it (dsgd_sync_step, dsgd_plan_run, dsgd_load_csr_f64, the *_f64 twins of fp32 calls).  The
// kernels are in dsgd_cs64.hpp (column slices) and dsgd_rp64.hpp (the row-parallel family).
//
// The sections: 1 state and conversions; 2 column-slice plans; 3 the row-parallel step -- its buffers, Rp64Step (the description
// of one step) and the enqueue functions, the ONLY launch sites of the family; 4 requests; 5 an epoch in one call; 6 resident
// plans; 7 ... across ranks; 8 running a plan -- plan_run64 chooses among 2, 6 and 7, so it stands behind them, with the run
// entry points and the requests that ARE one-step column-slice plans (sync_step64, async_step64).
//
// Forward declarations.  This file holds none.  ONE is left in dsgd_hip.hip, of cs64_refused (section 2) in front of plan_finish:
// plan_finish words the refusal of a column-slice layout that an fp64 plan cannot hold, and this file needs plan_finish -- a true
// cycle between the shared plan code and the mode.  Everything else is defined before its first use.
#pragma once

// ======== 1. State and conversions ========
// ... and with a communicator attached (dsgd_comm_init_f64) the plans: the persistent column-slice kernel cannot hold a collective
static int refuse_fp64_comm(dsgd_ctx* c, const char* what) {
  if (c->fp64 && c->comm)
    return fail(DSGD_EUNSUPPORTED, "%s is not available in an fp64 context with a communicator attached (dsgd_sync_step_f64 is "
                                   "the step that spans the ranks)", what);
  return DSGD_OK;
}
static int require_fp64(dsgd_ctx* c, const char* what) {
  if (!c->fp64) return fail(DSGD_ESTATE, "%s needs an fp64 context (dsgd_config.flags = DSGD_F_FP64)", what);
  return DSGD_OK;
}
// Double data loaded: what a resident plan or dsgd_comm_init_f64's communicator would need is refused (nothing changed, the
// context usable; dsgd_comm_init_f64v attaches one whose gather slots hold both words)
static int refuse_val64(dsgd_ctx* c, const char* what) {
  if (c->d_val64)
    return fail(DSGD_EUNSUPPORTED, "%s is not available on Double feature values (dsgd_load_csr_f64): the column-slice kernels hold "
                                   "float values in registers and a communicator's gather slots one word per column; "
                                   "dsgd_sync_step_f64 / dsgd_async_step_f64 serve Double data", what);
  return DSGD_OK;
}

static int put64(dsgd_ctx* c, const double* h, double* d_rank) {   // key order (host) -> rank order (device), filtered
  HIP_TRY(hipMemcpyAsync(c->d_io64, h, sizeof(double) * c->dp, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(dsgd_permute64_in_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, c->d_io64, d_rank, c->d_perm, c->dp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DSGD_OK;
}
static int take64(dsgd_ctx* c, const double* d_rank, double* h) {   // rank order (device) -> key order (host)
  hipLaunchKernelGGL(dsgd_permute64_out_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_rank, c->d_io64, c->d_perm, c->dp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h, c->d_io64, sizeof(double) * c->dp, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DSGD_OK;
}

int dsgd_set_weights_f64(dsgd_ctx* c, const double* w) {
  DSGD_TRY(check_ctx(c));
  if (!w) return fail(DSGD_EINVAL, "null w");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_set_weights_f64"));
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));
  return put64(c, w, c->d_w64);
}

int dsgd_get_weights_f64(dsgd_ctx* c, double* w_out) {
  DSGD_TRY(check_ctx(c));
  if (!w_out) return fail(DSGD_EINVAL, "null w_out");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_get_weights_f64"));
  DSGD_TRY(bind(c));
  return take64(c, c->d_w64, w_out);
}

int dsgd_set_dim_sparsity_f64(dsgd_ctx* c, const double* ds) {
  DSGD_TRY(check_ctx(c));
  if (!ds) return fail(DSGD_EINVAL, "null ds");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_set_dim_sparsity_f64"));
  DSGD_TRY(bind(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(put64(c, ds, c->d_ds64));
  c->have_ds = true;
  return DSGD_OK;
}

int dsgd_get_dim_sparsity_f64(dsgd_ctx* c, double* ds_out) {
  DSGD_TRY(check_ctx(c));
  if (!ds_out) return fail(DSGD_EINVAL, "null ds_out");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_get_dim_sparsity_f64"));
  DSGD_TRY(bind(c));
  return take64(c, c->d_ds64, ds_out);
}

int dsgd_precision(dsgd_ctx* c, int32_t* bits_out) {
  DSGD_TRY(check_ctx(c));
  if (!bits_out) return fail(DSGD_EINVAL, "null bits_out");
  *bits_out = c->fp64 ? 64 : 32;
  return DSGD_OK;
}

// ======== 2. Column-slice plans (csrc/dsgd_cs64.hpp) ========
// the fp64 weights (and a copy of dimSparsity) slice-major
static int cs64_slice(dsgd_ctx* c) {
  if (c->cs_w_G == CS64_G) return DSGD_OK;
  const int Sp = cs64_sp(c->dp), n = CS64_G * Sp;
  DSGD_TRY(c->d_cs_w64.reserve((size_t)n));
  DSGD_TRY(c->d_cs_ds64.reserve((size_t)n));
  hipLaunchKernelGGL(dsgd_cs64_slice_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_w64, c->d_cs_w64, c->dp, Sp);
  hipLaunchKernelGGL(dsgd_cs64_slice_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_ds64, c->d_cs_ds64, c->dp, Sp);
  HIP_TRY(hipGetLastError());
  c->cs_w_G = CS64_G;
  return DSGD_OK;
}
// the steps [step_begin, step_end) of a plan in an fp64 context (csrc/dsgd_cs64.hpp): ONE launch.  async: the asynchronous
// iterations of a one-worker plan (dsgd_cs64_async_kernel), `delta` ([CS64_G][Sp]) receiving their updates or null
static int launch_cs64(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, double lr, bool async = false,
                       double* delta = nullptr) {
  const int Sp = cs64_sp(c->dp), n = CS64_G * Sp;
  if (!c->d_cs64_x) {
    DSGD_TRY(c->d_cs64_x.alloc((size_t)2 * CS64_G * CS64_XSTRIDE2));
    HIP_TRY(hipMemsetAsync(c->d_cs64_x, 0, sizeof(unsigned long long) * 2 * CS64_G * CS64_XSTRIDE2, c->stream));
  }
  if (!c->d_cs_sync) {
    DSGD_TRY(c->d_cs_sync.alloc(2));
    HIP_TRY(hipMemsetAsync(c->d_cs_sync, 0, sizeof(unsigned int) * 2, c->stream));
  }
  DSGD_TRY(cs64_slice(c));   // they stay slice-major until something else binds
  const unsigned long long n_launch = (unsigned long long)(step_end - step_begin);
  if ((unsigned long long)c->cs64_tag0 + n_launch + 1ull >= (1ull << 32)) {   // (the tags would wrap: start the count again)
    HIP_TRY(hipMemsetAsync(c->d_cs64_x, 0, sizeof(unsigned long long) * 2 * CS64_G * CS64_XSTRIDE2, c->stream));
    c->cs64_tag0 = 0;
  }
  Cs64Args a;
  a.hdr = p->d_cs_hdr;
  a.slot_meta = p->d_cs_meta;
  a.row_first = p->d_cs_rf;
  a.col = p->d_cs_col;
  a.val = p->d_cs_val;
  a.clist = p->d_cs_cl;
  a.w = c->d_cs_w64;
  a.ds = c->d_cs_ds64;
  a.xbuf = c->d_cs64_x;
  a.sync = c->d_cs_sync;
  a.sc = c->d_sc;
  a.n_steps_plan = p->n_steps;
  a.step_begin = step_begin;
  a.step_end = step_end;
  a.slot_stride = p->cs_slot_stride;
  a.row_stride = p->cs_row_stride;
  a.cl_stride = p->cs_cl_stride;
  a.tag0 = c->cs64_tag0;
  c->cs64_tag0 += (unsigned int)n_launch;
  a.lr = lr;
  a.lambda = c->cfg.lambda;
  a.vexp = c->vexp;
  a.dp = c->dp;
  a.K = p->n_workers;
  a.gate_rec = p->d_gate_rec;
  a.s_rec = p->d_s_rec;
  a.gate_words = p->gate_words;
  const size_t lds = (size_t)cs64_lds_bytes(c->dp, a.K);
  c->ctr_known = false;
  if (async && p->cs_spl == 1)
    hipLaunchKernelGGL((dsgd_cs64_async_kernel<CS_THREADS, 1, 4>), dim3(CS64_G), dim3(CS_THREADS), lds, c->stream, a, delta);
  else if (async)
    hipLaunchKernelGGL((dsgd_cs64_async_kernel<CS_THREADS, 2, 8>), dim3(CS64_G), dim3(CS_THREADS), lds, c->stream, a, delta);
  else if (p->cs_spl == 1)
    hipLaunchKernelGGL((dsgd_cs64_step_kernel<CS_THREADS, 1, 4>), dim3(CS64_G), dim3(CS_THREADS), lds, c->stream, a);
  else
    hipLaunchKernelGGL((dsgd_cs64_step_kernel<CS_THREADS, 2, 8>), dim3(CS64_G), dim3(CS_THREADS), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = async ? "dsgd_cs64_async_kernel" : "dsgd_cs64_step_kernel";
  c->last_shift = p->cs_shift[(size_t)(step_end - 1)] + 32;
  return DSGD_OK;
}
// what a one-step fp64 plan of n_workers lists and `rows` rows in all can hold (plan_frame's refusals, word for word): the
// calls that run such a plan on float data keep these limits on Double data, where the row-parallel pair serves them
static int cs64_step_limits(dsgd_ctx* c, int n_workers, long long rows) {
  if (n_workers > CS64_MAX_K)
    return fail(DSGD_EUNSUPPORTED, "fp64 plans host at most %d workers per step (this plan has %d)", CS64_MAX_K, n_workers);
  if (rows > CS_MAX_SLOTS)
    return fail(DSGD_EUNSUPPORTED, "fp64 plans take at most %d rows per step (this plan has a step of %lld)", CS_MAX_SLOTS, rows);
  if (cs64_lds_bytes(c->dp, n_workers) > CS64_LDS_MAX || c->dp < 4 * CS64_G)
    return fail(DSGD_EUNSUPPORTED, "fp64 plans: a model of %d features needs %lld bytes of LDS per slice at %d workers (at most %lld; "
                                   "at least %d features)", c->cfg.n_features, cs64_lds_bytes(c->dp, n_workers), n_workers, CS64_LDS_MAX,
                4 * CS64_G - 1);
  return DSGD_OK;
}
static int cs64_refused(dsgd_ctx* c) {
  return fail(DSGD_EUNSUPPORTED, "fp64 plan: a row index outside the loaded data, or a step whose layout exceeds dsgd_cs64_step_kernel "
                                 "(%d slots or %d columns of one slice per step), or a layout beyond DSGD_CS_MAX_MB = %d MiB", CS_MAX_SLOTS,
              CS_MAX_CLT * CS_THREADS, c->k.cs_max_mb);
}

// ======== 3. The row-parallel step (csrc/dsgd_rp64.hpp): its buffers, its description, its enqueue functions ========
// (SlaveImpl.gradient in Double and synchronous steps of any number of workers and rows)
static int rp64_ensure(dsgd_ctx* c, int n_workers) {
  DSGD_TRY(c->d_rp64_s.reserve(1));
  DSGD_TRY(c->d_rp64_g.reserve((size_t)c->dp));
  if (c->rp64_k < n_workers) {   // (zeroed once; every finish leaves them zeroed)
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->rp64_k = 0;
    const long long stride = ((long long)c->dp + 63) & ~63LL;
    const int cap = std::max(n_workers, 4);
    DSGD_TRY(c->d_rp64_acc.alloc((size_t)stride * (size_t)cap));
    HIP_TRY(hipMemsetAsync(c->d_rp64_acc, 0, sizeof(unsigned long long) * (size_t)stride * (size_t)cap, c->stream));
    c->rp64_stride = stride;
    c->rp64_k = cap;
  }
  // the second word of a column sum, in the shape of the first: Double data only (a float-data context never allocates it)
  if (c->d_val64 && !(c->d_rp64v_lo && c->rp64v_k >= c->rp64_k && c->rp64v_stride == c->rp64_stride)) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->rp64v_k = 0;
    const size_t words = (size_t)c->rp64_stride * (size_t)c->rp64_k;
    DSGD_TRY(c->d_rp64v_lo.alloc(words));
    HIP_TRY(hipMemsetAsync(c->d_rp64v_lo, 0, sizeof(unsigned long long) * words, c->stream));
    c->rp64v_k = c->rp64_k;
    c->rp64v_stride = c->rp64_stride;
  }
  return DSGD_OK;
}
// ---- ... across ranks (a communicator attached with dsgd_comm_init_f64 or dsgd_comm_init_f64v; csrc/dsgd_rp64_gather.hpp) ----
static long long rp64_gather_pad(int world) { return ((long long)world + 63) & ~63LL; }
static void rp64_gather_drop(dsgd_ctx* c) {   // (after a failure half way: the next step starts from a zeroed buffer)
  (void)hipStreamSynchronize(c->stream);
  c->d_rp64_gath.reset();
  c->d_rp64_gsegs.reset();
  c->rp64_gk = 0;
  c->rp64_gwords = 0;
}
// K slots of `words` planes each (1: float values, 2: Double values); a buffer of the other width is replaced
static int rp64_gather_ensure(dsgd_ctx* c, int K, int words) {
  DSGD_TRY(c->h_rp64_ranks.reserve(64));
  if (c->rp64_gk >= K && c->rp64_gwords == words && c->d_rp64_gath) return DSGD_OK;
  rp64_gather_drop(c);
  const long long stride = rp64_gather_stride(c->dp);
  const size_t n_words = (size_t)rp64_gather_pad(c->world) + (size_t)rp64_gather_slot_words(c->dp, words) * (size_t)K;
  DSGD_TRY(c->d_rp64_gath.alloc(n_words));
  DSGD_TRY(c->d_rp64_gsegs.alloc((size_t)K));
  HIP_TRY(hipMemsetAsync(c->d_rp64_gath, 0, sizeof(unsigned long long) * n_words, c->stream));
  c->rp64_gstride = stride;
  c->rp64_gk = K;
  c->rp64_gwords = words;
  return DSGD_OK;
}
// the K worker slots' messages: one per slot and plane, cut at RP64_MSG_WORDS (a step's, and a plan run's per step)
static int rp64_gather_slots(dsgd_ctx* c, int K) {
  const int words = c->rp64_gwords;
  unsigned long long* slots = c->d_rp64_gath + rp64_gather_pad(c->world);
  for (long long g = 0; g < (long long)K * words; ++g)   // (plane g % words of worker g / words)
    for (long long off = 0; off < c->rp64_gstride; off += RP64_MSG_WORDS) {
      unsigned long long* at = slots + g * c->rp64_gstride + off;
      const size_t n = (size_t)std::min<long long>(RP64_MSG_WORDS, c->rp64_gstride - off);
      const int r = rccl::AllReduce(at, at, n, rccl::kInt64, rccl::kSum, c->comm, c->stream);
      if (r) return fail(DSGD_ERCCL, "ncclAllReduce(worker %lld's sums): %s", g / words, rccl::GetErrorString(r));
    }
  return DSGD_OK;
}
// Whose accumulators a step sums into: the context's own, or under a communicator this rank's slots of the gather buffer
// (rp64_gather_ensure came first) -- with this rank's word in front of the slots (dsgd_sync_step_f64: the ranks agree per
// step) or without (a plan run: they agreed once per call).  The finish of a gather step folds every rank's workers.
enum Rp64Where { RP64_LOCAL, RP64_GATHER_WORD, RP64_GATHER_PLAN };
// ONE step of the family as the host enqueues it: the arguments of the two bodies, which finish runs, whose accumulators, and
// the value type -- chosen HERE, once, from the data the context holds.
struct Rp64Step {
  Rp64Args a;
  Rp64FinishArgs f;
  int mode;    // RP64_GRADIENT (worker 0's gradient into d_rp64_g), RP64_STEP, RP64_ASYNC (one worker; delta: key order, may be null)
  Rp64Where where;
  bool v64;
};
// The step of n_workers lists idx / segs, the longest of max_items rows (rp64_ensure came first).  The workgroups a worker's
// list is spread over: one per 16 rows of the longest list, all lists together at most two per compute unit (each workgroup
// flushes its hot words once).  The weights stay in whichever layout they are, slice-major between plan runs.  Double data
// can meet slice-major weights too: plans are refused at their CREATION on Double data, but a plan made on float data outlives
// dsgd_load_csr_f64 (it is laid out again for the new data and runs on the values rounded to float), and its run leaves the
// weights slice-major for the next dsgd_gradient_f64 (w = NULL), dsgd_sync_step_f64 or dsgd_async_step_f64.  The bodies read
// either layout through rp64_at; tests/test_gpu_fp64_values.py takes that path.
static Rp64Step rp64_step(dsgd_ctx* c, int n_workers, long long max_items, int mode, Rp64Where where, double lr, double* delta, const int* idx,
                          const WorkSeg* segs) {
  constexpr long long rows_per_block = RP64_THREADS / RP64_GROUP;
  Rp64Step s;
  Rp64Args& a = s.a;
  Rp64FinishArgs& f = s.f;
  s.mode = mode;
  s.where = where;
  s.v64 = c->d_val64 != nullptr;
  const bool sliced = c->cs_w_G == CS64_G;
  const int Sp = sliced ? cs64_sp(c->dp) : 0;
  double* w = sliced ? c->d_cs_w64 : c->d_w64;
  a.w = w;
  a.ds = c->d_ds64;
  a.Sp = Sp;
  a.dp = c->dp;
  a.vexp = c->vexp;
  a.K = n_workers;
  a.idx = idx;
  a.segs = segs;
  a.blocks_per_worker = std::max<long long>(1, std::min<long long>((max_items + rows_per_block - 1) / rows_per_block,
                                                                   std::max<long long>(1, (long long)c->n_cu * 2 / n_workers)));
  a.with_s = mode == RP64_ASYNC ? 0 : 1;   // (the asynchronous iteration: s from dsgd_rp64v_s_sliced_kernel)
  a.acc[0] = c->d_rp64_acc;
  a.acc[1] = s.v64 ? c->d_rp64v_lo : nullptr;
  a.acc_stride = c->rp64_stride;
  a.lambda = c->cfg.lambda;
  a.s_out = c->d_rp64_s;
  a.sc = c->d_sc;
  a.rank_word = nullptr;
  f.acc[0] = a.acc[0];
  f.acc[1] = a.acc[1];
  f.acc_stride = a.acc_stride;
  f.segs = segs;
  f.K = n_workers;
  f.dp = c->dp;
  f.vexp = c->vexp;
  f.Sp = Sp;
  f.s = c->d_rp64_s;
  f.perm = c->d_perm;
  f.g_out = mode == RP64_ASYNC ? delta : c->d_rp64_g;
  f.w = w;
  f.lr = lr;
  if (where != RP64_LOCAL) {   // this rank's slots of the gather buffer; the finish over every rank's workers
    unsigned long long* slots = c->d_rp64_gath + rp64_gather_pad(c->world);
    const long long slot = c->rp64_gstride * c->rp64_gwords;
    a.acc[0] = slots + (long long)c->rank * n_workers * slot;
    a.acc[1] = s.v64 ? a.acc[0] + c->rp64_gstride : nullptr;   // (the LO plane, directly behind the HI plane)
    a.acc_stride = slot;
    if (where == RP64_GATHER_WORD) a.rank_word = c->d_rp64_gath + c->rank;
    f.acc[0] = slots;
    f.acc[1] = s.v64 ? slots + c->rp64_gstride : nullptr;
    f.acc_stride = slot;
    f.segs = c->d_rp64_gsegs;
    f.K = n_workers * c->world;
  }
  return s;
}
// the workgroups of a step's gradient (or fused) launch: the lists' and the one that computes s
static long long rp64_grid(const Rp64Step& s) { return s.a.blocks_per_worker * s.a.K + s.a.with_s; }

// The enqueue functions: every launch of the family is here and nowhere else.  They return hipGetLastError() behind their
// launches; the callers word the failure (rp64_launched: the common wording) and clean up.  Gradient and finish are enqueued
// separately: under a communicator the slots' messages and a header kernel go between them.
//
// The gradient of a step: plain; recording (rec: the gate record of a local plan's step, whose mask the caller zeroed in front --
// s always from the last workgroup here); or fused with its finish in ONE launch (fused: a local step whose grid is resident as
// a whole, dsgd_sync_steps_f64).
static hipError_t rp64_enqueue_grad(dsgd_ctx* c, Rp64Step& s, const Rp64Rec* rec = nullptr, const Rp64StepSync* fused = nullptr) {
  if ((rec || fused) && s.where != RP64_LOCAL) return hipErrorInvalidValue;   // (no such kernel; nothing asks)
  if (rec) s.a.with_s = 1;
  const dim3 gg((unsigned)rp64_grid(s)), th(RP64_THREADS);
  if (s.v64) {
    const CsrView64 m = view64(c);
    if (fused)
      hipLaunchKernelGGL(dsgd_rp64v_step_kernel, gg, th, 0, c->stream, m, s.a, s.f, *fused);
    else if (rec)
      hipLaunchKernelGGL(dsgd_rp64v_grad_rec_kernel, gg, th, 0, c->stream, m, s.a, *rec);
    else if (s.where == RP64_GATHER_WORD)
      hipLaunchKernelGGL(dsgd_rp64v_grad_gather_kernel, gg, th, 0, c->stream, m, s.a);
    else if (s.where == RP64_GATHER_PLAN)
      hipLaunchKernelGGL(dsgd_rp64v_grad_gather_plan_kernel, gg, th, 0, c->stream, m, s.a);
    else
      hipLaunchKernelGGL(dsgd_rp64v_grad_kernel, gg, th, 0, c->stream, m, s.a);
  } else {
    const CsrView m = view(c);
    if (fused)
      hipLaunchKernelGGL(dsgd_rp64_step_kernel, gg, th, 0, c->stream, m, s.a, s.f, *fused);
    else if (rec)
      hipLaunchKernelGGL(dsgd_rp64_grad_rec_kernel, gg, th, 0, c->stream, m, s.a, *rec);
    else if (s.where == RP64_GATHER_WORD)
      hipLaunchKernelGGL(dsgd_rp64_grad_gather_kernel, gg, th, 0, c->stream, m, s.a);
    else if (s.where == RP64_GATHER_PLAN)
      hipLaunchKernelGGL(dsgd_rp64_grad_gather_plan_kernel, gg, th, 0, c->stream, m, s.a);
    else
      hipLaunchKernelGGL(dsgd_rp64_grad_kernel, gg, th, 0, c->stream, m, s.a);
  }
  return hipGetLastError();
}
// the finish of a step's MODE on either value type (float values: the asynchronous iteration has a kernel of its own name)
template <int MODE>
static void rp64_launch_finish(dsgd_ctx* c, const Rp64Step& s) {
  const dim3 fg((unsigned)std::min<long long>(((long long)c->dp + RP64_THREADS - 1) / RP64_THREADS, (long long)c->n_cu * 4)), th(RP64_THREADS);
  if (s.v64)
    hipLaunchKernelGGL(dsgd_rp64v_finish_kernel<MODE>, fg, th, 0, c->stream, s.f);
  else if (MODE == RP64_ASYNC)
    hipLaunchKernelGGL(dsgd_rp64_finish_async_kernel, fg, th, 0, c->stream, s.f);
  else
    hipLaunchKernelGGL(dsgd_rp64_finish_kernel<MODE == RP64_STEP>, fg, th, 0, c->stream, s.f);
}
// The finish of a step (not of a fused one, which holds its own).  The asynchronous iteration: s first, in the order of the
// float data's asynchronous kernel (the same bits on values a float holds), between the gradient and the finish.
static hipError_t rp64_enqueue_finish(dsgd_ctx* c, const Rp64Step& s) {
  if (s.mode == RP64_ASYNC) {
    hipLaunchKernelGGL(dsgd_rp64v_s_sliced_kernel, dim3(1), dim3(CS_THREADS), 0, c->stream, s.a.w, c->d_ds64, s.a.Sp, c->dp, c->cfg.lambda, c->d_rp64_s);
    rp64_launch_finish<RP64_ASYNC>(c, s);
  } else if (s.mode == RP64_STEP) {
    rp64_launch_finish<RP64_STEP>(c, s);
  } else {
    rp64_launch_finish<RP64_GRADIENT>(c, s);
  }
  return hipGetLastError();
}
static int rp64_launched(hipError_t e) { return e == hipSuccess ? DSGD_OK : fail(DSGD_EHIP, "hipGetLastError(): %s", hipGetErrorString(e)); }
// the longest of the K lists of step t in a plan's or a call's offsets
template <typename T>
static long long rp64_longest(const T* offsets, long long t, int K) {
  long long mx = 0;
  for (int k = 0; k < K; ++k) mx = std::max<long long>(mx, offsets[t * K + k + 1] - offsets[t * K + k]);
  return mx;
}

// ======== 4. Requests: one gradient, one synchronous step (one process or across ranks), a peer's update ========
// the lists are host data: checked here, before anything moves (an index outside the data changes nothing)
static int rp64_check_lists(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers) {
  for (int k = 0; k < n_workers; ++k) {
    if (n_per_worker[k] <= 0 || !idx_per_worker[k])
      return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors (worker %d)", k);   // ref: math/Vec.scala:129
    for (int64_t t = 0; t < n_per_worker[k]; ++t)
      if (idx_per_worker[k][t] < 0 || idx_per_worker[k][t] >= c->n_rows)
        return fail(DSGD_ERANGE, "sample index %d of worker %d outside the %lld loaded rows", idx_per_worker[k][t], k, c->n_rows);
  }
  return DSGD_OK;
}
// Behind the gradient kernel: the ranks' words first -- every rank must have been called with the same number of hosted
// workers on the same value type, or the ranks would enqueue different numbers of messages and a collective that only some
// ranks join never completes; this is the one host read of the step besides its statistics -- then the worker slots, one
// message per slot and plane (cut at RP64_MSG_WORDS), then the headers.  Returns with the finish still to launch.
static int rp64_gather(dsgd_ctx* c, int k) {
  const int W = c->world, K = k * W, words = c->rp64_gwords;
  const long long slot = c->rp64_gstride * words;
  const unsigned long long mine = rp64_rank_word(k, words == 2);
  unsigned long long* slots = c->d_rp64_gath + rp64_gather_pad(W);
  int r = rccl::AllReduce(c->d_rp64_gath, c->d_rp64_gath, (size_t)W, rccl::kInt64, rccl::kSum, c->comm, c->stream);
  if (r) return fail(DSGD_ERCCL, "ncclAllReduce(hosted workers): %s", rccl::GetErrorString(r));
  HIP_TRY(hipMemcpyAsync(c->h_rp64_ranks, c->d_rp64_gath, sizeof(unsigned long long) * (size_t)W, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int q = 0; q < W; ++q)
    if (c->h_rp64_ranks[q] != mine) {
      // nothing of this step has left the rank besides these words: its own slots and the words are zeroed again
      const unsigned long long theirs = c->h_rp64_ranks[q];
      HIP_TRY(hipMemsetAsync(c->d_rp64_gath, 0, sizeof(unsigned long long) * (size_t)W, c->stream));
      HIP_TRY(hipMemsetAsync(slots + (long long)c->rank * k * slot, 0, sizeof(unsigned long long) * (size_t)k * (size_t)slot, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (rp64_rank_word_v64(theirs) != (words == 2))
        return fail(DSGD_EINVAL, "rank %d holds %s feature values, this rank (%d) %s ones: every rank of a step holds the same value "
                                 "type (dsgd_load_csr / dsgd_load_csr_f64; the weights are unchanged)", q, rp64_rank_word_v64(theirs) ? "Double" : "float",
                    c->rank, words == 2 ? "Double" : "float");
      return fail(DSGD_EINVAL, "rank %d was called with %llu hosted workers, this rank (%d) with %d: every rank of a step hosts the "
                               "same number (the weights are unchanged)", q, (unsigned long long)(unsigned int)rp64_rank_word_k(theirs), c->rank, k);
    }
  DSGD_TRY(rp64_gather_slots(c, K));
  hipLaunchKernelGGL(dsgd_rp64_header_kernel, dim3(1), dim3(RP64_THREADS), 0, c->stream, c->d_rp64_gath, W, slots, slot, K, c->dp,
                     c->d_rp64_gsegs, c->d_sc);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
// A request's step over the staged lists (c->cur_idx, c->d_segs), on the context's float or Double values (rp64_ensure came
// first): the gradient, under a communicator (gather: rp64_gather_ensure came first, with one plane per slot on float values and
// two on Double ones) the ranks' agreement and the slots' messages, the finish.
static int rp64_launch(dsgd_ctx* c, int n_workers, long long max_items, int mode, double lr, double* delta = nullptr, bool gather = false) {
  const bool v64 = c->d_val64 != nullptr;
  if (gather && (mode != RP64_STEP || c->rp64_gwords != (v64 ? 2 : 1)))   // (the gather buffer is a step's, in the planes of this value type; the entry points never ask)
    return fail(DSGD_ESTATE, "internal: no row-parallel fp64 kernel for %s on %s values", "this gather", v64 ? "Double" : "float");
  Rp64Step s = rp64_step(c, n_workers, max_items, mode, gather ? RP64_GATHER_WORD : RP64_LOCAL, lr, delta, c->cur_idx, c->d_segs);
  DSGD_TRY(rp64_launched(rp64_enqueue_grad(c, s)));
  if (gather) DSGD_TRY(rp64_gather(c, n_workers));
  return rp64_launched(rp64_enqueue_finish(c, s));
}

int dsgd_gradient_f64(dsgd_ctx* c, const double* w, const int32_t* idx, int64_t n, double* g_out, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!g_out) return fail(DSGD_EINVAL, "null g_out");
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");  // ref: math/Vec.scala:129
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_gradient_f64"));
  DSGD_TRY(bind(c, w == nullptr));   // (the request's weights replace the resident ones: rank order then)
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));   // the accumulators and (with w != NULL) the weights belong to the running engine
  DSGD_TRY(prepare_layout(c));
  const int64_t nn = n;
  DSGD_TRY(rp64_check_lists(c, &idx, &nn, 1));
  if (w) {
    DSGD_TRY(put64(c, w, c->d_w64));
    c->s_dirty = true;
  }
  DSGD_TRY(rp64_ensure(c, 1));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(rp64_launch(c, 1, mx, RP64_GRADIENT, 0.0));
  const size_t bytes = sizeof(double) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_out, bytes));
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_rp64_g, bytes, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  memcpy(g_out, c->pin_out.p, bytes);
  DSGD_TRY(check_err_flag(c));
  if (stats) {
    stats->n_samples = n;
    stats->n_active = (int64_t)c->h_sc->n_active;
  }
  return DSGD_OK;
}

// the row-parallel step of one process (locked, bound, layout ready)
static int sync_step64_rows(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers, double lr,
                            dsgd_batch_stats* stats) {
  DSGD_TRY(rp64_check_lists(c, idx_per_worker, n_per_worker, n_workers));
  DSGD_TRY(rp64_ensure(c, n_workers));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
  DSGD_TRY(rp64_launch(c, n_workers, mx, RP64_STEP, lr));
  c->s_dirty = true;
  return finish_stats(c, stats, tot);
}

// the step of n_workers hosted workers under a communicator (locked, bound, layout ready): the oracle's synchronous step over
// n_workers * world workers in rank-major order; the statistics are the job's
static int sync_step64_ranks(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers, double lr,
                             dsgd_batch_stats* stats) {
  if (n_workers > 0x7fffffff / c->world) return fail(DSGD_EINVAL, "n_workers * world overflows");
  DSGD_TRY(rp64_check_lists(c, idx_per_worker, n_per_worker, n_workers));
  DSGD_TRY(rp64_ensure(c, 1));   // (s and the request's gradient; the local accumulators are not used)
  DSGD_TRY(rp64_gather_ensure(c, n_workers * c->world, c->d_val64 ? 2 : 1));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
  int rc = rp64_launch(c, n_workers, mx, RP64_STEP, lr, nullptr, true);
  if (rc == DSGD_OK) {
    c->s_dirty = true;
    rc = finish_stats(c, stats, tot);
    if (rc == DSGD_OK && stats) stats->n_samples = (int64_t)c->h_sc->n_samples;
  }
  if (rc != DSGD_OK && rc != DSGD_EINVAL) rp64_gather_drop(c);   // (DSGD_EINVAL: the ranks disagreed, the buffer is clean)
  return rc;
}

int dsgd_sync_step_f64(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers, double lr,
                       dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !idx_per_worker || !n_per_worker) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors (no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_sync_step_f64"));
  DSGD_TRY(bind(c, true));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  if (c->comm) return sync_step64_ranks(c, idx_per_worker, n_per_worker, n_workers, lr, stats);
  return sync_step64_rows(c, idx_per_worker, n_per_worker, n_workers, lr, stats);
}

int dsgd_update_grad_f64(dsgd_ctx* c, const int32_t* key, const double* dv, int64_t nnz) {
  DSGD_TRY(check_ctx(c));
  if (nnz < 0 || (nnz > 0 && (!key || !dv))) return fail(DSGD_EINVAL, "bad update arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_update_grad_f64"));
  if (nnz == 0) return DSGD_OK;
  {   // the keys are host data: validated here, before anything moves (a Sparse delta holds each key once)
    std::vector<unsigned char> seen((size_t)c->dp, 0);
    for (int64_t i = 0; i < nnz; ++i)
      if (key[i] < 0 || key[i] >= c->dp) return fail(DSGD_ERANGE, "key %d at position %lld outside [0, %d]", key[i], (long long)i, c->dp - 1);
    for (int64_t i = 0; i < nnz; ++i) {
      if (seen[(size_t)key[i]]) return fail(DSGD_EINVAL, "key %d repeated at position %lld: a Sparse delta has unique keys", key[i], (long long)i);
      seen[(size_t)key[i]] = 1;
    }
  }
  DSGD_TRY(bind(c, true));   // (the weights stay in whichever layout they are: slice-major between plan runs)
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(c->d_upd64_key.reserve((size_t)std::max<long long>(nnz, 4096)));
  DSGD_TRY(c->d_upd64_dv.reserve((size_t)std::max<long long>(nnz, 4096)));
  HIP_TRY(hipMemcpyAsync(c->d_upd64_key, key, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_upd64_dv, dv, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
  const bool sliced = c->cs_w_G == CS64_G;
  const int Sp = sliced ? cs64_sp(c->dp) : 0;
  double* w = sliced ? c->d_cs_w64 : c->d_w64;
  const int n = sliced ? CS64_G * Sp : c->dp;
  hipLaunchKernelGGL(dsgd_update64_kernel, dim3((unsigned)std::min<long long>((nnz + 255) / 256, (long long)c->n_cu * 4)), dim3(256), 0,
                     c->stream, c->d_upd64_key, c->d_upd64_dv, (int)nnz, c->d_perm, w, Sp);
  hipLaunchKernelGGL(dsgd_filter64_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, w, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->s_dirty = true;
  return DSGD_OK;
}


// ======== 5. An epoch's steps in one call ========
// how many workgroups of the fused kernel a compute unit holds: asked once per kernel.  A step takes the fused form only where
// its grid is at most that figure x the compute units (a grid that is not resident as a whole would wait for itself); the
// grids of rp64_step are at most two workgroups per unit and one more.
static int rp64_fused_cap(dsgd_ctx* c, bool v64) {
  const int i = v64 ? 1 : 0;
  if (c->rp64_occ_known[i]) return DSGD_OK;
  int n = 0;
  const hipError_t e = v64 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dsgd_rp64v_step_kernel, RP64_THREADS, 0)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dsgd_rp64_step_kernel, RP64_THREADS, 0);
  if (e != hipSuccess) return fail(DSGD_EHIP, "hipOccupancyMaxActiveBlocksPerMultiprocessor: %s", hipGetErrorString(e));
  c->rp64_occ[i] = std::max(0, n);
  c->rp64_occ_known[i] = true;
  return DSGD_OK;
}
// The caller's flat lists of n_steps x K workers (csrc/dsgd_plan_check.hpp: flat_lists_check), by rp64_check_lists' rules over
// every step in one pass: host data, checked before anything moves.  rows_known: false where no data is loaded yet.
static int rp64_check_flat(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int K, bool rows_known) {
  const FlatListsCheck v = flat_lists_check(idx, n_idx, offsets, n_steps, K, rows_known ? c->n_rows : -1);
  const long long step = v.list / K, worker = v.list % K;
  switch (v.kind) {
    case FLAT_LISTS_OK: return DSGD_OK;
    case FLAT_LISTS_FIRST_OFFSET: return fail(DSGD_EINVAL, "offsets[0] must be 0");
    case FLAT_LISTS_END: return fail(DSGD_EINVAL, "offsets end at %lld but idx holds %lld entries", v.value, (long long)n_idx);
    case FLAT_LISTS_OFFSETS:
      return fail(DSGD_EINVAL, "offsets decrease or leave idx at list %lld (step %lld, worker %lld)", v.list, step, worker);
    case FLAT_LISTS_EMPTY: return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors (step %lld, worker %lld)", step, worker);   // ref: math/Vec.scala:129
    case FLAT_LISTS_INDEX: break;
  }
  return fail(DSGD_ERANGE, "sample index %d at position %lld outside the %lld loaded rows", (int)v.value, v.pos, c->n_rows);
}
static int rp64_steps_ensure(dsgd_ctx* c, long long n_lists, long long n_steps) {
  if (c->d_rp64_ssegs.cap() < (size_t)n_lists || c->d_rp64_cum.cap() < (size_t)n_steps) HIP_TRY(hipStreamSynchronize(c->stream));
  DSGD_TRY(c->d_rp64_ssegs.reserve((size_t)n_lists));
  DSGD_TRY(c->d_rp64_cum.reserve((size_t)n_steps));
  if (!c->d_rp64_sync) {
    DSGD_TRY(c->h_rp64_sync.alloc(2));
    DSGD_TRY(c->d_rp64_sync.alloc(2));
    HIP_TRY(hipMemsetAsync(c->d_rp64_sync, 0, sizeof(unsigned long long) * 2, c->stream));
    c->rp64_target = 0;
  }
  return DSGD_OK;
}

int dsgd_sync_steps_f64(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers, double lr,
                        int64_t* active_per_step_out, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || n_steps < 1 || n_workers < 1 || n_idx < 0) return fail(DSGD_EINVAL, "bad arguments (null lists, no steps or no workers)");
  if (n_steps > INT64_MAX / n_workers) return fail(DSGD_EINVAL, "n_steps * n_workers overflows");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_sync_steps_f64"));
  if (c->comm)
    return fail(DSGD_EUNSUPPORTED, "dsgd_sync_steps_f64 is not available with a communicator attached: the gather needs a host read per "
                                   "step (dsgd_sync_step_f64 is the step that spans the ranks)");
  DSGD_TRY(bind(c, true));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  // the lists are host data: every step checked here, in one pass, by rp64_check_lists' rules, before anything moves
  const int K = n_workers;
  const int64_t n_lists = n_steps * K;
  DSGD_TRY(rp64_check_flat(c, idx, n_idx, offsets, n_steps, K, true));
  DSGD_TRY(prepare_layout(c));
  const bool v64 = c->d_val64 != nullptr;
  if (c->k.rp64_fused) DSGD_TRY(rp64_fused_cap(c, v64));
  DSGD_TRY(rp64_ensure(c, K));
  DSGD_TRY(rp64_steps_ensure(c, n_lists, n_steps));
  DSGD_TRY(reset_counters(c));
  // ONE upload: the index array and the list ranges of every step
  DSGD_TRY(ensure_idx(c, n_idx));
  DSGD_TRY(send_idx(c, idx, n_idx));
  c->cur_idx = c->d_idx;
  DSGD_TRY(pin_acquire(c->pin_segs, sizeof(WorkSeg) * (size_t)n_lists));
  {
    WorkSeg* sg = static_cast<WorkSeg*>(c->pin_segs.p.get());
    for (int64_t i = 0; i < n_lists; ++i) {
      sg[i].begin = offsets[i];
      sg[i].end = offsets[i + 1];
    }
  }
  HIP_TRY(hipMemcpyAsync(c->d_rp64_ssegs, c->pin_segs.p, sizeof(WorkSeg) * (size_t)n_lists, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_segs));
  const long long fused_max = c->k.rp64_fused ? (long long)c->rp64_occ[v64 ? 1 : 0] * c->n_cu : 0;
  // every step's word of `cum` starts as all ones: a step that ran as a whole overwrites its word with the call's running
  // n_active (the fused kernel itself; for the two launches a copy on the stream, which is needed only where the counts are
  // asked for or fused launches share the call)
  constexpr unsigned long long NOT_RUN = ~0ull;
  HIP_TRY(hipMemsetAsync(c->d_rp64_cum, 0xff, sizeof(unsigned long long) * (size_t)n_steps, c->stream));
  // a fused launch that gave up (bit 62 of the arrival counter): read behind a synchronisation
  auto gave_up = [&](bool* yes) -> int {
    HIP_TRY(hipMemcpyAsync(c->h_rp64_sync, c->d_rp64_sync, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *yes = (c->h_rp64_sync[0] & RP64_GAVE_UP) != 0;
    return DSGD_OK;
  };
  long long n_fused = 0, n_pairs = 0;
  bool fused_unchecked = false, aborted = false;
  c->ctr_known = false;   // (n_active runs on through the call)
  for (int64_t t = 0; t < n_steps && !aborted; ++t) {
    Rp64Step s = rp64_step(c, K, rp64_longest(offsets, t, K), RP64_STEP, RP64_LOCAL, lr, nullptr, c->d_idx, c->d_rp64_ssegs + t * K);
    const long long grid = rp64_grid(s);
    if (grid <= fused_max) {   // resident as a whole: ONE launch
      Rp64StepSync y;
      y.arrived = c->d_rp64_sync;
      c->rp64_target += (unsigned long long)grid;
      y.target = c->rp64_target;
      y.wait_ticks = c->rp64_wait_ticks;
      y.cum = c->d_rp64_cum + t;
      DSGD_TRY(rp64_launched(rp64_enqueue_grad(c, s, nullptr, &y)));
      ++n_fused;
      fused_unchecked = true;
    } else {                   // the two launches of dsgd_sync_step_f64, back to back
      // The existing kernels know nothing of a fused launch that gave up in front of them, so a call that mixes the forms (a
      // grid beyond the fused cap: more than 2,000 workers) synchronises ONCE at each change from fused launches to the pair
      // and stops there if one gave up: no step runs behind an aborted one.
      if (fused_unchecked) {
        DSGD_TRY(gave_up(&aborted));
        fused_unchecked = false;
        if (aborted) break;
      }
      DSGD_TRY(rp64_launched(rp64_enqueue_grad(c, s)));
      DSGD_TRY(rp64_launched(rp64_enqueue_finish(c, s)));
      if (active_per_step_out || c->k.rp64_fused)
        HIP_TRY(hipMemcpyAsync(c->d_rp64_cum + t, &c->d_sc->n_active, sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
      ++n_pairs;
    }
  }
  // (dsgd_grad_kernel_name: which form served the call's steps)
  c->last_grad_kernel = n_fused && n_pairs ? (v64 ? "dsgd_rp64v_step_kernel+dsgd_rp64v_grad_kernel" : "dsgd_rp64_step_kernel+dsgd_rp64_grad_kernel")
                        : n_fused ? (v64 ? "dsgd_rp64v_step_kernel" : "dsgd_rp64_step_kernel")
                                  : (v64 ? "dsgd_rp64v_grad_kernel" : "dsgd_rp64_grad_kernel");
  c->s_dirty = true;
  const bool want_cum = active_per_step_out != nullptr || n_fused > 0;
  if (want_cum) {
    DSGD_TRY(pin_acquire(c->pin_out, sizeof(unsigned long long) * (size_t)n_steps));
    HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_rp64_cum, sizeof(unsigned long long) * (size_t)n_steps, hipMemcpyDeviceToHost, c->stream));
  }
  c->h_rp64_sync[0] = 0;
  if (n_fused) HIP_TRY(hipMemcpyAsync(c->h_rp64_sync, c->d_rp64_sync, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(finish_stats(c, nullptr, n_idx));   // the ONE synchronisation of the call
  const unsigned long long* cum = want_cum ? static_cast<const unsigned long long*>(c->pin_out.p.get()) : nullptr;
  if (aborted || (c->h_rp64_sync[0] & RP64_GAVE_UP) != 0) {
    // A fused launch gave up waiting for its own grid.  The bit is set only while that launch's arrivals are incomplete and
    // every workgroup that waits sees it, so NO workgroup of that launch ran phase 2 and every later launch returned on entry:
    // the weights are those behind the last step whose word of `cum` is written.  The sums the aborted step left are zeroed
    // and the counter starts again.
    long long done = 0;
    while (done < n_steps && cum[done] != NOT_RUN) ++done;
    const unsigned long long seen = c->h_rp64_sync[0] & ~RP64_GAVE_UP, target = c->rp64_target;
    HIP_TRY(hipMemsetAsync(c->d_rp64_sync, 0, sizeof(unsigned long long) * 2, c->stream));
    c->rp64_target = 0;
    HIP_TRY(hipMemsetAsync(c->d_rp64_acc, 0, sizeof(unsigned long long) * (size_t)c->rp64_stride * (size_t)c->rp64_k, c->stream));
    if (c->d_rp64v_lo)
      HIP_TRY(hipMemsetAsync(c->d_rp64v_lo, 0, sizeof(unsigned long long) * (size_t)c->rp64v_stride * (size_t)c->rp64v_k, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return fail(DSGD_ESTATE, "step %lld of %lld: the fused step's workgroups gave up waiting for each other (%llu arrivals seen, the call's last "
                             "target %llu); the last completed step is %lld and the weights are those behind it%s (DSGD_RP64_FUSED=0 "
                             "selects the two-launch queue)",
                done, (long long)n_steps, seen, target, done - 1, done ? "" : " (-1: no step ran, the weights are unchanged)");
  }
  if (active_per_step_out)
    for (int64_t t = 0; t < n_steps; ++t) active_per_step_out[t] = (int64_t)(cum[t] - (t ? cum[t - 1] : 0ull));
  if (stats) {
    stats->n_samples = n_idx;
    stats->n_active = (int64_t)c->h_sc->n_active;
  }
  return DSGD_OK;
}

// ======== 6. Resident row-parallel plans ========
// The caller's lists as a row-parallel plan: dsgd_sync_steps_f64's checks, then the lists and their ranges resident.
int dsgd_plan_create_rp64_n(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                            dsgd_plan** out) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || !out || n_steps < 1 || n_workers < 1 || n_idx < 0) return fail(DSGD_EINVAL, "bad plan arguments (null pointers, no steps or no workers)");
  if (n_steps > INT64_MAX / n_workers) return fail(DSGD_EINVAL, "n_steps * n_workers overflows");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_plan_create_rp64_n"));   // (with a communicator attached too: local, the rank's own rows)
  DSGD_TRY(bind(c, true));   // (nothing here touches w: slice-major weights stay as they are)
  DSGD_TRY(rp64_check_flat(c, idx, n_idx, offsets, n_steps, n_workers, c->d_row_ptr != nullptr));   // (without data the lists are judged at the first run: plan_revalidate)
  dsgd_plan* p = nullptr;
  DSGD_TRY(plan_frame(c, offsets, n_steps, n_workers, &p, true));
  p->h_idx.assign(idx, idx + n_idx);
  hipError_t e = hipMemcpyAsync(p->d_idx, idx, sizeof(int) * (size_t)n_idx, hipMemcpyHostToDevice, c->build_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->build_stream);
  if (e != hipSuccess) {
    plan_abandon(c, p);
    return fail(DSGD_EHIP, "plan upload: %s", hipGetErrorString(e));
  }
  return plan_finish(c, p, out);
}
// The steps [step_begin, step_end) of a row-parallel plan (locked, bound with the weights in their layout, revalidated, layout
// ready): per step rp64_step over the plan's resident ranges and the pair of dsgd_sync_step_f64 -- or, async, one worker's
// iteration as dsgd_async_step_f64 takes it on Double data -- enqueued on the launch stream; no upload, no synchronisation.
// The fused one-launch step is not used: its give-up protocol needs a host read inside the call.
static int plan_run_rp64(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, double lr, bool async) {
  const int K = p->n_workers;
  if (p->built_pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  if (step_end <= step_begin) return DSGD_OK;
  const bool v64 = c->d_val64 != nullptr;
  const bool rec = p->d_gate_rec != nullptr;
  DSGD_TRY(rp64_ensure(c, K));
  c->ctr_known = false;   // (n_active runs on until dsgd_synchronize)
  for (long long t = step_begin; t < step_end; ++t) {
    Rp64Step s = rp64_step(c, K, rp64_longest(p->offsets.data(), t, K), async ? RP64_ASYNC : RP64_STEP, RP64_LOCAL, lr, nullptr, p->d_idx,
                           p->d_segs + t * K);
    Rp64Rec r;
    if (rec) {   // (the asynchronous iteration's s comes from the sliced kernel: the record's from the gradient's last workgroup)
      r.mask = p->d_gate_rec + (size_t)t * p->gate_words;
      r.s_used = p->d_s_rec + t;
      r.step_base = p->offsets[(size_t)(t * K)];
      HIP_TRY(hipMemsetAsync(r.mask, 0, sizeof(unsigned int) * (size_t)p->gate_words, c->stream));
    }
    DSGD_TRY(rp64_launched(rp64_enqueue_grad(c, s, rec ? &r : nullptr)));
    DSGD_TRY(rp64_launched(rp64_enqueue_finish(c, s)));
  }
  c->last_grad_kernel = rec ? (v64 ? "dsgd_rp64v_grad_rec_kernel" : "dsgd_rp64_grad_rec_kernel") : (v64 ? "dsgd_rp64v_grad_kernel" : "dsgd_rp64_grad_kernel");
  c->s_dirty = true;
  c->pending_samples += p->offsets[(size_t)(step_end * K)] - p->offsets[(size_t)(step_begin * K)];
  return DSGD_OK;
}

// ======== 7. Resident row-parallel plans across ranks ========
// ... under a communicator (dsgd_comm_init_f64 / dsgd_comm_init_f64v; include/dsgd.h "ACROSS RANKS", csrc/dsgd_rp64_gather.hpp): a
// COLLECTIVE call.  The ranks agree ONCE -- the [world] words in front of the gather buffer's slots, each rank's rp64_call_word
// (its plan's hosted workers, its value type, the steps of the call) in its own position, all-reduced and read back: the
// call's one host read -- and then every step is enqueued with no synchronisation in between: the gather form of the gradient
// kernel without a rank word, the slots' messages as rp64_gather cuts them, dsgd_rp64_header_plan_kernel, and the finish of a
// single context over the k * world slots.  Ranks that disagree all return DSGD_EINVAL in front of the first slot message:
// nothing but the words has travelled, and they are zero again.  The job's samples and active rows run on in the
// context's scalars until dsgd_synchronize.  A collective error half way: the gather buffer is dropped, DSGD_ERCCL, the
// weights are those behind the last completed step.
static int plan_run_rp64_ranks(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, double lr) {
  const int k = p->n_workers, W = c->world;
  const long long steps = step_end - step_begin;
  if (p->d_gate_rec)
    return fail(DSGD_EUNSUPPORTED, "dsgd_plan_run_f64: a plan that keeps a record (dsgd_plan_record) does not run with a communicator "
                                   "attached; switch the record off or detach (nothing ran)");
  if (k > 0x7fffffff / W) return fail(DSGD_EINVAL, "n_workers * world overflows");
  if (steps > RP64_CALL_MAX_STEPS)
    return fail(DSGD_EINVAL, "a plan run under a communicator takes at most %lld steps per call (%lld asked): cut the range", RP64_CALL_MAX_STEPS,
                steps);
  if (p->built_pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  const bool v64 = c->d_val64 != nullptr;
  const int K = k * W, words = v64 ? 2 : 1;
  DSGD_TRY(rp64_ensure(c, 1));   // (s; the local accumulators are not used)
  DSGD_TRY(rp64_gather_ensure(c, K, words));
  // ---- the agreement: own word up, the words all-reduced, read back, zeroed again ----
  const unsigned long long mine = rp64_call_word(k, v64, steps);
  c->h_rp64_ranks[c->rank] = mine;
  // (any failure from here to the read: the words may be left non-zero, so the buffer goes and the next call starts from a zeroed one)
  hipError_t he = hipMemcpyAsync(c->d_rp64_gath + c->rank, &c->h_rp64_ranks[c->rank], sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream);
  if (he == hipSuccess) {
    int r = rccl::AllReduce(c->d_rp64_gath, c->d_rp64_gath, (size_t)W, rccl::kInt64, rccl::kSum, c->comm, c->stream);
    if (r) {
      rp64_gather_drop(c);
      return fail(DSGD_ERCCL, "ncclAllReduce(the plan run's agreement): %s", rccl::GetErrorString(r));
    }
    he = hipMemcpyAsync(c->h_rp64_ranks, c->d_rp64_gath, sizeof(unsigned long long) * (size_t)W, hipMemcpyDeviceToHost, c->stream);
  }
  if (he == hipSuccess) he = hipMemsetAsync(c->d_rp64_gath, 0, sizeof(unsigned long long) * (size_t)W, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he != hipSuccess) {
    rp64_gather_drop(c);
    return fail(DSGD_EHIP, "the plan run's agreement: %s (nothing ran, the weights are unchanged)", hipGetErrorString(he));
  }
  for (int q = 0; q < W; ++q) {
    const unsigned long long theirs = c->h_rp64_ranks[q];
    if (theirs == mine) continue;
    if (rp64_call_word_v64(theirs) != v64)
      return fail(DSGD_EINVAL, "rank %d holds %s feature values, this rank (%d) %s ones: every rank of a plan run holds the same value type "
                               "(dsgd_load_csr / dsgd_load_csr_f64; nothing ran, the weights are unchanged)", q,
                  rp64_call_word_v64(theirs) ? "Double" : "float", c->rank, v64 ? "Double" : "float");
    if (rp64_call_word_k(theirs) != k)
      return fail(DSGD_EINVAL, "rank %d runs a plan of %d hosted workers, this rank (%d) one of %d: every rank of a plan run hosts the same "
                               "number (nothing ran, the weights are unchanged)", q, rp64_call_word_k(theirs), c->rank, k);
    return fail(DSGD_EINVAL, "rank %d runs %lld steps, this rank (%d) %lld: every rank of a plan run runs the same number (nothing ran, the "
                             "weights are unchanged)", q, rp64_call_word_steps(theirs), c->rank, steps);
  }
  if (steps == 0) return DSGD_OK;
  // ---- the steps, back to back ----
  if (!c->job_pending) {   // (the job's rows run on from zero: a step under the communicator leaves its own count behind)
    HIP_TRY(hipMemsetAsync(&c->d_sc->n_samples, 0, sizeof(unsigned long long), c->stream));
    c->job_pending = true;
  }
  unsigned long long* slots = c->d_rp64_gath + rp64_gather_pad(W);
  const long long slot = c->rp64_gstride * words;
  c->ctr_known = false;   // (n_active runs on until dsgd_synchronize)
  c->s_dirty = true;
  c->last_grad_kernel = v64 ? "dsgd_rp64v_grad_gather_plan_kernel" : "dsgd_rp64_grad_gather_plan_kernel";
  for (long long t = step_begin; t < step_end; ++t) {
    Rp64Step s = rp64_step(c, k, rp64_longest(p->offsets.data(), t, k), RP64_STEP, RP64_GATHER_PLAN, lr, nullptr, p->d_idx, p->d_segs + t * k);
    hipError_t e = rp64_enqueue_grad(c, s);
    int rc = e == hipSuccess ? rp64_gather_slots(c, K) : fail(DSGD_EHIP, "step %lld's gradient launch: %s", t, hipGetErrorString(e));
    if (rc == DSGD_OK) {
      hipLaunchKernelGGL(dsgd_rp64_header_plan_kernel, dim3(1), dim3(RP64_THREADS), 0, c->stream, slots, slot, K, c->dp, c->d_rp64_gsegs, c->d_sc);
      e = rp64_enqueue_finish(c, s);
      if (e != hipSuccess) rc = fail(DSGD_EHIP, "step %lld's finish launch: %s", t, hipGetErrorString(e));
    }
    if (rc != DSGD_OK) {   // (half way: the next call starts from a zeroed buffer; the weights are those behind step t - 1)
      char msg[sizeof(g_err)];
      snprintf(msg, sizeof(msg), "%s", g_err);
      rp64_gather_drop(c);
      return fail(rc, "%s (the weights are those behind step %lld)", msg, t - 1);
    }
  }
  return DSGD_OK;
}

// ======== 8. Running a plan in an fp64 context, and the requests that are one-step column-slice plans ========
// the steps of a plan in an fp64 context (locked; bound with the slice-major weights kept); async: see launch_cs64
static int plan_run64(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, double lr, bool async = false,
                      double* delta = nullptr) {
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(plan_revalidate(c, p));   // (a plan from before the last load: DSGD_ERANGE here, before anything is enqueued)
  DSGD_TRY(prepare_layout(c));
  if (p->rp64 && c->comm) {   // (the asynchronous entry point refused the communicator before it came here)
    if (async) return fail(DSGD_ESTATE, "internal: an asynchronous plan run under a communicator");
    return plan_run_rp64_ranks(c, p, step_begin, step_end, lr);
  }
  if (p->rp64) return plan_run_rp64(c, p, step_begin, step_end, lr, async);
  if (p->cs_layout != c->layout_gen) {
    DSGD_TRY(cs_build(c, p));
    if (p->cs_device_built && c->build_stream) {
      HIP_TRY(hipEventRecord(p->built_ev, c->build_stream));
      p->built_pending = true;
    }
  }
  if (p->built_pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  // (route_plan also asks for no communicator, which the line this replaced did not: every caller has refused one by here --
  //  refuse_fp64_comm in the plan entry points, REQ_F64_RANKS ahead of sync_step64 -- so the condition is the old one)
  if (plan_route(c, p) != PLAN_CS64) return cs64_refused(c);
  if (step_end > step_begin) DSGD_TRY(launch_cs64(c, p, step_begin, step_end, lr, async, delta));
  c->pending_samples += p->offsets[step_end * p->n_workers] - p->offsets[step_begin * p->n_workers];
  return DSGD_OK;
}

int dsgd_plan_run_f64(dsgd_ctx* c, dsgd_plan* p, int64_t step_begin, int64_t step_end, double lr) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(plan_steps_check(p, step_begin, step_end));
  if (p->lg) return fail(DSGD_EUNSUPPORTED, "dsgd_plan_run_f64: a logistic plan runs through dsgd_plan_run, on an fp32 context");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_plan_run_f64"));
  if (!p->rp64) DSGD_TRY(refuse_fp64_comm(c, "dsgd_plan_run_f64"));   // (a row-parallel plan spans the ranks: plan_run_rp64_ranks)
  DSGD_TRY(bind(c, true));
  return plan_run64(c, p, step_begin, step_end, lr);
}

// ---- the fp64 asynchronous iteration (include/dsgd.h "THE FP64 MODE"; core/Slave.scala:79-111, 177-185) ----
int dsgd_plan_run_async_f64(dsgd_ctx* c, dsgd_plan* p, int64_t step_begin, int64_t step_end, double lr) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(plan_steps_check(p, step_begin, step_end));
  if (p->lg) return fail(DSGD_EUNSUPPORTED, "dsgd_plan_run_async_f64: a logistic plan's asynchronous iterations run through dsgd_plan_run_async_lg, on an fp32 context");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, "dsgd_plan_run_async_f64"));
  DSGD_TRY(refuse_fp64_comm(c, "dsgd_plan_run_async_f64"));
  if (p->n_workers != 1)
    return fail(DSGD_EINVAL, "an asynchronous iteration is one worker's: this plan has %d workers per step", p->n_workers);
  DSGD_TRY(bind(c, true));
  return plan_run64(c, p, step_begin, step_end, lr, true, nullptr);
}

// a per-request step in an fp64 context (locked, bound, layout ready): a one-step plan, created, run and given back here
static int sync_step64(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int n_workers, double lr,
                       dsgd_batch_stats* stats) {
  std::vector<int64_t> offsets((size_t)n_workers + 1, 0);
  for (int k = 0; k < n_workers; ++k) {
    if (n_per_worker[k] <= 0)
      return fail(DSGD_EINVAL, "worker %d has an empty sample list: Vec.sum requires a non-empty list", k);
    if (!idx_per_worker[k]) return fail(DSGD_EINVAL, "null index list for worker %d", k);
    for (int64_t t = 0; t < n_per_worker[k]; ++t)
      if (idx_per_worker[k][t] < 0 || idx_per_worker[k][t] >= c->n_rows)
        return fail(DSGD_ERANGE, "sample index %d of worker %d outside the %lld loaded rows", idx_per_worker[k][t], k, c->n_rows);
    offsets[(size_t)k + 1] = offsets[(size_t)k] + n_per_worker[k];
  }
  dsgd_plan* p = nullptr;
  DSGD_TRY(plan_frame(c, offsets.data(), 1, n_workers, &p));
  p->h_idx.resize((size_t)offsets[(size_t)n_workers]);
  for (int k = 0; k < n_workers; ++k)
    std::copy(idx_per_worker[k], idx_per_worker[k] + n_per_worker[k], p->h_idx.begin() + offsets[(size_t)k]);
  hipError_t e = hipMemcpyAsync(p->d_idx, p->h_idx.data(), sizeof(int) * p->h_idx.size(), hipMemcpyHostToDevice, c->build_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->build_stream);
  if (e != hipSuccess) {
    plan_abandon(c, p);
    return fail(DSGD_EHIP, "sync step upload: %s", hipGetErrorString(e));
  }
  DSGD_TRY(plan_finish(c, p, &p));
  int rc = reset_counters(c);
  if (rc == DSGD_OK) {
    rc = plan_run64(c, p, 0, 1, lr);
    if (rc == DSGD_OK) c->pending_samples -= offsets[(size_t)n_workers];   // (a request reports its own samples, below)
  }
  if (p->built_pending) (void)hipStreamWaitEvent(c->stream, p->built_ev, 0);
  plan_release(c, p);   // (the blocks go back behind the step: an event on the launch stream)
  DSGD_TRY(rc);
  return finish_stats(c, stats, offsets[(size_t)n_workers]);
}

// dsgd_async_step_f64 (sparse_cap < 0: the delta dense into delta_out, which may be NULL) and dsgd_async_step_sparse_f64
// (sparse_cap >= 0: the delta compacted into the mapped buffer, for sp_deliver behind the call's synchronisation)
static int async_step64(dsgd_ctx* c, const char* what, const int32_t* idx, int64_t n, double lr, double* delta_out, int64_t sparse_cap,
                        int32_t* sp_key, double* sp_val, int64_t* sp_nnz, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n <= 0 || !idx) return fail(DSGD_EINVAL, "Cannot sum an empty list of vectors");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(require_fp64(c, what));
  DSGD_TRY(refuse_fp64_comm(c, what));
  DSGD_TRY(bind(c, true));
  DSGD_TRY(require_data(c));
  DSGD_TRY(require_ds(c));
  DSGD_TRY(require_sync_mode(c));
  DSGD_TRY(prepare_layout(c));
  const bool sparse = sparse_cap >= 0;
  const bool want_delta = delta_out || sparse;
  for (int64_t t = 0; t < n; ++t)
    if (idx[t] < 0 || idx[t] >= c->n_rows) return fail(DSGD_ERANGE, "sample index %d outside the %lld loaded rows", idx[t], c->n_rows);
  // a one-step, one-worker plan: created, run and given back here (as sync_step64)
  const int64_t offsets[2] = {0, n};
  dsgd_plan* p = nullptr;
  if (sparse) {
    DSGD_TRY(sp_async_cap(c, idx, n, sparse_cap));   // (before anything runs: a delta is never lost)
    DSGD_TRY(sp_ensure(c));
  }
  if (c->d_val64) {   // Double data: the row-parallel pair with the asynchronous finish; the delta in key order as it is written
    DSGD_TRY(cs64_step_limits(c, 1, n));   // (the one-step plan's refusals, as on float data)
    if (want_delta) DSGD_TRY(c->d_cs_dl64.reserve((size_t)CS64_G * cs64_sp(c->dp) + (size_t)c->dp));
    DSGD_TRY(rp64_ensure(c, 1));
    DSGD_TRY(reset_counters(c));
    long long mx = 0, tot = 0;
    const int64_t nn = n;
    DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
    DSGD_TRY(rp64_launch(c, 1, mx, RP64_ASYNC, lr, want_delta ? c->d_cs_dl64 : nullptr));
    c->s_dirty = true;
    if (sparse) DSGD_TRY((sp_compact<double, double, false>(c, c->d_cs_dl64, nullptr)));
    DSGD_TRY(finish_stats(c, stats, n));
    if (delta_out) {   // (key order already: through the pinned buffer, as the gradient goes out)
      const size_t bytes = sizeof(double) * (size_t)c->dp;
      DSGD_TRY(pin_acquire(c->pin_out, bytes));
      HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_cs_dl64, bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      memcpy(delta_out, c->pin_out.p, bytes);
    }
    if (sparse) return sp_deliver<double>(c, sp_key, sp_val, sparse_cap, sp_nnz);
    return DSGD_OK;
  }
  DSGD_TRY(plan_frame(c, offsets, 1, 1, &p));
  p->h_idx.assign(idx, idx + n);
  hipError_t e = hipMemcpyAsync(p->d_idx, p->h_idx.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->build_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->build_stream);
  if (e != hipSuccess) {
    plan_abandon(c, p);
    return fail(DSGD_EHIP, "async step upload: %s", hipGetErrorString(e));
  }
  DSGD_TRY(plan_finish(c, p, &p));
  const int Sp = cs64_sp(c->dp);
  int rc = DSGD_OK;
  if (want_delta && c->d_cs_dl64.reserve((size_t)CS64_G * Sp + (size_t)c->dp) != DSGD_OK)
    rc = fail(DSGD_ENOMEM, "out of device memory (the delta of an async step)");
  if (rc == DSGD_OK && want_delta && hipMemsetAsync(c->d_cs_dl64, 0, sizeof(double) * (size_t)CS64_G * Sp, c->stream) != hipSuccess)
    rc = fail(DSGD_EHIP, "hipMemsetAsync");
  if (rc == DSGD_OK) rc = reset_counters(c);
  if (rc == DSGD_OK) {
    rc = plan_run64(c, p, 0, 1, lr, true, want_delta ? c->d_cs_dl64 : nullptr);
    if (rc == DSGD_OK) c->pending_samples -= n;   // (a request reports its own samples, below)
  }
  if (p->built_pending) (void)hipStreamWaitEvent(c->stream, p->built_ev, 0);
  plan_release(c, p);   // (the blocks go back behind the step: an event on the launch stream)
  DSGD_TRY(rc);
  double* rank = want_delta ? c->d_cs_dl64 + (size_t)CS64_G * Sp : nullptr;
  if (sparse) {   // slice-major -> rank order -> the pairs, all in front of the call's synchronisation
    hipLaunchKernelGGL(dsgd_cs64_unslice_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, c->d_cs_dl64, rank, c->dp, Sp);
    HIP_TRY(hipGetLastError());
    DSGD_TRY((sp_compact<double, double, false>(c, rank, c->d_perm)));
  }
  DSGD_TRY(finish_stats(c, stats, n));
  if (delta_out) {   // slice-major -> rank order -> key order
    hipLaunchKernelGGL(dsgd_cs64_unslice_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, c->d_cs_dl64, rank, c->dp, Sp);
    HIP_TRY(hipGetLastError());
    DSGD_TRY(take64(c, rank, delta_out));
  }
  if (sparse) return sp_deliver<double>(c, sp_key, sp_val, sparse_cap, sp_nnz);
  return DSGD_OK;
}

int dsgd_async_step_f64(dsgd_ctx* c, const int32_t* idx, int64_t n, double lr, double* delta_out, dsgd_batch_stats* stats) {
  return async_step64(c, "dsgd_async_step_f64", idx, n, lr, delta_out, -1, nullptr, nullptr, nullptr, stats);
}

int dsgd_async_step_sparse_f64(dsgd_ctx* c, const int32_t* idx, int64_t n, double lr, int32_t* d_key, double* d_val, int64_t cap,
                               int64_t* d_nnz, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(sp_check_out(d_key, d_val, cap, d_nnz));
  return async_step64(c, "dsgd_async_step_sparse_f64", idx, n, lr, nullptr, cap, d_key, d_val, d_nnz, stats);
}
