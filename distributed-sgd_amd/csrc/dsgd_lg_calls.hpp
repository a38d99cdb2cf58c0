// Host side of the logistic model (include/dsgd.h "THE LOGISTIC MODEL"; device code: csrc/dsgd_logistic.hpp and, for the
// distributed and sampled evaluation at the end of this file, csrc/dsgd_lg_eval.hpp; the shift, the grids, the tables and the
// validation of lists, ranges and offsets: csrc/dsgd_lg_host.hpp).  Included by dsgd_hip.hip inside its
// extern "C" block, behind the helpers it uses (bind, stage_lists, upload_segs, set_weights_locked, finish_stats).
//
// Every check runs on the host before anything of the call is enqueued: a refused call leaves the weights, the accumulators
// and the context's flags as they were.  Every call returns behind its kernels (ONE synchronisation).

// (LgScope: csrc/dsgd_hip.hip, in front of the plans' entry points)
static int lg_refuse(dsgd_ctx* c, const char* what, LgScope scope) {
  if (c->fp64)
    return fail(DSGD_EUNSUPPORTED, "%s is not available in an fp64 context: the logistic model runs on the fp32 engine's weights and dot", what);
  if (c->comm && !c->comm_lg)
    return fail(DSGD_EUNSUPPORTED, "%s is not available with a communicator attached: the logistic model's steps do not span ranks "
                                   "(dsgd_comm_init_lg attaches one they span)", what);
  if (c->comm && scope == LG_ONE_PROCESS)
    return fail(DSGD_EUNSUPPORTED, "%s is not available with a communicator attached: device-drawn lists and column slices do not span ranks", what);
  return DSGD_OK;
}
// what every call asks first (locked): the mode, the device, the data, the engine
// (keep_sliced: a plan on column slices keeps the weights slice-major between its runs, as the SVM's -- bind)
static int lg_enter(dsgd_ctx* c, const char* what, LgScope scope, bool* nsq_fresh, bool keep_sliced = false) {
  DSGD_TRY(lg_refuse(c, what, scope));
  DSGD_TRY(bind(c, keep_sliced));
  *nsq_fresh = c->lg_nsq_stamp + 1 == c->bind_count;   // (no other entry point has bound since the logistic call that left |w|^2)
  DSGD_TRY(require_data(c));
  if (c->async_running)
    return fail(DSGD_ESTATE, "%s: the lock-free engine is running (dsgd_async_stop / dsgd_async_wait first)", what);
  return DSGD_OK;
}
static int lg_report(dsgd_ctx* c, const char* what, const LgCheck& v, int n_workers) {
  switch (v.kind) {
    case LG_OK: return DSGD_OK;
    case LG_NO_WORKERS: return fail(DSGD_EINVAL, "%s: bad arguments (a null table, no workers or no steps)", what);
    case LG_EMPTY: return fail(DSGD_EINVAL, "%s: Cannot sum an empty list of vectors (worker %lld has no rows)", what, v.worker % std::max(1, n_workers));
    case LG_TOO_LONG: return fail(DSGD_EINVAL, "%s: worker %lld lists %lld rows, more than 2^40", what, v.worker % std::max(1, n_workers), v.value);
    case LG_FIRST_OFFSET: return fail(DSGD_EINVAL, "%s: offsets[0] must be 0", what);
    case LG_END: return fail(DSGD_EINVAL, "%s: offsets end at %lld, not at n_idx", what, v.value);
    case LG_OFFSETS: return fail(DSGD_EINVAL, "%s: offsets decrease or leave idx at list %lld", what, v.worker);
    case LG_INDEX: break;
  }
  return fail(DSGD_ERANGE, "%s: row %lld (worker %lld, position %lld) is outside the %lld loaded rows", what, v.value, v.worker, v.pos, c->n_rows);
}

static void lg_drop(dsgd_ctx* c) {   // (after a failure half way: the next call starts from a zeroed buffer)
  (void)hipStreamSynchronize(c->stream);
  c->d_lg_acc.reset();
  c->lg_k = 0;
}
// room for n_workers hosted workers: under dsgd_comm_init_lg's communicator the slots of every rank's (csrc/dsgd_lg_gather.hpp)
static int lg_ensure(dsgd_ctx* c, int n_workers) {
  DSGD_TRY(c->d_lg_g.reserve((size_t)c->dp));
  // (the |w|^2 words, then one word per evaluation workgroup: up to LG_MAX_RANGES ranges of n_cu workgroups each)
  DSGD_TRY(c->d_lg_part.reserve((size_t)lg_finish_blocks(c->dp) + (size_t)c->n_cu * LG_MAX_RANGES));
  DSGD_TRY(c->d_lg_tally.reserve((size_t)LG_MAX_RANGES * LG_TALLY_WORDS));
  const int world = c->comm && c->comm_lg ? c->world : 1;
  if (n_workers > 0x7fffffff / LGG_MAX_WORLD) return fail(DSGD_EINVAL, "%d workers: too many", n_workers);
  const int need = n_workers * world;
  if (c->lg_k < need || c->lg_world != world || !c->d_lg_acc) {   // (zeroed once; every finish leaves the slots zeroed)
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->lg_k = 0;
    const int cap = std::max(need, 4);
    const size_t words = (size_t)lgg_total_words(world, cap, c->dp);
    DSGD_TRY(c->d_lg_acc.alloc(words));
    HIP_TRY(hipMemsetAsync(c->d_lg_acc, 0, sizeof(unsigned long long) * words, c->stream));
    c->lg_stride = lgg_stride(c->dp);
    c->lg_k = cap;
    c->lg_world = world;
  }
  return DSGD_OK;
}

// Whose slots a call's launches sum into and what its finish folds: the context's own k workers on its own vexp (lg_local), or
// across ranks this rank's block of the K = k * world slots, the call's agreed vexp and the gathered finish (lg_agree).
struct LgCall {
  bool ranks = false;
  int k = 0, K = 0, vexp = 0;
  unsigned long long* own = nullptr;   // the first slot of this rank's workers
  unsigned long long* all = nullptr;   // slot 0
  unsigned long long* hdr = nullptr;   // ranks: the K header words of a step
};
static LgCall lg_local(dsgd_ctx* c, int k) {   // (lg_ensure came first)
  LgCall q;
  q.k = q.K = k;
  q.vexp = c->vexp;
  q.own = q.all = c->d_lg_acc + lgg_slots_at(c->lg_world, c->lg_k);
  return q;
}
// The agreement of a collective call (lg_ensure(c, k) came first; every local check has passed; nothing of the call is enqueued):
// this rank's k, steps and vexp into its words of the zeroed record, the record all-reduced, read back and zeroed again -- the
// call's one extra host read.  Ranks that differ in k or in the steps ALL return DSGD_EINVAL here.
static int lg_agree(dsgd_ctx* c, const char* what, int k, long long steps, LgCall* q) {
  *q = lg_local(c, k);
  if (!c->comm || !c->comm_lg) return DSGD_OK;
  const int W = c->world;
  DSGD_TRY(c->h_lg_rec.reserve((size_t)LGG_MAX_WORLD * LGG_REC_WORDS));
  long long* h = c->h_lg_rec;
  long long* mine = h + lgg_record_at(c->rank);
  mine[LGG_REC_K] = k;
  mine[LGG_REC_STEPS] = steps;
  mine[LGG_REC_VEXP] = c->vexp;
  unsigned long long* rec = c->d_lg_acc;
  const size_t rec_bytes = sizeof(unsigned long long) * (size_t)W * LGG_REC_WORDS;
  // (any failure from here to the read may leave the record non-zero: the buffer goes, the next call starts from a zeroed one)
  hipError_t he = hipMemcpyAsync(rec + lgg_record_at(c->rank), mine, sizeof(long long) * LGG_REC_WORDS, hipMemcpyHostToDevice, c->stream);
  if (he == hipSuccess) {
    const int r = rccl::AllReduce(rec, rec, (size_t)W * LGG_REC_WORDS, rccl::kInt64, rccl::kSum, c->comm, c->stream);
    if (r) {
      lg_drop(c);
      return fail(DSGD_ERCCL, "%s: ncclAllReduce(the call's agreement): %s", what, rccl::GetErrorString(r));
    }
    he = hipMemcpyAsync(h, rec, rec_bytes, hipMemcpyDeviceToHost, c->stream);
  }
  if (he == hipSuccess) he = hipMemsetAsync(rec, 0, rec_bytes, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he != hipSuccess) {
    lg_drop(c);
    return fail(DSGD_EHIP, "%s: the call's agreement: %s (nothing ran, the weights are unchanged)", what, hipGetErrorString(he));
  }
  const LggVerdict v = lgg_judge(h, W, c->rank);
  if (v.fault == LGG_K_DIFFERS)
    return fail(DSGD_EINVAL, "%s: rank %d hosts %lld workers, this rank (%d) %d: every rank of a step hosts the same number (nothing ran, "
                             "the weights are unchanged)", what, v.bad_rank, v.theirs, c->rank, k);
  if (v.fault == LGG_STEPS_DIFFER)
    return fail(DSGD_EINVAL, "%s: rank %d runs %lld steps, this rank (%d) %lld: every rank of a call runs the same number (nothing ran, "
                             "the weights are unchanged)", what, v.bad_rank, v.theirs, c->rank, steps);
  q->ranks = true;
  q->K = k * W;
  q->vexp = v.vexp;   // (the call's only: c->vexp stays the shard's own, for the SVM and the local calls)
  q->own = q->all + lgg_global_worker(c->rank, k, 0) * c->lg_stride;
  q->hdr = c->d_lg_acc + lgg_step_header_at(W, c->lg_k, q->K);
  return DSGD_OK;
}

// The finish behind a gradient launch of either form (row-wise or by column lists): one column per lane.  Across ranks first
// the step's header words, then ONE in-place all-reduce over the header block and the K slots (cut at LGG_MSG_WORDS), then the
// gathered finish over every rank's workers.
static int lg_launch_finish(dsgd_ctx* c, const LgCall& q, int mode, float lr, const WorkSeg* segs) {
  const dim3 th(LG_THREADS);
  LgFinishArgs f;
  f.acc = q.all;
  f.acc_stride = c->lg_stride;
  f.segs = segs;
  f.K = q.K;
  f.dp = c->dp;
  f.vexp = q.vexp;
  f.perm = c->d_perm;
  f.g_out = c->d_lg_g;
  f.w = c->d_w;
  f.lr = (double)lr;
  f.lambda = c->cfg.lambda;
  f.nsq_part = c->d_lg_part;
  f.hdr = q.hdr;
  f.sc = c->d_sc;
  const dim3 fg((unsigned)lg_finish_blocks(c->dp));
  if (q.ranks) {
    if (mode != LG_STEP) return fail(DSGD_ESTATE, "internal: a gradient across ranks");
    hipLaunchKernelGGL(dsgd_lg_header_kernel, dim3(1), th, 0, c->stream, q.hdr, q.K, (int)lgg_global_worker(c->rank, q.k, 0), q.k, segs);
    HIP_TRY(hipGetLastError());
    const long long words = lgg_step_words(c->dp, q.K);   // (the slots follow the step's header words: one run of words)
    for (long long off = 0; off < words; off += LGG_MSG_WORDS) {
      unsigned long long* at = q.hdr + off;
      const int r = rccl::AllReduce(at, at, (size_t)std::min<long long>(LGG_MSG_WORDS, words - off), rccl::kInt64, rccl::kSum, c->comm, c->stream);
      if (r) return fail(DSGD_ERCCL, "ncclAllReduce(the workers' sums): %s", rccl::GetErrorString(r));
    }
    hipLaunchKernelGGL((dsgd_lg_finish_kernel<LG_STEP, true>), fg, th, 0, c->stream, f);
  } else if (mode == LG_STEP) {
    hipLaunchKernelGGL(dsgd_lg_finish_kernel<LG_STEP>, fg, th, 0, c->stream, f);
  } else {
    hipLaunchKernelGGL(dsgd_lg_finish_kernel<LG_GRADIENT>, fg, th, 0, c->stream, f);
  }
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
// The two launches of one worker's gradient (LG_GRADIENT) or of a step (LG_STEP) over q.k lists of positions in `idx` (list) or
// q.k row ranges (segs hold the rows), the longest of `longest` rows.  lg_ensure and lg_agree (or lg_local) came first.
static int lg_launch(dsgd_ctx* c, bool list, const LgCall& q, long long longest, int mode, float lr, const int* idx, const WorkSeg* segs) {
  const int K = q.k;
  LgArgs a;
  a.w = c->d_w;
  a.dp = c->dp;
  a.vexp = q.vexp;
  a.K = K;
  a.idx = idx;
  a.segs = segs;
  // lists: two workgroups per compute unit at the most, as the fp64 row-parallel family (each flushes its LDS head once);
  // ranges are long streams of rows: four, for the loads in flight
  a.blocks_per_worker = lg_blocks_per_worker(longest, K, c->n_cu, list ? 2 : 4);
  a.acc = q.own;
  a.acc_stride = c->lg_stride;
  a.sc = c->d_sc;
  const dim3 gg((unsigned)(a.blocks_per_worker * K)), th(LG_THREADS);
  const CsrView m = view(c);
  if (list)
    hipLaunchKernelGGL(dsgd_lg_grad_kernel, gg, th, 0, c->stream, m, a);
  else
    hipLaunchKernelGGL(dsgd_lg_grad_range_kernel, gg, th, 0, c->stream, m, a);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = list ? "dsgd_lg_grad_kernel" : "dsgd_lg_grad_range_kernel";
  return lg_launch_finish(c, q, mode, lr, segs);
}
// Behind the last step of a call across ranks: the header words go, BEHIND the finish on the stream (never by a finish workgroup
// while others still read them).  rc: what the steps' enqueueing returned -- a failure half way drops the buffer.
static int lg_steps_end(dsgd_ctx* c, const LgCall& q, int rc) {
  if (!q.ranks) return rc;
  if (rc == DSGD_OK) {
    const hipError_t e = hipMemsetAsync(q.hdr, 0, sizeof(unsigned long long) * (size_t)q.K, c->stream);
    if (e != hipSuccess) rc = fail(DSGD_EHIP, "clearing the header words: %s", hipGetErrorString(e));
  }
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    lg_drop(c);
    return fail(rc, "%s (the weights are those behind the last completed step)", msg);
  }
  return DSGD_OK;
}
// behind a step's launches: the weights moved (the SVM's s and |w|^2 are stale), |w|^2 of the new ones is in d_lg_part; the
// one synchronisation; every row contributes.  Across ranks the rows are the JOB's, counted by the gathered finishes of the
// call's `counted_steps` steps (a call that reports one step's rows divides).
static int lg_step_done(dsgd_ctx* c, const LgCall& q, dsgd_batch_stats* stats, long long total, long long counted_steps = 1) {
  c->s_dirty = true;
  c->lg_nsq_stamp = c->bind_count;
  const int rc = finish_stats(c, stats, total);
  if (rc != DSGD_OK) c->lg_nsq_stamp = ~0ull - 1;
  if (rc == DSGD_OK && stats) {
    if (q.ranks) stats->n_samples = (int64_t)(c->h_sc->n_samples / (unsigned long long)counted_steps);
    stats->n_active = stats->n_samples;
  }
  return rc;
}

// ---- resident logistic plans: the lists and their ranges only, no layout (as a row-parallel fp64 plan) ----
// The caller's lists: dsgd_lg_sync_steps' checks on the host, then the lists resident (the build stream, blocks from the cache).
int dsgd_plan_create_lg_n(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                          dsgd_plan** out) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || !out || n_steps < 1 || n_workers < 1 || n_idx < 1)
    return fail(DSGD_EINVAL, "dsgd_plan_create_lg_n: bad arguments (null pointers, no steps, no workers or no rows)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lg_refuse(c, "dsgd_plan_create_lg_n", LG_SPANS));
  DSGD_TRY(bind(c, true));   // (nothing here touches w: slice-major weights stay as they are)
  DSGD_TRY(require_data(c));
  const LgCheck v = lg_check_flat(idx, n_idx, offsets, n_steps, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_plan_create_lg_n", v, n_workers));
  dsgd_plan* p = nullptr;
  DSGD_TRY(plan_frame(c, offsets, n_steps, n_workers, &p, false, true));
  p->h_idx.assign(idx, idx + n_idx);
  hipError_t e = hipMemcpyAsync(p->d_idx, idx, sizeof(int) * (size_t)n_idx, hipMemcpyHostToDevice, c->build_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->build_stream);
  if (e != hipSuccess) {
    plan_abandon(c, p);
    return fail(DSGD_EHIP, "plan upload: %s", hipGetErrorString(e));
  }
  return plan_finish(c, p, out);
}
// ... drawn by the device from the reference's stream: dsgd_plan_create_from_seed's arguments, limits, refusals and
// *jstate / *n_steps_out / *draws_out (csrc/dsgd_seed_host.hpp, csrc/dsgd_shuffle.hpp as they stand)
int dsgd_plan_create_from_seed_lg(dsgd_ctx* c, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end, int32_t n_splits,
                                  int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out) {
  return plan_from_seed_whole(c, "dsgd_plan_create_from_seed_lg", false, jstate, split_begin, split_end, n_splits, max_samples, batch_size, out,
                              n_steps_out, draws_out, true);
}
// ... a rank's window of the JOB's lists: dsgd_plan_create_from_seed_job's arguments, limits, refusals and outputs (ONE stream over
// all n_job workers, the lists of workers first .. first + n_local - 1, any batch size).  A local call: no collective, accepted
// without a communicator and under dsgd_comm_init_lg's (the scope of dsgd_plan_create_lg_n); dsgd_plan_run on the plan is the
// collective run of that call's plans.  No column-slice twin: slices do not span ranks.
int dsgd_plan_create_from_seed_job_lg(dsgd_ctx* c, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first, int32_t n_local,
                                      const int64_t* split_begin, int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out,
                                      int64_t* draws_out) {
  return plan_from_seed_job(c, "dsgd_plan_create_from_seed_job_lg", false, jstate, job_len, n_job, first, n_local, split_begin, max_samples,
                            batch_size, out, n_steps_out, draws_out, true);
}

// ---- logistic plans on column slices (csrc/dsgd_lg_cs.hpp; the decline rule: csrc/dsgd_lg_cs_host.hpp) ----
static_assert(LG_CS_MAX_SLICE_COLS == CS_MAX_SLICE_COLS, "one cap on a slice's columns for both models");
// A logistic plan just made additionally gets its column slices: the SVM plans' device builder as it stands (cs_build ->
// dsgd_cs_layout_kernel, pass 1 and 2) on the build stream, behind the plan's lists, into blocks from the plan cache that
// the plan owns.  Where lg_cs_pick_G finds no slice count, a step holds more than CS_MAX_SLOTS rows or slots, or the cache
// cannot hold the layout, the builder declines softly: the plan is a plain logistic plan (plan code 7).
static int lg_plan_add_slices(dsgd_ctx* c, dsgd_plan* p) {
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(bind(c, true));   // (nothing here touches w)
  p->lg_cs = true;
  if (c->async_running) return DSGD_OK;   // (the lock-free engine owns the launch stream: no layout, the row form)
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(cs_build(c, p));
  if (c->build_stream) {   // the plan's set-up now ends behind the layout kernels
    HIP_TRY(hipEventRecord(p->built_ev, c->build_stream));
    p->built_pending = true;
  }
  return DSGD_OK;
}
// dsgd_plan_create_lg_n's arguments, checks and refusals; the plan additionally has its column slices laid out
int dsgd_plan_create_lg_cs_n(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                             dsgd_plan** out) {
  DSGD_TRY(check_ctx(c));
  if (!out) return fail(DSGD_EINVAL, "dsgd_plan_create_lg_cs_n: bad arguments (null pointers, no steps, no workers or no rows)");
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DSGD_TRY(lg_refuse(c, "dsgd_plan_create_lg_cs_n", LG_ONE_PROCESS));
  }
  dsgd_plan* p = nullptr;
  DSGD_TRY(dsgd_plan_create_lg_n(c, idx, n_idx, offsets, n_steps, n_workers, &p));
  const int rc = lg_plan_add_slices(c, p);
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    (void)dsgd_plan_destroy(c, p);
    return fail(rc, "%s", msg);
  }
  *out = p;
  return DSGD_OK;
}
// ... and dsgd_plan_create_from_seed_lg's: the same lists, *jstate, *n_steps_out and *draws_out
int dsgd_plan_create_from_seed_lg_cs(dsgd_ctx* c, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end, int32_t n_splits,
                                     int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out) {
  DSGD_TRY(check_ctx(c));
  if (!jstate || !out || !n_steps_out) return fail(DSGD_EINVAL, "bad arguments");
  const uint64_t state_before = *jstate;
  dsgd_plan* p = nullptr;
  DSGD_TRY(dsgd_plan_create_from_seed_lg(c, jstate, split_begin, split_end, n_splits, max_samples, batch_size, &p, n_steps_out, draws_out));
  if (p) {   // (an epoch of no steps has no plan)
    const int rc = lg_plan_add_slices(c, p);
    if (rc != DSGD_OK) {   // as if nothing had been drawn
      char msg[sizeof(g_err)];
      snprintf(msg, sizeof(msg), "%s", g_err);
      (void)dsgd_plan_destroy(c, p);
      *jstate = state_before;
      *n_steps_out = 0;
      if (draws_out) *draws_out = 0;
      return fail(rc, "%s", msg);
    }
  }
  *out = p;
  return DSGD_OK;
}
// The steps [step_begin, step_end) of a logistic plan whose column slices are current: ONE launch of dsgd_lg_cs_step_kernel.
// plan_run_lg made the refusals, bound with the slice-major weights kept and waited for the plan's set-up.
// async: the asynchronous iterations of a one-worker plan instead (dsgd_plan_run_async_lg): ONE launch of dsgd_lg_cs_async_kernel.
static int plan_run_lg_cs(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, double lr, bool async = false) {
  const int K = p->n_workers, G = p->cs_G;
  // the weights slice-major for G slices; dimSparsity with them where the context has one (an SVM slice launch that finds
  // the weights sliced for its G reads both)
  if (c->cs_w_G != G) {
    if (c->have_ds) {
      DSGD_TRY(cs_ensure_sliced(c, G));
    } else {
      DSGD_TRY(cs_unslice(c));
      const int Sp = cs_sp(c->dp, G), n = G * Sp;
      const size_t cap = (size_t)(c->dp + (CS_MAX_G + 1) * 8);
      DSGD_TRY(c->d_cs_w.reserve(cap));
      hipLaunchKernelGGL(dsgd_cs_slice_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_w, c->d_cs_w, c->dp, G, Sp);
      HIP_TRY(hipGetLastError());
      c->cs_w_G = G;
    }
  }
  LgCsArgs la;
  CsArgs& a = la.cs;
  a.hdr = p->d_cs_hdr;
  a.slot_meta = p->d_cs_meta;
  a.row_first = p->d_cs_rf;
  a.col = p->d_cs_col;
  a.val = p->d_cs_val;
  a.clist = p->d_cs_cl;
  a.cl_stride = p->cs_cl_stride;
  cs_common_args(c, a, G, K, (float)lr);
  a.tprof = nullptr;
  a.test_skip_publish = 0;
  a.n_steps_plan = p->n_steps;
  a.step_begin = step_begin;
  a.step_end = step_end;
  a.slot_stride = p->cs_slot_stride;
  a.row_stride = p->cs_row_stride;
  la.segs = p->d_segs;
  la.lr = lr;
  la.lambda = c->cfg.lambda;
  const size_t lds = sizeof(float) * (size_t)lg_cs_lds(c->dp, G, K).words;
  DSGD_TRY(cs_take_tags(c, (unsigned long long)(step_end - step_begin), &a.tag0));   // (the one counter of both models' launches)
  if (async && p->cs_spl == 1)
    hipLaunchKernelGGL(dsgd_lg_cs_async_kernel<1>, dim3((unsigned)G), dim3(CS_THREADS), lds, c->stream, la);
  else if (async)
    hipLaunchKernelGGL(dsgd_lg_cs_async_kernel<2>, dim3((unsigned)G), dim3(CS_THREADS), lds, c->stream, la);
  else if (p->cs_spl == 1)
    hipLaunchKernelGGL(dsgd_lg_cs_step_kernel<1>, dim3((unsigned)G), dim3(CS_THREADS), lds, c->stream, la);
  else
    hipLaunchKernelGGL(dsgd_lg_cs_step_kernel<2>, dim3((unsigned)G), dim3(CS_THREADS), lds, c->stream, la);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = async ? "dsgd_lg_cs_async_kernel" : "dsgd_lg_cs_step_kernel";
  c->fused_apply_pending = false;
  c->s_lazy = false;
  c->nsq_dirty = false;
  return DSGD_OK;
}
// The steps [step_begin, step_end) of a logistic plan (dsgd_plan_run holds the lock and has checked the range): per step the
// two launches of dsgd_lg_sync_step over the plan's resident lists -- no upload, no host synchronisation.  Every refusal comes
// before the first launch.  dsgd_synchronize reports the rows (every row contributes: n_active == n_samples).
static int plan_run_lg(dsgd_ctx* c, dsgd_plan* p, long long step_begin, long long step_end, float lr) {
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_plan_run (a logistic plan)", p->lg_cs ? LG_ONE_PROCESS : LG_SPANS, &fresh, p->lg_cs));
  DSGD_TRY(plan_revalidate(c, p));   // (a plan from before the last load: DSGD_ERANGE here, before anything is enqueued)
  DSGD_TRY(prepare_layout(c));
  const int K = p->n_workers;
  // a plan made with its column slices runs on them while they are current; declined or stale: the two launches below
  const bool slices = p->lg_cs && plan_route(c, p) == PLAN_LG_CS && ensure_cs_exchange(c) == DSGD_OK;
  if (p->lg_cs && !slices) DSGD_TRY(cs_unslice(c));   // (bound with the slice-major weights kept: the row form reads d_w)
  if (!slices) DSGD_TRY(lg_ensure(c, K));
  if (p->built_pending) {   // the plan's set-up ran beside the launch stream: wait for it, once
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  LgCall q;
  if (!slices) DSGD_TRY(lg_agree(c, "dsgd_plan_run (a logistic plan)", K, std::max<long long>(0, step_end - step_begin), &q));   // (an empty run takes part)
  if (step_end <= step_begin) {
    if (fresh) c->lg_nsq_stamp = c->bind_count;   // (the weights are the ones |w|^2 was taken from)
    return DSGD_OK;
  }
  c->s_dirty = true;
  c->lg_nsq_stamp = ~0ull - 1;
  if (q.ranks && !c->job_pending) {   // (the job's rows run on from zero in n_samples until dsgd_synchronize, as the fp64 plans')
    HIP_TRY(hipMemsetAsync(&c->d_sc->n_samples, 0, sizeof(unsigned long long), c->stream));
    c->job_pending = true;
  }
  if (slices) {   // ONE launch; it leaves no |w'|^2 words: the next evaluation takes them from dsgd_lg_nsq_kernel
    DSGD_TRY(plan_run_lg_cs(c, p, step_begin, step_end, lr));
  } else {
    int rc = DSGD_OK;
    for (long long t = step_begin; t < step_end && rc == DSGD_OK; ++t) {
      long long mx = 0;
      for (int k = 0; k < K; ++k) mx = std::max<long long>(mx, p->offsets[(size_t)(t * K + k + 1)] - p->offsets[(size_t)(t * K + k)]);
      rc = lg_launch(c, true, q, mx, LG_STEP, lr, p->d_idx, p->d_segs + t * K);
    }
    DSGD_TRY(lg_steps_end(c, q, rc));
    c->lg_nsq_stamp = c->bind_count;   // (the last finish left |w'|^2 in d_lg_part)
  }
  if (q.ranks) return DSGD_OK;   // (the device counts the job's rows)
  const long long rows = p->offsets[(size_t)(step_end * K)] - p->offsets[(size_t)(step_begin * K)];
  c->pending_samples += rows;
  c->lg_pending_active += rows;
  return DSGD_OK;
}

int dsgd_lg_gradient(dsgd_ctx* c, const float* w, const int32_t* idx, int64_t n, float* g_out, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!g_out) return fail(DSGD_EINVAL, "dsgd_lg_gradient: null g_out");
  if (n < 1 || !idx) return fail(DSGD_EINVAL, "dsgd_lg_gradient: Cannot sum an empty list of vectors");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_gradient", LG_STAYS_LOCAL, &fresh));
  const int64_t nn = n;
  const LgCheck v = lg_check_lists(&idx, &nn, 1, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_gradient", v, 1));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(lg_ensure(c, 1));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  DSGD_TRY(lg_launch(c, true, lg_local(c, 1), mx, LG_GRADIENT, 0.0f, c->cur_idx, c->d_segs));
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_out, bytes));
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_lg_g, bytes, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(finish_stats(c, stats, tot));   // the one synchronisation of the call
  memcpy(g_out, c->pin_out.p, bytes);
  if (stats) stats->n_active = tot;
  if (fresh && !w) c->lg_nsq_stamp = c->bind_count;   // (the weights are the ones |w|^2 was taken from)
  return DSGD_OK;
}

int dsgd_lg_sync_step(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers, float lr,
                      dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !idx_per_worker || !n_per_worker) return fail(DSGD_EINVAL, "dsgd_lg_sync_step: Cannot sum an empty list of vectors (no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_sync_step", LG_SPANS, &fresh));
  const LgCheck v = lg_check_lists(idx_per_worker, n_per_worker, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_sync_step", v, n_workers));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(lg_ensure(c, n_workers));
  LgCall q;
  DSGD_TRY(lg_agree(c, "dsgd_lg_sync_step", n_workers, 1, &q));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
  DSGD_TRY(lg_steps_end(c, q, lg_launch(c, true, q, mx, LG_STEP, lr, c->cur_idx, c->d_segs)));
  return lg_step_done(c, q, stats, tot);
}

// the row ranges of a whole-split call as the WorkSegs in c->d_segs
static int lg_upload_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int n_workers) {
  std::vector<WorkSeg> segs((size_t)n_workers);
  for (int k = 0; k < n_workers; ++k) {
    segs[(size_t)k].begin = row_begin[k];
    segs[(size_t)k].end = row_end[k];
  }
  return upload_segs(c, segs);
}
int dsgd_lg_sync_step_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, float lr, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "dsgd_lg_sync_step_ranges: Cannot sum an empty list of vectors (no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_sync_step_ranges", LG_SPANS, &fresh));
  const LgCheck v = lg_check_ranges(row_begin, row_end, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_sync_step_ranges", v, n_workers));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(lg_ensure(c, n_workers));
  LgCall q;
  DSGD_TRY(lg_agree(c, "dsgd_lg_sync_step_ranges", n_workers, 1, &q));
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(lg_upload_ranges(c, row_begin, row_end, n_workers));
  DSGD_TRY(lg_steps_end(c, q, lg_launch(c, false, q, v.longest, LG_STEP, lr, nullptr, c->d_segs)));
  return lg_step_done(c, q, stats, v.total);
}

// ---- whole-split steps by column lists (csrc/dsgd_lg_cols.hpp; the sizes: csrc/dsgd_lg_cols_host.hpp) ----
// The layout of these ranges (c->d_segs holds them; the stream may be busy): DSGD_OK with *out, or 1 = none to be had -- too
// many entries or positions (remembered for the configuration), or no memory (this call only): the caller's row form.
static int lgc_layout(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int K, long long longest, dsgd_ctx::LgColsLayout** out) {
  std::vector<long long> key;
  long long n_ent = 0;
  for (int k = 0; k < K; ++k) {
    key.push_back(row_begin[k]);
    key.push_back(row_end[k]);
    n_ent += c->h_row_ptr[(size_t)row_end[k]] - c->h_row_ptr[(size_t)row_begin[k]];
  }
  if (auto* e = c->lgc_cache.find(key, 0, c->layout_gen)) {
    if (e->declined) return 1;   // (declined before: not tried again step after step)
    *out = &e->layout;
    return DSGD_OK;
  }
  DSGD_TRY(layout_room(c, c->lgc_cache));
  dsgd_ctx::LgColsLayout L;
  LgcPlan plan;
  std::vector<long long> base((size_t)K);
  if (lgc_plan(row_begin, row_end, K, n_ent, c->dp, c->lg_stride, c->n_cu, &plan, base.data()) != LGC_OK) {
    c->lgc_cache.insert_declined(std::move(key), 0, c->layout_gen);   // remembered as declined
    return 1;
  }
  std::vector<int> pos_base(base.begin(), base.end());   // (below 2^31: lgc_plan)
  LAYOUT_SOFT(L.d_pos_base.try_alloc((size_t)K));
  LAYOUT_SOFT(L.d_cq.try_alloc((size_t)plan.positions));
  LAYOUT_SOFT(L.d_ent.try_alloc((size_t)plan.n_pad));
  LAYOUT_SOFT(L.d_shares.try_alloc((size_t)plan.n_shares));
  LAYOUT_SOFT(hipMemcpyAsync(L.d_pos_base, pos_base.data(), sizeof(int) * (size_t)K, hipMemcpyHostToDevice, c->stream));
  LAYOUT_SOFT(hipMemsetAsync(L.d_ent + (plan.n_pad - plan.share), 0, sizeof(uint2) * (size_t)plan.share, c->stream));   // the last share's padding
  const dim3 grid = tcol_row_grid(longest, K);
  ColSort sort;
  LAYOUT_SOFT(sort.count(c, grid, K * c->dp));   // (also: pos_base is a local)
  if (sort.tot[0] != (unsigned long long)n_ent)   // (the stream is idle: count returned behind its kernels)
    return fail(DSGD_ESTATE, "logistic column lists: the device counted %llu entries in the ranges, the host %lld", sort.tot[0], n_ent);
  L.n_ent = n_ent;
  L.share = plan.share;
  L.n_wg = (int)plan.n_shares;
  LAYOUT_SOFT(L.d_slot_of_cid.try_alloc((size_t)std::max<unsigned long long>(1, sort.tot[1])));
  sort.shares(c, L.n_ent, L.share, L.n_wg, L.d_shares);
  hipLaunchKernelGGL(dsgd_lgc_fill_kernel, grid, dim3(TC_THREADS), 0, c->stream, view(c), c->d_segs, c->dp, sort.d_ptr.get(), sort.d_cursor.get(),
                     sort.d_cid.get(), L.d_pos_base.get(), c->lg_stride, L.d_ent.get(), L.d_slot_of_cid.get());
  LAYOUT_SOFT(hipGetLastError());
  LAYOUT_SOFT(hipStreamSynchronize(c->stream));
  *out = &c->lgc_cache.insert(std::move(key), 0, c->layout_gen, std::move(L))->layout;
  return DSGD_OK;
}
// the three launches of one step over the ranges in c->d_segs, by their layout
static int lgc_launch(dsgd_ctx* c, const LgCall& call, const dsgd_ctx::LgColsLayout& L, long long longest, float lr) {
  const int K = call.k;
  LgcCoefArgs q;
  q.w = c->d_w;
  q.vexp = call.vexp;
  q.K = K;
  q.segs = c->d_segs;
  q.pos_base = L.d_pos_base;
  q.blocks_per_worker = lg_blocks_per_worker(longest, K, c->n_cu, 8);   // (no LDS: the 2,048 lanes a compute unit holds)
  q.cq = L.d_cq;
  q.sc = c->d_sc;
  hipLaunchKernelGGL(dsgd_lg_coef_kernel, dim3((unsigned)(q.blocks_per_worker * K)), dim3(LG_THREADS), 0, c->stream, view(c), q);
  HIP_TRY(hipGetLastError());
  LgcGradArgs g;
  g.ent = L.d_ent;
  g.shares = L.d_shares;
  g.slot_of_cid = L.d_slot_of_cid;
  g.cq = L.d_cq;
  g.acc = call.own;   // (the layout's words are `worker * lg_stride + column` from here)
  g.n_ent = L.n_ent;
  g.share = L.share;
  hipLaunchKernelGGL(dsgd_lg_cgrad_kernel, dim3((unsigned)L.n_wg), dim3(LGC_THREADS), 0, c->stream, g);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = "dsgd_lg_cgrad_kernel";
  return lg_launch_finish(c, call, LG_STEP, lr, c->d_segs);
}

int dsgd_lg_sync_steps_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, int64_t n_steps, float lr,
                              dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "dsgd_lg_sync_steps_ranges: Cannot sum an empty list of vectors (no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_sync_steps_ranges", LG_SPANS, &fresh));
  const LgCheck v = lg_check_ranges(row_begin, row_end, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_sync_steps_ranges", v, n_workers));
  if (n_steps < 1) return lg_report(c, "dsgd_lg_sync_steps_ranges", lg_fault(LG_NO_WORKERS, -1, -1, n_steps), n_workers);
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(lg_ensure(c, n_workers));
  LgCall q;
  DSGD_TRY(lg_agree(c, "dsgd_lg_sync_steps_ranges", n_workers, n_steps, &q));
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(lg_upload_ranges(c, row_begin, row_end, n_workers));
  dsgd_ctx::LgColsLayout* L = nullptr;
  const int lrc = lgc_layout(c, row_begin, row_end, n_workers, v.longest, &L);
  if (lrc != DSGD_OK && lrc != 1) return lrc;
  c->s_dirty = true;   // (from the first launch on the weights move)
  c->lg_nsq_stamp = ~0ull - 1;
  // three launches per step (no layout: the row form's two), back to back on the stream: no host synchronisation in between
  int rc = DSGD_OK;
  for (int64_t t = 0; t < n_steps && rc == DSGD_OK; ++t)
    rc = L ? lgc_launch(c, q, *L, v.longest, lr) : lg_launch(c, false, q, v.longest, LG_STEP, lr, nullptr, c->d_segs);
  DSGD_TRY(lg_steps_end(c, q, rc));
  return lg_step_done(c, q, stats, v.total, n_steps);
}

int dsgd_lg_sync_steps(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers, float lr,
                       dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || n_steps < 1 || n_workers < 1 || n_idx < 1) return fail(DSGD_EINVAL, "dsgd_lg_sync_steps: bad arguments (null lists, no steps or no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_sync_steps", LG_SPANS, &fresh));
  const int K = n_workers;
  const LgCheck v = lg_check_flat(idx, n_idx, offsets, n_steps, K, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_sync_steps", v, K));
  const int64_t n_lists = n_steps * K;
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(lg_ensure(c, K));
  LgCall q;
  DSGD_TRY(lg_agree(c, "dsgd_lg_sync_steps", K, n_steps, &q));
  if (c->d_lg_ssegs.cap() < (size_t)n_lists) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lg_ssegs.reserve((size_t)n_lists));
  }
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
  HIP_TRY(hipMemcpyAsync(c->d_lg_ssegs, c->pin_segs.p, sizeof(WorkSeg) * (size_t)n_lists, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_segs));
  // two launches per step, back to back on the stream: no host synchronisation in between
  int rc = DSGD_OK;
  for (int64_t t = 0; t < n_steps && rc == DSGD_OK; ++t) {
    long long mx = 0;
    for (int k = 0; k < K; ++k) mx = std::max<long long>(mx, offsets[t * K + k + 1] - offsets[t * K + k]);
    rc = lg_launch(c, true, q, mx, LG_STEP, lr, c->d_idx, c->d_lg_ssegs + t * K);
  }
  DSGD_TRY(lg_steps_end(c, q, rc));
  return lg_step_done(c, q, stats, n_idx);
}

int dsgd_lg_loss_acc(dsgd_ctx* c, const float* w, int64_t row_begin, int64_t row_end, double* loss, double* acc) {
  DSGD_TRY(check_ctx(c));
  if (!loss && !acc) return fail(DSGD_EINVAL, "dsgd_lg_loss_acc: null loss and acc");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_loss_acc", LG_STAYS_LOCAL, &fresh));
  const LgCheck v = lg_check_ranges(&row_begin, &row_end, 1, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_loss_acc", v, 1));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(lg_ensure(c, 1));
  const long long nb = lg_finish_blocks(c->dp);
  if (w || !fresh) {   // |w|^2 of weights the logistic finish did not write: the finish's grid and tree, the same bits
    hipLaunchKernelGGL(dsgd_lg_nsq_kernel, dim3((unsigned)nb), dim3(LG_THREADS), 0, c->stream, c->d_w, 0LL, c->dp, c->d_lg_part);
    HIP_TRY(hipGetLastError());
  }
  DSGD_TRY(reset_counters(c));
  const long long rows = row_end - row_begin;
  const long long grid = lg_eval_blocks(rows, c->n_cu);
  // small ranges do not amortise staging 160 KiB of weights per workgroup: a small tile (the rule of dsgd_loss_acc)
  int hw = rows >= 4096 ? c->hw_eval : std::min(c->hw_eval, 1024);
  while (lg_eval_lds_floats(hw) > DSGD_LDS_FLOATS) hw -= 64;
  const size_t lds = sizeof(float) * (size_t)lg_eval_lds_floats(hw);
  hipLaunchKernelGGL(dsgd_lg_eval_kernel, dim3((unsigned)grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_w, (long long)row_begin,
                     (long long)row_end, c->d_sc, hw, c->d_lg_part + nb);
  HIP_TRY(hipGetLastError());
  const size_t words = (size_t)(nb + grid);
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(double) * words));
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_lg_part, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  c->lg_nsq_stamp = c->bind_count;
  const double* part = static_cast<const double*>(c->pin_out.p.get());
  double nsq = 0.0, ls = 0.0;   // (in order: the same bits on every call)
  for (long long i = 0; i < nb; ++i) nsq += part[i];
  for (long long i = 0; i < grid; ++i) ls += part[nb + i];
  const double n = (double)rows;
  if (loss) *loss = c->cfg.lambda * nsq + ls / n;
  if (acc) *acc = (double)c->h_sc->counts[0] / n;
  return DSGD_OK;
}

// dsgd_lg_loss_acc over up to LG_MAX_RANGES ranges (an epoch's train and test passes) in ONE launch with ONE synchronisation:
// every range's figures are the bits of dsgd_lg_loss_acc on that range alone (csrc/dsgd_lg_host.hpp: lg_eval_table)
int dsgd_lg_loss_acc_ranges(dsgd_ctx* c, const float* w, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges, double* loss_out,
                            double* acc_out) {
  DSGD_TRY(check_ctx(c));
  if (!row_begin || !row_end || n_ranges < 1 || (!loss_out && !acc_out))
    return fail(DSGD_EINVAL, "dsgd_lg_loss_acc_ranges: bad arguments (null ranges, no range, or null loss_out and acc_out)");
  if (n_ranges > LG_MAX_RANGES) return fail(DSGD_EINVAL, "dsgd_lg_loss_acc_ranges: %d ranges, more than the %d of one call", n_ranges, LG_MAX_RANGES);
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_loss_acc_ranges", LG_STAYS_LOCAL, &fresh));
  const LgCheck v = lg_check_ranges(row_begin, row_end, n_ranges, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_loss_acc_ranges", v, n_ranges));
  LgEvalTable t;
  if (!lg_eval_table(row_begin, row_end, n_ranges, c->n_cu, &t)) return fail(DSGD_EINVAL, "dsgd_lg_loss_acc_ranges: no grid for %d ranges", n_ranges);
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(lg_ensure(c, 1));
  const long long nb = lg_finish_blocks(c->dp);
  if (w || !fresh) {   // (as dsgd_lg_loss_acc: the finish's grid and tree, the same bits)
    hipLaunchKernelGGL(dsgd_lg_nsq_kernel, dim3((unsigned)nb), dim3(LG_THREADS), 0, c->stream, c->d_w, 0LL, c->dp, c->d_lg_part);
    HIP_TRY(hipGetLastError());
  }
  DSGD_TRY(reset_counters(c));
  HIP_TRY(hipMemsetAsync(c->d_lg_tally, 0, sizeof(unsigned long long) * LG_MAX_RANGES * LG_TALLY_WORDS, c->stream));
  // ONE tile size for the launch, by its longest range (dsgd_lg_loss_acc's rule for that range); the size moves no bit of any
  // range: row_dot reads the same float from the tile as from memory and adds in the same order
  int hw = v.longest >= 4096 ? c->hw_eval : std::min(c->hw_eval, 1024);
  while (lg_eval_lds_floats(hw) > DSGD_LDS_FLOATS) hw -= 64;
  const size_t lds = sizeof(float) * (size_t)lg_eval_lds_floats(hw);
  hipLaunchKernelGGL(dsgd_lg_eval_ranges_kernel, dim3((unsigned)t.grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_w, t, c->d_lg_tally.get(),
                     hw, c->d_lg_part + nb);
  HIP_TRY(hipGetLastError());
  const size_t words = (size_t)(nb + t.grid), tally_words = (size_t)LG_MAX_RANGES * LG_TALLY_WORDS;
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(double) * words + sizeof(unsigned long long) * tally_words));
  double* part = static_cast<double*>(c->pin_out.p.get());
  unsigned long long* tally = reinterpret_cast<unsigned long long*>(part + words);
  HIP_TRY(hipMemcpyAsync(part, c->d_lg_part, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tally, c->d_lg_tally, sizeof(unsigned long long) * tally_words, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  c->lg_nsq_stamp = c->bind_count;
  double nsq = 0.0;   // (in order: the same bits on every call)
  for (long long i = 0; i < nb; ++i) nsq += part[i];
  for (int r = 0; r < t.n; ++r) {
    double ls = 0.0;
    for (int i = 0; i < t.r[r].n_blocks; ++i) ls += part[nb + t.r[r].first_block + i];
    const double n = (double)(t.r[r].row_end - t.r[r].row_begin);
    if (loss_out) loss_out[r] = c->cfg.lambda * nsq + ls / n;
    if (acc_out) acc_out[r] = (double)tally[(size_t)r * LG_TALLY_WORDS] / n;
  }
  return DSGD_OK;
}

int dsgd_lg_predict(dsgd_ctx* c, const float* w, const int32_t* idx, int64_t n, float* p_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 1 || !idx || !p_out) return fail(DSGD_EINVAL, "dsgd_lg_predict: bad arguments (a null pointer or no rows)");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_predict", LG_STAYS_LOCAL, &fresh));
  const int64_t nn = n;
  const LgCheck v = lg_check_lists(&idx, &nn, 1, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_predict", v, 1));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(ensure_idx(c, n));
  if ((size_t)n > c->d_lg_p.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lg_p.reserve((size_t)std::max<long long>(n, 4096)));
  }
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(send_idx(c, idx, n));
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(float) * (size_t)n));
  hipLaunchKernelGGL(dsgd_lg_predict_kernel, dim3((unsigned)grid_for(c, n, LG_GROUP)), dim3(LG_THREADS), 0, c->stream, view(c), c->d_w, c->d_idx,
                     (long long)n, c->d_lg_p, c->d_sc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_lg_p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));
  memcpy(p_out, c->pin_out.p, sizeof(float) * (size_t)n);
  DSGD_TRY(check_err_flag(c));
  if (fresh && !w) c->lg_nsq_stamp = c->bind_count;
  return DSGD_OK;
}

// ---- distributed and sampled evaluation (csrc/dsgd_lg_eval.hpp; ref: core/Master.scala:61-118) ----
// the tile of an evaluation launch whose longest range (or list) has `rows` rows, and `extra` floats of LDS behind
// dsgd_lg_eval_kernel's: dsgd_lg_loss_acc's rule (small ranges do not amortise staging 160 KiB per workgroup)
static int lg_eval_hw(dsgd_ctx* c, long long rows, int extra) {
  int hw = rows >= 4096 ? c->hw_eval : std::min(c->hw_eval, 1024);
  while (hw > 0 && lg_eval_lds_floats(hw) + extra > DSGD_LDS_FLOATS) hw -= 64;
  return std::max(hw, 0);
}
// |w|^2 of weights the logistic finish did not write, as dsgd_lg_loss_acc takes it: the finish's grid and tree, the same bits
static int lg_nsq_if_stale(dsgd_ctx* c, bool stale) {
  if (!stale) return DSGD_OK;
  hipLaunchKernelGGL(dsgd_lg_nsq_kernel, dim3((unsigned)lg_finish_blocks(c->dp)), dim3(LG_THREADS), 0, c->stream, c->d_w, 0LL, c->dp, c->d_lg_part);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// the verdict of lg_pred_table (csrc/dsgd_lg_host.hpp) in the words and with the codes of the SVM's dsgd_predict_ranges
static int lg_report(dsgd_ctx* c, const char* what, const LgPredTable& t, const int64_t* row_begin, const int64_t* row_end) {
  switch (t.fault) {
    case LGP_OK: return DSGD_OK;
    case LGP_ARGS: return fail(DSGD_EINVAL, "%s: bad arguments (null ranges or no range)", what);
    case LGP_TOO_MANY: return fail(DSGD_EINVAL, "%s: more than %d ranges in one call", what, LG_PRED_MAX_RANGES);
    case LGP_REVERSED:
      return fail(DSGD_EINVAL, "%s: range %d: begin %lld > end %lld", what, t.range, (long long)row_begin[t.range], (long long)row_end[t.range]);
    case LGP_OUTSIDE:
      return fail(DSGD_ERANGE, "%s: rows [%lld, %lld) of range %d outside the %lld loaded rows", what, (long long)row_begin[t.range],
                  (long long)row_end[t.range], t.range, c->n_rows);
    case LGP_OVERLAP:
      return fail(DSGD_EINVAL, "%s: ranges %d and %d overlap: [%lld, %lld) and [%lld, %lld)", what, t.range, t.other, (long long)row_begin[t.range],
                  (long long)row_end[t.range], (long long)row_begin[t.other], (long long)row_end[t.other]);
    case LGP_NO_ROWS: break;
  }
  return fail(DSGD_EINVAL, "%s: no rows in any range: reduce on an empty prediction map", what);
}

int dsgd_lg_predict_ranges(dsgd_ctx* c, const float* w, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges, int8_t* class_out,
                           float* proba_out, int64_t* counts_out, double* range_loss_out, double* loss, double* acc) {
  const char* what = "dsgd_lg_predict_ranges";
  DSGD_TRY(check_ctx(c));
  if (n_ranges < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "%s: bad arguments (null ranges or no range)", what);
  if (n_ranges > LG_PRED_MAX_RANGES) return fail(DSGD_EINVAL, "%s: %d ranges in one call (at most %d)", what, n_ranges, LG_PRED_MAX_RANGES);
  if (!class_out && !proba_out && !counts_out && !range_loss_out && !loss && !acc) return fail(DSGD_EINVAL, "%s: every output is null", what);
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, what, LG_STAYS_LOCAL, &fresh));
  const int K = n_ranges;
  const size_t tab_words = (size_t)lg_pred_tab_words(K);
  std::vector<long long> tab(tab_words);
  long long* first_block = tab.data();
  long long* out_off = tab.data() + (2 * K + 1);
  const LgPredTable t = lg_pred_table(row_begin, row_end, K, c->n_cu, c->n_rows, first_block, tab.data() + (K + 1), out_off);
  DSGD_TRY(lg_report(c, what, t, row_begin, row_end));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(lg_ensure(c, 1));
  const size_t total = (size_t)t.total, grid = (size_t)t.grid, tally_words = (size_t)K * LG_TALLY_WORDS;
  if (!c->d_lg_pred_tab || grid > c->d_lg_pred_part.cap() || (class_out && total > c->d_lg_cls.cap()) || (proba_out && total > c->d_lg_p.cap())) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lg_pred_tab.reserve((size_t)lg_pred_tab_words(LG_PRED_MAX_RANGES)));
    DSGD_TRY(c->d_lg_pred_tally.reserve((size_t)LG_PRED_MAX_RANGES * LG_TALLY_WORDS));
    DSGD_TRY(c->d_lg_pred_part.reserve(std::max<size_t>(grid, (size_t)c->n_cu), Grow::twice));
    if (class_out) DSGD_TRY(c->d_lg_cls.reserve(std::max<size_t>(total, 4096), Grow::twice));
    if (proba_out) DSGD_TRY(c->d_lg_p.reserve(std::max<size_t>(total, 4096), Grow::twice));
  }
  const long long nb = lg_finish_blocks(c->dp);
  DSGD_TRY(lg_nsq_if_stale(c, w || !fresh));
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(pin_acquire(c->pin_idx, sizeof(long long) * tab_words));
  memcpy(c->pin_idx.p, tab.data(), sizeof(long long) * tab_words);
  HIP_TRY(hipMemcpyAsync(c->d_lg_pred_tab, c->pin_idx.p, sizeof(long long) * tab_words, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_idx));
  HIP_TRY(hipMemsetAsync(c->d_lg_pred_tally, 0, sizeof(unsigned long long) * tally_words, c->stream));
  // ONE tile size for the launch, by its longest range (dsgd_lg_loss_acc's rule for that range): the size moves no bit
  const int hw = lg_eval_hw(c, t.longest, 2 * lg_pred_tab_words(K));
  const size_t lds = sizeof(float) * (size_t)lg_pred_lds_floats(hw, K);
  LgPredArgs a;
  a.tab = c->d_lg_pred_tab;
  a.K = K;
  a.cls = class_out ? c->d_lg_cls.get() : nullptr;
  a.proba = proba_out ? c->d_lg_p.get() : nullptr;
  a.tally = c->d_lg_pred_tally;
  a.loss_part = c->d_lg_pred_part;
  hipLaunchKernelGGL(dsgd_lg_predict_ranges_kernel, dim3((unsigned)grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_w, a, hw);
  HIP_TRY(hipGetLastError());
  // every reply through the pinned buffer: the |w|^2 words, the workgroups' loss words, the tallies, the probabilities, the bytes
  const size_t part_words = (size_t)nb + grid;
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(double) * part_words + sizeof(unsigned long long) * tally_words + (proba_out ? sizeof(float) * total : 0) +
                                       (class_out ? total : 0)));
  double* part = static_cast<double*>(c->pin_out.p.get());
  unsigned long long* tally = reinterpret_cast<unsigned long long*>(part + part_words);
  float* h_proba = reinterpret_cast<float*>(tally + tally_words);
  signed char* h_cls = reinterpret_cast<signed char*>(h_proba + (proba_out ? total : 0));
  HIP_TRY(hipMemcpyAsync(part, c->d_lg_part, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(part + nb, c->d_lg_pred_part, sizeof(double) * grid, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tally, c->d_lg_pred_tally, sizeof(unsigned long long) * tally_words, hipMemcpyDeviceToHost, c->stream));
  if (proba_out) HIP_TRY(hipMemcpyAsync(h_proba, c->d_lg_p, sizeof(float) * total, hipMemcpyDeviceToHost, c->stream));
  if (class_out) HIP_TRY(hipMemcpyAsync(h_cls, c->d_lg_cls, total, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  c->lg_nsq_stamp = c->bind_count;
  for (int r = 0; r < K; ++r) {   // (before anything is written)
    const unsigned long long* tr = tally + (size_t)r * LG_TALLY_WORDS;
    const long long rows = out_off[r + 1] - out_off[r];
    if ((long long)(tr[0] + tr[1] + tr[2]) != rows)
      return fail(DSGD_ESTATE, "internal: %llu rows tallied of the %lld of range %d", tr[0] + tr[1] + tr[2], rows, r);
  }
  double nsq = 0.0, ls_all = 0.0;   // (in order: the same bits on every call)
  for (long long i = 0; i < nb; ++i) nsq += part[i];
  unsigned long long right = 0;
  for (int r = 0; r < K; ++r) {
    const unsigned long long* tr = tally + (size_t)r * LG_TALLY_WORDS;
    const long long rows = out_off[r + 1] - out_off[r];
    double ls = 0.0;
    for (long long i = first_block[r]; i < first_block[r + 1]; ++i) ls += part[nb + i];
    ls_all += ls;
    right += tr[0];
    if (range_loss_out) range_loss_out[r] = rows ? c->cfg.lambda * nsq + ls / (double)rows : 0.0;   // (dsgd_lg_loss_acc's expression)
    for (int j = 0; counts_out && j < 3; ++j) counts_out[3 * r + j] = (int64_t)tr[j];
  }
  if (proba_out) memcpy(proba_out, h_proba, sizeof(float) * total);
  if (class_out) memcpy(class_out, h_cls, total);
  if (loss) *loss = c->cfg.lambda * nsq + ls_all / (double)t.total;
  if (acc) *acc = (double)right / (double)t.total;
  return DSGD_OK;
}

// after a collective of dsgd_lg_eval_job that failed half way: the record goes, the next call starts from a zeroed one (as lg_drop)
static void lge_drop(dsgd_ctx* c) {
  (void)hipStreamSynchronize(c->stream);
  c->d_lge_rec.reset();
}
// The JOB's evaluation on every rank (csrc/dsgd_lg_eval_job.hpp; include/dsgd.h "ACROSS RANKS"): this rank's n_local ranges take the
// positions rank * n_local + j of K = n_local * world.  All local checks, the agreement (lg_agree's record with n_local where a step
// puts k and -1 where it puts its steps: a rank in a step and a rank in an evaluation disagree too), ONE launch of
// dsgd_lg_predict_ranges_kernel as it stands, dsgd_lg_eval_fold_kernel, ONE in-place all-reduce of the record, one read-back,
// lge_fold.  Every output has the bits dsgd_lg_predict_ranges returns on ONE context over the ranks' rows in rank order.
int dsgd_lg_eval_job(dsgd_ctx* c, const float* w, const int64_t* row_begin, const int64_t* row_end, int32_t n_local, int64_t* counts_out,
                     double* range_loss_out, double* loss, double* acc, int32_t* K_out) {
  const char* what = "dsgd_lg_eval_job";
  DSGD_TRY(check_ctx(c));
  if (n_local < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "%s: bad arguments (null ranges or no range)", what);
  if (!counts_out && !range_loss_out && !loss && !acc) return fail(DSGD_EINVAL, "%s: every output is null", what);
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, what, LG_SPANS, &fresh));
  const bool ranks = c->comm && c->comm_lg;
  const int world = ranks ? c->world : 1, rank = ranks ? c->rank : 0;
  if (n_local > LG_PRED_MAX_RANGES / world)
    return fail(DSGD_EINVAL, "%s: %d ranges on each of %d ranks (at most %d in the job)", what, n_local, world, LG_PRED_MAX_RANGES);
  const int k = n_local, K = k * world;
  const size_t tab_words = (size_t)lg_pred_tab_words(k);
  std::vector<long long> tab(tab_words);
  long long* first_block = tab.data();
  long long* out_off = tab.data() + (2 * k + 1);
  const LgPredTable t = lg_pred_table(row_begin, row_end, k, c->n_cu, c->n_rows, first_block, tab.data() + (k + 1), out_off);
  DSGD_TRY(lg_report(c, what, t, row_begin, row_end));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(lg_ensure(c, 1));
  const size_t grid = (size_t)t.grid, tally_words = (size_t)k * LG_TALLY_WORDS, rec_words = (size_t)lge_words(K);
  if (!c->d_lg_pred_tab || !c->d_lge_rec || grid > c->d_lg_pred_part.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lg_pred_tab.reserve((size_t)lg_pred_tab_words(LG_PRED_MAX_RANGES)));
    DSGD_TRY(c->d_lg_pred_tally.reserve((size_t)LG_PRED_MAX_RANGES * LG_TALLY_WORDS));
    DSGD_TRY(c->d_lg_pred_part.reserve(std::max<size_t>(grid, (size_t)c->n_cu), Grow::twice));
    if (!c->d_lge_rec) {   // (zeroed once: the kernel writes or zeroes every word a call's all-reduce covers)
      const size_t cap = (size_t)lge_words(LG_PRED_MAX_RANGES);
      DSGD_TRY(c->d_lge_rec.alloc(cap));
      HIP_TRY(hipMemsetAsync(c->d_lge_rec, 0, sizeof(unsigned long long) * cap, c->stream));
    }
  }
  const long long nb = lg_finish_blocks(c->dp);
  const size_t pin_bytes = sizeof(double) * (size_t)nb + sizeof(unsigned long long) * rec_words;
  DSGD_TRY(pin_acquire(c->pin_out, pin_bytes));   // (what can fail for want of memory comes before the agreement)
  LgCall q;
  DSGD_TRY(lg_agree(c, what, k, -1, &q));   // (ranks that differ ALL return DSGD_EINVAL here: nothing ran)
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(lg_nsq_if_stale(c, w || !fresh));
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(pin_acquire(c->pin_idx, sizeof(long long) * tab_words));
  memcpy(c->pin_idx.p, tab.data(), sizeof(long long) * tab_words);
  HIP_TRY(hipMemcpyAsync(c->d_lg_pred_tab, c->pin_idx.p, sizeof(long long) * tab_words, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_idx));
  HIP_TRY(hipMemsetAsync(c->d_lg_pred_tally, 0, sizeof(unsigned long long) * tally_words, c->stream));
  const int hw = lg_eval_hw(c, t.longest, 2 * lg_pred_tab_words(k));   // (the size moves no bit)
  const size_t lds = sizeof(float) * (size_t)lg_pred_lds_floats(hw, k);
  LgPredArgs a;
  a.tab = c->d_lg_pred_tab;
  a.K = k;
  a.cls = nullptr;
  a.proba = nullptr;
  a.tally = c->d_lg_pred_tally;
  a.loss_part = c->d_lg_pred_part;
  hipLaunchKernelGGL(dsgd_lg_predict_ranges_kernel, dim3((unsigned)grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_w, a, hw);
  HIP_TRY(hipGetLastError());
  LgeArgs e;
  e.first_block = c->d_lg_pred_tab;   // (the table's first array)
  e.loss_part = c->d_lg_pred_part;
  e.tally = c->d_lg_pred_tally;
  e.rec = c->d_lge_rec;
  e.k = k;
  e.K = K;
  e.first = (int)lgg_global_worker(rank, k, 0);
  hipLaunchKernelGGL(dsgd_lg_eval_fold_kernel, dim3((unsigned)k), dim3(LGE_THREADS), 0, c->stream, e);
  HIP_TRY(hipGetLastError());
  if (q.ranks) {   // the exact all-gather: every word is non-zero on at most one rank
    const int r = rccl::AllReduce(c->d_lge_rec.get(), c->d_lge_rec.get(), rec_words, rccl::kInt64, rccl::kSum, c->comm, c->stream);
    if (r) {
      lge_drop(c);
      return fail(DSGD_ERCCL, "%s: ncclAllReduce(the job's ranges): %s", what, rccl::GetErrorString(r));
    }
  }
  double* part = static_cast<double*>(c->pin_out.p.get());
  unsigned long long* rec = reinterpret_cast<unsigned long long*>(part + nb);
  int rc = DSGD_OK;
  hipError_t he = hipMemcpyAsync(part, c->d_lg_part, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, c->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(rec, c->d_lge_rec, sizeof(unsigned long long) * rec_words, hipMemcpyDeviceToHost, c->stream);
  if (he != hipSuccess) rc = fail(DSGD_EHIP, "%s: reading the record back: %s", what, hipGetErrorString(he));
  if (rc == DSGD_OK) rc = read_scalars(c);   // the one synchronisation behind the agreement
  if (rc == DSGD_OK) rc = check_err_flag(c);
  if (rc != DSGD_OK) {
    if (q.ranks) {
      char msg[sizeof(g_err)];
      snprintf(msg, sizeof(msg), "%s", g_err);
      lge_drop(c);
      return fail(rc, "%s", msg);
    }
    return rc;
  }
  c->lg_nsq_stamp = c->bind_count;
  for (int j = 0; j < k; ++j) {   // (this rank's own ranges, before anything is written)
    const unsigned long long* b = rec + lge_at(e.first + j);
    const long long rows = out_off[j + 1] - out_off[j];
    if (b[LGE_WRITERS] == 1ull && (long long)(b[LGE_RIGHT] + b[LGE_ZERO] + b[LGE_WRONG]) != rows)
      return fail(DSGD_ESTATE, "internal: %llu rows tallied of the %lld of range %d", b[LGE_RIGHT] + b[LGE_ZERO] + b[LGE_WRONG], rows, j);
  }
  double nsq = 0.0;   // (in order: the same bits on every call and every replica)
  for (long long i = 0; i < nb; ++i) nsq += part[i];
  const LgeFold f = lge_fold(rec, K, c->cfg.lambda, nsq, counts_out, range_loss_out, loss, acc);
  if (f.bad_pos >= 0)
    return fail(DSGD_ESTATE, "%s: position %d of the job's %d ranges was written by %lld ranks, not by one: the ranks do not agree about "
                             "the job (nothing was written)", what, f.bad_pos, K, f.writers);
  if (K_out) *K_out = K;
  return DSGD_OK;
}

// |w|^2 where stale, ONE launch over the n >= 1 rows c->d_idx names, the replies and the fold (entered, the weights resident, the
// list enqueued on the context's stream).  Outputs are written when everything has succeeded, idx_out (n entries) among them.
static int lg_eval_list_run(dsgd_ctx* c, long long n, bool nsq_stale, double* loss, double* acc, int64_t* counts, int32_t* idx_out) {
  DSGD_TRY(lg_ensure(c, 1));
  const long long nb = lg_finish_blocks(c->dp);
  DSGD_TRY(lg_nsq_if_stale(c, nsq_stale));
  DSGD_TRY(reset_counters(c));
  const long long grid = lg_eval_blocks(n, c->n_cu);   // (dsgd_lg_loss_acc's grid over n rows: at most n_cu words behind the |w|^2 ones)
  const int hw = lg_eval_hw(c, n, 0);
  const size_t lds = sizeof(float) * (size_t)lg_eval_lds_floats(hw);
  hipLaunchKernelGGL(dsgd_lg_eval_list_kernel, dim3((unsigned)grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_w, c->d_idx.get(), n, c->d_sc,
                     hw, c->d_lg_part + nb);
  HIP_TRY(hipGetLastError());
  const size_t words = (size_t)(nb + grid);
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(double) * words + (idx_out ? sizeof(int) * (size_t)n : 0)));
  double* part = static_cast<double*>(c->pin_out.p.get());
  int* h_idx = reinterpret_cast<int*>(part + words);
  HIP_TRY(hipMemcpyAsync(part, c->d_lg_part, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
  if (idx_out) HIP_TRY(hipMemcpyAsync(h_idx, c->d_idx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  c->lg_nsq_stamp = c->bind_count;
  long long t3[3];
  for (int j = 0; j < 3; ++j) t3[j] = (long long)c->h_sc->counts[j];
  if (t3[0] + t3[1] + t3[2] != n) return fail(DSGD_ESTATE, "internal: %lld rows tallied of %lld", t3[0] + t3[1] + t3[2], n);
  double nsq = 0.0, ls = 0.0;   // (in order: the same bits on every call)
  for (long long i = 0; i < nb; ++i) nsq += part[i];
  for (long long i = 0; i < grid; ++i) ls += part[nb + i];
  if (loss) *loss = c->cfg.lambda * nsq + ls / (double)n;   // (dsgd_lg_loss_acc's expression)
  if (acc) *acc = (double)t3[0] / (double)n;
  for (int j = 0; counts && j < 3; ++j) counts[j] = (int64_t)t3[j];
  if (idx_out) memcpy(idx_out, h_idx, sizeof(int) * (size_t)n);
  return DSGD_OK;
}

int dsgd_lg_loss_acc_list(dsgd_ctx* c, const float* w, const int32_t* idx, int64_t n, double* loss, double* acc, int64_t* counts) {
  const char* what = "dsgd_lg_loss_acc_list";
  DSGD_TRY(check_ctx(c));
  if (!idx || n < 1)   // samples.map(...).reduce on an empty collection throws (ref: SparseSVM.scala:21-23)
    return fail(DSGD_EINVAL, "%s: no list, or an empty one (reduce on an empty sample list)", what);
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, what, LG_STAYS_LOCAL, &fresh));
  const int64_t nn = n;
  const LgCheck v = lg_check_lists(&idx, &nn, 1, c->n_rows);
  DSGD_TRY(lg_report(c, what, v, 1));
  DSGD_TRY(prepare_layout(c));
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(ensure_idx(c, n));
  DSGD_TRY(send_idx(c, idx, n));
  return lg_eval_list_run(c, n, w || !fresh, loss, acc, counts, nullptr);
}

// (csrc/dsgd_hip.hip, with the SVM's dsgd_loss_acc_sampled: the first n entries of Random.shuffle(0 until len) into c->d_idx)
static int sampled_draw(dsgd_ctx* c, const char* what, unsigned long long s0, int64_t row_begin, long long len, long long n, long long* draws);

// dsgd_loss_acc_sampled word for word -- the same draw (sampled_draw as it stands), the same limits, the same refusals with
// *jstate untouched -- with the logistic family's entry checks and the logistic fold over the list
int dsgd_lg_loss_acc_sampled(dsgd_ctx* c, const float* w, uint64_t* jstate, int64_t row_begin, int64_t row_end, int64_t samples_count, double* loss,
                             double* acc, int64_t* counts, int32_t* idx_out, int64_t* n_out, int64_t* draws_out) {
  const char* what = "dsgd_lg_loss_acc_sampled";
  DSGD_TRY(check_ctx(c));
  if (!jstate) return fail(DSGD_EINVAL, "%s: null jstate", what);
  if (samples_count < 1 || row_begin >= row_end)   // (the JVM would have spent the shuffle's draws before .reduce throws; not here)
    return fail(DSGD_EINVAL, "%s: an empty sample (samples_count %lld of rows [%lld, %lld)): reduce on an empty sample list", what,
                (long long)samples_count, (long long)row_begin, (long long)row_end);
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, what, LG_STAYS_LOCAL, &fresh));
  DSGD_TRY(lg_report(c, what, lg_check_ranges(&row_begin, &row_end, 1, c->n_rows), 1));   // (the window leaves the rows: DSGD_ERANGE)
  const long long len = row_end - row_begin, n = std::min<long long>(samples_count, len);   // (the reference's `take`)
  if (len > JR_MAX_LEN)
    return fail(DSGD_EUNSUPPORTED, "%s draws windows up to %d rows (dsgd_jrand_shuffle, then dsgd_lg_loss_acc_list)", what, JR_MAX_LEN);
  DSGD_TRY(prepare_layout(c));
  const unsigned long long s0 = *jstate & JR_MASK;
  long long draws = 0;
  DSGD_TRY(sampled_draw(c, what, s0, row_begin, len, n, &draws));   // (a refusal leaves the weights as they were)
  if (w) DSGD_TRY(set_weights_locked(c, w));
  DSGD_TRY(lg_eval_list_run(c, n, w || !fresh, loss, acc, counts, idx_out));
  *jstate = jr_jump_dev(s0, (unsigned long long)draws);
  if (n_out) *n_out = n;
  if (draws_out) *draws_out = draws;
  return DSGD_OK;
}

// ---- the asynchronous iteration (include/dsgd.h "THE LOGISTIC MODEL": ASYNCHRONOUS; core/Slave.scala:79-111, 177-185) ----
// The two launches of ONE update over the n positions `seg` names in idx: lg_grad_body with K = 1 into the first slot, then the
// asynchronous finish (csrc/dsgd_logistic.hpp).  d_delta: NULL or dp doubles, rank order.  lg_ensure(c, 1) came first.
static int lg_async_launch(dsgd_ctx* c, long long n, double lr, const int* idx, const WorkSeg* seg, double* d_delta) {
  const LgCall q = lg_local(c, 1);
  LgArgs a;
  a.w = c->d_w;
  a.dp = c->dp;
  a.vexp = q.vexp;
  a.K = 1;
  a.idx = idx;
  a.segs = seg;
  a.blocks_per_worker = lg_blocks_per_worker(n, 1, c->n_cu, 2);
  a.acc = q.own;
  a.acc_stride = c->lg_stride;
  a.sc = c->d_sc;
  hipLaunchKernelGGL(dsgd_lg_grad_kernel, dim3((unsigned)a.blocks_per_worker), dim3(LG_THREADS), 0, c->stream, view(c), a);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = "dsgd_lg_grad_kernel";
  LgAsyncArgs f;
  f.acc = q.own;
  f.seg = seg;
  f.dp = c->dp;
  f.vexp = q.vexp;
  f.w = c->d_w;
  f.lr = lr;
  f.lambda = c->cfg.lambda;
  f.nsq_part = c->d_lg_part;
  f.delta = d_delta;
  hipLaunchKernelGGL(dsgd_lg_async_finish_kernel, dim3((unsigned)lg_finish_blocks(c->dp)), dim3(LG_THREADS), 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

int dsgd_lg_async_step(dsgd_ctx* c, const int32_t* idx, int64_t n, double lr, double* delta_out, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n < 1 || !idx) return fail(DSGD_EINVAL, "dsgd_lg_async_step: Cannot take the mean of an empty list of vectors");
  std::lock_guard<std::mutex> lk(c->mu);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_async_step", LG_ONE_PROCESS, &fresh));
  const int64_t nn = n;
  const LgCheck v = lg_check_lists(&idx, &nn, 1, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_async_step", v, 1));
  DSGD_TRY(prepare_layout(c));
  DSGD_TRY(lg_ensure(c, 1));
  const size_t bytes = sizeof(double) * (size_t)c->dp;
  if (delta_out) {   // everything that can fail for want of memory comes before the first launch: a failing call changes nothing
    if (c->d_lg_delta.cap() < 2 * (size_t)c->dp) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      DSGD_TRY(c->d_lg_delta.reserve(2 * (size_t)c->dp));
    }
    DSGD_TRY(pin_acquire(c->pin_out, bytes));
  }
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, &idx, &nn, 1, &mx, &tot));
  double* d_rank = delta_out ? c->d_lg_delta.get() : nullptr;
  DSGD_TRY(lg_async_launch(c, tot, lr, c->cur_idx, c->d_segs, d_rank));
  if (delta_out) {   // the delta into key order, then to the host behind the call's one synchronisation
    double* d_key = d_rank + c->dp;
    hipLaunchKernelGGL(dsgd_permute64_out_kernel, dim3((c->dp + 255) / 256), dim3(256), 0, c->stream, d_rank, d_key, c->d_perm, c->dp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->pin_out.p, d_key, bytes, hipMemcpyDeviceToHost, c->stream));
  }
  DSGD_TRY(lg_step_done(c, lg_local(c, 1), stats, tot));
  if (delta_out) memcpy(delta_out, c->pin_out.p, bytes);
  return DSGD_OK;
}

// (dsgd_lg_update_grad, the peer's side of the delta: csrc/dsgd_hip.hip, beside dsgd_update_grad)

// Updates [first_update, first_update + n_updates) of the zero-lag schedule as a ONE-worker logistic plan whose lists the device
// draws (dsgd_async_lists_kernel as it stands): dsgd_async_plan_create's arguments; any batch size.
int dsgd_async_plan_create_lg(dsgd_ctx* c, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                              uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out) {
  return async_plan_impl(c, "dsgd_async_plan_create_lg", false, true, assigned_begin, assigned_end, n_workers, batch, seed, positional_bug,
                         first_update, n_updates, out);
}
// ... additionally with its column slices laid out.  What the slices can never hold is refused here, before anything is drawn: a
// batch beyond CS_MAX_SLOTS rows, a model lg_cs_pick_G(dp, 1) finds no slice count for.  The builder's softer declines (slots,
// the plan cache) leave a plain logistic plan, whose asynchronous run is the row form's.
int dsgd_async_plan_create_lg_cs(dsgd_ctx* c, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                                 uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out) {
  const char* what = "dsgd_async_plan_create_lg_cs";
  DSGD_TRY(check_ctx(c));
  if (!assigned_begin || !assigned_end || !out || n_workers < 1 || batch < 1 || first_update < 0 || n_updates < 1)
    return fail(DSGD_EINVAL, "bad async plan arguments");
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DSGD_TRY(lg_refuse(c, what, LG_ONE_PROCESS));
    if (batch > CS_MAX_SLOTS)
      return fail(DSGD_EUNSUPPORTED, "%s: column slices take at most %d rows per update (batch %d); dsgd_async_plan_create_lg takes any", what,
                  CS_MAX_SLOTS, batch);
    if (lg_cs_pick_G(c->dp, 1) == 0)
      return fail(DSGD_EUNSUPPORTED, "%s: a model of %d features does not fit %d column slices (%d words of LDS per slice, at most %d; at "
                                     "least %d features); dsgd_async_plan_create_lg takes any", what, c->cfg.n_features, LG_CS_G,
                  lg_cs_lds_words(c->dp, LG_CS_G, 1), DSGD_LDS_FLOATS, 4 * LG_CS_G - 1);
  }
  dsgd_plan* p = nullptr;
  DSGD_TRY(dsgd_async_plan_create_lg(c, assigned_begin, assigned_end, n_workers, batch, seed, positional_bug, first_update, n_updates, &p));
  const int rc = lg_plan_add_slices(c, p);
  if (rc != DSGD_OK) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    (void)dsgd_plan_destroy(c, p);
    return fail(rc, "%s", msg);
  }
  *out = p;
  return DSGD_OK;
}

// The asynchronous iterations [step_begin, step_end) of ANY one-worker logistic plan on the resident weights: per update the two
// launches of dsgd_lg_async_step over the plan's resident lists, no host synchronisation in between -- or, where the plan's
// column slices are current, ONE launch of dsgd_lg_cs_async_kernel for the whole range.  Every refusal comes before the first
// launch.  dsgd_synchronize reports the rows.
int dsgd_plan_run_async_lg(dsgd_ctx* c, dsgd_plan* p, int64_t step_begin, int64_t step_end, double lr) {
  const char* what = "dsgd_plan_run_async_lg";
  DSGD_TRY(check_ctx(c));
  DSGD_TRY(plan_steps_check(p, step_begin, step_end));
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lg_refuse(c, what, LG_ONE_PROCESS));
  if (!p->lg) return fail(DSGD_EUNSUPPORTED, "%s: not a logistic plan (dsgd_plan_run_async_f64 runs the SVM's, on an fp64 context)", what);
  if (p->n_workers != 1)
    return fail(DSGD_EINVAL, "%s: an asynchronous iteration is one worker's: this plan has %d workers per step", what, p->n_workers);
  bool fresh = false;
  DSGD_TRY(lg_enter(c, what, LG_ONE_PROCESS, &fresh, p->lg_cs));
  DSGD_TRY(plan_revalidate(c, p));   // (a plan from before the last load: DSGD_ERANGE here, before anything is enqueued)
  DSGD_TRY(prepare_layout(c));
  const bool slices = p->lg_cs && plan_route(c, p) == PLAN_LG_CS && ensure_cs_exchange(c) == DSGD_OK;
  if (p->lg_cs && !slices) DSGD_TRY(cs_unslice(c));   // (bound with the slice-major weights kept: the row form reads d_w)
  if (!slices) DSGD_TRY(lg_ensure(c, 1));
  if (p->built_pending) {   // the plan's set-up ran beside the launch stream: wait for it, once
    HIP_TRY(hipStreamWaitEvent(c->stream, p->built_ev, 0));
    p->built_pending = false;
  }
  if (step_end <= step_begin) {
    if (fresh) c->lg_nsq_stamp = c->bind_count;   // (the weights are the ones |w|^2 was taken from)
    return DSGD_OK;
  }
  c->s_dirty = true;
  c->lg_nsq_stamp = ~0ull - 1;
  if (slices) {   // ONE launch; it leaves no |w'|^2 words: the next evaluation takes them from dsgd_lg_nsq_kernel
    DSGD_TRY(plan_run_lg_cs(c, p, step_begin, step_end, lr, true));
  } else {
    for (long long t = step_begin; t < step_end; ++t)
      DSGD_TRY(lg_async_launch(c, p->offsets[(size_t)t + 1] - p->offsets[(size_t)t], lr, p->d_idx, p->d_segs + t, nullptr));
    c->lg_nsq_stamp = c->bind_count;   // (the last finish left |w'|^2 in d_lg_part)
  }
  const long long rows = p->offsets[(size_t)step_end] - p->offsets[(size_t)step_begin];
  c->pending_samples += rows;
  c->lg_pending_active += rows;
  return DSGD_OK;
}
