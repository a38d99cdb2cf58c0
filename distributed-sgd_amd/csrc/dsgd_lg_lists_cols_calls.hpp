// Host side of the topics' and softmax's LIST steps by column lists (include/dsgd.h dsgd_lg_topics_sync_steps_cols,
// dsgd_lg_softmax_sync_steps_cols; device code: csrc/dsgd_lg_lists_cols.hpp; the owner word, the repeat check and the route:
// csrc/dsgd_lg_lists_cols_host.hpp, which tests/cpp/lg_lists_cols_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip
// inside its extern "C" block, behind dsgd_lg_softmax_calls.hpp.  The layout is the single model's over the ONE range
// [0, n_rows) (lgc_layout and its cache: made once per loaded matrix); the coefficient table is the ranges' (d_lgt_cq); the owner
// table d_lgl_owner is all LGL_NONE between steps (lgt_drop drops it with the rows it names).
//
// Checks, refusals and the single synchronisation are the list calls'.  A step the column lists cannot serve (lgl_route) runs
// through the list launches inside the same call: nothing the list call accepts is refused, and every step leaves its bits.

// the coefficients of the step's K lists, by the ENTRY POINT's model (softmax: dsgd_lg_softmax_sync_steps_cols; the topics' call
// serves classes as one-vs-rest on their one-hot planes, as every dsgd_lg_topics_* call does) and the context's form
static int lgl_launch_coef(dsgd_ctx* c, bool softmax, int K, long long longest, const WorkSeg* segs, long long base) {
  LglCoefArgs q;
  q.wi = c->d_lgt_w;
  q.pi = c->d_lgt_planes;
  q.T = c->lgt_T;
  q.tp = lgti_tp(c->lgt_T);
  q.vexp = c->vexp;
  q.K = K;
  q.idx = c->d_idx;
  q.segs = segs;
  q.base = base;
  const int gw = lgtw_group_width(q.tp);
  q.blocks_per_worker = lgtw_blocks_per_worker(longest, K, c->n_cu, gw);   // (lgtc_coef_args' grid)
  q.cq = c->d_lgt_cq;
  q.sc = c->d_sc;
  const dim3 grid((unsigned)(q.blocks_per_worker * K)), th(LG_THREADS);
#define LGL_COEF(KERNEL, P) hipLaunchKernelGGL(KERNEL<P>, grid, th, 0, c->stream, view(c), q)
  if (softmax && !c->lgt_wide) {
    const int nq = lgsi_quads(q.tp);
    if (nq == 1) LGL_COEF(dsgd_lgl_smax_few_coef_kernel, 1);
    else if (nq == 2) LGL_COEF(dsgd_lgl_smax_few_coef_kernel, 2);
    else if (nq == 4) LGL_COEF(dsgd_lgl_smax_few_coef_kernel, 4);
    else LGL_COEF(dsgd_lgl_smax_few_coef_kernel, 8);
  } else if (softmax) {
    if (gw == 16) LGL_COEF(dsgd_lgl_smax_coef_kernel, 16);
    else if (gw == 32) LGL_COEF(dsgd_lgl_smax_coef_kernel, 32);
    else LGL_COEF(dsgd_lgl_smax_coef_kernel, 64);
  } else {
    if (gw == 16) LGL_COEF(dsgd_lgl_topics_coef_kernel, 16);
    else if (gw == 32) LGL_COEF(dsgd_lgl_topics_coef_kernel, 32);
    else LGL_COEF(dsgd_lgl_topics_coef_kernel, 64);
  }
#undef LGL_COEF
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// the FIVE launches of one step over the K lists `segs` of c->d_idx, by the matrix's layout
static int lgl_launch(dsgd_ctx* c, bool softmax, int K, const dsgd_ctx::LgColsLayout& L, long long longest, float lr, const WorkSeg* segs, long long base) {
  LglMarkArgs m;
  m.idx = c->d_idx;
  m.segs = segs;
  m.base = base;
  m.n_rows = c->n_rows;
  m.blocks_per_worker = lgl_mark_blocks(longest, K, c->n_cu);
  m.owner = c->d_lgl_owner;
  m.sc = c->d_sc;
  const dim3 mgrid((unsigned)m.blocks_per_worker, (unsigned)K), mth(LGL_THREADS);
  hipLaunchKernelGGL(dsgd_lgl_mark_kernel, mgrid, mth, 0, c->stream, m);
  HIP_TRY(hipGetLastError());
  DSGD_TRY(lgl_launch_coef(c, softmax, K, longest, segs, base));
  const int tp = lgti_tp(c->lgt_T), gw = lgtw_group_width(tp);
  LglGradArgs q;
  q.g.ent = L.d_ent;
  q.g.shares = L.d_shares;
  q.g.slot_of_cid = L.d_slot_of_cid;
  q.g.cq = c->d_lgt_cq;
  q.g.acc = c->d_lgt_acc;
  q.g.acc_stride = lgti_acc_stride(c->dp, tp);
  q.g.n_ent = L.n_ent;
  q.g.share = L.share;
  q.g.tp = tp;
  q.g.lg_stride = (unsigned int)c->lg_stride;
  q.owner = c->d_lgl_owner;
  const dim3 ggrid((unsigned)L.n_wg, (unsigned)K), gth(LGC_THREADS);
  if (gw == 16) hipLaunchKernelGGL(dsgd_lgl_cgrad_kernel<16>, ggrid, gth, 0, c->stream, q);
  else if (gw == 32) hipLaunchKernelGGL(dsgd_lgl_cgrad_kernel<32>, ggrid, gth, 0, c->stream, q);
  else hipLaunchKernelGGL(dsgd_lgl_cgrad_kernel<64>, ggrid, gth, 0, c->stream, q);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = "dsgd_lgl_cgrad_kernel";
  DSGD_TRY(c->lgt_wide ? lgtw_launch_finish(c, K, lr, segs) : lgti_launch_finish(c, K, lr, segs));
  hipLaunchKernelGGL(dsgd_lgl_clear_kernel, mgrid, mth, 0, c->stream, m);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// the matrix's layout, the coefficient table for `positions` rows and the owner table: false = not to be had (the list form serves)
static int lgl_tables(dsgd_ctx* c, long long positions, const dsgd_ctx::LgColsLayout** out, bool* ok) {
  *ok = false;
  const int64_t zero = 0, rows = c->n_rows;
  const long long words = lgtc_table_words(positions, lgti_tp(c->lgt_T));
  if (words < 0) return DSGD_OK;
  DSGD_TRY(lg_ensure(c, 1));   // (lg_stride, the unit of the layout's slot words)
  if (!c->lgc_cache.find({0, (long long)rows}, 0, c->layout_gen))   // (lgc_layout's key: a cached layout needs no ranges in d_segs)
    DSGD_TRY(lg_upload_ranges(c, &zero, &rows, 1));                // (what lgc_layout lays out; the list steps read d_lgt_ssegs)
  dsgd_ctx::LgColsLayout* L = nullptr;
  const int lrc = lgc_layout(c, &zero, &rows, 1, rows, &L);
  if (lrc == 1) return DSGD_OK;
  if (lrc != DSGD_OK) return lrc;
  if (c->d_lgt_cq.cap() < (size_t)words || c->d_lgl_owner.cap() < (size_t)rows) HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->d_lgt_cq.cap() < (size_t)words && c->d_lgt_cq.try_alloc((size_t)words) != hipSuccess) {
    (void)hipGetLastError();
    return DSGD_OK;
  }
  if (c->d_lgl_owner.cap() < (size_t)rows) {
    if (c->d_lgl_owner.try_alloc((size_t)rows) != hipSuccess) {
      (void)hipGetLastError();
      return DSGD_OK;
    }
    HIP_TRY(hipMemsetAsync(c->d_lgl_owner, 0xff, sizeof(unsigned int) * (size_t)rows, c->stream));   // every word LGL_NONE
  }
  *out = L;
  *ok = true;
  return DSGD_OK;
}

typedef int (*LglListLaunch)(dsgd_ctx*, int, long long, float, const int*, const WorkSeg*);
static int lgl_steps(dsgd_ctx* c, const char* what, bool softmax, LgtEnter enter, LglListLaunch list_launch, const int32_t* idx, int64_t n_idx,
                     const int64_t* offsets, int64_t n_steps, int32_t n_workers, float lr, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || n_steps < 1 || n_workers < 1 || n_idx < 1)
    return fail(DSGD_EINVAL, "%s: bad arguments (null lists, no steps or no workers)", what);
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(enter(c, what));
  const int K = n_workers;
  const LgCheck v = lgt_check_steps(idx, n_idx, offsets, n_steps, K, c->n_rows);
  DSGD_TRY(lg_report(c, what, v, K));
  DSGD_TRY(lgt_ready(c, what));
  if (!c->lgt_il)
    return fail(DSGD_EUNSUPPORTED, "%s: the topics are in the planar form (dsgd_lg_topics_set): the column lists serve the topics of "
                                   "dsgd_lg_topics_set_il and dsgd_lg_topics_set_wide (dsgd_lg_topics_sync_steps serves these)", what);
  // what serves each step: known on the host, before anything is allocated or enqueued
  std::vector<LglRoute> route((size_t)n_steps);
  long long most = 0;
  {
    std::vector<uint64_t> seen((size_t)lgl_seen_words(c->n_rows), 0);
    for (int64_t t = 0; t < n_steps; ++t) {
      const long long b = offsets[t * K], e = offsets[(t + 1) * K];
      const bool fits = lgl_route(e - b, K, false, true) == LGL_COLS;   // (a step beyond the limits is not walked again)
      route[(size_t)t] = lgl_route(e - b, K, fits && lgl_step_repeats(idx, b, e, seen.data()), true);
      if (route[(size_t)t] == LGL_COLS) most = std::max(most, e - b);
    }
  }
  const int64_t n_lists = n_steps * K;
  DSGD_TRY(lgt_ensure(c, K));
  if (c->d_lgt_ssegs.cap() < (size_t)n_lists) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lgt_ssegs.reserve((size_t)n_lists));
  }
  DSGD_TRY(reset_counters(c));
  const dsgd_ctx::LgColsLayout* L = nullptr;
  if (most > 0) {
    bool ok = false;
    DSGD_TRY(lgl_tables(c, most, &L, &ok));
    if (!ok)
      for (auto& r : route) r = lgl_route(0, K, false, false);
  }
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
  HIP_TRY(hipMemcpyAsync(c->d_lgt_ssegs, c->pin_segs.p, sizeof(WorkSeg) * (size_t)n_lists, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_segs));
  // five launches per step (the list form's two), back to back on the stream: no host synchronisation in between
  int rc = DSGD_OK;
  for (int64_t t = 0; t < n_steps && rc == DSGD_OK; ++t) {
    long long mx = 0;
    for (int k = 0; k < K; ++k) mx = std::max<long long>(mx, offsets[t * K + k + 1] - offsets[t * K + k]);
    if (route[(size_t)t] == LGL_COLS) {
      rc = lgl_launch(c, softmax, K, *L, mx, lr, c->d_lgt_ssegs + t * K, offsets[t * K]);
    } else {
      c->last_grad_kernel = c->lgt_wide ? "dsgd_lg_topics_wide_grad_kernel" : "dsgd_lg_topics_il_grad_kernel";   // (softmax's launch names its own)
      rc = list_launch(c, K, mx, lr, c->d_idx, c->d_lgt_ssegs + t * K);
    }
  }
  rc = lgt_step_done(c, rc, stats, n_idx);
  if (rc != DSGD_OK) c->d_lgl_owner.reset();   // (behind lgt_step_done's synchronisation: a step may have stopped between mark and clear)
  return rc;
}

int dsgd_lg_topics_sync_steps_cols(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                                   float lr, dsgd_batch_stats* stats) {
  return lgl_steps(c, "dsgd_lg_topics_sync_steps_cols", false, lgt_enter, lgt_launch, idx, n_idx, offsets, n_steps, n_workers, lr, stats);
}

int dsgd_lg_softmax_sync_steps_cols(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                                    float lr, dsgd_batch_stats* stats) {
  return lgl_steps(c, "dsgd_lg_softmax_sync_steps_cols", true, lgsm_enter, lgsm_launch, idx, n_idx, offsets, n_steps, n_workers, lr, stats);
}
