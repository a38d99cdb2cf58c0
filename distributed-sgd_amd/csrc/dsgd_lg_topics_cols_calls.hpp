// Host side of the topics' whole-split steps by column lists (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS, ROW RANGES;
// device code: csrc/dsgd_lg_topics_cols.hpp; sizes and limits: csrc/dsgd_lg_topics_cols_host.hpp, which
// tests/cpp/lg_topics_cols_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip inside its extern "C" block, behind
// dsgd_lg_topics_calls.hpp: dsgd_lg_topics_sync_step_ranges and dsgd_lg_topics_sync_steps_ranges, one function per launch site.
// The layout of the entries is the single model's (lgc_layout and its cache, csrc/dsgd_lg_calls.hpp): a configuration laid out
// for either serves both.  The coefficient table cq[position][TP] is the context's own (d_lgt_cq; lgt_drop drops it).

// what the coefficients of the ranges in c->d_segs are launched with (dsgd_lg_topics_coef_kernel and dsgd_lg_softmax_coef_kernel alike)
static LgtcCoefArgs lgtc_coef_args(dsgd_ctx* c, int K, const dsgd_ctx::LgColsLayout& L, long long longest) {
  const int tp = lgti_tp(c->lgt_T);
  LgtcCoefArgs q;
  q.wi = c->d_lgt_w;
  q.pi = c->d_lgt_planes;
  q.T = c->lgt_T;
  q.tp = tp;
  q.vexp = c->vexp;
  q.K = K;
  q.segs = c->d_segs;
  q.pos_base = L.d_pos_base;
  q.blocks_per_worker = lgtw_blocks_per_worker(longest, K, c->n_cu, lgtw_group_width(tp));
  q.cq = c->d_lgt_cq;
  q.sc = c->d_sc;
  return q;
}
// the column-wise gradient from the coefficient table and the form's finish: the step's second and third launch
static int lgtc_launch_grad_finish(dsgd_ctx* c, int K, const dsgd_ctx::LgColsLayout& L, float lr) {
  const int tp = lgti_tp(c->lgt_T), gw = lgtw_group_width(tp);
  const dim3 th(LG_THREADS);
  LgtcGradArgs g;
  g.ent = L.d_ent;
  g.shares = L.d_shares;
  g.slot_of_cid = L.d_slot_of_cid;
  g.cq = c->d_lgt_cq;
  g.acc = c->d_lgt_acc;
  g.acc_stride = lgti_acc_stride(c->dp, tp);
  g.n_ent = L.n_ent;
  g.share = L.share;
  g.tp = tp;
  g.lg_stride = (unsigned int)c->lg_stride;   // (the layout's words are `worker * lg_stride + rank`; below 2^31: lgc_plan)
  const dim3 ggrid((unsigned)L.n_wg), gth(LGC_THREADS);
  if (gw == 16) hipLaunchKernelGGL(dsgd_lg_topics_cgrad_kernel<16>, ggrid, gth, 0, c->stream, g);
  else if (gw == 32) hipLaunchKernelGGL(dsgd_lg_topics_cgrad_kernel<32>, ggrid, gth, 0, c->stream, g);
  else hipLaunchKernelGGL(dsgd_lg_topics_cgrad_kernel<64>, ggrid, gth, 0, c->stream, g);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = "dsgd_lg_topics_cgrad_kernel";
  LgtiFinishArgs f = lgti_finish_args(c);
  f.acc = c->d_lgt_acc;
  f.acc_stride = g.acc_stride;
  f.segs = c->d_segs;
  f.K = K;
  f.lr = (double)lr;
  const dim3 fgrid((unsigned)lg_finish_blocks(c->dp));
  if (c->lgt_wide) hipLaunchKernelGGL(dsgd_lg_topics_wide_finish_kernel<true>, fgrid, th, 0, c->stream, f);
  else hipLaunchKernelGGL(dsgd_lg_topics_il_finish_kernel<true>, fgrid, th, 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
// the THREE launches of one step over the ranges in c->d_segs, by their layout
static int lgtc_launch(dsgd_ctx* c, int K, const dsgd_ctx::LgColsLayout& L, long long longest, float lr) {
  const LgtcCoefArgs q = lgtc_coef_args(c, K, L, longest);
  const int gw = lgtw_group_width(q.tp);
  const dim3 cgrid((unsigned)(q.blocks_per_worker * K)), th(LG_THREADS);
  if (gw == 16) hipLaunchKernelGGL(dsgd_lg_topics_coef_kernel<16>, cgrid, th, 0, c->stream, view(c), q);
  else if (gw == 32) hipLaunchKernelGGL(dsgd_lg_topics_coef_kernel<32>, cgrid, th, 0, c->stream, view(c), q);
  else hipLaunchKernelGGL(dsgd_lg_topics_coef_kernel<64>, cgrid, th, 0, c->stream, view(c), q);
  HIP_TRY(hipGetLastError());
  return lgtc_launch_grad_finish(c, K, L, lr);
}

// both calls (the one-step call is n_steps = 1 of the other).  There is NO row-form fallback over ranges for the topics: where no
// layout can be had the call fails, before any weight moves.
// (shared with dsgd_lg_softmax_sync_steps_ranges: `enter` is what the call asks first, `launch` one step's three launches)
typedef int (*LgtEnter)(dsgd_ctx*, const char*);
typedef int (*LgtcLaunch)(dsgd_ctx*, int, const dsgd_ctx::LgColsLayout&, long long, float);
static int lgtc_steps(dsgd_ctx* c, const char* what, LgtEnter enter, LgtcLaunch launch, const int64_t* row_begin, const int64_t* row_end,
                      int32_t n_workers, int64_t n_steps, float lr, dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !row_begin || !row_end) return fail(DSGD_EINVAL, "%s: Cannot sum an empty list of vectors (no workers)", what);
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(enter(c, what));
  const LgCheck v = lg_check_ranges(row_begin, row_end, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, what, v, n_workers));
  if (n_steps < 1) return fail(DSGD_EINVAL, "%s: %lld steps", what, (long long)n_steps);
  DSGD_TRY(lgt_ready(c, what));
  if (!c->lgt_il)
    return fail(DSGD_ESTATE, "%s: the topics are in the planar form (dsgd_lg_topics_set): row ranges serve the topics of "
                             "dsgd_lg_topics_set_il and dsgd_lg_topics_set_wide", what);
  const int K = n_workers, tp = lgti_tp(c->lgt_T);
  // what lgc_layout would decline, and the table's size: known on the host, before anything is allocated or enqueued
  long long n_ent = 0;
  for (int k = 0; k < K; ++k) n_ent += c->h_row_ptr[(size_t)row_end[k]] - c->h_row_ptr[(size_t)row_begin[k]];
  DSGD_TRY(lg_ensure(c, 1));   // (lg_stride, the unit of the layout's slot words: the single model's, whoever lays the ranges out)
  LgcPlan plan;
  std::vector<long long> base((size_t)K);
  const LgcFault pf = lgc_plan(row_begin, row_end, K, n_ent, c->dp, c->lg_stride, c->n_cu, &plan, base.data());
  const long long words = pf == LGC_OK ? lgtc_table_words(plan.positions, tp) : -1;
  if (const char* why = lgtc_refusal(pf, words))
    return fail(DSGD_EUNSUPPORTED, "%s: these ranges cannot be laid out by column (%s): the topics have no row form over ranges "
                                   "(dsgd_lg_topics_sync_steps over lists serves any rows)", what, why);
  DSGD_TRY(lgt_ensure(c, K));
  if (c->d_lgt_cq.cap() < (size_t)words) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_lgt_cq.try_alloc((size_t)words) != hipSuccess) {
      (void)hipGetLastError();
      return fail(DSGD_ENOMEM, "%s: no device memory for the coefficient table (%lld bytes)", what, 8 * words);
    }
  }
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(lg_upload_ranges(c, row_begin, row_end, K));
  dsgd_ctx::LgColsLayout* L = nullptr;
  const int lrc = lgc_layout(c, row_begin, row_end, K, v.longest, &L);
  if (lrc == 1) return fail(DSGD_ENOMEM, "%s: no device memory for the column lists of these ranges", what);   // (the plan passed above)
  if (lrc != DSGD_OK) return lrc;
  // three launches per step, back to back on the stream: no host synchronisation in between
  int rc = DSGD_OK;
  for (int64_t t = 0; t < n_steps && rc == DSGD_OK; ++t) rc = launch(c, K, *L, v.longest, lr);
  rc = lgt_step_done(c, rc, stats, v.total);
  return rc;
}

int dsgd_lg_topics_sync_step_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, float lr,
                                    dsgd_batch_stats* stats) {
  return lgtc_steps(c, "dsgd_lg_topics_sync_step_ranges", lgt_enter, lgtc_launch, row_begin, row_end, n_workers, 1, lr, stats);
}

int dsgd_lg_topics_sync_steps_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, int64_t n_steps, float lr,
                                     dsgd_batch_stats* stats) {
  return lgtc_steps(c, "dsgd_lg_topics_sync_steps_ranges", lgt_enter, lgtc_launch, row_begin, row_end, n_workers, n_steps, lr, stats);
}
