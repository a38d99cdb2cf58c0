// Host side of SOFTMAX regression over the wide topic layout (include/dsgd.h "THE LOGISTIC MODEL": SOFTMAX; device code:
// csrc/dsgd_lg_softmax.hpp; sizes, checks and the order of the host's sums: csrc/dsgd_lg_softmax_host.hpp, which
// tests/cpp/lg_softmax_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip inside its extern "C" block, behind
// dsgd_lg_topics_cols_calls.hpp: the dsgd_lg_softmax_* entry points, one function per launch site; the steps run the topics' shared bodies.  The context's blocks are the
// wide topics' (dsgd_lg_topics_set_wide's body lays them out from the one-hot planes), so dsgd_lg_topics_set_weights /
// _get_weights carry the weights and every dsgd_lg_topics_* call keeps serving the context as one-vs-rest on those planes; only
// the mark c->lgt_softmax and the launches below are this model's.  Classes set by dsgd_lg_softmax_set_il (interleaved and not
// wide: csrc/dsgd_lg_softmax_il_calls.hpp) are served by the same calls: each launch function below hands them to its lgsi_ side.
//
// Every check runs on the host before anything of the call is enqueued: a refused call leaves the classes, the weights and the
// context's flags as they were.  Every call returns behind its kernels (ONE synchronisation).

// what every softmax call but dsgd_lg_softmax_set asks first (locked): the topic calls' rules with a running lock-free engine
// refused as a mode (DSGD_EUNSUPPORTED), then classes set BY dsgd_lg_softmax_set
static int lgsm_enter(dsgd_ctx* c, const char* what) {
  if (c->async_running)
    return fail(DSGD_EUNSUPPORTED, "%s is not available while the lock-free engine runs (dsgd_async_stop / dsgd_async_wait first)", what);
  DSGD_TRY(lgt_enter(c, what));
  if (!c->lgt_softmax)
    return fail(DSGD_ESTATE, "%s: the context's topics are not classes (dsgd_lg_softmax_set; any dsgd_lg_topics_set* replaces them)", what);
  return DSGD_OK;
}

int dsgd_lg_softmax_set(dsgd_ctx* c, int32_t C, const uint8_t* cls) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  if (lgsm_check_set(C, nullptr, 0).kind == LGSM_BAD_C)   // (C alone: in range before anything else is looked at)
    return fail(DSGD_ERANGE, "dsgd_lg_softmax_set: %d classes, outside {0} and [%d, %d]", (int)C, LG_SOFTMAX_MIN, LG_SOFTMAX_MAX);
  if (c->async_running)
    return fail(DSGD_EUNSUPPORTED, "dsgd_lg_softmax_set is not available while the lock-free engine runs (dsgd_async_stop / dsgd_async_wait first)");
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_softmax_set", LG_ONE_PROCESS, &fresh));
  if (C == 0) {
    lgt_drop(c);
    return DSGD_OK;
  }
  const LgsmCheck v = lgsm_check_set(C, cls, c->n_rows);
  switch (v.kind) {
    case LGSM_OK: break;
    case LGSM_BAD_C: return fail(DSGD_ERANGE, "dsgd_lg_softmax_set: %d classes", (int)C);
    case LGSM_NULL: return fail(DSGD_EINVAL, "dsgd_lg_softmax_set: null classes");
    case LGSM_NO_ROWS: return fail(DSGD_ESTATE, "dsgd_lg_softmax_set: no rows loaded");
    case LGSM_ENTRY: return fail(DSGD_ERANGE, "dsgd_lg_softmax_set: row %lld has class %d of %d", v.row, v.value, (int)C);
  }
  std::vector<int8_t> planes((size_t)C * (size_t)c->n_rows);
  lgsm_one_hot(cls, C, c->n_rows, planes.data());
  DSGD_TRY(lgtw_install(c, C, planes.data()));
  c->lgt_softmax = true;
  return DSGD_OK;
}

// how many classes are set now (0: none, or topics that are not classes)
int dsgd_lg_softmax_count(dsgd_ctx* c, int32_t* C_out) {
  DSGD_TRY(check_ctx(c));
  if (!C_out) return fail(DSGD_EINVAL, "dsgd_lg_softmax_count: null C_out");
  std::lock_guard<std::mutex> lk(c->mu);
  *C_out = c->lgt_softmax && c->lgt_T && c->layout_ready && c->lgt_gen == c->layout_gen ? c->lgt_T : 0;
  return DSGD_OK;
}

// The TWO launches of one step over K lists, whatever C: the wide form's arguments and finish around the softmax gradient
static int lgsm_launch(dsgd_ctx* c, int K, long long longest, float lr, const int* idx, const WorkSeg* segs) {
  if (!c->lgt_wide) return lgsi_launch(c, K, longest, lr, idx, segs);   // (classes set by dsgd_lg_softmax_set_il)
  const LgtiArgs a = lgtw_grad_args(c, K, longest, idx, segs);
  const int gw = lgtw_group_width(a.tp);
  const dim3 grid((unsigned)(a.blocks_per_worker * K)), th(LG_THREADS);
  if (gw == 16) hipLaunchKernelGGL(dsgd_lg_softmax_grad_kernel<16>, grid, th, 0, c->stream, view(c), a);
  else if (gw == 32) hipLaunchKernelGGL(dsgd_lg_softmax_grad_kernel<32>, grid, th, 0, c->stream, view(c), a);
  else hipLaunchKernelGGL(dsgd_lg_softmax_grad_kernel<64>, grid, th, 0, c->stream, view(c), a);
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = "dsgd_lg_softmax_grad_kernel";
  return lgtw_launch_finish(c, K, lr, segs);
}

// the THREE launches of one step over the ranges in c->d_segs, by their layout: the softmax coefficients, then the topics'
// column-wise gradient and the wide finish as they are
static int lgsm_launch_ranges(dsgd_ctx* c, int K, const dsgd_ctx::LgColsLayout& L, long long longest, float lr) {
  if (!c->lgt_wide) return lgsi_launch_ranges(c, K, L, longest, lr);
  const LgtcCoefArgs q = lgtc_coef_args(c, K, L, longest);
  const int gw = lgtw_group_width(q.tp);
  const dim3 cgrid((unsigned)(q.blocks_per_worker * K)), th(LG_THREADS);
  if (gw == 16) hipLaunchKernelGGL(dsgd_lg_softmax_coef_kernel<16>, cgrid, th, 0, c->stream, view(c), q);
  else if (gw == 32) hipLaunchKernelGGL(dsgd_lg_softmax_coef_kernel<32>, cgrid, th, 0, c->stream, view(c), q);
  else hipLaunchKernelGGL(dsgd_lg_softmax_coef_kernel<64>, cgrid, th, 0, c->stream, view(c), q);
  HIP_TRY(hipGetLastError());
  return lgtc_launch_grad_finish(c, K, L, lr);
}

// The list steps follow dsgd_lg_topics_sync_step / _sync_steps line for line behind lgsm_enter, with lgsm_launch (those two keep their
// checks in their own text, which tests/test_lg_topics_host.py reads); over ranges the body is the topics' own (lgtc_steps), and
// there is NO row-form fallback, as for the topics.
int dsgd_lg_softmax_sync_step(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers, float lr,
                             dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !idx_per_worker || !n_per_worker)
    return fail(DSGD_EINVAL, "dsgd_lg_softmax_sync_step: Cannot sum an empty list of vectors (no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgsm_enter(c, "dsgd_lg_softmax_sync_step"));
  const LgCheck v = lgt_check_step(idx_per_worker, n_per_worker, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_softmax_sync_step", v, n_workers));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_softmax_sync_step"));
  DSGD_TRY(lgt_ensure(c, n_workers));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
  return lgt_step_done(c, lgsm_launch(c, n_workers, mx, lr, c->cur_idx, c->d_segs), stats, tot);
}

int dsgd_lg_softmax_sync_steps(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers, float lr,
                              dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || n_steps < 1 || n_workers < 1 || n_idx < 1)
    return fail(DSGD_EINVAL, "dsgd_lg_softmax_sync_steps: bad arguments (null lists, no steps or no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgsm_enter(c, "dsgd_lg_softmax_sync_steps"));
  const int K = n_workers;
  const LgCheck v = lgt_check_steps(idx, n_idx, offsets, n_steps, K, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_softmax_sync_steps", v, K));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_softmax_sync_steps"));
  const int64_t n_lists = n_steps * K;
  DSGD_TRY(lgt_ensure(c, K));
  if (c->d_lgt_ssegs.cap() < (size_t)n_lists) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lgt_ssegs.reserve((size_t)n_lists));
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
  HIP_TRY(hipMemcpyAsync(c->d_lgt_ssegs, c->pin_segs.p, sizeof(WorkSeg) * (size_t)n_lists, hipMemcpyHostToDevice, c->stream));
  DSGD_TRY(pin_sent(c, c->pin_segs));
  // two launches per step whatever T, back to back on the stream: no host synchronisation in between
  int rc = DSGD_OK;
  for (int64_t t = 0; t < n_steps && rc == DSGD_OK; ++t) {
    long long mx = 0;
    for (int k = 0; k < K; ++k) mx = std::max<long long>(mx, offsets[t * K + k + 1] - offsets[t * K + k]);
    rc = lgsm_launch(c, K, mx, lr, c->d_idx, c->d_lgt_ssegs + t * K);
  }
  return lgt_step_done(c, rc, stats, n_idx);
}

int dsgd_lg_softmax_sync_steps_ranges(dsgd_ctx* c, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, int64_t n_steps, float lr,
                                      dsgd_batch_stats* stats) {
  return lgtc_steps(c, "dsgd_lg_softmax_sync_steps_ranges", lgsm_enter, lgsm_launch_ranges, row_begin, row_end, n_workers, n_steps, lr, stats);
}

// the evaluation of rows [row_begin, row_end) in `grid` workgroups with a tile of hw ranks, by the context's form: the loss words into `part`
static int lgsm_launch_eval(dsgd_ctx* c, long long row_begin, long long row_end, long long grid, int hw, double* part) {
  if (!c->lgt_wide) return lgsi_launch_eval(c, row_begin, row_end, grid, hw, part);
  const int C = c->lgt_T;
  const size_t lds = sizeof(float) * (size_t)lgsm_eval_lds_floats(hw, C);
  const dim3 g((unsigned)grid), th(LGSM_EVAL_THREADS);
  const int gw = lgtw_group_width(lgti_tp(C));
#define LGSM_EVAL(GW)                                                                                                                         \
  hipLaunchKernelGGL(dsgd_lg_softmax_eval_kernel<GW>, g, th, lds, c->stream, view(c), c->d_lgt_w.get(), c->d_lgt_planes.get(), C, row_begin, \
                     row_end, c->d_lgt_tally.get(), hw, part)
  if (gw == 16) LGSM_EVAL(16);
  else if (gw == 32) LGSM_EVAL(32);
  else LGSM_EVAL(64);
#undef LGSM_EVAL
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// the classes (and, where dp_out is not null, the probabilities) of the n rows in c->d_idx, by the context's form
static int lgsm_launch_predict(dsgd_ctx* c, long long n, float* dp_out) {
  if (!c->lgt_wide) return lgsi_launch_predict(c, n, dp_out);
  const int C = c->lgt_T;
  const int gw = lgtw_group_width(lgti_tp(C));
  const dim3 g((unsigned)grid_for(c, n, gw)), th(LG_THREADS);
#define LGSM_PREDICT(GW)                                                                                                  \
  hipLaunchKernelGGL(dsgd_lg_softmax_predict_kernel<GW>, g, th, 0, c->stream, view(c), c->d_lgt_w.get(), C, c->d_idx.get(), n, \
                     c->d_lgsm_cls.get(), dp_out, c->d_sc.get())
  if (gw == 16) LGSM_PREDICT(16);
  else if (gw == 32) LGSM_PREDICT(32);
  else LGSM_PREDICT(64);
#undef LGSM_PREDICT
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

int dsgd_lg_softmax_loss_acc(dsgd_ctx* c, int64_t row_begin, int64_t row_end, double* loss, double* acc) {
  DSGD_TRY(check_ctx(c));
  if (!loss && !acc) return fail(DSGD_EINVAL, "dsgd_lg_softmax_loss_acc: null loss and acc");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgsm_enter(c, "dsgd_lg_softmax_loss_acc"));
  const LgCheck v = lgt_check_range(row_begin, row_end, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_softmax_loss_acc", v, 1));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_softmax_loss_acc"));
  const int C = c->lgt_T;
  if (c->lgt_nsq_stale) DSGD_TRY(c->lgt_wide ? lgtw_launch_nsq(c) : lgti_launch_nsq(c));   // |w_c|^2 of weights the finish did not write: the finish's grid and tree
  DSGD_TRY(reset_counters(c));
  HIP_TRY(hipMemsetAsync(c->d_lgt_tally, 0, sizeof(unsigned long long) * (size_t)C * LG_TALLY_WORDS, c->stream));
  const long long rows = row_end - row_begin;
  const long long grid = lgsm_eval_blocks(rows, c->n_cu);
  const int hw = lgsm_eval_hw(rows, std::min(c->hw_eval, c->dp), C);
  double* part = c->d_lgt_part + lgt_loss_at(C, 0, c->dp, c->n_cu);   // (the first class's n_cu loss words: grid <= n_cu)
  DSGD_TRY(lgsm_launch_eval(c, row_begin, row_end, grid, hw, part));
  const size_t words = (size_t)lgt_part_words(C, c->dp, c->n_cu), tally_words = LG_TALLY_WORDS;
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(double) * words + sizeof(unsigned long long) * tally_words));
  double* hpart = static_cast<double*>(c->pin_out.p.get());
  unsigned long long* tally = reinterpret_cast<unsigned long long*>(hpart + words);
  HIP_TRY(hipMemcpyAsync(hpart, c->d_lgt_part, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tally, c->d_lgt_tally, sizeof(unsigned long long) * tally_words, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  c->lgt_nsq_stale = false;
  lgsm_fold(hpart, tally, C, c->dp, c->n_cu, grid, rows, c->cfg.lambda, loss, acc);
  return DSGD_OK;
}

int dsgd_lg_softmax_predict(dsgd_ctx* c, const int32_t* idx, int64_t n, uint8_t* cls_out, float* p_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 1 || !idx || !cls_out) return fail(DSGD_EINVAL, "dsgd_lg_softmax_predict: bad arguments (a null pointer or no rows)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgsm_enter(c, "dsgd_lg_softmax_predict"));
  const LgCheck v = lgt_check_list(idx, n, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_softmax_predict", v, 1));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_softmax_predict"));
  const int C = c->lgt_T;
  const size_t out = p_out ? (size_t)C * (size_t)n : 0;
  DSGD_TRY(ensure_idx(c, n));
  if (out > c->d_lgt_p.cap() || (size_t)n > c->d_lgsm_cls.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out) DSGD_TRY(c->d_lgt_p.reserve(std::max<size_t>(out, 4096)));
    DSGD_TRY(c->d_lgsm_cls.reserve(std::max<size_t>((size_t)n, 4096)));
  }
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(send_idx(c, idx, n));
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(float) * out + (size_t)n));
  DSGD_TRY(lgsm_launch_predict(c, n, p_out ? c->d_lgt_p.get() : nullptr));
  char* host = static_cast<char*>(c->pin_out.p.get());
  if (out) HIP_TRY(hipMemcpyAsync(host, c->d_lgt_p, sizeof(float) * out, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(host + sizeof(float) * out, c->d_lgsm_cls, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));
  DSGD_TRY(check_err_flag(c));
  if (out) memcpy(p_out, host, sizeof(float) * out);
  memcpy(cls_out, host + sizeof(float) * out, (size_t)n);
  return DSGD_OK;
}
