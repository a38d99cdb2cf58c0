// Host side of the logistic model over SEVERAL TOPICS (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS; device code:
// csrc/dsgd_lg_topics.hpp; every check, size and the order of the host's sums: csrc/dsgd_lg_topics_host.hpp, which
// tests/cpp/lg_topics_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip inside its extern "C" block, behind
// dsgd_lg_calls.hpp, whose lg_enter and lg_report it uses.
//
// Every check runs on the host before anything of the call is enqueued: a refused call leaves the topics, the context's own
// weights and labels and its flags as they were.  Every call returns behind its kernels (ONE synchronisation).

// the topics go: with the rows they label (dsgd_load_csr), by T = 0, or when the column ranking they are stored in went
static void lgt_drop(dsgd_ctx* c) {
  if (c->lgt_T) (void)hipStreamSynchronize(c->stream);
  c->lgt_T = 0;
  c->lgt_k = 0;
  c->d_lgt_planes.reset();
  c->d_lgt_w.reset();
  c->d_lgt_acc.reset();
  c->d_lgt_part.reset();
  c->d_lgt_tally.reset();
  c->d_lgt_p.reset();
  c->d_lgt_ssegs.reset();
}

// what every topic call but dsgd_lg_topics_set asks first (locked): lg_enter's rules, ANY communicator refused, topics set.
// Nothing of the topics changes here.
static int lgt_enter(dsgd_ctx* c, const char* what) {
  bool fresh = false;
  DSGD_TRY(lg_enter(c, what, LG_ONE_PROCESS, &fresh));   // (LG_ONE_PROCESS: ANY communicator is refused)
  if (!c->lgt_T) return fail(DSGD_ESTATE, "%s: no topics set (dsgd_lg_topics_set; dsgd_load_csr drops them)", what);
  return DSGD_OK;
}
// ... and BEHIND the call's argument checks (a call refused for its arguments has changed nothing): the topics' weights are in
// the rank order of the layout they were set under.  A context ranks its columns again only around a communicator
// (dsgd_comm_init* / dsgd_comm_destroy, which leave the layout ready under a new layout_gen); then the topics go, and the call
// says so
static int lgt_ready(dsgd_ctx* c, const char* what) {
  if (c->layout_ready && c->lgt_gen == c->layout_gen) return DSGD_OK;
  lgt_drop(c);
  return fail(DSGD_ESTATE, "%s: the columns were ranked again since dsgd_lg_topics_set: the topics were dropped, set them again", what);
}

int dsgd_lg_topics_set(dsgd_ctx* c, int32_t T, const int8_t* planes) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  {
    const LgtCheck v = lgt_check_set(T, nullptr, 0);   // (T alone: in range before anything else is looked at)
    if (v.kind == LGT_BAD_T) return fail(DSGD_EINVAL, "dsgd_lg_topics_set: %d topics, outside [0, %d]", (int)T, LG_TOPICS_MAX);
  }
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_topics_set", LG_ONE_PROCESS, &fresh));
  if (T == 0) {
    lgt_drop(c);
    return DSGD_OK;
  }
  const LgtCheck v = lgt_check_set(T, planes, c->n_rows);
  switch (v.kind) {
    case LGT_OK: break;
    case LGT_BAD_T: return fail(DSGD_EINVAL, "dsgd_lg_topics_set: %d topics, outside [0, %d]", (int)T, LG_TOPICS_MAX);
    case LGT_NULL: return fail(DSGD_EINVAL, "dsgd_lg_topics_set: null planes");
    case LGT_NO_ROWS: return fail(DSGD_ESTATE, "dsgd_lg_topics_set: no rows loaded");
    case LGT_ENTRY:
      return fail(DSGD_EINVAL, "dsgd_lg_topics_set: plane %d, row %lld = %d, expected +1/-1", v.topic, v.row, v.value);
  }
  DSGD_TRY(prepare_layout(c));
  // the new blocks first: an allocation failure leaves the context (and the topics it had) as it was
  const size_t plane_bytes = (size_t)T * (size_t)c->n_rows;
  const size_t w_words = (size_t)T * (size_t)lgt_w_stride(c->dp);
  const size_t part_words = (size_t)lgt_part_words(T, c->dp, c->n_cu);
  DevBuf<signed char> planes_new;
  DevBuf<float> w_new;
  DevBuf<double> part_new;
  DevBuf<unsigned long long> tally_new;
  DSGD_TRY(planes_new.alloc(plane_bytes));
  DSGD_TRY(w_new.alloc(w_words));
  DSGD_TRY(part_new.alloc(part_words));
  DSGD_TRY(tally_new.alloc((size_t)T * LG_TALLY_WORDS));
  HIP_TRY(hipMemcpyAsync(planes_new, planes, plane_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(w_new, 0, sizeof(float) * w_words, c->stream));   // (topic weights start at zero)
  HIP_TRY(hipStreamSynchronize(c->stream));   // (the caller's planes are free again; what the old blocks served is done)
  lgt_drop(c);
  c->d_lgt_planes = std::move(planes_new);
  c->d_lgt_w = std::move(w_new);
  c->d_lgt_part = std::move(part_new);
  c->d_lgt_tally = std::move(tally_new);
  c->lgt_T = T;
  c->lgt_gen = c->layout_gen;
  c->lgt_nsq_stale = true;
  return DSGD_OK;
}

// how many topics are set now (0: none): what sizes the arrays of the calls below
int dsgd_lg_topics_count(dsgd_ctx* c, int32_t* T_out) {
  DSGD_TRY(check_ctx(c));
  if (!T_out) return fail(DSGD_EINVAL, "dsgd_lg_topics_count: null T_out");
  std::lock_guard<std::mutex> lk(c->mu);
  *T_out = c->lgt_T && c->layout_ready && c->lgt_gen == c->layout_gen ? c->lgt_T : 0;
  return DSGD_OK;
}

int dsgd_lg_topics_set_weights(dsgd_ctx* c, const float* W) {
  DSGD_TRY(check_ctx(c));
  if (!W) return fail(DSGD_EINVAL, "dsgd_lg_topics_set_weights: null W");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgt_enter(c, "dsgd_lg_topics_set_weights"));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_topics_set_weights"));
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  for (int t = 0; t < c->lgt_T; ++t) {   // (key order -> rank order through the context's staging vector, topic by topic)
    DSGD_TRY(pin_acquire(c->pin_w, bytes));
    memcpy(c->pin_w.p, W + (size_t)t * (size_t)c->dp, bytes);
    HIP_TRY(hipMemcpyAsync(c->d_io, c->pin_w.p, bytes, hipMemcpyHostToDevice, c->stream));
    DSGD_TRY(pin_sent(c, c->pin_w));
    DSGD_TRY(launch_permute_in(c, c->d_io, c->d_lgt_w + (size_t)t * (size_t)lgt_w_stride(c->dp)));
  }
  c->lgt_nsq_stale = true;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DSGD_OK;
}

int dsgd_lg_topics_get_weights(dsgd_ctx* c, float* W_out) {
  DSGD_TRY(check_ctx(c));
  if (!W_out) return fail(DSGD_EINVAL, "dsgd_lg_topics_get_weights: null W_out");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgt_enter(c, "dsgd_lg_topics_get_weights"));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_topics_get_weights"));
  const size_t bytes = sizeof(float) * (size_t)c->dp;
  DSGD_TRY(pin_acquire(c->pin_out, bytes * (size_t)c->lgt_T));
  for (int t = 0; t < c->lgt_T; ++t) {
    DSGD_TRY(launch_permute_out(c, c->d_lgt_w + (size_t)t * (size_t)lgt_w_stride(c->dp), c->d_io));
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(c->pin_out.p.get()) + (size_t)t * bytes, c->d_io, bytes, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(W_out, c->pin_out.p, bytes * (size_t)c->lgt_T);
  return DSGD_OK;
}

// room for the column sums of n_workers workers under every topic (zeroed once; every finish leaves the words zeroed)
static int lgt_ensure(dsgd_ctx* c, int n_workers) {
  if (c->lgt_k >= n_workers && c->d_lgt_acc) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->lgt_k = 0;
  const int cap = std::max(n_workers, 4);
  const size_t words = (size_t)lgt_acc_words(c->lgt_T, cap, c->dp);
  DSGD_TRY(c->d_lgt_acc.alloc(words));
  HIP_TRY(hipMemsetAsync(c->d_lgt_acc, 0, sizeof(unsigned long long) * words, c->stream));
  c->lgt_k = cap;
  return DSGD_OK;
}

// The TWO launches of one step over K lists of positions in `idx`, the longest of `longest` rows, whatever T
static int lgt_launch(dsgd_ctx* c, int K, long long longest, float lr, const int* idx, const WorkSeg* segs) {
  LgtArgs a;
  a.w = c->d_lgt_w;
  a.w_stride = lgt_w_stride(c->dp);
  a.planes = c->d_lgt_planes;
  a.T = c->lgt_T;
  a.hot = lgt_hot(c->lgt_T);
  a.dp = c->dp;
  a.vexp = c->vexp;
  a.K = K;
  a.idx = idx;
  a.segs = segs;
  a.blocks_per_worker = lg_blocks_per_worker(longest, K, c->n_cu, 2);   // (dsgd_lg_sync_step's grid for lists)
  a.acc = c->d_lgt_acc;
  a.acc_stride = lgt_acc_stride(c->dp);
  a.sc = c->d_sc;
  const dim3 th(LG_THREADS);
  hipLaunchKernelGGL(dsgd_lg_topics_grad_kernel, dim3((unsigned)(a.blocks_per_worker * K)), th, 0, c->stream, view(c), a);
  HIP_TRY(hipGetLastError());
  LgtFinishArgs f;
  f.acc = c->d_lgt_acc;
  f.acc_stride = a.acc_stride;
  f.segs = segs;
  f.K = K;
  f.dp = c->dp;
  f.vexp = c->vexp;
  f.w = c->d_lgt_w;
  f.w_stride = a.w_stride;
  f.lr = (double)lr;
  f.lambda = c->cfg.lambda;
  f.nsq_part = c->d_lgt_part;
  hipLaunchKernelGGL(dsgd_lg_topics_finish_kernel, dim3((unsigned)lg_finish_blocks(c->dp), (unsigned)c->lgt_T), th, 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
// behind a call's steps: the one synchronisation; every row contributes.  After a failure the sums may be half added: the
// accumulators go, the next call starts from zeroed ones
static int lgt_step_done(dsgd_ctx* c, int rc, dsgd_batch_stats* stats, long long total) {
  if (rc == DSGD_OK) rc = finish_stats(c, stats, total);
  if (rc != DSGD_OK) {
    (void)hipStreamSynchronize(c->stream);
    c->d_lgt_acc.reset();
    c->lgt_k = 0;
    c->lgt_nsq_stale = true;
    return rc;
  }
  c->lgt_nsq_stale = false;   // (|w_t'|^2 of the new weights is in d_lgt_part)
  if (stats) stats->n_active = stats->n_samples;
  return DSGD_OK;
}

int dsgd_lg_topics_sync_step(dsgd_ctx* c, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers, float lr,
                             dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (n_workers < 1 || !idx_per_worker || !n_per_worker)
    return fail(DSGD_EINVAL, "dsgd_lg_topics_sync_step: Cannot sum an empty list of vectors (no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgt_enter(c, "dsgd_lg_topics_sync_step"));
  const LgCheck v = lgt_check_step(idx_per_worker, n_per_worker, n_workers, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_topics_sync_step", v, n_workers));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_topics_sync_step"));
  DSGD_TRY(lgt_ensure(c, n_workers));
  DSGD_TRY(reset_counters(c));
  long long mx = 0, tot = 0;
  DSGD_TRY(stage_lists(c, idx_per_worker, n_per_worker, n_workers, &mx, &tot));
  return lgt_step_done(c, lgt_launch(c, n_workers, mx, lr, c->cur_idx, c->d_segs), stats, tot);
}

int dsgd_lg_topics_sync_steps(dsgd_ctx* c, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers, float lr,
                              dsgd_batch_stats* stats) {
  DSGD_TRY(check_ctx(c));
  if (!idx || !offsets || n_steps < 1 || n_workers < 1 || n_idx < 1)
    return fail(DSGD_EINVAL, "dsgd_lg_topics_sync_steps: bad arguments (null lists, no steps or no workers)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgt_enter(c, "dsgd_lg_topics_sync_steps"));
  const int K = n_workers;
  const LgCheck v = lgt_check_steps(idx, n_idx, offsets, n_steps, K, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_topics_sync_steps", v, K));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_topics_sync_steps"));
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
    rc = lgt_launch(c, K, mx, lr, c->d_idx, c->d_lgt_ssegs + t * K);
  }
  return lgt_step_done(c, rc, stats, n_idx);
}

int dsgd_lg_topics_loss_acc(dsgd_ctx* c, int64_t row_begin, int64_t row_end, double* loss, double* acc) {
  DSGD_TRY(check_ctx(c));
  if (!loss && !acc) return fail(DSGD_EINVAL, "dsgd_lg_topics_loss_acc: null loss and acc");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgt_enter(c, "dsgd_lg_topics_loss_acc"));
  const LgCheck v = lgt_check_range(row_begin, row_end, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_topics_loss_acc", v, 1));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_topics_loss_acc"));
  const int T = c->lgt_T;
  const long long nb = lg_finish_blocks(c->dp);
  if (c->lgt_nsq_stale) {   // |w_t|^2 of weights the finish did not write: the finish's grid and tree, the same bits
    hipLaunchKernelGGL(dsgd_lg_nsq_kernel, dim3((unsigned)nb, (unsigned)T), dim3(LG_THREADS), 0, c->stream, c->d_lgt_w.get(),
                       lgt_w_stride(c->dp), c->dp, c->d_lgt_part.get());
    HIP_TRY(hipGetLastError());
  }
  DSGD_TRY(reset_counters(c));
  HIP_TRY(hipMemsetAsync(c->d_lgt_tally, 0, sizeof(unsigned long long) * (size_t)T * LG_TALLY_WORDS, c->stream));
  const long long rows = row_end - row_begin;
  const long long grid = lg_eval_blocks(rows, c->n_cu);
  const int hw = lgt_eval_hw(rows, std::min(c->hw_eval, c->dp), T);
  const size_t lds = sizeof(float) * (size_t)lgt_eval_lds_floats(hw, T);
  hipLaunchKernelGGL(dsgd_lg_topics_eval_kernel, dim3((unsigned)grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_lgt_w.get(),
                     lgt_w_stride(c->dp), c->d_lgt_planes.get(), T, (long long)row_begin, (long long)row_end, c->d_lgt_tally.get(), hw,
                     c->d_lgt_part + lgt_loss_at(T, 0, c->dp, c->n_cu), (long long)c->n_cu);
  HIP_TRY(hipGetLastError());
  const size_t words = (size_t)lgt_part_words(T, c->dp, c->n_cu), tally_words = (size_t)T * LG_TALLY_WORDS;
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(double) * words + sizeof(unsigned long long) * tally_words));
  double* part = static_cast<double*>(c->pin_out.p.get());
  unsigned long long* tally = reinterpret_cast<unsigned long long*>(part + words);
  HIP_TRY(hipMemcpyAsync(part, c->d_lgt_part, sizeof(double) * words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tally, c->d_lgt_tally, sizeof(unsigned long long) * tally_words, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));   // the one synchronisation of the call
  DSGD_TRY(check_err_flag(c));
  c->lgt_nsq_stale = false;
  lgt_fold(part, tally, T, c->dp, c->n_cu, grid, rows, c->cfg.lambda, loss, acc);
  return DSGD_OK;
}

int dsgd_lg_topics_predict(dsgd_ctx* c, const int32_t* idx, int64_t n, float* p_out) {
  DSGD_TRY(check_ctx(c));
  if (n < 1 || !idx || !p_out) return fail(DSGD_EINVAL, "dsgd_lg_topics_predict: bad arguments (a null pointer or no rows)");
  std::lock_guard<std::mutex> lk(c->mu);
  DSGD_TRY(lgt_enter(c, "dsgd_lg_topics_predict"));
  const LgCheck v = lgt_check_list(idx, n, c->n_rows);
  DSGD_TRY(lg_report(c, "dsgd_lg_topics_predict", v, 1));
  DSGD_TRY(lgt_ready(c, "dsgd_lg_topics_predict"));
  const int T = c->lgt_T;
  const size_t out = (size_t)T * (size_t)n;
  DSGD_TRY(ensure_idx(c, n));
  if (out > c->d_lgt_p.cap()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSGD_TRY(c->d_lgt_p.reserve(std::max<size_t>(out, 4096)));
  }
  DSGD_TRY(reset_counters(c));
  DSGD_TRY(send_idx(c, idx, n));
  DSGD_TRY(pin_acquire(c->pin_out, sizeof(float) * out));
  hipLaunchKernelGGL(dsgd_lg_topics_predict_kernel, dim3((unsigned)grid_for(c, n, LG_GROUP)), dim3(LG_THREADS), 0, c->stream, view(c),
                     c->d_lgt_w.get(), lgt_w_stride(c->dp), T, c->d_idx.get(), (long long)n, c->d_lgt_p.get(), c->d_sc.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->pin_out.p, c->d_lgt_p, sizeof(float) * out, hipMemcpyDeviceToHost, c->stream));
  DSGD_TRY(read_scalars(c));
  memcpy(p_out, c->pin_out.p, sizeof(float) * out);
  DSGD_TRY(check_err_flag(c));
  return DSGD_OK;
}
