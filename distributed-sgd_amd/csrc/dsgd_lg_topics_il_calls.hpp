// Host side of the INTERLEAVED form of the logistic model over several topics (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL
// TOPICS, INTERLEAVED; device code: csrc/dsgd_lg_topics_il.hpp; sizes and checks: csrc/dsgd_lg_topics_il_host.hpp, which
// tests/cpp/lg_topics_il_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip inside its extern "C" block, in front of
// dsgd_lg_topics_calls.hpp: dsgd_lg_topics_set_il here, and what the dsgd_lg_topics_* calls there launch when the context's
// topics are interleaved (c->lgt_il) -- one function per launch site.  The context's blocks are the planar form's under the
// interleaved shapes: d_lgt_planes is Pi, d_lgt_w is Wi, d_lgt_acc is acc[k][rank][TP].

static int lgti_install(dsgd_ctx* c, int32_t T, const int8_t* planes);
int dsgd_lg_topics_set_il(dsgd_ctx* c, int32_t T, const int8_t* planes) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  {
    const LgtCheck v = lgti_check_set(T, nullptr, 0);   // (T alone: in range before anything else is looked at)
    if (v.kind == LGT_BAD_T) return fail(DSGD_EINVAL, "dsgd_lg_topics_set_il: %d topics, outside [0, %d]", (int)T, LG_TOPICS_IL_MAX);
  }
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_topics_set_il", LG_ONE_PROCESS, &fresh));
  if (T == 0) {
    lgt_drop(c);
    return DSGD_OK;
  }
  const LgtCheck v = lgti_check_set(T, planes, c->n_rows);
  switch (v.kind) {
    case LGT_OK: break;
    case LGT_BAD_T: return fail(DSGD_EINVAL, "dsgd_lg_topics_set_il: %d topics, outside [0, %d]", (int)T, LG_TOPICS_IL_MAX);
    case LGT_NULL: return fail(DSGD_EINVAL, "dsgd_lg_topics_set_il: null planes");
    case LGT_NO_ROWS: return fail(DSGD_ESTATE, "dsgd_lg_topics_set_il: no rows loaded");
    case LGT_ENTRY:
      return fail(DSGD_EINVAL, "dsgd_lg_topics_set_il: plane %d, row %lld = %d, expected +1/-1", v.topic, v.row, v.value);
  }
  return lgti_install(c, T, planes);
}

// the interleaved setter's body behind its checks (locked; planes: T x n_rows checked entries): dsgd_lg_topics_set_il above and
// dsgd_lg_softmax_set_il (csrc/dsgd_lg_softmax_il_calls.hpp), whose planes are one-hot
static int lgti_install(dsgd_ctx* c, int32_t T, const int8_t* planes) {
  DSGD_TRY(prepare_layout(c));
  // the new blocks first: an allocation failure leaves the context (and the topics it had, in either form) as it was
  const int tp = lgti_tp(T);
  const size_t plane_bytes = (size_t)lgti_plane_bytes(c->n_rows, tp);
  const size_t w_words = (size_t)lgti_w_words(c->dp, tp);
  DevBuf<signed char> planes_new;
  DevBuf<float> w_new, io_new;
  DevBuf<double> part_new;
  DevBuf<unsigned long long> tally_new;
  DSGD_TRY(planes_new.alloc(plane_bytes));
  DSGD_TRY(w_new.alloc(w_words));
  DSGD_TRY(io_new.alloc((size_t)lgt_w_stride(c->dp)));
  DSGD_TRY(part_new.alloc((size_t)lgt_part_words(T, c->dp, c->n_cu)));
  DSGD_TRY(tally_new.alloc((size_t)T * LG_TALLY_WORDS));
  DSGD_TRY(pin_acquire(c->pin_out, plane_bytes));   // Pi[row][TP] is laid out on the host, once
  lgti_interleave_planes(planes, T, c->n_rows, static_cast<int8_t*>(c->pin_out.p.get()));
  HIP_TRY(hipMemcpyAsync(planes_new, c->pin_out.p, plane_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(w_new, 0, sizeof(float) * w_words, c->stream));   // (topic weights start at zero; the padding topics' stay there)
  HIP_TRY(hipStreamSynchronize(c->stream));
  lgt_drop(c);
  c->d_lgt_planes = std::move(planes_new);
  c->d_lgt_w = std::move(w_new);
  c->d_lgti_io = std::move(io_new);
  c->d_lgt_part = std::move(part_new);
  c->d_lgt_tally = std::move(tally_new);
  c->lgt_T = T;
  c->lgt_il = true;
  c->lgt_gen = c->layout_gen;
  c->lgt_nsq_stale = true;
  return DSGD_OK;
}

// topic t's rank-order vector d_lgti_io into Wi / out of it
static int lgti_pack(dsgd_ctx* c, int t, bool in) {
  const dim3 grid((unsigned)lg_finish_blocks(c->dp)), th(LG_THREADS);
  if (in) hipLaunchKernelGGL(dsgd_lg_topics_il_pack_kernel<true>, grid, th, 0, c->stream, c->d_lgti_io.get(), c->d_lgt_w.get(), c->dp, lgti_tp(c->lgt_T), t);
  else hipLaunchKernelGGL(dsgd_lg_topics_il_pack_kernel<false>, grid, th, 0, c->stream, c->d_lgti_io.get(), c->d_lgt_w.get(), c->dp, lgti_tp(c->lgt_T), t);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

static LgtiFinishArgs lgti_finish_args(dsgd_ctx* c) {
  LgtiFinishArgs f = {};
  f.dp = c->dp;
  f.vexp = c->vexp;
  f.T = c->lgt_T;
  f.tp = lgti_tp(c->lgt_T);
  f.wi = c->d_lgt_w;
  f.lambda = c->cfg.lambda;
  f.nsq_part = c->d_lgt_part;
  return f;
}

// what the gradient over K lists is launched with (dsgd_lg_topics_il_grad_kernel and dsgd_lg_softmax_il_grad_kernel alike)
static LgtiArgs lgti_grad_args(dsgd_ctx* c, int K, long long longest, const int* idx, const WorkSeg* segs) {
  LgtiArgs a;
  a.wi = c->d_lgt_w;
  a.pi = c->d_lgt_planes;
  a.T = c->lgt_T;
  a.tp = lgti_tp(c->lgt_T);
  a.hot = lgti_hot(a.tp);
  a.dp = c->dp;
  a.vexp = c->vexp;
  a.K = K;
  a.idx = idx;
  a.segs = segs;
  a.blocks_per_worker = lg_blocks_per_worker(longest, K, c->n_cu, 2);   // (dsgd_lg_sync_step's grid for lists)
  a.acc = c->d_lgt_acc;
  a.acc_stride = lgti_acc_stride(c->dp, a.tp);
  a.sc = c->d_sc;
  return a;
}
// the interleaved finish over K workers' sums (`segs`: it reads the lengths)
static int lgti_launch_finish(dsgd_ctx* c, int K, float lr, const WorkSeg* segs) {
  LgtiFinishArgs f = lgti_finish_args(c);
  f.acc = c->d_lgt_acc;
  f.acc_stride = lgti_acc_stride(c->dp, f.tp);
  f.segs = segs;
  f.K = K;
  f.lr = (double)lr;
  hipLaunchKernelGGL(dsgd_lg_topics_il_finish_kernel<true>, dim3((unsigned)lg_finish_blocks(c->dp)), dim3(LG_THREADS), 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// The TWO launches of one step over K lists, whatever T (lgt_launch's interleaved side)
static int lgti_launch(dsgd_ctx* c, int K, long long longest, float lr, const int* idx, const WorkSeg* segs) {
  const LgtiArgs a = lgti_grad_args(c, K, longest, idx, segs);
  hipLaunchKernelGGL(dsgd_lg_topics_il_grad_kernel<LGTI_TB>, dim3((unsigned)(a.blocks_per_worker * K)), dim3(LG_THREADS), 0, c->stream, view(c), a);
  HIP_TRY(hipGetLastError());
  return lgti_launch_finish(c, K, lr, segs);
}

// |w_t|^2 of weights the finish did not write: the finish's grid and tree
static int lgti_launch_nsq(dsgd_ctx* c) {
  hipLaunchKernelGGL(dsgd_lg_topics_il_finish_kernel<false>, dim3((unsigned)lg_finish_blocks(c->dp)), dim3(LG_THREADS), 0, c->stream, lgti_finish_args(c));
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

static int lgti_launch_eval(dsgd_ctx* c, long long row_begin, long long row_end, long long grid) {
  const int T = c->lgt_T;
  const int hw = lgti_eval_hw(row_end - row_begin, std::min(c->hw_eval, c->dp), T);
  const size_t lds = sizeof(float) * (size_t)lgti_eval_lds_floats(hw, T);
  hipLaunchKernelGGL(dsgd_lg_topics_il_eval_kernel, dim3((unsigned)grid), dim3(LG_EVAL_THREADS), lds, c->stream, view(c), c->d_lgt_w.get(),
                     c->d_lgt_planes.get(), T, row_begin, row_end, c->d_lgt_tally.get(), hw, c->d_lgt_part + lgt_loss_at(T, 0, c->dp, c->n_cu),
                     (long long)c->n_cu);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

static int lgti_launch_predict(dsgd_ctx* c, long long n) {
  hipLaunchKernelGGL(dsgd_lg_topics_il_predict_kernel, dim3((unsigned)grid_for(c, n, LG_GROUP)), dim3(LG_THREADS), 0, c->stream, view(c),
                     c->d_lgt_w.get(), c->lgt_T, c->d_idx.get(), n, c->d_lgt_p.get(), c->d_sc.get());
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
