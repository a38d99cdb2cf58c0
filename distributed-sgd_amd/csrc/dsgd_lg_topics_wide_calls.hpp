// Host side of the WIDE form of the logistic model over several topics (include/dsgd.h "THE LOGISTIC MODEL": SEVERAL TOPICS,
// WIDE; device code: csrc/dsgd_lg_topics_wide.hpp; sizes and checks: csrc/dsgd_lg_topics_wide_host.hpp, which
// tests/cpp/lg_topics_wide_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip inside its extern "C" block, behind
// dsgd_lg_topics_il_calls.hpp and in front of dsgd_lg_topics_calls.hpp: dsgd_lg_topics_set_wide here, and what the
// dsgd_lg_topics_* calls there launch when the context's topics are wide (c->lgt_wide) -- one function per launch site.  The
// context's blocks are the interleaved form's, shape for shape (c->lgt_il is set as well: packing, the sizes of the column sums
// and the staging vector are shared); only the kernels differ.

static int lgtw_install(dsgd_ctx* c, int32_t T, const int8_t* planes);
int dsgd_lg_topics_set_wide(dsgd_ctx* c, int32_t T, const int8_t* planes) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  {
    const LgtCheck v = lgtw_check_set(T, nullptr, 0);   // (T alone: in range before anything else is looked at)
    if (v.kind == LGT_BAD_T) return fail(DSGD_EINVAL, "dsgd_lg_topics_set_wide: %d topics, outside [0, %d]", (int)T, LG_TOPICS_WIDE_MAX);
  }
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_topics_set_wide", LG_ONE_PROCESS, &fresh));
  if (T == 0) {
    lgt_drop(c);
    return DSGD_OK;
  }
  const LgtCheck v = lgtw_check_set(T, planes, c->n_rows);
  switch (v.kind) {
    case LGT_OK: break;
    case LGT_BAD_T: return fail(DSGD_EINVAL, "dsgd_lg_topics_set_wide: %d topics, outside [0, %d]", (int)T, LG_TOPICS_WIDE_MAX);
    case LGT_NULL: return fail(DSGD_EINVAL, "dsgd_lg_topics_set_wide: null planes");
    case LGT_NO_ROWS: return fail(DSGD_ESTATE, "dsgd_lg_topics_set_wide: no rows loaded");
    case LGT_ENTRY:
      return fail(DSGD_EINVAL, "dsgd_lg_topics_set_wide: plane %d, row %lld = %d, expected +1/-1", v.topic, v.row, v.value);
  }
  return lgtw_install(c, T, planes);
}

// the wide setter's body behind its checks (locked; planes: T x n_rows checked entries): dsgd_lg_topics_set_wide above and
// dsgd_lg_softmax_set (csrc/dsgd_lg_softmax_calls.hpp), whose planes are one-hot
static int lgtw_install(dsgd_ctx* c, int32_t T, const int8_t* planes) {
  DSGD_TRY(prepare_layout(c));
  // the new blocks first: an allocation failure leaves the context (and the topics it had, in any form) as it was
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
  c->lgt_wide = true;
  c->lgt_gen = c->layout_gen;
  c->lgt_nsq_stale = true;
  return DSGD_OK;
}

// what the gradient over K lists is launched with (dsgd_lg_topics_wide_grad_kernel and dsgd_lg_softmax_grad_kernel alike)
static LgtiArgs lgtw_grad_args(dsgd_ctx* c, int K, long long longest, const int* idx, const WorkSeg* segs) {
  LgtiArgs a;
  a.wi = c->d_lgt_w;
  a.pi = c->d_lgt_planes;
  a.T = c->lgt_T;
  a.tp = lgti_tp(c->lgt_T);
  a.hot = lgtw_hot(a.tp);
  a.dp = c->dp;
  a.vexp = c->vexp;
  a.K = K;
  a.idx = idx;
  a.segs = segs;
  a.blocks_per_worker = lgtw_blocks_per_worker(longest, K, c->n_cu, lgtw_group_width(a.tp));
  a.acc = c->d_lgt_acc;
  a.acc_stride = lgti_acc_stride(c->dp, a.tp);
  a.sc = c->d_sc;
  return a;
}
// the wide finish over K workers' sums (the lists' ranges or the row ranges as `segs`: it reads the lengths)
static int lgtw_launch_finish(dsgd_ctx* c, int K, float lr, const WorkSeg* segs) {
  LgtiFinishArgs f = lgti_finish_args(c);
  f.acc = c->d_lgt_acc;
  f.acc_stride = lgti_acc_stride(c->dp, f.tp);
  f.segs = segs;
  f.K = K;
  f.lr = (double)lr;
  hipLaunchKernelGGL(dsgd_lg_topics_wide_finish_kernel<true>, dim3((unsigned)lg_finish_blocks(c->dp)), dim3(LG_THREADS), 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// The TWO launches of one step over K lists, whatever T (lgt_launch's wide side)
static int lgtw_launch(dsgd_ctx* c, int K, long long longest, float lr, const int* idx, const WorkSeg* segs) {
  const LgtiArgs a = lgtw_grad_args(c, K, longest, idx, segs);
  const int gw = lgtw_group_width(a.tp);
  const dim3 grid((unsigned)(a.blocks_per_worker * K)), th(LG_THREADS);
  if (gw == 16) hipLaunchKernelGGL(dsgd_lg_topics_wide_grad_kernel<16>, grid, th, 0, c->stream, view(c), a);
  else if (gw == 32) hipLaunchKernelGGL(dsgd_lg_topics_wide_grad_kernel<32>, grid, th, 0, c->stream, view(c), a);
  else hipLaunchKernelGGL(dsgd_lg_topics_wide_grad_kernel<64>, grid, th, 0, c->stream, view(c), a);
  HIP_TRY(hipGetLastError());
  return lgtw_launch_finish(c, K, lr, segs);
}

// |w_t|^2 of weights the finish did not write: the finish's grid and tree
static int lgtw_launch_nsq(dsgd_ctx* c) {
  hipLaunchKernelGGL(dsgd_lg_topics_wide_finish_kernel<false>, dim3((unsigned)lg_finish_blocks(c->dp)), dim3(LG_THREADS), 0, c->stream, lgti_finish_args(c));
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

static int lgtw_launch_eval(dsgd_ctx* c, long long row_begin, long long row_end, long long grid) {
  const int T = c->lgt_T;
  const int hw = lgtw_eval_hw(row_end - row_begin, std::min(c->hw_eval, c->dp), T);
  const size_t lds = sizeof(float) * (size_t)lgtw_eval_lds_floats(hw, T);
  double* part = c->d_lgt_part + lgt_loss_at(T, 0, c->dp, c->n_cu);
  const dim3 g((unsigned)grid), th(LG_EVAL_THREADS);
  const int gw = lgtw_group_width(lgti_tp(T));
#define LGTW_EVAL(GW)                                                                                                                             \
  hipLaunchKernelGGL(dsgd_lg_topics_wide_eval_kernel<GW>, g, th, lds, c->stream, view(c), c->d_lgt_w.get(), c->d_lgt_planes.get(), T, row_begin, \
                     row_end, c->d_lgt_tally.get(), hw, part, (long long)c->n_cu)
  if (gw == 16) LGTW_EVAL(16);
  else if (gw == 32) LGTW_EVAL(32);
  else LGTW_EVAL(64);
#undef LGTW_EVAL
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

static int lgtw_launch_predict(dsgd_ctx* c, long long n) {
  const int gw = lgtw_group_width(lgti_tp(c->lgt_T));
  const dim3 g((unsigned)grid_for(c, n, gw)), th(LG_THREADS);
#define LGTW_PREDICT(GW)                                                                                                                 \
  hipLaunchKernelGGL(dsgd_lg_topics_wide_predict_kernel<GW>, g, th, 0, c->stream, view(c), c->d_lgt_w.get(), c->lgt_T, c->d_idx.get(), n, \
                     c->d_lgt_p.get(), c->d_sc.get())
  if (gw == 16) LGTW_PREDICT(16);
  else if (gw == 32) LGTW_PREDICT(32);
  else LGTW_PREDICT(64);
#undef LGTW_PREDICT
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
