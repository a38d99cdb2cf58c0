// Host side of SOFTMAX regression over few classes, the lanes across the non-zeros (include/dsgd.h "THE LOGISTIC MODEL": SOFTMAX,
// FEW CLASSES; device code: csrc/dsgd_lg_softmax_il.hpp; sizes and checks: csrc/dsgd_lg_softmax_il_host.hpp, which
// tests/cpp/lg_softmax_il_host_test.cpp compiles on the CPU).  Included by dsgd_hip.hip inside its extern "C" block, behind
// dsgd_lg_topics_cols_calls.hpp and in front of dsgd_lg_softmax_calls.hpp: dsgd_lg_softmax_set_il here, and what the
// dsgd_lg_softmax_* calls there launch when the context's classes are interleaved and not wide (c->lgt_il && !c->lgt_wide) -- one
// function per launch site.  The context's blocks are the interleaved topics' (lgti_install lays them out from the one-hot
// planes), so every dsgd_lg_topics_* call keeps serving the context as interleaved one-vs-rest on those planes.

int dsgd_lg_softmax_set_il(dsgd_ctx* c, int32_t C, const uint8_t* cls) {
  DSGD_TRY(check_ctx(c));
  std::lock_guard<std::mutex> lk(c->mu);
  if (lgsi_check_set(C, nullptr, 0).kind == LGSM_BAD_C)   // (C alone: in range before anything else is looked at)
    return fail(DSGD_ERANGE, "dsgd_lg_softmax_set_il: %d classes, outside {0} and [%d, %d]", (int)C, LG_SOFTMAX_MIN, LG_SOFTMAX_IL_MAX);
  if (c->async_running)
    return fail(DSGD_EUNSUPPORTED, "dsgd_lg_softmax_set_il is not available while the lock-free engine runs (dsgd_async_stop / dsgd_async_wait first)");
  bool fresh = false;
  DSGD_TRY(lg_enter(c, "dsgd_lg_softmax_set_il", LG_ONE_PROCESS, &fresh));
  if (C == 0) {
    lgt_drop(c);
    return DSGD_OK;
  }
  const LgsmCheck v = lgsi_check_set(C, cls, c->n_rows);
  switch (v.kind) {
    case LGSM_OK: break;
    case LGSM_BAD_C: return fail(DSGD_ERANGE, "dsgd_lg_softmax_set_il: %d classes", (int)C);
    case LGSM_NULL: return fail(DSGD_EINVAL, "dsgd_lg_softmax_set_il: null classes");
    case LGSM_NO_ROWS: return fail(DSGD_ESTATE, "dsgd_lg_softmax_set_il: no rows loaded");
    case LGSM_ENTRY: return fail(DSGD_ERANGE, "dsgd_lg_softmax_set_il: row %lld has class %d of %d", v.row, v.value, (int)C);
  }
  std::vector<int8_t> planes((size_t)C * (size_t)c->n_rows);
  lgsm_one_hot(cls, C, c->n_rows, planes.data());
  DSGD_TRY(lgti_install(c, C, planes.data()));
  c->lgt_softmax = true;
  return DSGD_OK;
}

// a kernel family's instantiation for the context's TP
#define LGSI_BY_QUADS(nq, LAUNCH) \
  do {                            \
    if ((nq) == 1) LAUNCH(1);     \
    else if ((nq) == 2) LAUNCH(2); \
    else if ((nq) == 4) LAUNCH(4); \
    else LAUNCH(8);               \
  } while (0)

// The TWO launches of one step over K lists, whatever C (lgsm_launch's interleaved side): the interleaved gradient's arguments
// and finish around the softmax gradient
static int lgsi_launch(dsgd_ctx* c, int K, long long longest, float lr, const int* idx, const WorkSeg* segs) {
  const LgtiArgs a = lgti_grad_args(c, K, longest, idx, segs);
  const dim3 grid((unsigned)(a.blocks_per_worker * K)), th(LG_THREADS);
#define LGSI_GRAD(NQ) hipLaunchKernelGGL(dsgd_lg_softmax_il_grad_kernel<NQ>, grid, th, 0, c->stream, view(c), a)
  LGSI_BY_QUADS(lgsi_quads(a.tp), LGSI_GRAD);
#undef LGSI_GRAD
  HIP_TRY(hipGetLastError());
  c->last_grad_kernel = "dsgd_lg_softmax_il_grad_kernel";
  return lgti_launch_finish(c, K, lr, segs);
}

// the THREE launches of one step over the ranges in c->d_segs (lgsm_launch_ranges' interleaved side): the coefficients here, then
// the topics' column-wise gradient and the interleaved finish as they are
static int lgsi_launch_ranges(dsgd_ctx* c, int K, const dsgd_ctx::LgColsLayout& L, long long longest, float lr) {
  const LgtcCoefArgs q = lgtc_coef_args(c, K, L, longest);   // (the grid of a 16-lane group per row)
  const dim3 cgrid((unsigned)(q.blocks_per_worker * K)), th(LG_THREADS);
#define LGSI_COEF(NQ) hipLaunchKernelGGL(dsgd_lg_softmax_il_coef_kernel<NQ>, cgrid, th, 0, c->stream, view(c), q)
  LGSI_BY_QUADS(lgsi_quads(q.tp), LGSI_COEF);
#undef LGSI_COEF
  HIP_TRY(hipGetLastError());
  return lgtc_launch_grad_finish(c, K, L, lr);
}

// the evaluation of rows [row_begin, row_end) in `grid` workgroups with a tile of hw ranks: the loss words into `part`
static int lgsi_launch_eval(dsgd_ctx* c, long long row_begin, long long row_end, long long grid, int hw, double* part) {
  const int C = c->lgt_T;
  const size_t lds = sizeof(float) * (size_t)lgsm_eval_lds_floats(hw, C);
  const dim3 g((unsigned)grid), th(LGSM_EVAL_THREADS);
#define LGSI_EVAL(NQ)                                                                                                                            \
  hipLaunchKernelGGL(dsgd_lg_softmax_il_eval_kernel<NQ>, g, th, lds, c->stream, view(c), c->d_lgt_w.get(), c->d_lgt_planes.get(), C, row_begin, \
                     row_end, c->d_lgt_tally.get(), hw, part)
  LGSI_BY_QUADS(lgsi_quads(lgti_tp(C)), LGSI_EVAL);
#undef LGSI_EVAL
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}

// the classes (and, where dp_out is not null, the probabilities) of the n rows in c->d_idx
static int lgsi_launch_predict(dsgd_ctx* c, long long n, float* dp_out) {
  const int C = c->lgt_T;
  const dim3 g((unsigned)grid_for(c, n, LG_GROUP)), th(LG_THREADS);
#define LGSI_PREDICT(NQ)                                                                                                              \
  hipLaunchKernelGGL(dsgd_lg_softmax_il_predict_kernel<NQ>, g, th, 0, c->stream, view(c), c->d_lgt_w.get(), C, c->d_idx.get(), n, \
                     c->d_lgsm_cls.get(), dp_out, c->d_sc.get())
  LGSI_BY_QUADS(lgsi_quads(lgti_tp(C)), LGSI_PREDICT);
#undef LGSI_PREDICT
  HIP_TRY(hipGetLastError());
  return DSGD_OK;
}
#undef LGSI_BY_QUADS
