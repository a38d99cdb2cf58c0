// Host code of an epoch's lists drawn on the device, draw for draw the reference's stream (kernels: csrc/dsgd_shuffle.hpp;
// the host's arithmetic, which a CPU test runs on its own: csrc/dsgd_jr_walk.hpp).  Host only; included ONCE by dsgd_hip.hip,
// behind the plans' frame (plan_frame / plan_finish / plan_abandon) and dsgd_fp64_host.hpp's mode rules.
//
// The stream is a pure function of the seed and the lengths of the JOB's splits: the scan and the walk run over all of them.
// The plan holds the lists of the workers this context hosts, and only their start records and rejections go to the device.
//   dsgd_plan_create_from_seed / _rp64       the context hosts the whole job, a worker's length is split_end - split_begin,
//                                            batches up to JR_MAX_TAKE rows, up to JR_MAX_REJ rejections inside a shuffle,
//                                            dsgd_jr_slice_kernel; refused in an fp64 context with a communicator.
//   dsgd_plan_create_from_seed_job / _rp64   job workers first .. first + n_local - 1 of job_len, any batch size, up to
//                                            JR_JOB_MAX_REJ rejections, dsgd_jr_slice_job_kernel; the row-parallel form is a
//                                            LOCAL call that a communicator does not refuse (plan_run_rp64_ranks runs it).
//   dsgd_plan_create_from_seed_job_lg        (csrc/dsgd_lg_calls.hpp) the job form's draws into a LOGISTIC plan of an fp32 context:
//                                            a local call, accepted under dsgd_comm_init_lg (plan_run_lg runs it across the ranks).
// (_rp64: the same draws into a row-parallel plan -- an fp64 context, float or Double data, no limit of the column slices)
#pragma once

// slot `i` of the from-seed scratch with room for `bytes`
static hipError_t seed_scratch(dsgd_ctx* c, int i, size_t bytes, void** out) {
  DevBuf<void>& b = c->seed_scratch[i];
  const hipError_t e = b.cap() < bytes ? b.try_alloc(bytes + bytes / 4 + 4096) : hipSuccess;
  *out = b.get();
  return e;
}

// what one of the four entry points asks for
struct SeedRequest {
  const char* what;                 // the entry point, for the messages
  bool rp64;                        // a row-parallel plan (an fp64 context) instead of a column-slice one
  bool comm_ok;                     // a communicator does not refuse (a row-parallel plan spans the ranks at its run; creating it is local)
  bool job;                         // dsgd_jr_slice_job_kernel draws, and split_begin is worded as the hosted workers'
  std::vector<long long> len;       // rows of every worker of the job
  int first, n_local;               // the workers hosted here ...
  const int64_t* split_begin;       // ... and where their splits start in the rows loaded here (n_local entries)
  int batch_size, max_batch;        // max_batch: the largest batch one workgroup per list serves (the job form cuts chunks)
  int chunks;                       // workgroups per list
  int max_rej;                      // rejections inside one shuffle
  std::string too_large;            // the refusal of a batch beyond max_batch or a split beyond JR_MAX_LEN
  bool lg = false;                  // a logistic plan (an fp32 context: lg_refuse) instead of a column-slice one.  The whole-job
                                    // form is one process's; the job form is a local call that dsgd_comm_init_lg's communicator
                                    // does not refuse (dsgd_plan_run on the plan is the collective run of dsgd_plan_create_lg_n's)
  LgScope lg_scope() const { return job ? LG_SPANS : LG_ONE_PROCESS; }
};

struct SeedLaps {   // DSGD_SEED_PROF (tuning: where an epoch's 14 ms go)
  const bool on = getenv("DSGD_SEED_PROF") != nullptr;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char* at) const {
    if (on) fprintf(stderr, "[dsgd_plan_create_from_seed] %-28s %8.3f ms\n", at, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// ---- pass A on the device: the candidates for a rejection among the first `scan` raw values, as jr_walk takes them ----
struct SeedCandidates {
  std::vector<unsigned long long> base;
  std::vector<long long> ci;
  std::vector<unsigned int> cu;
  JrCandidates view() const { return JrCandidates{ci.data(), cu.data(), base.data(), (long long)base.size()}; }
};
static int seed_scan(dsgd_ctx* c, unsigned long long s0, long long scan, long long max_len, const SeedLaps& lap, SeedCandidates* out) {
  hipStream_t bs = c->build_stream;
  const int per_lane = (int)std::max<long long>(1, std::min<long long>(1024, (1LL << 30) / max_len));
  const long long span = (long long)JR_SCAN_THREADS * per_lane;
  const long long n_wg = (scan + span - 1) / span;
  const long long cap = (long long)((double)scan * (double)max_len / 2147483648.0 * 2.0) + 65536;
  long long* d_ci = nullptr;
  unsigned int* d_cu = nullptr;
  unsigned long long *d_base = nullptr, *d_tot = nullptr;
  hipError_t e = n_wg > 0x7fffffffLL ? hipErrorInvalidValue : seed_scratch(c, 0, sizeof(long long) * (size_t)cap, (void**)&d_ci);
  if (e == hipSuccess) e = seed_scratch(c, 1, sizeof(unsigned int) * (size_t)cap, (void**)&d_cu);
  if (e == hipSuccess) e = seed_scratch(c, 2, sizeof(unsigned long long) * (size_t)n_wg, (void**)&d_base);
  if (e == hipSuccess) e = seed_scratch(c, 3, sizeof(unsigned long long) * 2, (void**)&d_tot);
  if (e == hipSuccess) e = hipMemsetAsync(d_tot, 0, sizeof(unsigned long long) * 2, bs);
  out->base.assign((size_t)n_wg, 0ULL);
  out->ci.clear();
  out->cu.clear();
  unsigned long long tot[2] = {0, 0};
  if (e == hipSuccess) {
    JrScanArgs sa;
    sa.s0 = s0;
    sa.scan = scan;
    sa.per_lane = per_lane;
    sa.cand_min = (unsigned int)(0x80000000ULL - (unsigned long long)max_len);
    sa.cap = cap;
    sa.cand_i = d_ci;
    sa.cand_u = d_cu;
    sa.wg_base = d_base;
    sa.total = d_tot;
    hipLaunchKernelGGL(dsgd_jr_scan_kernel, dim3((unsigned)n_wg), dim3(JR_SCAN_THREADS), 0, bs, sa);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, bs);
  if (e == hipSuccess) e = hipMemcpyAsync(out->base.data(), d_base, sizeof(unsigned long long) * (size_t)n_wg, hipMemcpyDeviceToHost, bs);
  if (e == hipSuccess) e = hipStreamSynchronize(bs);
  if (e == hipSuccess && tot[1] == 0 && tot[0] > 0) {
    out->ci.resize((size_t)tot[0]);
    out->cu.resize((size_t)tot[0]);
    e = hipMemcpyAsync(out->ci.data(), d_ci, sizeof(long long) * out->ci.size(), hipMemcpyDeviceToHost, bs);
    if (e == hipSuccess) e = hipMemcpyAsync(out->cu.data(), d_cu, sizeof(unsigned int) * out->cu.size(), hipMemcpyDeviceToHost, bs);
    if (e == hipSuccess) e = hipStreamSynchronize(bs);
  }
  lap("scan + candidates on the host");
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(DSGD_EHIP, "scanning the random stream: %s", hipGetErrorString(e));
  }
  if (tot[1] != 0) return fail(DSGD_EUNSUPPORTED, "more rejection candidates than the device scan holds (draw the lists on the host)");
  return DSGD_OK;
}

// ---- pass B: the hosted workers' records to the device, the lists straight into d_idx_out (a plan's index buffer, or the
// scratch list of a sampled evaluation: dsgd_loss_acc_sampled) on stream `bs`, which is synchronised before the return ----
// (max_len: the longest split traced HERE -- the bitmap of the slice kernels; a caller with a plan abandons it on failure)
static int seed_draw(dsgd_ctx* c, const SeedRequest& r, const JrFrame& f, const JrWalked& w, unsigned long long s0, long long max_len,
                     int* d_idx_out, hipStream_t bs, const SeedLaps& lap) {
  const size_t n_local = (size_t)r.n_local;
  JrShuf* d_shuf = nullptr;
  int *d_rej = nullptr, *d_err = nullptr;
  long long *d_sb = nullptr, *d_off = nullptr;
  std::vector<long long> sb2(2 * n_local);   // job: begin | length, else begin | end
  for (size_t k = 0; k < n_local; ++k) {
    sb2[k] = r.split_begin[k];
    sb2[n_local + k] = r.len[(size_t)r.first + k] + (r.job ? 0 : (long long)r.split_begin[k]);
  }
  int h_err = 0;
  hipError_t e = seed_scratch(c, 4, sizeof(JrShuf) * (size_t)f.n_lists, (void**)&d_shuf);
  if (e == hipSuccess) e = seed_scratch(c, 5, sizeof(int) * std::max<size_t>(1, w.rej.size()), (void**)&d_rej);
  if (e == hipSuccess) e = seed_scratch(c, 6, sizeof(int), (void**)&d_err);
  if (e == hipSuccess) e = seed_scratch(c, 7, sizeof(long long) * sb2.size(), (void**)&d_sb);
  if (e == hipSuccess) e = seed_scratch(c, 8, sizeof(long long) * f.offsets.size(), (void**)&d_off);
  if (e == hipSuccess) e = hipMemcpyAsync(d_shuf, w.shuf.data(), sizeof(JrShuf) * (size_t)f.n_lists, hipMemcpyHostToDevice, bs);
  if (e == hipSuccess && !w.rej.empty()) e = hipMemcpyAsync(d_rej, w.rej.data(), sizeof(int) * w.rej.size(), hipMemcpyHostToDevice, bs);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, sizeof(int), bs);
  if (e == hipSuccess) e = hipMemcpyAsync(d_sb, sb2.data(), sizeof(long long) * sb2.size(), hipMemcpyHostToDevice, bs);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off, f.offsets.data(), sizeof(long long) * f.offsets.size(), hipMemcpyHostToDevice, bs);
  static const JrAffine back_one = jr_inverse_step();
  static const JrAffine back_block = jr_power(back_one, JR_SLICE_THREADS);
  if (e == hipSuccess && r.job) {
    JrSliceJobArgs a;
    a.s0 = s0;
    a.back_block = back_block;
    a.back_one = back_one;
    a.shuf = d_shuf;
    a.rej = d_rej;
    a.split_begin = d_sb;
    a.len = d_sb + n_local;
    a.offsets = d_off;
    a.idx_out = d_idx_out;
    a.n_local = r.n_local;
    a.batch_size = r.batch_size;
    a.chunks = r.chunks;
    a.err = d_err;
    hipLaunchKernelGGL(dsgd_jr_slice_job_kernel, dim3((unsigned)(f.n_lists * r.chunks)), dim3(JR_SLICE_THREADS), jr_slice_job_lds_bytes(max_len), bs, a);
    e = hipGetLastError();
  } else if (e == hipSuccess) {
    JrSliceArgs a;
    a.s0 = s0;
    a.back_block = back_block;
    a.back_one = back_one;
    a.shuf = d_shuf;
    a.rej = d_rej;
    a.split_begin = d_sb;
    a.split_end = d_sb + n_local;
    a.offsets = d_off;
    a.idx_out = d_idx_out;
    a.n_splits = r.n_local;
    a.batch_size = r.batch_size;
    a.err = d_err;
    hipLaunchKernelGGL(dsgd_jr_slice_kernel, dim3((unsigned)f.n_lists), dim3(JR_SLICE_THREADS), jr_slice_lds_bytes(max_len), bs, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, bs);
  if (e == hipSuccess) e = hipStreamSynchronize(bs);
  lap("lists drawn (slice kernel)");
  if (e != hipSuccess || h_err) {
    (void)hipGetLastError();
    if (h_err) return fail(DSGD_EUNSUPPORTED, "a shuffle left the limits of the device form (draw the lists on the host)");
    return fail(DSGD_EHIP, "drawing the lists: %s", hipGetErrorString(e));
  }
  return DSGD_OK;
}

// ---- pass A and the walk: where every hosted list's shuffle starts in the stream and what it rejects ----
// (max_len: the longest split of the JOB; the context bound and its build stream made; refuses before anything is drawn)
static int seed_walk(dsgd_ctx* c, const SeedRequest& r, const JrFrame& f, unsigned long long s0, long long max_len, const SeedLaps& lap,
                     JrWalked* w) {
  // scan, walk; a stream with more rejections than the margin scanned is scanned further and walked again
  long long scan = f.nominal + 64 + f.nominal / 4096;
  for (int attempt = 0;; ++attempt) {
    SeedCandidates cands;
    DSGD_TRY(seed_scan(c, s0, scan, max_len, lap, &cands));
    if (jr_walk(f, r.len, cands.view(), scan, w)) break;
    if (attempt >= 3) return fail(DSGD_EUNSUPPORTED, "the random stream keeps outrunning its scan (draw the lists on the host)");
    scan = w->scan_at_least + 64 + w->rej_total / 8;
  }
  lap("candidates walked");
  for (const JrShuf& s : w->shuf)
    if (s.rej_end - s.rej_begin > r.max_rej)
      return fail(DSGD_EUNSUPPORTED, "more than %d rejections inside one shuffle (draw the lists on the host)", r.max_rej);
  jr_select_hosted(f, w);
  return DSGD_OK;
}

// ---- a request from its refusals to its plan ----
static int plan_from_seed(dsgd_ctx* c, const SeedRequest& r, uint64_t* jstate, int64_t max_samples, dsgd_plan** out, int64_t* n_steps_out,
                          int64_t* draws_out) {
  {   // (refused with *out as it was)
    std::lock_guard<std::mutex> lk0(c->mu);
    if (r.lg) {
      DSGD_TRY(lg_refuse(c, r.what, r.lg_scope()));
    } else if (r.rp64) {
      DSGD_TRY(require_fp64(c, r.what));
      if (!r.comm_ok) DSGD_TRY(refuse_fp64_comm(c, r.what));
    } else {
      DSGD_TRY(refuse_val64(c, r.what));
    }
  }
  *out = nullptr;
  *n_steps_out = 0;
  if (draws_out) *draws_out = 0;
  const int n_splits = (int)r.len.size();
  long long max_len = 0, hosted_max = 0;
  for (int k = 0; k < n_splits; ++k) {
    if (r.len[(size_t)k] < 1 || (!r.job && r.split_begin[k] < 0)) return fail(DSGD_EINVAL, "worker %d has no rows", k);
    max_len = std::max(max_len, r.len[(size_t)k]);
  }
  for (int i = 0; i < r.n_local; ++i) {
    if (r.split_begin[i] < 0) return fail(DSGD_EINVAL, "hosted worker %d starts at a negative row", i);
    hosted_max = std::max(hosted_max, r.len[(size_t)(r.first + i)]);
  }
  if (r.batch_size > r.max_batch || max_len > JR_MAX_LEN) return fail(DSGD_EUNSUPPORTED, "%s", r.too_large.c_str());
  const long long n_steps = jr_epoch_steps(r.len, max_samples, r.batch_size);
  if (n_steps == 0) return DSGD_OK;
  if (r.job && n_steps * r.n_local * r.chunks > 0x7fffffffLL) return fail(DSGD_EUNSUPPORTED, "more lists than one launch draws (draw them on the host)");
  const JrFrame f = jr_frame(r.len, r.first, r.n_local, n_steps, r.batch_size);
  std::lock_guard<std::mutex> lk(c->mu);
  if (!r.comm_ok) DSGD_TRY(refuse_fp64_comm(c, r.what));
  if (!r.rp64) DSGD_TRY(refuse_val64(c, r.what));
  if (r.lg) DSGD_TRY(lg_refuse(c, r.what, r.lg_scope()));
  DSGD_TRY(bind(c, true));
  for (int i = 0; i < r.n_local; ++i)
    if (r.split_begin[i] + r.len[(size_t)(r.first + i)] > c->n_rows)
      return fail(DSGD_ERANGE, "worker %d's rows [%lld, %lld) outside the %lld loaded", r.first + i, (long long)r.split_begin[i],
                  (long long)(r.split_begin[i] + r.len[(size_t)(r.first + i)]), c->n_rows);
  DSGD_TRY(ensure_build_stream(c));
  const unsigned long long s0 = *jstate & JR_MASK;
  const SeedLaps lap;
  JrWalked w;
  DSGD_TRY(seed_walk(c, r, f, s0, max_len, lap, &w));
  // the plan's frame, then pass B straight into its index buffer
  dsgd_plan* p = nullptr;
  DSGD_TRY(plan_frame(c, f.offsets.data(), n_steps, r.n_local, &p, r.rp64, r.lg));
  lap("plan frame");
  p->idx_trusted = true;
  p->drawn = true;
  p->fits = false;   // (the one-workgroup kernel's test reads the lists on the host; these plans run on column slices)
  if (const int rc = seed_draw(c, r, f, w, s0, hosted_max, p->d_idx, c->build_stream, lap)) {
    plan_abandon(c, p);
    return rc;
  }
  DSGD_TRY(plan_finish(c, p, out));
  lap("plan laid out");
  *n_steps_out = n_steps;
  *jstate = jr_jump_dev(s0, (unsigned long long)(f.nominal + w.rej_total));
  if (draws_out) *draws_out = f.nominal + w.rej_total;
  return DSGD_OK;
}

// a job hosted whole: lengths end - begin, first = 0, n_local = n_splits
static int plan_from_seed_whole(dsgd_ctx* c, const char* what, bool rp64, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end,
                                int32_t n_splits, int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out,
                                bool lg = false) {
  DSGD_TRY(check_ctx(c));
  if (!jstate || !split_begin || !split_end || !out || !n_steps_out || n_splits < 1 || batch_size < 1) return fail(DSGD_EINVAL, "bad arguments");
  char msg[160];
  snprintf(msg, sizeof(msg), "device-drawn lists serve batches up to %d rows of splits up to %d rows (draw them on the host)", JR_MAX_TAKE, JR_MAX_LEN);
  SeedRequest r{what, rp64, false, false, {}, 0, n_splits, split_begin, batch_size, JR_MAX_TAKE, 1, JR_MAX_REJ, msg};
  r.lg = lg;
  for (int k = 0; k < n_splits; ++k) r.len.push_back((long long)(split_end[k] - split_begin[k]));
  return plan_from_seed(c, r, jstate, max_samples, out, n_steps_out, draws_out);
}
// a job's share of workers (include/dsgd.h): the stream over all n_job workers, the lists of the n_local hosted here
static int plan_from_seed_job(dsgd_ctx* c, const char* what, bool rp64, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first,
                              int32_t n_local, const int64_t* split_begin, int64_t max_samples, int32_t batch_size, dsgd_plan** out,
                              int64_t* n_steps_out, int64_t* draws_out, bool lg = false) {
  DSGD_TRY(check_ctx(c));
  if (!jstate || !split_begin || !job_len || !out || !n_steps_out || n_job < 1 || batch_size < 1) return fail(DSGD_EINVAL, "bad arguments");
  if (n_local < 1 || first < 0 || (long long)first + n_local > n_job)
    return fail(DSGD_EINVAL, "the hosted workers %d .. %lld are not workers of a job of %d", first, (long long)first + n_local - 1, n_job);
  char msg[160];
  snprintf(msg, sizeof(msg), "device-drawn lists serve splits up to %d rows (draw them on the host)", JR_MAX_LEN);
  const int chunks = (int)(((long long)batch_size + JR_MAX_TAKE - 1) / JR_MAX_TAKE);
  SeedRequest r{what, rp64, rp64, true, std::vector<long long>(job_len, job_len + n_job), first, n_local, split_begin, batch_size, 0x7fffffff, chunks,
                JR_JOB_MAX_REJ, msg};
  r.lg = lg;
  return plan_from_seed(c, r, jstate, max_samples, out, n_steps_out, draws_out);
}

int dsgd_plan_create_from_seed(dsgd_ctx* c, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end, int32_t n_splits,
                               int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out) {
  return plan_from_seed_whole(c, "dsgd_plan_create_from_seed", false, jstate, split_begin, split_end, n_splits, max_samples, batch_size, out,
                              n_steps_out, draws_out);
}
int dsgd_plan_create_from_seed_rp64(dsgd_ctx* c, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end, int32_t n_splits,
                                    int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out) {
  return plan_from_seed_whole(c, "dsgd_plan_create_from_seed_rp64", true, jstate, split_begin, split_end, n_splits, max_samples, batch_size, out,
                              n_steps_out, draws_out);
}
int dsgd_plan_create_from_seed_job(dsgd_ctx* c, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first, int32_t n_local,
                                   const int64_t* split_begin, int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out,
                                   int64_t* draws_out) {
  return plan_from_seed_job(c, "dsgd_plan_create_from_seed_job", false, jstate, job_len, n_job, first, n_local, split_begin, max_samples,
                            batch_size, out, n_steps_out, draws_out);
}
int dsgd_plan_create_from_seed_job_rp64(dsgd_ctx* c, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first, int32_t n_local,
                                        const int64_t* split_begin, int64_t max_samples, int32_t batch_size, dsgd_plan** out,
                                        int64_t* n_steps_out, int64_t* draws_out) {
  return plan_from_seed_job(c, "dsgd_plan_create_from_seed_job_rp64", true, jstate, job_len, n_job, first, n_local, split_begin, max_samples,
                            batch_size, out, n_steps_out, draws_out);
}
