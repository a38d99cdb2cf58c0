// Host side of the row chunks (device code: csrc/dsgd_fstep.hpp; the cut: csrc/dsgd_layout_host.hpp): the whole gradient of a
// row range in one launch.  Included by dsgd_hip.hip behind the helpers it uses (view, ensure_part, prof_begin, layout_room).

static int fstep_build(dsgd_ctx* c, const std::vector<StreamSeg>& row_segs, int n_wg, dsgd_ctx::FstepLayout& L);
// the layout of (ranges, n_wg): never declined -- a failed build is an error, and nothing is cached
static int fstep_layout(dsgd_ctx* c, const std::vector<StreamSeg>& row_segs, int n_wg, dsgd_ctx::FstepLayout** out) {
  std::vector<long long> key;
  for (const StreamSeg& sg : row_segs) {
    key.push_back(sg.row_begin);
    key.push_back(sg.row_end);
  }
  if (auto* e = c->fstep_cache.find(key, n_wg, c->layout_gen)) {
    if (!e->layout.d_chunks) DSGD_TRY(fstep_build(c, row_segs, n_wg, e->layout));   // (a re-cut that failed left it empty)
    *out = &e->layout;
    return DSGD_OK;
  }
  DSGD_TRY(layout_room(c, c->fstep_cache));
  dsgd_ctx::FstepLayout L;
  DSGD_TRY(fstep_build(c, row_segs, n_wg, L));
  *out = &c->fstep_cache.insert(std::move(key), n_wg, c->layout_gen, std::move(L))->layout;
  return DSGD_OK;
}
// the tile tables and chunk records of a configuration (L.share: the chunks' shares of their worker's weight, or empty)
static int fstep_build(dsgd_ctx* c, const std::vector<StreamSeg>& row_segs, int n_wg, dsgd_ctx::FstepLayout& L) {
  ChunkTables T;
  cut_row_chunks(row_segs, n_wg, L.share, c->h_hrp, c->h_ctp, c->wlong_rows, c->wlong_weight, c->h_label.data(), T);
  const std::vector<WTile>&wt = T.wt, &ct = T.ct;
  const std::vector<unsigned short>&meta = T.meta, &cmeta = T.cmeta;
  const std::vector<FChunk>& chunks = T.chunks;
  L.n_wg = n_wg;
  L.worst_rows = T.worst_rows;
  L.shift = -1;
  // (alloc drops the tables of the cut before)
  // One guard record in front of both tile tables; the kernel is handed the record behind it.  A chunk without a tile clamps
  // its record fetches to tile_end - 1 (w_fetch, c_map: unconditional scalar loads whose result is then not used), and for the
  // FIRST chunk of a launch -- a range that starts on rows of the long list -- that is index -1.
  const WTile guard = unused_wave_tile();
  hipError_t e = L.d_tiles.try_alloc(wt.size() + 1);
  if (e == hipSuccess) e = L.d_meta.try_alloc(meta.size());
  if (e == hipSuccess) e = L.d_ctiles.try_alloc(ct.size() + 1);
  if (e == hipSuccess) e = L.d_cmeta.try_alloc(cmeta.size());
  if (e == hipSuccess) e = L.d_chunks.try_alloc(chunks.size());
  if (e == hipSuccess) e = hipMemcpy(L.d_tiles, &guard, sizeof(WTile), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.d_tiles + 1, wt.data(), sizeof(WTile) * wt.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.d_meta, meta.data(), sizeof(unsigned short) * meta.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.d_ctiles, &guard, sizeof(WTile), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.d_ctiles + 1, ct.data(), sizeof(WTile) * ct.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.d_cmeta, cmeta.data(), sizeof(unsigned short) * cmeta.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(L.d_chunks, chunks.data(), sizeof(FChunk) * chunks.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess && !L.d_times) {
    e = L.d_times.try_alloc(chunks.size());
    if (e == hipSuccess) e = L.h_times.try_alloc(chunks.size());
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.times_ev.e, hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipMemset(L.d_times, 0, sizeof(unsigned long long) * chunks.size());
  L.launches = 0;
  L.times_pending = false;
  if (e != hipSuccess) {
    L = dsgd_ctx::FstepLayout();
    return fail(DSGD_EHIP, "row-chunk layout: %s", hipGetErrorString(e));
  }
  return DSGD_OK;
}
// Measured balance (opt-in, DSGD_FSTEP_REBALANCE=1): after FSTEP_CAL launches of a configuration the workgroups' summed durations come back (asynchronously);
// a later launch that finds them cuts the chunks again -- chunk b's share of the weight times (mean time / its time),
// within 15 % -- twice at most.  The slowest workgroup ends the launch: at N = 804,414 it ran 8 us behind the average of 75,
// the same workgroups every time (profiles/r06_fstep_wg_times.txt).  Integer sums: the re-cut changes no bit.
constexpr int FSTEP_CAL = 24;
static int fstep_maybe_rebalance(dsgd_ctx* c, const std::vector<StreamSeg>& row_segs, dsgd_ctx::FstepLayout* L) {
  if (!c->k.fstep_rebalance || L->rebalances >= 2 || !L->d_times || c->d_tprof) return DSGD_OK;
  const size_t n = (size_t)L->n_wg * row_segs.size();
  if (!L->times_pending) {
    if (L->launches >= FSTEP_CAL) {
      HIP_TRY(hipMemcpyAsync(L->h_times, L->d_times, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipEventRecord(L->times_ev, c->stream));
      L->times_pending = true;
    }
    return DSGD_OK;
  }
  if (hipEventQuery(L->times_ev) != hipSuccess) {
    (void)hipGetLastError();
    return DSGD_OK;
  }
  // (the copy covered exactly the launches enqueued in front of it; launches since then run on the old cut and are dropped)
  std::vector<double> share(n, 1.0);
  const bool had = L->share.size() == n;
  bool usable = true;
  for (size_t k = 0; k < row_segs.size() && usable; ++k) {
    double mean = 0.0;
    for (int b = 0; b < L->n_wg; ++b) mean += (double)L->h_times[k * (size_t)L->n_wg + (size_t)b];
    mean /= (double)L->n_wg;
    if (!(mean > 0.0)) usable = false;
    for (int b = 0; b < L->n_wg && usable; ++b) {
      const size_t i = k * (size_t)L->n_wg + (size_t)b;
      const double t = (double)L->h_times[i];
      double f = t > 0.0 ? mean / t : 1.0;
      f = std::min(1.15, std::max(0.85, f));
      share[i] = (had ? L->share[i] : 1.0) * f;
    }
  }
  L->times_pending = false;
  ++L->rebalances;
  if (!usable) return DSGD_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));   // (the tables in use go away)
  L->share = share;
  return fstep_build(c, row_segs, L->n_wg, *L);
}

// The packed copies of the split streams for the kernel's PACKED form, built once per split by the first chunked launch that
// may use them (on the launch stream, in front of that launch).  *packed: they are there.  No memory for them (6 bytes per
// hot slot + 4 per cold slot) is no error: the plain form runs, and the split is not asked again.
static int fstep_packed_streams(dsgd_ctx* c, bool* packed) {
  *packed = false;
  if (!fstep_packed_wanted(c->k, route_facts(c)) || c->packed_state < 0) return DSGD_OK;
  if (c->packed_state == 0) {
    const size_t nh = (size_t)(c->hot_nnz + WS_PAD), nc = (size_t)(c->coldm_nnz + WS_PAD);
    hipError_t e = c->d_hcolf.try_alloc(nh);
    if (e == hipSuccess) e = c->d_hvaly.try_alloc(nh);
    if (e == hipSuccess) e = c->d_cvaly.try_alloc(nc);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      c->d_hcolf.reset(), c->d_hvaly.reset(), c->d_cvaly.reset();
      c->packed_state = -1;
      return DSGD_OK;
    }
    // (the padding behind the streams: zero ranks without a flag, zero values)
    HIP_TRY(hipMemsetAsync(c->d_hcolf + c->hot_nnz, 0, sizeof(unsigned short) * WS_PAD, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_hvaly + c->hot_nnz, 0, sizeof(float) * WS_PAD, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_cvaly + c->coldm_nnz, 0, sizeof(float) * WS_PAD, c->stream));
    const int blocks = (int)std::max<long long>(1, std::min<long long>((c->n_rows + 3) / 4, (long long)c->n_cu * 16));
    hipLaunchKernelGGL(dsgd_pack_streams_kernel, dim3(blocks), dim3(256), 0, c->stream, c->n_rows, view(c).label, c->d_hrow_ptr,
                       c->d_ctp, c->d_hcol, c->d_hval, c->d_cval, c->d_hcolf, c->d_hvaly, c->d_cvaly);
    HIP_TRY(hipGetLastError());
    c->packed_state = 1;
  }
  *packed = true;
  return DSGD_OK;
}

static int launch_fstep(dsgd_ctx* c, const std::vector<StreamSeg>& row_segs, int n_wg) {
  const int n_workers = (int)row_segs.size();
  dsgd_ctx::FstepLayout* L = nullptr;
  DSGD_TRY(fstep_layout(c, row_segs, n_wg, &L));
  bool packed = false;
  DSGD_TRY(fstep_packed_streams(c, &packed));
  DSGD_TRY(fstep_maybe_rebalance(c, row_segs, L));
  ++L->launches;
  c->last_fstep_rebalances = L->rebalances;
  const int H = std::min(c->hsplit, c->dp);
  const int nc = c->dp - H;   // (fstep_possible: all of them inside the LDS tile)
  dim3 grid((unsigned)n_wg, (unsigned)n_workers);
  DSGD_TRY(ensure_part(c, c->d_part, &c->part_wgs, &c->part_stride, (long long)n_wg * n_workers, H));
  DSGD_TRY(ensure_part(c, c->d_partc, &c->partc_wgs, &c->partc_stride, (long long)n_wg * n_workers, nc));
  // LDS: the largest of the three phases' tiles
  const size_t lds_a = sizeof(float) * (size_t)(((nc + 3) & ~3) + 16 * CT_STRIP);
  const size_t lds_b = sizeof(float) * (size_t)(16 * WS_COEF_STRIDE + 2 * H + 64 + 4 + 4);   // (+ 4: the hot tiles' counter)
  const size_t lds_c = sizeof(float) * (size_t)(((nc + 64 + 3) & ~3) + 16 * CT_STRIP);
  const size_t lds = std::max(lds_a, std::max(lds_b, lds_c));
  // the fixed-point scale of the hot accumulators: one contribution per row and column, |contribution| <= 2^shift, a
  // chunk's rows known -- refined once per configuration by the data (dsgd_fstep_bound_kernel)
  const int shift0 = std::max(1, std::min(c->k.max_shift, 30 - rows_bits(L->worst_rows)));
  int shift = shift0;
  if (c->k.fix_bound && shift0 < c->k.max_shift) {
    if (L->shift < 0) {
      DSGD_TRY(c->d_bound.reserve(1));
      HIP_TRY(hipMemsetAsync(c->d_bound, 0, sizeof(unsigned int), c->stream));
      hipLaunchKernelGGL(dsgd_fstep_bound_kernel, grid, dim3(1024), sizeof(unsigned int) * (size_t)(H + 16), c->stream, c->d_hrow_ptr,
                         c->d_hcol, c->d_hval, L->d_chunks, view(c), c->d_wlong_rows, H, std::ldexp(1.0f, shift0 - c->vexp), c->d_bound);
      HIP_TRY(hipGetLastError());
      unsigned int amax = 0;
      HIP_TRY(hipMemcpyAsync(&amax, c->d_bound, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      L->shift = refine_shift(shift0, c->k.max_shift, amax, L->worst_rows);
    }
    shift = L->shift;
  }
  const float main_scale = std::ldexp(1.0f, shift - c->vexp);
  c->last_shift = std::min(shift, c->cold_shift);   // (the coarser of the two grids of this launch)
  CsrView mh = view(c);
  mh.row_ptr = c->d_hrow_ptr;
  mh.col = reinterpret_cast<const int*>(c->d_hcol.get());   // 16-bit ranks; the kernel reinterprets the pointer
  mh.val = c->d_hval;
  if (packed) {   // (the same slots, tile tables and chunk records: flags in the rank words, y * x as values)
    mh.col = reinterpret_cast<const int*>(c->d_hcolf.get());
    mh.val = c->d_hvaly;
  }
  unsigned long long* const wg_times = (c->k.fstep_rebalance && L->rebalances < 2) ? L->d_times.get() : nullptr;
  size_t slot = 0;
  DSGD_TRY(prof_begin(c, &slot));
  c->ctr_known = false;
  if (packed)
    hipLaunchKernelGGL(dsgd_fstep_kernel<true>, grid, dim3(1024), lds, c->stream, mh, view(c), L->d_tiles + 1, L->d_meta, L->d_ctiles + 1,
                       L->d_cmeta, (const void*)c->d_ccol, c->d_cvaly, L->d_chunks, c->d_w, c->d_g64, (long long)c->dp, c->d_sc, H, nc,
                       main_scale, c->fix_scale, c->d_coef8, c->d_dcold, c->d_wlong_rows, c->d_part, c->part_stride, c->d_partc,
                       c->partc_stride, c->d_tprof, wg_times);
  else
    hipLaunchKernelGGL(dsgd_fstep_kernel<false>, grid, dim3(1024), lds, c->stream, mh, view(c), L->d_tiles + 1, L->d_meta, L->d_ctiles + 1,
                       L->d_cmeta, (const void*)c->d_ccol, c->d_cval, L->d_chunks, c->d_w, c->d_g64, (long long)c->dp, c->d_sc, H, nc,
                       main_scale, c->fix_scale, c->d_coef8, c->d_dcold, c->d_wlong_rows, c->d_part, c->part_stride, c->d_partc,
                       c->partc_stride, c->d_tprof, wg_times);
  c->last_fstep_packed = packed;
  HIP_TRY(hipGetLastError());
  DSGD_TRY(prof_end(c, slot));
  c->last_grad_kernel = "dsgd_fstep_kernel";
  DSGD_TRY(ensure_redpart(c));
  c->fused_args = {H, n_wg, H, nc, n_wg, 1.0 / (double)main_scale, 1.0 / (double)c->fix_scale};
  c->fused_apply_pending = true;   // launched by launch_finish_sync, which knows lr
  return DSGD_OK;
}
