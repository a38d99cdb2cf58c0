// Host side of the column lists (device code: csrc/dsgd_tcol.hpp): whole-split steps of 10^3 .. 10^5 rows, and the device-side
// sort by (worker, column) that the logistic model's column lists share (csrc/dsgd_lg_calls.hpp: lgc_layout).  Included by
// dsgd_hip.hip behind the helpers it uses (view, prof_begin, ensure_redpart, layout_room).

static dim3 tcol_row_grid(long long mx, int n_workers) {
  return dim3((unsigned)std::max<long long>(1, std::min<long long>((mx + TC_ROWS_PER_WG - 1) / TC_ROWS_PER_WG, 8192)), (unsigned)n_workers);
}
// A layout builder's allocation or HIP call failed: declined for THIS call only (memory may be there the next time) -- the
// error cleared, the stream idle before the builder's buffers go, nothing remembered; 1 = the caller's other path.
static int layout_soft_fail(dsgd_ctx* c) {
  (void)hipGetLastError();
  (void)hipStreamSynchronize(c->stream);
  return 1;
}
#define LAYOUT_SOFT(expr)                                  \
  do {                                                     \
    if ((expr) != hipSuccess) return layout_soft_fail(c);  \
  } while (0)
// The sort of the entries of the ranges in c->d_segs by (worker, column), n_keys = workers x dp keys: per key its count, where
// its entries start, a cursor for the family's fill kernel and its compact id.  Scratch: released with the builder, the
// stream idle by then (every path out of a layout builder synchronises).
struct ColSort {
  int n_keys = 0;
  DevBuf<unsigned int> d_cnt, d_ptr, d_cursor;
  DevBuf<int> d_cid;
  DevBuf<unsigned long long> d_tot;
  unsigned long long tot[2] = {0, 0};   // entries, keys that have any
  // count and scan; returns behind them, with tot (the stream idle: whatever the caller enqueued from its locals is done too)
  hipError_t count(dsgd_ctx* c, dim3 grid, int n_keys_) {
    n_keys = n_keys_;
    hipError_t e = d_cnt.try_alloc((size_t)n_keys);
    if (e == hipSuccess) e = d_ptr.try_alloc((size_t)n_keys + 1);
    if (e == hipSuccess) e = d_cursor.try_alloc((size_t)n_keys);
    if (e == hipSuccess) e = d_cid.try_alloc((size_t)n_keys);
    if (e == hipSuccess) e = d_tot.try_alloc(2);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, sizeof(unsigned int) * (size_t)n_keys, c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dsgd_tc_count_kernel, grid, dim3(TC_THREADS), 0, c->stream, view(c), c->d_segs, c->dp, d_cnt);
    hipLaunchKernelGGL(dsgd_tc_scan_kernel, dim3(1), dim3(TC_THREADS), 0, c->stream, d_cnt, n_keys, d_ptr, d_cursor, d_cid, d_tot);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
  }
  // the gradient kernel's workgroups: n_shares shares of `share` entries each (enqueued; the caller checks behind its fill kernel)
  void shares(dsgd_ctx* c, long long n_ent, int share, int n_shares, TcShare* out) {
    hipLaunchKernelGGL(dsgd_tc_shares_kernel, dim3((unsigned)((n_shares + 255) / 256)), dim3(256), 0, c->stream, d_ptr, d_cid, n_keys, n_ent, share,
                       n_shares, out);
  }
};

// ---- column lists: whole-split steps of 10^3 .. 10^5 rows (csrc/dsgd_tcol.hpp) ----------------------------------------
// the layout of these ranges (c->d_segs holds them): 1 = not possible (too many entries, no memory: the caller's other path)
static int tcol_layout(dsgd_ctx* c, const std::vector<WorkSeg>& segs, long long mx, dsgd_ctx::TcolLayout** out) {
  const int n_workers = (int)segs.size();
  std::vector<long long> key;
  for (const WorkSeg& sg : segs) {
    key.push_back(sg.begin);
    key.push_back(sg.end);
  }
  if (auto* e = c->tcol_cache.find(key, 0, c->layout_gen)) {
    if (e->declined) return 1;   // (declined before -- too many entries: not tried again step after step)
    c->tcol_gate.hit();
    *out = &e->layout;
    return DSGD_OK;
  }
  if (!c->tcol_gate.miss()) return 1;   // (a caller that never repeats a configuration: the back-off, csrc/dsgd_route.hpp)
  DSGD_TRY(layout_room(c, c->tcol_cache));
  dsgd_ctx::TcolLayout L;
  // every worker's rows padded to whole 64-row blocks of the bitmap (a workgroup of the dot kernel writes two whole words)
  std::vector<int> bit_base((size_t)n_workers);
  long long bits = 0;
  for (int k = 0; k < n_workers; ++k) {
    bit_base[(size_t)k] = (int)bits;
    bits += ((segs[(size_t)k].end - segs[(size_t)k].begin + 63) / 64) * 64;
  }
  if (bits > TC_MAX_BITS) {   // remembered as declined: the caller's other path takes this configuration from now on
    c->tcol_cache.insert_declined(std::move(key), 0, c->layout_gen);
    return 1;
  }
  L.bm_words = (int)(((bits >> 5) + 3) & ~3LL);
  LAYOUT_SOFT(L.d_bit_base.try_alloc((size_t)n_workers));
  LAYOUT_SOFT(L.d_bitmap.try_alloc((size_t)L.bm_words));
  LAYOUT_SOFT(hipMemcpyAsync(L.d_bit_base, bit_base.data(), sizeof(int) * (size_t)n_workers, hipMemcpyHostToDevice, c->stream));
  LAYOUT_SOFT(hipMemsetAsync(L.d_bitmap, 0, sizeof(unsigned int) * (size_t)L.bm_words, c->stream));
  const dim3 grid = tcol_row_grid(mx, n_workers);
  ColSort sort;
  LAYOUT_SOFT(sort.count(c, grid, n_workers * c->dp));   // (also: bit_base is a local)
  if (sort.tot[0] == 0 || sort.tot[0] >= (1ULL << 31)) {   // (as above)
    c->tcol_cache.insert_declined(std::move(key), 0, c->layout_gen);
    return 1;
  }
  L.n_ent = (long long)sort.tot[0];
  long long share = (L.n_ent + c->n_cu - 1) / std::max(1, c->n_cu);
  share = std::max<long long>(1024, std::min<long long>(TC_MAX_SHARE, (share + 63) & ~63LL));
  if (c->k.tcol_share > 0) share = std::max<long long>(64, std::min<long long>(TC_MAX_SHARE, (c->k.tcol_share + 3) & ~3));   // (whole 16-byte pieces)
  L.share = (int)share;
  L.n_wg = (int)((L.n_ent + share - 1) / share);
  {   // whole 16-byte pieces; the last one's padding is zero
    const size_t n_pad = ((size_t)L.n_ent + 3) & ~(size_t)3;
    LAYOUT_SOFT(L.d_ent_pk.try_alloc(n_pad));
    LAYOUT_SOFT(L.d_ent_val.try_alloc(n_pad));
    LAYOUT_SOFT(hipMemsetAsync(L.d_ent_pk + (n_pad - 4), 0, sizeof(unsigned int) * 4, c->stream));
    LAYOUT_SOFT(hipMemsetAsync(L.d_ent_val + (n_pad - 4), 0, sizeof(float) * 4, c->stream));
  }
  LAYOUT_SOFT(L.d_shares.try_alloc((size_t)L.n_wg));
  LAYOUT_SOFT(L.d_key_of_cid.try_alloc((size_t)std::max<unsigned long long>(1, sort.tot[1])));
  sort.shares(c, L.n_ent, L.share, L.n_wg, L.d_shares);
  hipLaunchKernelGGL(dsgd_tc_fill_kernel, grid, dim3(TC_THREADS), 0, c->stream, view(c), c->d_segs, c->dp, sort.d_cursor, sort.d_cid, L.d_shares,
                     L.share, L.d_bit_base, L.d_ent_pk, L.d_ent_val, L.d_key_of_cid);
  LAYOUT_SOFT(hipGetLastError());
  LAYOUT_SOFT(hipStreamSynchronize(c->stream));
  *out = &c->tcol_cache.insert(std::move(key), 0, c->layout_gen, std::move(L))->layout;
  return DSGD_OK;
}
// the gradient of the ranges in c->d_segs by column lists; 1 = declined (nothing launched: the caller's other path)
static int launch_tcol(dsgd_ctx* c, const std::vector<WorkSeg>& segs, long long mx) {
  const int n_workers = (int)segs.size();
  dsgd_ctx::TcolLayout* L = nullptr;
  const int lrc = tcol_layout(c, segs, mx, &L);
  if (lrc != DSGD_OK) return lrc;
  const int shift = std::max(1, std::min(c->k.max_shift, 30));   // 64-bit sums: nothing to bound (|contribution| <= 2^shift)
  c->last_shift = shift;
  const float scale = std::ldexp(1.0f, shift - c->vexp);
  size_t slot = 0;
  DSGD_TRY(prof_begin(c, &slot));
  c->ctr_known = false;
  // 32 rows (512 lanes) per workgroup while that leaves the CUs a few workgroups each: finer grains fill them evenly
  // (18,519 rows: 290 workgroups of 64 rows leave 34 CUs with two and the rest with one)
  dim3 dgrid = tcol_row_grid(mx, n_workers);
  hipLaunchKernelGGL(dsgd_tc_dot_kernel<TC_THREADS>, dgrid, dim3(TC_THREADS), 0, c->stream, view(c), c->d_w, c->d_segs, L->d_bit_base,
                     L->d_bitmap, std::min(TC_WL, c->dp & ~3));
  HIP_TRY(hipGetLastError());
  TcGradArgs a;
  a.ent_pk = L->d_ent_pk;
  a.ent_val = L->d_ent_val;
  a.shares = L->d_shares;
  a.key_of_cid = L->d_key_of_cid;
  a.bitmap = L->d_bitmap;
  a.g64 = c->d_g64;
  a.sc = c->d_sc;
  a.n_ent = L->n_ent;
  a.share = L->share;
  a.bm_words = L->bm_words;
  a.scale = scale;
  {
    const dim3 g2((unsigned)L->n_wg);
    const size_t lds = sizeof(long long) * (size_t)L->share + sizeof(unsigned int) * (size_t)L->bm_words + 64;
    if (L->share <= 4 * TC_THREADS) hipLaunchKernelGGL(dsgd_tc_grad_kernel<1>, g2, dim3(TC_THREADS), lds, c->stream, a);
    else hipLaunchKernelGGL(dsgd_tc_grad_kernel<2>, g2, dim3(TC_THREADS), lds, c->stream, a);
  }
  HIP_TRY(hipGetLastError());
  DSGD_TRY(prof_end(c, slot));
  c->last_grad_kernel = "dsgd_tc_grad_kernel";
  DSGD_TRY(ensure_redpart(c));
  const double inv = 1.0 / (double)scale;
  c->fused_args = {0, 0, (c->dp + 3) & ~3, 0, 0, inv, inv};   // no partials: the exact sums are in the 64-bit accumulators
  c->fused_apply_pending = true;   // launched by launch_finish_sync, which knows lr
  return DSGD_OK;
}
