// Evaluation over a list of rows (ref: core/Master.scala:109-118): localSampledLoss / localSampledAccuracy fold loss and
// accuracy over `Random.shuffle(workingData.indices) take samplesCount map workingData`.  ONE launch evaluates the rows a
// device-resident int32 list names and leaves the three exact tallies {#p==y, #p==0, #p==-y} of dsgd_eval_kernel in
// DevScalars::counts[0..2] (and the list's length in counts[3], as the range kernels leave their row count).
//
// The dot of a row is the one dsgd_predict_ranges decides a row on -- row_dot<G, 4, true> over the hw hottest weights in LDS
// in fp32, row_dot64<16> on the rank-ordered Double weights in fp64 -- with its lanes per row and its weight tile, so what
// that call documents carries over: the implied predictions are dsgd_forward's / dsgd_forward_f64's, entry for entry.
//
// Workgroups are persistent: the group of lanes g takes the list positions g, g + n_groups, ...  An entry outside
// [0, n_rows) raises the context's error flag as dsgd_forward_kernel does and is skipped (the host answers DSGD_ERANGE and
// writes nothing).  A row named twice is counted twice: the reference's `map workingData` keeps duplicates.  The list holds
// ROW numbers: a sampled call's window base is added where the list is written (dsgd_jr_slice_job_kernel's split_begin),
// nowhere here.
//
// Tallies: a group's first lane counts in registers; block_tally3 folds them over the wave and the workgroup and issues ONE
// global atomic per counter and workgroup -- at most n_cu (fp32) or 8 n_cu (fp64, 256-lane groups) same-address atomics per
// counter and launch, which the L2 serves one after the other.
#pragma once

// fp32: 1024-lane workgroups, one per CU at most.  Dynamic LDS: hw floats of weights, then 4 words for the tallies (the
// launch allocates hw + 4 floats, as dsgd_eval_kernel's does: up to 160 KiB, one workgroup per CU whatever the registers).
template <int G>
__global__ void __launch_bounds__(1024) dsgd_eval_list_kernel(CsrView m, const float* __restrict__ w, const int* __restrict__ idx, long long n,
                                                             DevScalars* sc, int hw) {
  constexpr int UNR = 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wl = lds;
  for (int j = threadIdx.x; j < hw; j += blockDim.x) wl[j] = w[j];
  __syncthreads();
  const int sub = threadIdx.x % G;
  const long long group = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const long long n_groups = (long long)gridDim.x * blockDim.x / G;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {   // (uniform over the group)
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    RowRegs<G, UNR> r;
    const float d = row_dot<G, UNR, true>(m, m.row_ptr[row], m.row_ptr[row + 1], wl, w, hw, sub, r);
    const float yd = (float)m.label[row] * d;
    if (sub == 0) {
      if (yd < 0.0f) c0++;
      else if (yd > 0.0f) c2++;
      else c1++;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&sc->counts[3], (unsigned long long)n);
  block_tally3(c0, c1, c2, sc, reinterpret_cast<unsigned int*>(wl + hw));
}

// fp64 (float or Double feature values): 256-lane workgroups, one 16-lane group per row, no weight tile -- the launch of
// dsgd_predict64_kernel / dsgd_eval64_kernel.
template <typename V>
__device__ __forceinline__ void eval_list64_body(const CsrViewT<V>& m, const double* __restrict__ w, const int* __restrict__ idx, long long n,
                                                 DevScalars* sc, unsigned int threads) {
#pragma clang fp contract(off)
  __shared__ unsigned int tally[4];
  const int sub = threadIdx.x % 16;
  const long long group = ((long long)blockIdx.x * threads + threadIdx.x) / 16;
  const long long n_groups = (long long)gridDim.x * threads / 16;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (long long t = group; t < n; t += n_groups) {
    const long long row = idx[t];
    if (row < 0 || row >= m.n_rows) {
      if (sub == 0) atomicOr(&sc->err, 1);
      continue;
    }
    const double d = row_dot64<16>(m, row, w, 0, sub);
    const double yd = (double)m.label[row] * d;
    if (sub == 0) {
      if (yd < 0.0) c0++;
      else if (yd > 0.0) c2++;
      else c1++;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&sc->counts[3], (unsigned long long)n);
  block_tally3(c0, c1, c2, sc, tally);
}
__global__ void __launch_bounds__(256) dsgd_eval_list64_kernel(CsrView m, const double* __restrict__ w, const int* __restrict__ idx, long long n,
                                                              DevScalars* sc) {
  eval_list64_body(m, w, idx, n, sc, blockDim.x);
}
__global__ void __launch_bounds__(256) dsgd_eval_list64v_kernel(CsrView64 m, const double* __restrict__ w, const int* __restrict__ idx, long long n,
                                                               DevScalars* sc) {
  eval_list64_body(m, w, idx, n, sc, blockDim.x);
}
