// The reference's Sparse{map<int32, double>, size} form at the boundary (include/dsgd.h "SPARSE VALUES").
//   dsgd_sparse_compact_kernel  a device vector of dp slots (rank order, read through the key -> rank permutation, or key
//                               order when perm == nullptr) -> the (key, value) pairs with |(double)v| > 1e-20 (what
//                               math/Sparse.scala:104-118 keeps), keys ascending, and their exact count
//   dsgd_sparse_scatter_kernel  the pairs -> the resident weight vector, 0 elsewhere
// Included by dsgd_hip.hip after dsgd_cs64.hpp (filt, filt64, DevScalars).
#pragma once

// ---- compaction ---------------------------------------------------------------------------------------------------
// One launch for any dp >= 1.  A workgroup takes a TILE of SP_TILE consecutive KEYS (4 per lane: the lane's pairs stay in key
// order), in the order of a ticket -- so every tile in front of it belongs to a workgroup that is already running.  Lanes
// scan their counts across the wave (shuffles), waves across the workgroup (LDS), workgroups across the grid: a workgroup
// publishes its tile's count as ONE 8-byte granule {tag = the launch's epoch, count} (a relaxed agent-scope atomic store: the
// datum is the flag, no fence) and then sums the granules of the tiles in front of it, wave 0 polling 64 of them per pass.
// Nobody waits before it has published, so the chain cannot close on itself; the poll is bounded (SP_POLL_LIMIT) and a
// workgroup that gives up raises hdr[1] and writes nothing (the host then reports DSGD_ESTATE and resets the state).
// The epoch and the ticket base are launch arguments: the state needs no memset in front of a launch (these launches are
// never captured into a graph).  REG (fp32 gradient requests): the slot is regularised on the way -- g <- filt(g); on the
// support g <- filt(g + s), operation for operation dsgd_regularize_kernel -- and cleared behind the read, so ONE launch
// replaces regularise + permute-out + memset.  The output pointers may be host-mapped memory.
constexpr int SP_THREADS = 1024;
constexpr int SP_ITEMS = 4;
constexpr int SP_TILE = SP_THREADS * SP_ITEMS;
constexpr unsigned int SP_POLL_LIMIT = 1u << 20;
constexpr double SP_EPS = 1e-20;   // ref: math/Sparse.scala:104 (Sparse.epsilon)

// state: [0] the ticket counter (it only grows: a launch subtracts its base), [1] unused, [2 + t] tile t's granule
constexpr int SP_STATE_HEAD = 2;

template <typename TIn, typename TOut, bool REG>
__global__ void __launch_bounds__(SP_THREADS) dsgd_sparse_compact_kernel(TIn* in, const int* __restrict__ perm, int dp, const DevScalars* sc,
                                                                        unsigned long long* state, unsigned long long ticket_base,
                                                                        unsigned int epoch, int* key_out, TOut* val_out,
                                                                        unsigned long long* hdr /* [0] count, [1] gave up */) {
  __shared__ unsigned int s_tile, s_prefix, s_fail;
  __shared__ unsigned int s_wave[SP_THREADS / 64];
  if (threadIdx.x == 0)
    s_tile = (unsigned int)(__hip_atomic_fetch_add(&state[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - ticket_base);
  __syncthreads();
  const unsigned int tile = s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long j0 = (long long)tile * SP_TILE + (long long)threadIdx.x * SP_ITEMS;
  float s = 0.0f;
  bool add = false;
  if (REG) {
    s = sc->s_reg;
    add = (s != 0.0f) && (fabsf(s) > DSGD_EPS);
  }
  TOut v[SP_ITEMS];
  unsigned int keep = 0u;
#pragma unroll
  for (int k = 0; k < SP_ITEMS; ++k) {
    v[k] = (TOut)0;
    if (tile < gridDim.x && j0 + k < dp) {
      const int r = perm ? perm[j0 + k] : (int)(j0 + k);
      TIn x = in[r];
      if (REG) {
        float g = filt((float)x);
        if (add && g != 0.0f) g = filt(g + s);
        x = (TIn)g;
        in[r] = (TIn)0;
      }
      v[k] = (TOut)x;
      if (fabs((double)v[k]) > SP_EPS) keep |= 1u << k;
    }
  }
  const unsigned int cnt = (unsigned int)__popc(keep);
  unsigned int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned int wave_base = 0u, total = 0u;
#pragma unroll
  for (int i = 0; i < SP_THREADS / 64; ++i) {
    const unsigned int t = s_wave[i];
    if (i < wave) wave_base += t;
    total += t;
  }
  if (wave == 0) {
    if (lane == 0 && tile < gridDim.x)
      __hip_atomic_store(&state[SP_STATE_HEAD + tile], ((unsigned long long)epoch << 32) | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned int acc = 0u;
    bool ok = tile < gridDim.x;   // (a ticket beyond the grid: the state is not this launch's -- give up)
    for (unsigned int t0 = 0; ok && t0 < tile; t0 += 64) {   // (wave-uniform)
      const unsigned int t = t0 + lane;
      unsigned int val = 0u;
      bool have = t >= tile;
      for (unsigned int spin = 0;; ++spin) {
        if (!have) {
          const unsigned long long x = __hip_atomic_load(&state[SP_STATE_HEAD + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((unsigned int)(x >> 32) == epoch) {
            val = (unsigned int)x;
            have = true;
          }
        }
        if (__all(have)) break;
        if (spin > SP_POLL_LIMIT) {
          ok = false;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      acc += val;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
      s_prefix = acc;
      s_fail = ok ? 0u : 1u;
    }
  }
  __syncthreads();
  if (s_fail) {
    if (threadIdx.x == 0) hdr[1] = 1ull;
    return;
  }
  unsigned int pos = s_prefix + wave_base + incl - cnt;
#pragma unroll
  for (int k = 0; k < SP_ITEMS; ++k)
    if (keep & (1u << k)) {
      key_out[pos] = (int)(j0 + k);
      val_out[pos] = v[k];
      ++pos;
    }
  if (tile == gridDim.x - 1 && threadIdx.x == 0) hdr[0] = (unsigned long long)s_prefix + total;
}

// ---- scatter-in ---------------------------------------------------------------------------------------------------
// w <- 0, then w[perm[key[i]]] = filt(val[i]) -- what the dense setters store (dsgd_permute_in_kernel, dsgd_permute64_in_kernel,
// dsgd_promote64_in_kernel).  ONE launch without a hand-off between workgroups: a workgroup OWNS the ranks [lo, hi), clears
// them, and after its own barrier stores the pairs that land there (every workgroup reads all the keys: at most
// SP_SCATTER_BLOCKS times nnz gathers).  The keys are validated on the host (in range, each once): no two stores race.
constexpr int SP_SCATTER_BLOCKS = 16;

__device__ __forceinline__ float sp_store_filt(float v, float) { return filt(v); }
__device__ __forceinline__ double sp_store_filt(double v, double) { return filt64(v); }
__device__ __forceinline__ double sp_store_filt(float v, double) { return filt64((double)v); }

template <typename TIn, typename TW>
__global__ void __launch_bounds__(SP_THREADS) dsgd_sparse_scatter_kernel(const int* __restrict__ key, const TIn* __restrict__ val, int nnz,
                                                                        const int* __restrict__ perm, TW* w, int dp) {
  const int per = (dp + (int)gridDim.x - 1) / (int)gridDim.x;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < dp ? lo + per : dp;
  for (long long r = lo + threadIdx.x; r < hi; r += SP_THREADS) w[r] = (TW)0;
  __syncthreads();   // (a workgroup-scope fence: the clearing stores are in front of the ones below)
  for (int i = threadIdx.x; i < nnz; i += SP_THREADS) {
    const int r = perm[key[i]];
    if (r >= lo && r < hi) w[r] = sp_store_filt(val[i], (TW)0);
  }
}
