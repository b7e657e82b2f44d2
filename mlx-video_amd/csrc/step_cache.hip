// Step cache of the denoise loop (include/ltxk.h, "Step cache"): the device side of a TeaCache-style decision -
// how far block 0's modulated input has moved since the step before - and the residual arithmetic of a cached step.
//
// ltxk_step_cache_probe: cur, prev (rows, D) bf16 read as one run of n = rows * D elements, cut into chunks of
// SC_CHUNK = 8192 elements (a function of n only; the last chunk may be ragged, its missing elements count as +0, and adding
// +0 to a sum of absolute values changes no bit).  Two launches, the second ordered behind the first by the stream; no atomics
// and nobody waits for another workgroup:
//   1. sc_probe_kernel, grid (chunks): one workgroup of 256 threads per chunk.  Thread t owns the four 8-element vectors
//      v = 1024 * chunk + 256 * k + t, k = 0..3 (a wave reads 1 KiB of consecutive memory per load).  It loads cur and prev of
//      all four, stores prev <- cur (the 16 bytes it just read: the copy is exact, NaN payloads and negative zeros included),
//      and sums its 32 terms in ONE chain from 0, k ascending and inside a vector j ascending:
//        S_d term |f32(cur) - f32(prev)| (the subtraction rounds once, to fp32),  S_p term |f32(prev)| (exact).
//      Then the wave butterfly v <- v + v[lane ^ off], off = 32, 16, 8, 4, 2, 1 (common.h wave_sum: every lane ends with the
//      same bits), then thread 0 adds the four wave totals in ascending order, w0 + w1 + w2 + w3, and writes the chunk's two
//      partials: workspace[chunk] (S_d) and workspace[chunks + chunk] (S_p).
//   2. sc_merge_kernel, one workgroup: the partials staged through LDS 1024 at a time, one thread adds them in ascending chunk
//      order, S = 0 + p[0] + p[1] + ..., and writes sums[0] = S_d, sums[1] = S_p.
// The longest sequential fp32 addition chain (the tests' `depth`, tests/ref_step_cache.py): 31 in the thread (the first
// addition, to 0, is exact) + 6 butterfly levels + 3 wave totals + (chunks - 1) for the merge:
//   depth(rows, D) = SC_DEPTH_BASE + ceil(rows * D / 8192) - 1,  SC_DEPTH_BASE = 40.
// The order is a function of (rows, D) alone: nothing reads the grid, the CU count or the order workgroups finish in.
// LTXK_PROBE_INIT: launch 1 only, as a copy - no term is formed, neither the workspace nor sums is touched.
//
// ltxk_residual_store / ltxk_residual_apply: one 8-element vector per thread, in place; r <- rbf(f32(x) - f32(r)) and
// x <- rbf(f32(x) + f32(r)), rbf the round-to-nearest-even bf16 rounding of a materialised array.
#include "common.h"

namespace ltxk {

constexpr int SC_THREADS = 256;
constexpr int SC_VECS = 4;                                  // 8-element vectors per thread
constexpr int SC_CHUNK_VECS = SC_THREADS * SC_VECS;         // 1024
constexpr int SC_CHUNK = SC_CHUNK_VECS * 8;                 // 8192 elements
constexpr int SC_DEPTH_BASE = 40;
constexpr int SC_MERGE_TILE = 1024;
constexpr int64_t SC_MAX_CHUNKS = 1 << 22;                  // 2^35 elements: far above any token matrix, and the grid stays an int

__global__ __launch_bounds__(SC_THREADS) void sc_probe_kernel(const bf16* __restrict__ cur, bf16* __restrict__ prev, int64_t nvec,
                                                              float* __restrict__ part, int nchunks, int init) {
  __shared__ float red[2][SC_THREADS / LTXK_WAVE];
  const int tid = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.x * SC_CHUNK_VECS + tid;
  bf16x8 a[SC_VECS], b[SC_VECS];
#pragma unroll
  for (int k = 0; k < SC_VECS; ++k) {
    const int64_t v = v0 + k * SC_THREADS;
    if (v < nvec) {
      a[k] = *(const bf16x8*)(cur + v * 8);
      if (!init) b[k] = *(const bf16x8*)(prev + v * 8);
    }
  }
#pragma unroll
  for (int k = 0; k < SC_VECS; ++k) {
    const int64_t v = v0 + k * SC_THREADS;
    if (v < nvec) *(bf16x8*)(prev + v * 8) = a[k];
  }
  if (init) return;
  float sd = 0.f, sp = 0.f;
#pragma unroll
  for (int k = 0; k < SC_VECS; ++k) {
    const bool in = v0 + k * SC_THREADS < nvec;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float fa = in ? (float)a[k][j] : 0.f, fb = in ? (float)b[k][j] : 0.f;
      sd += fabsf(fa - fb);
      sp += fabsf(fb);
    }
  }
  sd = wave_sum(sd);
  sp = wave_sum(sp);
  if ((tid & (LTXK_WAVE - 1)) == 0) { red[0][tid >> 6] = sd; red[1][tid >> 6] = sp; }
  __syncthreads();
  if (tid == 0) {
    part[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[(size_t)nchunks + blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ __launch_bounds__(SC_THREADS) void sc_merge_kernel(const float* __restrict__ part, int nchunks, float* __restrict__ sums) {
  __shared__ float tile[2][SC_MERGE_TILE];
  float sd = 0.f, sp = 0.f;                       // thread 0's two chains
  for (int c0 = 0; c0 < nchunks; c0 += SC_MERGE_TILE) {
    const int m = nchunks - c0 < SC_MERGE_TILE ? nchunks - c0 : SC_MERGE_TILE;
    for (int i = threadIdx.x; i < m; i += SC_THREADS) {
      tile[0][i] = part[c0 + i];
      tile[1][i] = part[(size_t)nchunks + c0 + i];
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) { sd += tile[0][i]; sp += tile[1][i]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { sums[0] = sd; sums[1] = sp; }
}

template <bool STORE>
__global__ __launch_bounds__(SC_THREADS) void sc_residual_kernel(bf16* __restrict__ x, bf16* __restrict__ r, int64_t n8) {
  const int64_t idx = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (idx >= n8) return;
  const bf16x8 a = *(const bf16x8*)(x + idx * 8), b = *(const bf16x8*)(r + idx * 8);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)(STORE ? (float)a[j] - (float)b[j] : (float)a[j] + (float)b[j]);
  *(bf16x8*)((STORE ? r : x) + idx * 8) = o;
}

// two buffers of `bytes` bytes each share a byte (the kernels take both as __restrict__)
static inline bool sc_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)bytes && pb < pa + (uintptr_t)bytes;
}

static inline int64_t sc_chunks(int64_t rows, int32_t D) {
  if (rows < 1 || D < 8 || D % 8 != 0) return -1;
  if (rows > (SC_MAX_CHUNKS * SC_CHUNK) / D) return -1;
  return (rows * D + SC_CHUNK - 1) / SC_CHUNK;
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int64_t ltxk_step_cache_workspace_bytes(int64_t rows, int32_t D) {
  const int64_t c = sc_chunks(rows, D);
  return c < 0 ? -1 : 2 * c * 4;
}

extern "C" int32_t ltxk_step_cache_depth(int64_t rows, int32_t D) {
  const int64_t c = sc_chunks(rows, D);
  return c < 0 ? -1 : (int32_t)(SC_DEPTH_BASE + c - 1);
}

extern "C" int ltxk_step_cache_probe(const void* cur, void* prev, int64_t rows, int32_t D, int32_t flags, float* sums,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "ltxk_step_cache_probe";
  const int64_t nchunks = sc_chunks(rows, D);
  LTXK_CHECK_ARG(nchunks > 0, "%s: rows=%lld must be positive, D=%d a positive multiple of 8, rows * D at most 2^35", who, (long long)rows, D);
  LTXK_CHECK_ARG((flags & ~LTXK_PROBE_INIT) == 0, "%s: flags=%d must be 0 or LTXK_PROBE_INIT", who, flags);
  LTXK_CHECK_ARG(cur && prev && (((uintptr_t)cur | (uintptr_t)prev) & 15) == 0 && !sc_overlap(cur, prev, rows * D * 2),
                 "%s: cur / prev: null, overlapping or not 16-byte aligned", who);
  const int init = (flags & LTXK_PROBE_INIT) != 0;
  if (!init) {
    LTXK_CHECK_ARG(sums && workspace && (((uintptr_t)sums | (uintptr_t)workspace) & 3) == 0, "%s: sums / workspace: null or misaligned pointer", who);
    LTXK_CHECK_ARG(workspace_bytes >= 2 * nchunks * 4, "%s: workspace holds %lld bytes, %lld needed (2 * chunks * 4)", who,
                   (long long)workspace_bytes, (long long)(2 * nchunks * 4));
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t nvec = rows * D / 8;
  hipLaunchKernelGGL(sc_probe_kernel, dim3((unsigned)nchunks), dim3(SC_THREADS), 0, s, (const bf16*)cur, (bf16*)prev, nvec,
                     (float*)workspace, (int)nchunks, init);
  LTXK_CHECK_LAUNCH(who);
  if (!init) {
    hipLaunchKernelGGL(sc_merge_kernel, dim3(1), dim3(SC_THREADS), 0, s, (const float*)workspace, (int)nchunks, sums);
    LTXK_CHECK_LAUNCH(who);
  }
  return LTXK_OK;
}

static int sc_residual(const char* who, bool store, void* x, void* r, int64_t n, void* stream) {
  LTXK_CHECK_ARG(n > 0 && n % 8 == 0 && n / 8 <= (int64_t)SC_MAX_CHUNKS * SC_CHUNK_VECS, "%s: n=%lld must be a positive multiple of 8, at most 2^35",
                 who, (long long)n);
  LTXK_CHECK_ARG(x && r && (((uintptr_t)x | (uintptr_t)r) & 15) == 0 && !sc_overlap(x, r, n * 2), "%s: x / r: null, overlapping or not 16-byte aligned", who);
  const int64_t n8 = n / 8;
  const dim3 grid((unsigned)((n8 + SC_THREADS - 1) / SC_THREADS));
  if (store)
    hipLaunchKernelGGL(sc_residual_kernel<true>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, (bf16*)x, (bf16*)r, n8);
  else
    hipLaunchKernelGGL(sc_residual_kernel<false>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, (bf16*)x, (bf16*)r, n8);
  LTXK_CHECK_LAUNCH(who);
  return LTXK_OK;
}

extern "C" int ltxk_residual_store(const void* x, void* r, int64_t n, void* stream) {
  return sc_residual("ltxk_residual_store", true, (void*)x, r, n, stream);
}

extern "C" int ltxk_residual_apply(void* x, const void* r, int64_t n, void* stream) {
  return sc_residual("ltxk_residual_apply", false, x, (void*)r, n, stream);
}
