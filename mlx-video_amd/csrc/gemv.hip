// ltxk_gemv_w8: out[m,n] = bf16(acc * w_scale[n] + bias[n]), acc = A[m,:] . W[n,:] in fp32, for 1 <= M <= 8 rows of bf16
// activations over an (N,K) e4m3fn panel - the decode step of the Gemma-3 language model on fp8 panels, where a launch is a
// pure weight stream (one output row per batch row) and the MFMA tile forms multiply 63 empty rows, stage W through LDS and
// need a second launch to sum their K slices.
//
// Shape.  A wave owns GEMV_R = 2 rows of W at a time and streams them from global memory straight into VGPRs: a "pass" is
// one 16-byte load per lane = 1024 consecutive k of one row, lane l holding k = 1024 p + 16 l .. + 15.  GEMV_U = 4 passes of both
// rows (8 independent 1-KiB loads per wave) are issued before the first is used; W never touches LDS.  The M rows of A are
// staged ONCE per workgroup into LDS (32 KiB: 16384 / MT k per chunk, MT = M rounded up to 1, 2, 4 or 8; rows M .. MT-1 are
// zeros), in the image a pass reads without bank conflicts: per pass, the lanes' first 8 k (16 bytes each) contiguous, then
// their second 8.  When K fits one chunk (M = 1: K <= 16384) a workgroup keeps its A image over `groups` row sets.
//
// Arithmetic.  e4m3 -> fp32 by v_cvt_pk_f32_fp8 (exact), bf16 -> fp32 by a shift / a mask (exact), then one fp32 FMA per
// product into TWO accumulators per (row of W, row of A) and lane - even and odd k - in ascending k; after the last pass
// even + odd, then the wave's butterfly (32, 16, 8, 4, 2, 1), then * w_scale[n] (if given), + bias[n] (if given), each one fp32
// rounding, then one rounding to bf16.  That order is a function of K alone: the bits of out[m,n] depend on row m of A,
// row n of W, w_scale[n] and bias[n], and on nothing else - not on M (MT only adds independent chains), not on N, the other
// rows, the chunking of A or the grid.
//
// Edges.  K % 16 == 0, so a lane's 16 k are all inside a row or all outside: the ragged last pass is the same code under
// k < K per lane, and no load reaches past a row of W or of A.  The last wave's second row, when N is odd, and the waves past
// N are clamped to row N - 1 and store nothing.  No atomics, no scratch memory.
#include "common.h"

namespace ltxk {

constexpr int GEMV_THREADS = 256;
constexpr int GEMV_WAVES = GEMV_THREADS / LTXK_WAVE;
constexpr int GEMV_R = 2;                 // rows of W per wave and pass
constexpr int GEMV_U = 4;                 // passes in flight per row (2 at MT = 8)
constexpr int GEMV_PASS = 1024;           // k per pass: 64 lanes x 16 e4m3
constexpr int GEMV_LDS_K = 16384;         // bf16 elements of the A image (32 KiB), shared by the MT rows
constexpr int GEMV_MAX_M = 8;
constexpr int GEMV_MAX_GROUPS = 8;
constexpr int GEMV_WG_SLOTS = 256 * 4;    // 256 CUs x the 4 workgroups one holds (VGPRs; 5 by the LDS image)

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the 16 products of one lane and pass for one row of W (w: its 16 e4m3 bytes) and one row of A (lo / hi: k 0..7 / 8..15 as
// bf16 pairs), into the even / odd accumulator pair
__device__ __forceinline__ f32x2 gemv_fma16(u32x4 w, u32x4 lo, u32x4 hi, f32x2 acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned a01 = i < 2 ? lo[2 * i] : hi[2 * i - 4], a23 = i < 2 ? lo[2 * i + 1] : hi[2 * i - 3];
    const f32x2 w01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), w23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    const f32x2 x01 = {__uint_as_float(a01 << 16), __uint_as_float(a01 & 0xffff0000u)};
    const f32x2 x23 = {__uint_as_float(a23 << 16), __uint_as_float(a23 & 0xffff0000u)};
    acc = __builtin_elementwise_fma(x01, w01, acc);
    acc = __builtin_elementwise_fma(x23, w23, acc);
  }
  return acc;
}

template <int MT>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_w8_kernel(const bf16* __restrict__ A, int lda, const uint8_t* __restrict__ W,
                                                               const float* __restrict__ w_scale, const bf16* __restrict__ bias,
                                                               bf16* __restrict__ out, int ldo, int M, int N, int K, int groups) {
  constexpr int KC = GEMV_LDS_K / MT;                 // k per chunk of the A image
  constexpr int ROW_BYTES = KC * 2;
  constexpr int U = MT == 8 ? 2 : GEMV_U;            // (MT = 8: a chunk is two passes, and 8 rows of A fragments fill the registers)
  __shared__ __attribute__((aligned(16))) unsigned char sA[GEMV_LDS_K * 2];
  const int lane = threadIdx.x & (LTXK_WAVE - 1), wave = threadIdx.x >> 6;
  const int full = K / GEMV_PASS;                     // passes every lane takes part in
  const bool ragged = K % GEMV_PASS != 0;
  const bool one_chunk = K <= KC;

  for (int g = 0; g < groups; ++g) {
    const int64_t n0 = (((int64_t)blockIdx.x * groups + g) * GEMV_WAVES + wave) * GEMV_R;
    const bool live = n0 < N;                          // wave-uniform
    const uint8_t* wrow[GEMV_R];
#pragma unroll
    for (int r = 0; r < GEMV_R; ++r) {
      const int64_t n = n0 + r < N ? n0 + r : N - 1;
      wrow[r] = W + (size_t)n * (size_t)K + lane * 16;
    }
    f32x2 acc[GEMV_R][MT];
#pragma unroll
    for (int r = 0; r < GEMV_R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = f32x2{0.0f, 0.0f};

    for (int c0 = 0; c0 < K; c0 += KC) {
      if (!one_chunk || g == 0) {
        // stage k = c0 .. c0 + kc of the M rows (16-byte units; unit i of a row -> pass i / 128, lane i % 128 / 2, half i % 2)
        if (c0 > 0) __syncthreads();
        const int units = ((K - c0 < KC ? K - c0 : KC)) >> 3;
        for (int i = threadIdx.x; i < units; i += GEMV_THREADS) {
          const int dst = (i >> 7) * 2048 + (i & 1) * 1024 + ((i & 127) >> 1) * 16;
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m < M) v = *(const u32x4*)(A + (size_t)m * lda + c0 + i * 8);
            *(u32x4*)(sA + m * ROW_BYTES + dst) = v;
          }
        }
        __syncthreads();
      }
      if (!live) continue;
      const int pb = c0 / GEMV_PASS;
      const int pe = (c0 + KC) / GEMV_PASS < full ? (c0 + KC) / GEMV_PASS : full;
      const unsigned char* sl = sA + (lane * 16 - pb * 2048);      // + p * 2048: pass p of the row, chunk-relative
      int p = pb;
      for (; p + U <= pe; p += U) {
        u32x4 w[U][GEMV_R];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int r = 0; r < GEMV_R; ++r) w[u][r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + (size_t)(p + u) * GEMV_PASS));
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const u32x4 lo = *(const u32x4*)(sl + m * ROW_BYTES + (p + u) * 2048), hi = *(const u32x4*)(sl + m * ROW_BYTES + (p + u) * 2048 + 1024);
#pragma unroll
            for (int r = 0; r < GEMV_R; ++r) acc[r][m] = gemv_fma16(w[u][r], lo, hi, acc[r][m]);
          }
      }
      // the chunk's remaining whole passes, then the ragged one (the row's last, so the last chunk's): lanes with k < K only
      const bool tail = ragged && full >= pb && full < (c0 + KC) / GEMV_PASS;
      for (; p < pe + (tail ? 1 : 0); ++p) {
        if (p < full || p * GEMV_PASS + lane * 16 < K) {
          u32x4 w[GEMV_R];
#pragma unroll
          for (int r = 0; r < GEMV_R; ++r) w[r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + (size_t)p * GEMV_PASS));
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const u32x4 lo = *(const u32x4*)(sl + m * ROW_BYTES + p * 2048), hi = *(const u32x4*)(sl + m * ROW_BYTES + p * 2048 + 1024);
#pragma unroll
            for (int r = 0; r < GEMV_R; ++r) acc[r][m] = gemv_fma16(w[r], lo, hi, acc[r][m]);
          }
        }
      }
    }
    if (!live) continue;
#pragma unroll
    for (int r = 0; r < GEMV_R; ++r) {
      const int64_t n = n0 + r;
      const bool stored = n < N;
      const int64_t nc = stored ? n : N - 1;
      const float sc = w_scale ? w_scale[nc] : 1.0f;
      const float bv = bias ? (float)bias[nc] : 0.0f;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        float v = wave_sum(acc[r][m][0] + acc[r][m][1]);
        if (w_scale) v = v * sc;
        if (bias) v = v + bv;
        if (lane == 0 && stored && m < M) out[(size_t)m * ldo + n] = (bf16)v;
      }
    }
  }
}

template <int MT>
static void gemv_launch(const ltxk_gemm_args* a, const float* w_scale, int blocks, int groups, hipStream_t st) {
  hipLaunchKernelGGL(gemv_w8_kernel<MT>, dim3((unsigned)blocks), dim3(GEMV_THREADS), 0, st, (const bf16*)a->A, (int)a->lda,
                     (const uint8_t*)a->W, w_scale, (const bf16*)a->bias, (bf16*)a->out, (int)a->ldo, (int)a->M, (int)a->N, (int)a->K, groups);
}

}  // namespace ltxk

extern "C" int ltxk_gemv_w8(const ltxk_gemm_args* a, const float* w_scale, void* stream) {
  using namespace ltxk;
  const char* who = "ltxk_gemv_w8";
  LTXK_CHECK_ARG(a && a->A && a->W && a->out, "%s: A, W and out must not be NULL", who);
  LTXK_CHECK_ARG(a->M >= 1 && a->M <= GEMV_MAX_M, "%s: M=%d must lie in [1, %d]", who, a->M, GEMV_MAX_M);
  LTXK_CHECK_ARG(a->N >= 1, "%s: N=%d must be positive", who, a->N);
  LTXK_CHECK_ARG(a->K >= 16 && a->K % 16 == 0, "%s: K=%d must be a positive multiple of 16", who, a->K);
  LTXK_CHECK_ARG(a->epilogue == LTXK_EPI_BIAS, "%s: epilogue %d is not supported (LTXK_EPI_BIAS only)", who, a->epilogue);
  LTXK_CHECK_ARG(!a->resid && !a->gate && !a->gate_row, "%s: resid / gate / gate_row are not supported", who);
  LTXK_CHECK_ARG(!a->out_tokens_per_batch && !a->out2 && !a->n_split, "%s: transposed and split outputs are not supported", who);
  LTXK_CHECK_ARG(!a->sumsq, "%s: sumsq is not supported", who);
  LTXK_CHECK_ARG(!a->workspace && !a->workspace_bytes, "%s: takes no workspace (one launch, no K slices)", who);
  LTXK_CHECK_ARG(a->lda >= a->K && a->lda % 8 == 0 && ((uintptr_t)a->A & 15) == 0, "%s: lda=%d must be >= K and a multiple of 8, A 16-byte aligned", who, a->lda);
  LTXK_CHECK_ARG(((uintptr_t)a->W & 15) == 0, "%s: W must be 16-byte aligned", who);
  LTXK_CHECK_ARG(a->ldo >= a->N && ((uintptr_t)a->out & 1) == 0 && ((uintptr_t)a->bias & 1) == 0, "%s: ldo=%d must be >= N, out / bias bf16 aligned", who, a->ldo);
  LTXK_CHECK_ARG(((uintptr_t)w_scale & 3) == 0, "%s: w_scale must be 4-byte aligned", who);
  const int mt = a->M == 1 ? 1 : a->M == 2 ? 2 : a->M <= 4 ? 4 : 8;
  const int64_t sets = ((int64_t)a->N + GEMV_WAVES * GEMV_R - 1) / (GEMV_WAVES * GEMV_R);      // row sets of one workgroup pass
  int64_t groups = 1;
  if (a->K <= GEMV_LDS_K / mt) {                     // the A image is staged once: let a workgroup keep it over several row sets
    // (rounded up, so that up to GEMV_MAX_GROUPS x GEMV_WG_SLOTS row sets run as ONE round of resident workgroups, no short second one)
    groups = (sets + GEMV_WG_SLOTS - 1) / GEMV_WG_SLOTS;
    groups = groups > GEMV_MAX_GROUPS ? GEMV_MAX_GROUPS : groups;
  }
  const int64_t blocks = (sets + groups - 1) / groups;
  LTXK_CHECK_ARG(blocks <= (int64_t)INT32_MAX, "%s: too many rows", who);
  hipStream_t st = (hipStream_t)stream;
  switch (mt) {
    case 1: gemv_launch<1>(a, w_scale, (int)blocks, (int)groups, st); break;
    case 2: gemv_launch<2>(a, w_scale, (int)blocks, (int)groups, st); break;
    case 4: gemv_launch<4>(a, w_scale, (int)blocks, (int)groups, st); break;
    default: gemv_launch<8>(a, w_scale, (int)blocks, (int)groups, st); break;
  }
  LTXK_CHECK_LAUNCH(who);
  return LTXK_OK;
}
