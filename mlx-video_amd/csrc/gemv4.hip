// ltxk_gemv_w4: out[m,n] = bf16(A[m,:] . w[n,:] + bias[n]) in fp32, w[n,k] = e2m1(code[n,k]) * 2^(E[n, k/32] - 127), for
// 1 <= M <= 8 rows of bf16 activations over an (N,K) OCP MXFP4 panel: (N, K/2) bytes of two e2m1 codes each (element 2i in the
// low nibble of byte i) and (N, K/32) e8m0 block-scale bytes - the decode step of the Gemma-3 language model on 4-bit panels,
// a weight stream of 4.25 bits per weight.  csrc/gemv.hip (ltxk_gemv_w8) is the model; the geometry is this format's own.
//
// Shape.  One 16-byte load per lane is 32 codes = exactly one scale block, so a "pass" is 2048 consecutive k of one row: lane l
// holds k = 2048 p + 32 l .. + 31 and needs ONE scale, byte 64 p + l of the row's scale row.  The scale bytes arrive as BYTE
// loads, one per lane: the 64 lanes of a pass read 64 consecutive bytes (one request); a dword per four lanes plus a cross-lane
// move would need 4-byte aligned scale rows, and a scale row is K/32 bytes (65 at K = 2080).  A wave owns 2 rows of W at a time
// and streams codes and scales from global memory straight into VGPRs (nontemporal loads; neither touches LDS) through a ring
// of D slots (D = 4; 2 at MT = 4 and 1 at MT = 8, where a chunk of the A image holds no more): the first D passes of both rows
// - 2 D code loads and 2 D scale loads per lane, the whole row at Gemma's K = 3840 and 4096 - are requested before the A image
// is staged and before the first is used, and a slot is requested again as soon as its pass has been consumed.  (The
// refills sit under per-lane conditions, and the compiler then waits for every outstanding load in front of a pass: past the
// first D passes a wave has one pass in flight, and the other waves of the CU cover it.)  The M rows of A are staged ONCE per
// workgroup into LDS (32 KiB: 16384 / MT k per chunk, MT = M rounded up to 1, 2, 4 or 8; rows M .. MT-1 are zeros) in the
// image a pass reads without bank conflicts: a lane's 32 k are four 16-byte quarters, and per pass and row the 64 lanes' first
// quarters lie contiguous (1 KiB), then their second, third and fourth - every ds_read_b128 of a wave covers 1024 consecutive
// bytes.  When K fits one chunk a workgroup keeps its image over `groups` row sets, rounded up to one round of resident
// workgroups.  Registers (the compiler's resource remarks, ROCm 7 hipcc -O3): MT = 1 / 2 / 4 / 8: 117 / 154 / 128 / 137 VGPRs,
// no scratch in any instance; the kernel asks for the 4 / 3 / 4 / 3 waves per SIMD these allow (gemv4_waves).
//
// Arithmetic.  The scale operand 2^(E-127) is built in a register from the byte (E << 23 as fp32 bits; E = 0 the subnormal
// 2^-127, E = 255 NaN, as OCP defines it).  Two codes -> two fp32 by v_cvt_scalef32_pk_f32_fp4 (code * scale: exact), bf16 ->
// fp32 by a shift / a mask (exact), then one fp32 FMA per product into TWO accumulators per (row of W, row of A) and lane -
// even and odd k - in ascending k; after the last pass even + odd, then the wave's butterfly (32, 16, 8, 4, 2, 1), + bias[n]
// (if given; one fp32 rounding), then one rounding to bf16.  That order is a function of K alone: the bits of out[m,n] depend
// on row m of A, row n of the codes, its scale row and bias[n], and on nothing else - not on M (MT only adds independent
// chains), not on N, the other rows, the chunking of A or the grid.
//
// Edges.  K % 32 == 0, so a lane's 32 k and its scale are all inside a row or all outside: the ragged last pass is the same code
// under k < K per lane, and no load reaches past a row of the codes, of the scales or of A.  The last wave's second row, when N
// is odd, and the waves past N are clamped to row N - 1 and store nothing.  A lane outside a pass neither loads nor reads the
// (unstaged) A image for it.  No atomics, no scratch memory.
#include "common.h"

namespace ltxk {

constexpr int GEMV4_THREADS = 256;
constexpr int GEMV4_WAVES = GEMV4_THREADS / LTXK_WAVE;
constexpr int GEMV4_DEPTH = 4;             // ring slots = passes requested ahead per row (fewer where a chunk of the A image holds fewer)
constexpr int GEMV4_R = 2;                 // rows of W per wave and pass
// waves per SIMD (= workgroups per CU) an instance is compiled for: what its registers allow without scratch
constexpr int gemv4_waves(int mt) { return mt == 1 || mt == 4 ? 4 : 3; }
constexpr int GEMV4_PASS = 2048;           // k per pass: 64 lanes x 32 e2m1
constexpr int GEMV4_PASS_BYTES = 1024;     // its codes
constexpr int GEMV4_PASS_SCALES = 64;      // its scale bytes
constexpr int GEMV4_LDS_K = 16384;         // bf16 elements of the A image (32 KiB), shared by the MT rows
constexpr int GEMV4_MAX_M = 8;
constexpr int GEMV4_MAX_GROUPS = 8;
constexpr int GEMV4_CUS = 256;             // x gemv4_waves(MT) workgroups each = one round of resident workgroups

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 2^(E-127) from an e8m0 byte
__device__ __forceinline__ float gemv4_scale(unsigned e) {
  return __uint_as_float(e == 0u ? 0x00400000u : e == 255u ? 0x7fc00000u : e << 23);
}

// the 8 products of one lane, pass and quarter (k 8i .. 8i+7 of the lane's 32) for one row of W (w: the quarter's 8 codes, byte
// j = k 8i+2j, +1; sc: their block's scale) and one row of A (x[j]: the same k widened), into the even / odd accumulator pair
__device__ __forceinline__ f32x2 gemv4_fma8(unsigned w, float sc, const f32x2 (&x)[4], f32x2 acc) {
  acc = __builtin_elementwise_fma(x[0], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0), acc);
  acc = __builtin_elementwise_fma(x[1], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1), acc);
  acc = __builtin_elementwise_fma(x[2], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 2), acc);
  acc = __builtin_elementwise_fma(x[3], __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 3), acc);
  return acc;
}

template <int MT>
__global__ __launch_bounds__(GEMV4_THREADS) __attribute__((amdgpu_waves_per_eu(gemv4_waves(MT)))) void gemv_w4_kernel(const bf16* __restrict__ A, int lda, const uint8_t* __restrict__ W,
                                                                const uint8_t* __restrict__ S, const bf16* __restrict__ bias,
                                                                bf16* __restrict__ out, int ldo, int M, int N, int K, int groups) {
  constexpr int R = GEMV4_R;
  constexpr int KC = GEMV4_LDS_K / MT;                // k per chunk of the A image
  constexpr int ROW_BYTES = KC * 2;
  constexpr int CHUNK_PASSES = KC / GEMV4_PASS;
  constexpr int D = CHUNK_PASSES < GEMV4_DEPTH ? CHUNK_PASSES : GEMV4_DEPTH;
  __shared__ __attribute__((aligned(16))) unsigned char sA[GEMV4_LDS_K * 2];
  const int lane = threadIdx.x & (LTXK_WAVE - 1), wave = threadIdx.x >> 6;
  const int passes = (K + GEMV4_PASS - 1) / GEMV4_PASS;      // of a row, the ragged last one included
  const bool one_chunk = K <= KC;

  for (int g = 0; g < groups; ++g) {
    const int64_t n0 = (((int64_t)blockIdx.x * groups + g) * GEMV4_WAVES + wave) * R;
    const bool live = n0 < N;                          // wave-uniform
    const uint8_t* wrow[R];
    const uint8_t* srow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t n = n0 + r < N ? n0 + r : N - 1;
      wrow[r] = W + (size_t)n * (size_t)(K >> 1) + lane * 16;
      srow[r] = S + (size_t)n * (size_t)(K >> 5) + lane;
    }
    f32x2 acc[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = f32x2{0.0f, 0.0f};

    for (int c0 = 0; c0 < K; c0 += KC) {
      const int pb = c0 / GEMV4_PASS;
      const int pe = pb + CHUNK_PASSES < passes ? pb + CHUNK_PASSES : passes;      // the chunk's passes: pb .. pe - 1
      // a lane takes part in pass p of the chunk when its 32 k lie inside the row (K % 32 == 0: all of them or none)
      auto mine = [&](int p) { return p < pe && p * GEMV4_PASS + lane * 32 < K; };
      // the ring: slot j holds the codes and the scale byte of pass p + j for the R rows.  The first D passes are requested
      // BEFORE the A image is staged (W does not wait for A), and a slot is requested again as soon as its pass is taken out.
      u32x4 w[D][R];
      unsigned e[D][R];
#pragma unroll
      for (int j = 0; j < D; ++j)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          w[j][r] = u32x4{0u, 0u, 0u, 0u};
          e[j][r] = 127u;
          if (live && mine(pb + j)) {
            w[j][r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + (size_t)(pb + j) * GEMV4_PASS_BYTES));
            e[j][r] = __builtin_nontemporal_load(srow[r] + (size_t)(pb + j) * GEMV4_PASS_SCALES);
          }
        }
      if (!one_chunk || g == 0) {
        // stage k = c0 .. c0 + kc of the M rows (16-byte units; unit i of a row -> pass i / 256, lane i % 256 / 4, quarter i % 4)
        if (c0 > 0) __syncthreads();
        const int units = ((K - c0 < KC ? K - c0 : KC)) >> 3;
        for (int i = threadIdx.x; i < units; i += GEMV4_THREADS) {
          const int dst = (i >> 8) * 4096 + (i & 3) * 1024 + ((i & 255) >> 2) * 16;
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
      const unsigned char* sl = sA + lane * 16;      // + (p - pb) * 4096: pass p of the row, chunk-relative
#pragma unroll 1
      for (int p = pb; p < pe; p += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
          float sc[R];
#pragma unroll
          for (int r = 0; r < R; ++r) sc[r] = gemv4_scale(e[j][r]);
          if (mine(p + j)) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
              for (int i = 0; i < 4; ++i) {          // quarter by quarter: 16 bytes of A, widened once for the R rows
                const u32x4 a = *(const u32x4*)(sl + m * ROW_BYTES + (p + j - pb) * 4096 + i * 1024);
                f32x2 x[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) x[t] = f32x2{__uint_as_float(a[t] << 16), __uint_as_float(a[t] & 0xffff0000u)};
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][m] = gemv4_fma8(w[j][r][i], sc[r], x, acc[r][m]);
              }
          }
          if (mine(p + j + D)) {          // the slot is free: request the pass D ahead into it
#pragma unroll
            for (int r = 0; r < R; ++r) {
              w[j][r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + (size_t)(p + j + D) * GEMV4_PASS_BYTES));
              e[j][r] = __builtin_nontemporal_load(srow[r] + (size_t)(p + j + D) * GEMV4_PASS_SCALES);
            }
          }
        }
      }
    }
    if (!live) continue;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t n = n0 + r;
      const bool stored = n < N;
      const int64_t nc = stored ? n : N - 1;
      const float bv = bias ? (float)bias[nc] : 0.0f;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        float v = wave_sum(acc[r][m][0] + acc[r][m][1]);
        if (bias) v = v + bv;
        if (lane == 0 && stored && m < M) out[(size_t)m * ldo + n] = (bf16)v;
      }
    }
  }
}

template <int MT>
static void gemv4_launch(const ltxk_gemm_args* a, const uint8_t* scales, int blocks, int groups, hipStream_t st) {
  hipLaunchKernelGGL(gemv_w4_kernel<MT>, dim3((unsigned)blocks), dim3(GEMV4_THREADS), 0, st, (const bf16*)a->A, (int)a->lda,
                     (const uint8_t*)a->W, scales, (const bf16*)a->bias, (bf16*)a->out, (int)a->ldo, (int)a->M, (int)a->N, (int)a->K, groups);
}

}  // namespace ltxk

extern "C" int ltxk_gemv_w4(const ltxk_gemm_args* a, const uint8_t* w_block_scales, void* stream) {
  using namespace ltxk;
  const char* who = "ltxk_gemv_w4";
  LTXK_CHECK_ARG(a && a->A && a->W && a->out, "%s: A, W and out must not be NULL", who);
  LTXK_CHECK_ARG(w_block_scales, "%s: w_block_scales must not be NULL", who);
  LTXK_CHECK_ARG(a->M >= 1 && a->M <= GEMV4_MAX_M, "%s: M=%d must lie in [1, %d]", who, a->M, GEMV4_MAX_M);
  LTXK_CHECK_ARG(a->N >= 1, "%s: N=%d must be positive", who, a->N);
  LTXK_CHECK_ARG(a->K >= 32 && a->K % 32 == 0, "%s: K=%d must be a positive multiple of 32 (one scale block)", who, a->K);
  LTXK_CHECK_ARG(a->epilogue == LTXK_EPI_BIAS, "%s: epilogue %d is not supported (LTXK_EPI_BIAS only)", who, a->epilogue);
  LTXK_CHECK_ARG(!a->resid && !a->gate && !a->gate_row, "%s: resid / gate / gate_row are not supported", who);
  LTXK_CHECK_ARG(!a->out_tokens_per_batch && !a->out2 && !a->n_split, "%s: transposed and split outputs are not supported", who);
  LTXK_CHECK_ARG(!a->sumsq, "%s: sumsq is not supported", who);
  LTXK_CHECK_ARG(!a->workspace && !a->workspace_bytes, "%s: takes no workspace (one launch, no K slices)", who);
  LTXK_CHECK_ARG(a->lda >= a->K && a->lda % 8 == 0 && ((uintptr_t)a->A & 15) == 0, "%s: lda=%d must be >= K and a multiple of 8, A 16-byte aligned", who, a->lda);
  LTXK_CHECK_ARG(((uintptr_t)a->W & 15) == 0, "%s: W must be 16-byte aligned", who);
  LTXK_CHECK_ARG(((uintptr_t)w_block_scales & 3) == 0, "%s: w_block_scales must be 4-byte aligned", who);
  LTXK_CHECK_ARG(a->ldo >= a->N && ((uintptr_t)a->out & 1) == 0 && ((uintptr_t)a->bias & 1) == 0, "%s: ldo=%d must be >= N, out / bias bf16 aligned", who, a->ldo);
  const int mt = a->M == 1 ? 1 : a->M == 2 ? 2 : a->M <= 4 ? 4 : 8;
  const int64_t sets = ((int64_t)a->N + GEMV4_WAVES * GEMV4_R - 1) / (GEMV4_WAVES * GEMV4_R);      // row sets of one workgroup pass
  int64_t groups = 1;
  if (a->K <= GEMV4_LDS_K / mt) {                    // the A image is staged once: let a workgroup keep it over several row sets
    // (rounded up, so that up to GEMV4_MAX_GROUPS x slots row sets run as ONE round of resident workgroups, no short second one)
    const int64_t slots = (int64_t)GEMV4_CUS * gemv4_waves(mt);
    groups = (sets + slots - 1) / slots;
    groups = groups > GEMV4_MAX_GROUPS ? GEMV4_MAX_GROUPS : groups;
  }
  const int64_t blocks = (sets + groups - 1) / groups;
  LTXK_CHECK_ARG(blocks <= (int64_t)INT32_MAX, "%s: too many rows", who);
  hipStream_t st = (hipStream_t)stream;
  switch (mt) {
    case 1: gemv4_launch<1>(a, w_block_scales, (int)blocks, (int)groups, st); break;
    case 2: gemv4_launch<2>(a, w_block_scales, (int)blocks, (int)groups, st); break;
    case 4: gemv4_launch<4>(a, w_block_scales, (int)blocks, (int)groups, st); break;
    default: gemv4_launch<8>(a, w_block_scales, (int)blocks, (int)groups, st); break;
  }
  LTXK_CHECK_LAUNCH(who);
  return LTXK_OK;
}
