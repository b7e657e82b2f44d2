// What follows the main loop of the MFMA kernels (gemm_core.h): fp32 accumulators -> stored bf16.  Every formula and rounding
// point of the dense (gemm.hip) and implicit-GEMM (conv3d.hip) epilogues is defined here once; the tile bodies, the split-K
// epilogue and the conv finalize kernel call these, which is what makes their outputs agree bit for bit.
// Values only: operand prefetch, counted waits and the "uses" that keep dead prefetches alive belong to the callers.
// -ffp-contract=off (Makefile): every expression below rounds as written.
#pragma once
#include "common.h"

namespace ltxk {

// four fp32 -> the stored bf16x4, each rounded to nearest even
__device__ __forceinline__ bf16x4 to_bf16x4(const float (&y)[4]) {
  const f32x4 v = {y[0], y[1], y[2], y[3]};
  return __builtin_convertvector(v, bf16x4);
}

// ---- the epilogue value: one of the six LTXK_EPI_* formulas on 4 accumulators ----
// y = rbf(acc + bias) or rbf(acc) (two branches: they differ on -0.0), then
//   BIAS y | BIAS_GELU gelu(y) | BIAS_SILU silu(y) | BIAS_GATE_RES r + rbf(y * g) | BIAS_RES r + y | SCALE_RES r + rbf(alpha * acc)
// rounded once more to the stored bf16.  Operands an epilogue does not name are ignored.
__device__ __forceinline__ void epi_biased(const f32x4& acc, bool has_bias, bf16x4 bias, float (&y)[4]) {
  if (has_bias) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = rbf(acc[j] + (float)bias[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = rbf(acc[j]);
  }
}
// (y: what epi_biased gave)
template <int EPI>
__device__ __forceinline__ bf16x4 epi_finish(float (&y)[4], const f32x4& acc, bf16x4 resid, bf16x4 gate, float alpha) {
  if constexpr (EPI == LTXK_EPI_BIAS_GELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = gelu_tanh_f(y[j]);
  } else if constexpr (EPI == LTXK_EPI_BIAS_SILU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = silu_f(y[j]);
  } else if constexpr (EPI == LTXK_EPI_BIAS_GATE_RES) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (float)resid[j] + rbf(y[j] * (float)gate[j]);
  } else if constexpr (EPI == LTXK_EPI_BIAS_RES) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (float)resid[j] + y[j];
  } else if constexpr (EPI == LTXK_EPI_SCALE_RES) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (float)resid[j] + rbf(alpha * acc[j]);
  }
  return to_bf16x4(y);
}
template <int EPI>
__device__ __forceinline__ bf16x4 epi_value(const f32x4& acc, bool has_bias, bf16x4 bias, bf16x4 resid, bf16x4 gate, float alpha) {
  float y[4];
  epi_biased(acc, has_bias, bias, y);
  return epi_finish<EPI>(y, acc, resid, gate, alpha);
}

// the same with the epilogue chosen at run time (splitk_epilogue_kernel; the host has checked epi): one bias add, then the switch
__device__ __forceinline__ bf16x4 epi_value(int epi, const f32x4& acc, bool has_bias, bf16x4 bias, bf16x4 resid, bf16x4 gate, float alpha) {
  float y[4];
  epi_biased(acc, has_bias, bias, y);
  switch (epi) {
    case LTXK_EPI_BIAS_GELU: return epi_finish<LTXK_EPI_BIAS_GELU>(y, acc, resid, gate, alpha);
    case LTXK_EPI_BIAS_SILU: return epi_finish<LTXK_EPI_BIAS_SILU>(y, acc, resid, gate, alpha);
    case LTXK_EPI_BIAS_GATE_RES: return epi_finish<LTXK_EPI_BIAS_GATE_RES>(y, acc, resid, gate, alpha);
    case LTXK_EPI_BIAS_RES: return epi_finish<LTXK_EPI_BIAS_RES>(y, acc, resid, gate, alpha);
    case LTXK_EPI_SCALE_RES: return epi_finish<LTXK_EPI_SCALE_RES>(y, acc, resid, gate, alpha);
    default: return epi_finish<LTXK_EPI_BIAS>(y, acc, resid, gate, alpha);
  }
}

// ---- the convolution's value: rbf(acc + bias), then rbf(. + resid) - as floats (the fused PixelNorm continues from them) ----
// (bf16 of it is epi_value<LTXK_EPI_BIAS> / <LTXK_EPI_BIAS_RES> with a bias: bf16(r + y) and bf16(rbf(y + r)) are the same bits)
template <bool RES>
__device__ __forceinline__ void conv_value(const f32x4& acc, bf16x4 bias, bf16x4 resid, float (&y)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = rbf(acc[j] + (float)bias[j]);
  if constexpr (RES) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = rbf(y[j] + (float)resid[j]);
  }
}

// ---- the tap convolution's value (conv_taps.hip): conv_value, then the mean with one or two more tensors (summed in fp32 in
// the order y, a1, a2, divided, rounded once), as floats; its two outputs follow from y ----
// (NMEAN = 0: no mean.  Operands a form does not name are ignored.)
__device__ __forceinline__ void taps_value(const f32x4& acc, bf16x4 bias, bool has_res, bf16x4 resid, int n_mean, bf16x4 a1, bf16x4 a2,
                                           float (&y)[4]) {
  if (has_res) conv_value<true>(acc, bias, resid, y);
  else conv_value<false>(acc, bias, resid, y);
  if (n_mean == 2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = rbf((y[j] + (float)a1[j]) / 2.0f);
  } else if (n_mean == 3) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = rbf(((y[j] + (float)a1[j]) + (float)a2[j]) / 3.0f);
  }
}
// leaky ReLU as the reference writes it: max(y, bf16(y * slope))
__device__ __forceinline__ bf16x4 taps_leaky(const float (&y)[4], float slope) {
  float t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = fmaxf(y[j], rbf(y[j] * slope));
  return to_bf16x4(t);
}
// conv_post + tanh: fp32, never rounded to bf16
__device__ __forceinline__ f32x4 taps_tanh(const f32x4& acc, bf16x4 bias) {
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = tanhf(acc[j] + (float)bias[j]);
  return o;
}

// ---- the transposed (V^T / split-output) store: token m, column nrel of its block -> out[(m / T) * rows + nrel][m % T] ----
struct TransOut {
  bf16* out;
  int rows, ld, T, M;                  // rows per batch (N - n_split), row stride, tokens per batch, tokens in all
  __device__ __forceinline__ bf16* at(int m, int nrel) const {
    const int b = m / T, t = m - b * T;
    return out + ((size_t)b * rows + nrel) * ld + t;
  }
  // 4 consecutive tokens m..m+3 of column nrel, bf16(acc + b): one 8-byte store where the four stay inside one batch row
  // (T % 4 == 0) and inside M, element stores otherwise
  __device__ __forceinline__ void store4(int m, int nrel, const f32x4& acc, float b) const {
    const bf16x4 o = __builtin_convertvector(acc + b, bf16x4);
    if ((T & 3) == 0 && m + 3 < M) {
      *(bf16x4*)at(m, nrel) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (m + j < M) *at(m + j, nrel) = o[j];
    }
  }
};

// ---- the row statistic: squares of the STORED bf16 values, added one by one; then the four lanes that share (lane & 15) ----
__device__ __forceinline__ float add_squares(float ss, bf16x4 o) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float f = (float)o[j];
    ss += f * f;
  }
  return ss;
}
__device__ __forceinline__ float wave_row_sum(float ss) { return lane_xor32_sum(lane_xor16_sum(ss)); }

// ---- the line image: a wave transposes its (ROWS x RB/2 columns) block of bf16x4 pieces through LDS of its own (rows of RB =
// 128 or 64 bytes, 16-byte chunks XOR-swizzled by row) and stores whole rows of it, 16 bytes per lane.  The accumulator layout
// is row = lane & 15 (+ 16 per MFMA row block), columns 16 * nt + 4 * (lane >> 4) .. + 3.  The caller owns the barrier in
// front of the first put (the ring is being reused) and the check that the images fit. ----
template <int RB, int ROWS>
struct LineImage {
  static constexpr int CPR = RB / 16, RPI = 64 / CPR;      // 16-byte chunks per row (8 / 4), rows per store instruction (8 / 16)
  char* base;
  int lane;
  __device__ __forceinline__ void put(int row, int nt, bf16x4 o) const {
    const int cg = lane >> 4;
    *(bf16x4*)(base + row * RB + (((nt * 2 + (cg >> 1)) ^ (row & (CPR - 1))) << 4) + (cg & 1) * 8) = o;
  }
  // rows m_base .. m_base + ROWS - 1, columns n_base .. n_base + RB/2 - 1 of dst (row stride ld), clipped to M x N (N % 8 == 0)
  __device__ __forceinline__ void flush(bf16* dst, int ld, int m_base, int n_base, int M, int N) const {
    const int c = lane & (CPR - 1);
    const int n = n_base + c * 8;
#pragma unroll
    for (int i = 0; i < ROWS / RPI; ++i) {
      const int r = i * RPI + lane / CPR;
      const int m = m_base + r;
      const bf16x8 v = *(const bf16x8*)(base + r * RB + ((c ^ (r & (CPR - 1))) << 4));
      if (m < M && n < N) *(bf16x8*)(dst + (size_t)m * ld + n) = v;
    }
  }
};

// ---- split-K: the S fp32 slices of one f32x4 (slice s at src + s * slab), added strictly in slice order; four independent
// loads in flight ----
__device__ __forceinline__ f32x4 sum_slices(const float* src, size_t slab, int S) {
  f32x4 a = *(const f32x4*)src;
  int sl = 1;
  for (; sl + 4 <= S; sl += 4) {
    const f32x4 b0 = *(const f32x4*)(src + (size_t)sl * slab), b1 = *(const f32x4*)(src + (size_t)(sl + 1) * slab);
    const f32x4 b2 = *(const f32x4*)(src + (size_t)(sl + 2) * slab), b3 = *(const f32x4*)(src + (size_t)(sl + 3) * slab);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ((a[j] + b0[j]) + b1[j]) + b2[j] + b3[j];
  }
  for (; sl < S; ++sl) {
    const f32x4 b = *(const f32x4*)(src + (size_t)sl * slab);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += b[j];
  }
  return a;
}

}  // namespace ltxk
