// The learned-weight RMSNorm + rotation chain of the row kernels (elementwise.hip, text_ops.hip): every formula and rounding
// point is defined here once, and each of those kernels calls it, which is what makes their entry points agree bit for bit.
// Attention's fused query preparation (fa_prep_q / fa16_prep_q, attention.hip) restates norm_rope in its own prologue and is
// held to it by the fused-versus-unfused bit equality of tests/test_kernels_gpu.py and tests/test_attn_forms_gpu.py.
// Values only: which addresses a lane reads, when it requests them and how the row's sum of squares is reduced belong
// to the callers.  -ffp-contract=off (Makefile): every expression below rounds as written.
#pragma once
#include "common.h"

namespace ltxk {

// 8 cos and 8 sin of one work item: fp32, 8 consecutive table entries each
struct RopeTab {
  f32x4 c0, c1, s0, s1;
};
__device__ __forceinline__ RopeTab rope_load(const float* cosb, const float* sinb, size_t off) {
  RopeTab t;
  t.c0 = *(const f32x4*)(cosb + off); t.c1 = *(const f32x4*)(cosb + off + 4);
  t.s0 = *(const f32x4*)(sinb + off); t.s1 = *(const f32x4*)(sinb + off + 4);
  return t;
}

// (x * rstd) * w in fp32, not yet rounded; ONE_PLUS: Gemma's weight 1 + w, formed in fp32
template <bool ONE_PLUS>
__device__ __forceinline__ float norm_w(float x, float rstd, float w) {
  return x * rstd * (ONE_PLUS ? 1.0f + w : w);
}

// a: 8 elements of a head's first half, b: their rotation partners in the second half (wa, wb: their weights).
//   x1 = rbf(norm_w(a)), x2 = rbf(norm_w(b));  rope: oa = bf16(x1*c - s*x2), ob = bf16(x2*c + s*x1);  else oa = bf16(x1), ob = bf16(x2)
// `rope` is uniform over the launch; without it `tab` is not read.
template <bool ONE_PLUS = false>
__device__ __forceinline__ void norm_rope(bf16x8 a, bf16x8 b, float rstd, bf16x8 wa, bf16x8 wb, bool rope, RopeTab tab,
                                          bf16x8& oa, bf16x8& ob) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x1 = rbf(norm_w<ONE_PLUS>((float)a[j], rstd, (float)wa[j]));
    const float x2 = rbf(norm_w<ONE_PLUS>((float)b[j], rstd, (float)wb[j]));
    if (rope) {
      const float c = j < 4 ? tab.c0[j & 3] : tab.c1[j & 3], sn = j < 4 ? tab.s0[j & 3] : tab.s1[j & 3];
      oa[j] = (bf16)(x1 * c - sn * x2);
      ob[j] = (bf16)(x2 * c + sn * x1);
    } else {
      oa[j] = (bf16)x1;
      ob[j] = (bf16)x2;
    }
  }
}

}  // namespace ltxk
