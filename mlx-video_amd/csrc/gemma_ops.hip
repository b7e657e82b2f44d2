// Row kernels of the Gemma-3 text encoder (include/ltxk.h, "Gemma-3 text encoder"): the scaled embedding gather, Gemma's
// (1 + w) RMSNorm with the decoder layer's post-norm residual add, the per-head q/k norm + rotate-half RoPE at head dim 256,
// and the gate * up product of the GeGLU feed-forward.  Conventions are those of text_ops.hip: every access is a 16-byte
// vector, a row is reduced by one wave (one group of 16 lanes for a head) in a fixed order that depends on its width only,
// nothing uses an atomic, and each result is rounded to bf16 once with the arithmetic in front of it in fp32.
#include "common.h"
#include <math.h>

namespace ltxk {

// out[m,:] = bf16(table[ids[m],:] * s); an id outside [0, V) reads row 0 or V-1 (the host validates the ids it is given)
__global__ void embed_rows_kernel(const bf16* __restrict__ table, int V, int D, const int32_t* __restrict__ ids, bf16* __restrict__ out,
                                  int ldo, int M, float s) {
  const int cpr = D >> 3;
  const int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= (int64_t)M * cpr) return;
  const int m = (int)(ci / cpr), cc = (int)(ci - (int64_t)m * cpr) * 8;
  int id = ids[m];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  const bf16x8 v = *(const bf16x8*)(table + (size_t)id * D + cc);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)v[j] * s);
  *(bf16x8*)(out + (size_t)m * ldo + cc) = o;
}

// Gemma RMSNorm of rows of any width D % 8 == 0 (D <= 8192): one wave per row, GEMMA_ROWS_PER_WG rows per workgroup, the row
// in registers.  The sum of squares: a lane adds its elements in ascending order, then the wave's butterfly.
constexpr int GEMMA_MAXC = 16;          // 16-byte chunks per lane: 64 x 16 x 8 = 8192 elements
constexpr int GEMMA_ROWS_PER_WG = 4;

__global__ __launch_bounds__(64 * GEMMA_ROWS_PER_WG) void rmsnorm_weight_rows_kernel(
    const bf16* __restrict__ x, int ldx, const bf16* __restrict__ w, const bf16* resid, int ldr, bf16* y, int ldy, int M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * GEMMA_ROWS_PER_WG + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16* xr = x + (size_t)row * ldx;
  const int cpr = D >> 3;
  bf16x8 v[GEMMA_MAXC];
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < GEMMA_MAXC; ++i) {
    const int c = i * 64 + lane;
    if (c < cpr) {
      v[i] = *(const bf16x8*)(xr + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[i][j];
        sq += f * f;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
  bf16* yr = y + (size_t)row * ldy;
  const bf16* rr = resid ? resid + (size_t)row * ldr : nullptr;
#pragma unroll
  for (int i = 0; i < GEMMA_MAXC; ++i) {
    const int c = i * 64 + lane;
    if (c < cpr) {
      const bf16x8 wv = *(const bf16x8*)(w + c * 8);
      bf16x8 o;
      if (rr) {
        const bf16x8 rv = *(const bf16x8*)(rr + c * 8);          // read before the store: y may be resid
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)rv[j] + rbf((float)v[i][j] * rstd * (1.0f + (float)wv[j])));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)v[i][j] * rstd * (1.0f + (float)wv[j]));
      }
      *(bf16x8*)(yr + c * 8) = o;
    }
  }
}

// Per-head RMSNorm (1 + w) + rotate-half RoPE at head dim 256, in place on the first (Hq + Hkv) heads of a row.  A work item
// is 8 elements of a head's first half and their 8 rotation partners 128 columns up; a head is 16 items = one aligned group
// of 16 lanes, which reduces the head's 256 squares itself (16 per lane in ascending order, then the group's butterfly).
constexpr int HEADNORM_DH = 256;

__global__ __launch_bounds__(256) void headnorm_rope_kernel(bf16* __restrict__ buf, int ld, int M, int Hq, int Hkv,
                                                            const bf16* __restrict__ qw, const bf16* __restrict__ kw,
                                                            const float* __restrict__ cosb, const float* __restrict__ sinb, int T, float eps) {
  const int NH = Hq + Hkv;
  const int64_t heads = (int64_t)M * NH;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hg_raw = gid >> 4;
  const bool live = hg_raw < heads;               // uniform over a group of 16 lanes
  const int64_t hg = live ? hg_raw : heads - 1;
  const int it = (int)(gid & 15);
  const int row = (int)(hg / NH), hh = (int)(hg - (int64_t)row * NH);
  const int t = row % T;
  bf16* xp = buf + (size_t)row * ld + (size_t)hh * HEADNORM_DH + it * 8;
  const bf16x8 a = *(const bf16x8*)xp;
  const bf16x8 b = *(const bf16x8*)(xp + 128);
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float fa = (float)a[j], fb = (float)b[j];
    sq += fa * fa + fb * fb;
  }
  const float rstd = rsqrtf(group_sum<16>(sq) / (float)HEADNORM_DH + eps);
  const bf16* wp = (hh < Hq ? qw : kw) + it * 8;
  const bf16x8 wa = *(const bf16x8*)wp;
  const bf16x8 wb = *(const bf16x8*)(wp + 128);
  const size_t off = (size_t)t * 128 + it * 8;
  const f32x4 c0 = *(const f32x4*)(cosb + off), c1 = *(const f32x4*)(cosb + off + 4);
  const f32x4 s0 = *(const f32x4*)(sinb + off), s1 = *(const f32x4*)(sinb + off + 4);
  bf16x8 oa, ob;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x1 = rbf((float)a[j] * rstd * (1.0f + (float)wa[j]));
    const float x2 = rbf((float)b[j] * rstd * (1.0f + (float)wb[j]));
    const float c = j < 4 ? c0[j & 3] : c1[j & 3], sn = j < 4 ? s0[j & 3] : s1[j & 3];
    oa[j] = (bf16)(x1 * c - x2 * sn);
    ob[j] = (bf16)(x2 * c + x1 * sn);
  }
  if (live) {
    *(bf16x8*)xp = oa;
    *(bf16x8*)(xp + 128) = ob;
  }
}

// out[m,f] = bf16(bf16(gelu_tanh(g[m,f])) * u[m,f]), gu = [g | u] (M, 2F); out may be gu itself (a thread reads its g and u
// chunks before it stores over g).  gelu_tanh(x) = x (1 + tanh u) / 2 = x / (1 + exp(-2u)), u = sqrt(2/pi) (x + 0.044715 x^3): the
// quotient form has no cancellation on the negative side, where 1 + tanh u loses every digit below x ~ -4; expf and a correctly
// rounded division instead of gelu_tanh_f's exp2 / rcp pair, the GEMM epilogue's economy that a memory-bound pass does not need.
// exp(-2u) = inf (x below about -10) gives -0, the limit.
__device__ __forceinline__ float gelu_tanh_exact_f(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return x / (1.0f + expf(-2.0f * u));
}

__global__ void geglu_tanh_kernel(const bf16* gu, int ld, bf16* out, int ldo, int M, int F) {
  const int cpr = F >> 3;
  const int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= (int64_t)M * cpr) return;
  const int m = (int)(ci / cpr), cc = (int)(ci - (int64_t)m * cpr) * 8;
  const bf16x8 gv = *(const bf16x8*)(gu + (size_t)m * ld + cc);
  const bf16x8 uv = *(const bf16x8*)(gu + (size_t)m * ld + F + cc);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)(rbf(gelu_tanh_exact_f((float)gv[j])) * (float)uv[j]);
  *(bf16x8*)(out + (size_t)m * ldo + cc) = o;
}

}  // namespace ltxk

using namespace ltxk;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int ltxk_embed_rows(const void* table, int32_t V, int32_t D, const int32_t* ids, void* out, int32_t ldo, int32_t M,
                               float s, void* stream) {
  LTXK_CHECK_ARG(table && ids && out && V > 0 && M > 0 && D > 0, "ltxk_embed_rows: bad arguments");
  LTXK_CHECK_ARG(D % 8 == 0 && D <= 512 * GEMMA_MAXC, "ltxk_embed_rows: D=%d must be a multiple of 8, at most %d", D, 512 * GEMMA_MAXC);
  LTXK_CHECK_ARG(ldo >= D && ldo % 8 == 0 && aligned16(table) && aligned16(out) && ((uintptr_t)ids & 3) == 0,
                 "ltxk_embed_rows: ldo must be >= D and a multiple of 8, table / out 16-byte aligned");
  const int64_t chunks = (int64_t)M * (D / 8);
  LTXK_CHECK_ARG((chunks + 255) / 256 <= (int64_t)INT32_MAX, "ltxk_embed_rows: too large");
  hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)table, V, D,
                     ids, (bf16*)out, ldo, M, s);
  LTXK_CHECK_LAUNCH("ltxk_embed_rows");
  return LTXK_OK;
}

extern "C" int ltxk_rmsnorm_weight_rows(const void* x, int32_t ldx, const void* weight, const void* resid, int32_t ldr, void* y,
                                        int32_t ldy, int32_t M, int32_t D, float eps, void* stream) {
  LTXK_CHECK_ARG(x && weight && y && M > 0 && D > 0, "ltxk_rmsnorm_weight_rows: bad arguments");
  LTXK_CHECK_ARG(D % 8 == 0 && D <= 512 * GEMMA_MAXC, "ltxk_rmsnorm_weight_rows: D=%d must be a multiple of 8, at most %d", D, 512 * GEMMA_MAXC);
  LTXK_CHECK_ARG(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(weight),
                 "ltxk_rmsnorm_weight_rows: row strides must be >= D and multiples of 8, pointers 16-byte aligned");
  LTXK_CHECK_ARG(!resid || (ldr >= D && ldr % 8 == 0 && aligned16(resid)),
                 "ltxk_rmsnorm_weight_rows: resid must be 16-byte aligned with ldr >= D, a multiple of 8");
  hipLaunchKernelGGL(rmsnorm_weight_rows_kernel, dim3((M + GEMMA_ROWS_PER_WG - 1) / GEMMA_ROWS_PER_WG), dim3(64 * GEMMA_ROWS_PER_WG), 0,
                     (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)weight, (const bf16*)resid, ldr, (bf16*)y, ldy, M, D, eps);
  LTXK_CHECK_LAUNCH("ltxk_rmsnorm_weight_rows");
  return LTXK_OK;
}

extern "C" int ltxk_headnorm_rope(void* buf, int32_t ld, int32_t M, int32_t Hq, int32_t Hkv, const void* q_weight, const void* k_weight,
                                  const float* cos, const float* sin, int32_t T, float eps, void* stream) {
  LTXK_CHECK_ARG(buf && q_weight && k_weight && cos && sin && M > 0 && T > 0, "ltxk_headnorm_rope: bad arguments");
  LTXK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && (int64_t)(Hq + Hkv) * HEADNORM_DH <= (int64_t)ld, "ltxk_headnorm_rope: ld=%d must be >= (Hq + Hkv) * 256, Hq=%d Hkv=%d",
                 ld, Hq, Hkv);
  LTXK_CHECK_ARG(ld % 8 == 0 && aligned16(buf) && aligned16(q_weight) && aligned16(k_weight) && aligned16(cos) && aligned16(sin),
                 "ltxk_headnorm_rope: ld must be a multiple of 8, pointers 16-byte aligned");
  const int64_t groups = ((int64_t)M * (Hq + Hkv) * 16 + 255) / 256;
  LTXK_CHECK_ARG(groups <= (int64_t)INT32_MAX, "ltxk_headnorm_rope: too many rows");
  hipLaunchKernelGGL(headnorm_rope_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, Hq, Hkv,
                     (const bf16*)q_weight, (const bf16*)k_weight, cos, sin, T, eps);
  LTXK_CHECK_LAUNCH("ltxk_headnorm_rope");
  return LTXK_OK;
}

extern "C" int ltxk_geglu_tanh(const void* gu, int32_t ld, void* out, int32_t ldo, int32_t M, int32_t F, void* stream) {
  LTXK_CHECK_ARG(gu && out && M > 0 && F > 0 && F % 8 == 0, "ltxk_geglu_tanh: bad arguments (F must be a multiple of 8)");
  LTXK_CHECK_ARG((int64_t)ld >= 2 * (int64_t)F && ldo >= F && ld % 8 == 0 && ldo % 8 == 0 && aligned16(gu) && aligned16(out),
                 "ltxk_geglu_tanh: ld must be >= 2F, ldo >= F, both multiples of 8, pointers 16-byte aligned");
  const int64_t chunks = (int64_t)M * (F / 8);
  LTXK_CHECK_ARG((chunks + 255) / 256 <= (int64_t)INT32_MAX, "ltxk_geglu_tanh: too large");
  hipLaunchKernelGGL(geglu_tanh_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)gu, ld,
                     (bf16*)out, ldo, M, F);
  LTXK_CHECK_LAUNCH("ltxk_geglu_tanh");
  return LTXK_OK;
}
