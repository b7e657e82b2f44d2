// The x0-space guiders of the guided step (include/ltxk.h, "CFG* and APG"): CFGStarRescalingGuider and LtxAPGGuider of
// ltx_core/components/guiders.py.  Each needs per-sample dot products over the whole (C,S) prediction before one element of
// the step tail can be computed, so a step is: reduction pass(es) -> a small fp32 record per sample in device memory -> the
// tail kernel, which reads the derived scalars from that record.  Nothing here is read back by the host.
//
// Determinism: a reduction pass is two launches.  guider_partial_kernel has the grid of cfg_euler_kernel - one wave per
// (64 tokens, 8 channels, sample): 8 serial fp32 terms per lane, then the wave butterfly - and stores one fp32 partial per
// wave at an index that depends on (C, S) alone.  guider_finish_kernel, one 256-thread workgroup per sample, adds that
// sample's partials in float64: thread t takes partials t, t+256, ... in order, then a fixed LDS tree.  No atomics; neither
// the batch size nor the device's CU count enters the order of a single addition.
#include "common.h"
#include <math.h>

namespace ltxk {

constexpr int REC = LTXK_GUIDER_RECORD_FLOATS;
constexpr int FIN_THREADS = 256;

// what a reduction pass sums (q0, q1), per sample
enum {
  PASS_STAR = 0,      // sum r(p*n), sum r(n*n)                       -> a
  PASS_APG_NORM = 1,  // sum r(g*g), sum r(p*p), g = r(p - n)         -> nrm, f        (norm_threshold > 0 only)
  PASS_APG_PROJ = 2   // sum r(g*p), sum r(p*p), g (rescaled by f)    -> c
};

// the two denoised predictions of one element, with the rounding points of the reference's bf16 arrays
__device__ __forceinline__ float denoised(float x, float sigma, float v) { return rbf(x - sigma * v); }

// APG's guidance vector: g = r(p - n), rescaled by the record's clamp factor when norm_threshold > 0
__device__ __forceinline__ float apg_guidance(float p, float n, bool clamp, float f) {
  float g = rbf(p - n);
  if (clamp) g = rbf(g * f);
  return g;
}

template <int PASS>
__global__ __launch_bounds__(64) void guider_partial_kernel(const bf16* __restrict__ vp, const bf16* __restrict__ vn,
                                                            const bf16* __restrict__ lat, const float* __restrict__ rec,
                                                            float* __restrict__ part, int C, int S, float sigma,
                                                            const float* __restrict__ sig_dev, int clamp) {
  if (sig_dev) sigma = sig_dev[0];
  const int s = blockIdx.x * 64 + threadIdx.x;
  const int cg = blockIdx.y, b = blockIdx.z;
  float q0 = 0.f, q1 = 0.f;
  if (s < S) {              // lanes past S add zeros: every lane takes part in the butterfly
    const size_t tokoff = ((size_t)b * S + s) * C + cg * 8;
    const bf16x8 pv = *(const bf16x8*)(vp + tokoff);
    const bf16x8 nv = *(const bf16x8*)(vn + tokoff);
    float f = 1.f;
    if (PASS == PASS_APG_PROJ && clamp) f = rec[(size_t)b * REC + 4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = (float)lat[((size_t)b * C + cg * 8 + j) * S + s];
      const float p = denoised(x, sigma, (float)pv[j]);
      const float n = denoised(x, sigma, (float)nv[j]);
      if constexpr (PASS == PASS_STAR) {
        q0 += rbf(p * n);
        q1 += rbf(n * n);
      } else if constexpr (PASS == PASS_APG_NORM) {
        const float g = apg_guidance(p, n, false, 1.f);
        q0 += rbf(g * g);
        q1 += rbf(p * p);
      } else {
        const float g = apg_guidance(p, n, clamp != 0, f);
        q0 += rbf(g * p);
        q1 += rbf(p * p);
      }
    }
  }
  q0 = wave_sum(q0);
  q1 = wave_sum(q1);
  if (threadIdx.x == 0) {
    const size_t P = (size_t)gridDim.x * gridDim.y;
    const size_t i = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[((size_t)b * 2 + 0) * P + i] = q0;
    part[((size_t)b * 2 + 1) * P + i] = q1;
  }
}

// One workgroup per sample: the float64 sum of the sample's partials, then the scalars derived from it.
// r(.) of a reduced value: the fp64 sum is stored as fp32 in the record (the raw sum) and that fp32 is rounded to bf16.
__global__ __launch_bounds__(FIN_THREADS) void guider_finish_kernel(const float* __restrict__ part, float* __restrict__ rec,
                                                                     int P, int pass, float norm_threshold) {
  __shared__ double red[2][FIN_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* p0 = part + ((size_t)b * 2 + 0) * P;
  const float* p1 = part + ((size_t)b * 2 + 1) * P;
  double a0 = 0.0, a1 = 0.0;
  for (int i = t; i < P; i += FIN_THREADS) {
    a0 += (double)p0[i];
    a1 += (double)p1[i];
  }
  red[0][t] = a0;
  red[1][t] = a1;
  __syncthreads();
  for (int w = FIN_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w) {
      red[0][t] += red[0][t + w];
      red[1][t] += red[1][t + w];
    }
    __syncthreads();
  }
  if (t != 0) return;
  const float s0 = (float)red[0][0], s1 = (float)red[1][0];
  float* r = rec + (size_t)b * REC;
  if (pass == PASS_STAR) {
    r[0] = s0;                                                 // sum r(p*n)
    r[1] = s1;                                                 // sum r(n*n)
    r[2] = 0.f;
    r[3] = 0.f;
    r[4] = 1.f;
    r[5] = rbf(__fdiv_rn(rbf(s0), rbf(rbf(s1) + 1e-8f)));      // a
  } else if (pass == PASS_APG_NORM) {
    const float nrm = rbf(__fsqrt_rn(rbf(rbf(s0) + 1e-8f)));
    r[0] = s0;                                                 // sum r(g*g), g before the clamp
    r[2] = s1;                                                 // sum r(p*p)
    r[3] = nrm;
    r[4] = fminf(1.f, rbf(__fdiv_rn(norm_threshold, nrm)));    // f
    r[1] = 0.f;                                                // the projection pass that follows fills these two
    r[5] = 0.f;
  } else {
    r[1] = s0;                                                 // sum r(g*p)
    r[2] = s1;                                                 // sum r(p*p)
    if (!(norm_threshold > 0.f)) {
      r[0] = 0.f;
      r[3] = 0.f;
      r[4] = 1.f;
    }
    r[5] = rbf(__fdiv_rn(rbf(s0), rbf(rbf(s1) + 1e-8f)));      // c
  }
  r[6] = 0.f;      // reserved
  r[7] = 0.f;
}

// The step tail of cfg_euler_kernel with the guider's delta in x0 space in place of the velocity-space CFG combine.
template <int GUIDER, bool STG>
__global__ void guider_euler_kernel(const bf16* __restrict__ vp, const bf16* __restrict__ vn, const bf16* __restrict__ vq,
                                    const bf16* __restrict__ lat, bf16* __restrict__ out, const bf16* __restrict__ clean,
                                    const float* __restrict__ mask, const float* __restrict__ rec, int B, int C, int S,
                                    float cfg, float stg, float eta, int clamp, float sigma, float sigma_next,
                                    const float* __restrict__ sig_dev, int flags) {
  if (sig_dev) {
    sigma = sig_dev[0];
    sigma_next = sig_dev[1];
  }
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = blockIdx.y, b = blockIdx.z;
  if (s >= S) return;
  const float f = rec[(size_t)b * REC + 4], coef = rec[(size_t)b * REC + 5];
  const float k = cfg - 1.0f;
  const size_t tokoff = ((size_t)b * S + s) * C + cg * 8;
  const bf16x8 pv = *(const bf16x8*)(vp + tokoff);
  const bf16x8 nv = *(const bf16x8*)(vn + tokoff);
  bf16x8 qv;
  if constexpr (STG) qv = *(const bf16x8*)(vq + tokoff);
  float m = 1.f;
  if (mask) m = mask[(size_t)b * S + s];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const size_t li = ((size_t)b * C + cg * 8 + j) * S + s;
    const float x = (float)lat[li];
    const float p = denoised(x, sigma, (float)pv[j]);
    const float n = denoised(x, sigma, (float)nv[j]);
    float d;
    if constexpr (GUIDER == LTXK_GUIDER_CFG_STAR) {
      d = rbf(k * rbf(p - rbf(coef * n)));
    } else {
      const float g = apg_guidance(p, n, clamp != 0, f);
      const float par = rbf(coef * p);
      d = rbf(k * rbf(rbf(par * eta) + rbf(g - par)));
    }
    float x0 = rbf(p + d);
    if constexpr (STG) x0 = rbf(x0 + rbf(stg * rbf(p - denoised(x, sigma, (float)qv[j]))));
    if (mask) x0 = rbf(rbf(x0 * m) + rbf((float)clean[li] * rbf(1.0f - m)));
    float o = x0;
    if (flags & LTXK_STEP_BF16_EULER) {
      o = x0 + rbf(__fdiv_rn(rbf(sigma_next * rbf(x - x0)), sigma));
    } else if (sigma_next > 0.f) {
      const float t1 = x - x0;
      const float t2 = sigma_next * t1;
      o = x0 + __fdiv_rn(t2, sigma);
    }
    out[li] = (bf16)o;
  }
}

static inline int64_t partials_per_sample(int32_t C, int32_t S) { return (int64_t)(C / 8) * ((S + 63) / 64); }

static int check_guider_common(const ltxk_guider_args* a, const char* name) {
  LTXK_CHECK_ARG(a != nullptr, "%s: null args", name);
  LTXK_CHECK_ARG(a->guider == LTXK_GUIDER_CFG_STAR || a->guider == LTXK_GUIDER_APG,
                 "%s: unknown guider %d (LTXK_GUIDER_CFG_STAR or LTXK_GUIDER_APG)", name, (int)a->guider);
  LTXK_CHECK_ARG(a->v_neg != nullptr, "%s: null v_neg (the guiders compare the positive with the negative prediction)", name);
  LTXK_CHECK_ARG(a->v_pos && a->latent && a->record && a->B > 0 && a->S > 0 && a->C > 0 && a->C % 8 == 0, "%s: bad arguments", name);
  LTXK_CHECK_ARG(a->B <= 65535 && a->C / 8 <= 65535, "%s: B and C/8 must fit a grid dimension (65535)", name);
  LTXK_CHECK_ARG((((uintptr_t)a->v_pos | (uintptr_t)a->v_neg | (uintptr_t)a->v_pert) & 15) == 0,
                 "%s: the token tensors must be 16-byte aligned", name);
  LTXK_CHECK_ARG(isfinite(a->eta), "%s: eta must be finite", name);
  LTXK_CHECK_ARG(a->norm_threshold >= 0.f && isfinite(a->norm_threshold), "%s: norm_threshold must be finite and >= 0", name);
  LTXK_CHECK_ARG(a->sigmas_dev != nullptr || a->sigma > 0.f, "%s: sigma must be > 0", name);
  return LTXK_OK;
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_guider_args_sizeof(void) { return (int)sizeof(ltxk_guider_args); }

extern "C" int64_t ltxk_guidance_sums_workspace_bytes(int32_t B, int32_t C, int32_t S) {
  if (B <= 0 || C <= 0 || S <= 0 || C % 8 != 0) return -1;
  return (int64_t)B * 2 * partials_per_sample(C, S) * (int64_t)sizeof(float);
}

template <int PASS>
static void launch_pass(const ltxk_guider_args* a, int P, int clamp, hipStream_t st) {
  hipLaunchKernelGGL(guider_partial_kernel<PASS>, dim3((a->S + 63) / 64, a->C / 8, a->B), dim3(64), 0, st,
                     (const bf16*)a->v_pos, (const bf16*)a->v_neg, (const bf16*)a->latent, (const float*)a->record,
                     (float*)a->workspace, (int)a->C, (int)a->S, a->sigma, a->sigmas_dev, clamp);
  hipLaunchKernelGGL(guider_finish_kernel, dim3(a->B), dim3(FIN_THREADS), 0, st, (const float*)a->workspace, a->record, P,
                     PASS, a->norm_threshold);
}

extern "C" int ltxk_guidance_sums(const ltxk_guider_args* a, void* stream) {
  const char* name = "ltxk_guidance_sums";
  if (int rc = check_guider_common(a, name)) return rc;
  const int64_t P = partials_per_sample(a->C, a->S);
  LTXK_CHECK_ARG(P <= INT32_MAX, "%s: (C/8) * ceil(S/64) must fit 31 bits", name);
  LTXK_CHECK_ARG(a->workspace != nullptr && a->workspace_bytes >= ltxk_guidance_sums_workspace_bytes(a->B, a->C, a->S),
                 "%s: workspace of %lld bytes needed (ltxk_guidance_sums_workspace_bytes)", name,
                 (long long)ltxk_guidance_sums_workspace_bytes(a->B, a->C, a->S));
  LTXK_CHECK_ARG(((uintptr_t)a->workspace & 3) == 0 && ((uintptr_t)a->record & 3) == 0, "%s: workspace / record misaligned", name);
  hipStream_t st = (hipStream_t)stream;
  if (a->guider == LTXK_GUIDER_CFG_STAR) {
    launch_pass<PASS_STAR>(a, (int)P, 0, st);
  } else {
    const int clamp = a->norm_threshold > 0.f;
    if (clamp) launch_pass<PASS_APG_NORM>(a, (int)P, 0, st);
    launch_pass<PASS_APG_PROJ>(a, (int)P, clamp, st);      // with the clamp: reads f from the record the first pass wrote
  }
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}

template <int GUIDER, bool STG>
static void launch_tail(const ltxk_guider_args* a, hipStream_t st) {
  hipLaunchKernelGGL((guider_euler_kernel<GUIDER, STG>), dim3((a->S + 63) / 64, a->C / 8, a->B), dim3(64), 0, st,
                     (const bf16*)a->v_pos, (const bf16*)a->v_neg, (const bf16*)a->v_pert, (const bf16*)a->latent, (bf16*)a->out,
                     (const bf16*)a->clean, a->mask, (const float*)a->record, (int)a->B, (int)a->C, (int)a->S, a->cfg_scale,
                     a->stg_scale, a->eta, (int)(a->norm_threshold > 0.f), a->sigma, a->sigma_next, a->sigmas_dev, (int)a->flags);
}

extern "C" int ltxk_guider_euler_step(const ltxk_guider_args* a, void* stream) {
  const char* name = "ltxk_guider_euler_step";
  if (int rc = check_guider_common(a, name)) return rc;
  LTXK_CHECK_ARG(a->out != nullptr, "%s: null out", name);
  LTXK_CHECK_ARG((a->clean == nullptr) == (a->mask == nullptr), "%s: clean and mask must both be set or both NULL", name);
  hipStream_t st = (hipStream_t)stream;
  const bool stg = a->v_pert != nullptr;
  if (a->guider == LTXK_GUIDER_CFG_STAR) {
    if (stg) launch_tail<LTXK_GUIDER_CFG_STAR, true>(a, st); else launch_tail<LTXK_GUIDER_CFG_STAR, false>(a, st);
  } else {
    if (stg) launch_tail<LTXK_GUIDER_APG, true>(a, st); else launch_tail<LTXK_GUIDER_APG, false>(a, st);
  }
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}
