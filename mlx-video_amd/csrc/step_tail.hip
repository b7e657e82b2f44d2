// The denoise-step tail (include/ltxk.h, "One denoise-step tail" .. "CFG* and APG"): guidance -> x0 -> mask blend -> Euler,
// one launch of step_tail_kernel<GUIDER, STG> for every form, behind ltxk_cfg_euler_step(_dev), ltxk_guided_euler_step and
// ltxk_guider_euler_step; and the reductions of the x0-space guiders (ltxk_guidance_sums), CFGStarRescalingGuider and
// LtxAPGGuider of ltx_core/components/guiders.py.  Those need per-sample dot products over the whole (C,S) prediction before
// one element of the tail can be computed, so such a step is: reduction pass(es) -> a small fp32 record per sample in device
// memory -> the tail kernel, which reads the derived scalars from that record.  Nothing here is read back by the host.
//
// Determinism: a reduction pass is two launches.  guider_partial_kernel has the grid of step_tail_kernel - one wave per
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

// the denoised prediction of one element, with the rounding point of the reference's bf16 arrays
__device__ __forceinline__ float denoised(float x, float sigma, float v) { return rbf(x - sigma * v); }

// APG's guidance vector: g = r(p - n), rescaled by the record's clamp factor when norm_threshold > 0
__device__ __forceinline__ float apg_guidance(float p, float n, bool clamp, float f) {
  float g = rbf(p - n);
  if (clamp) g = rbf(g * f);
  return g;
}

__device__ __forceinline__ float mask_blend(float x0, float clean, float m) {
  return rbf(rbf(x0 * m) + rbf(clean * rbf(1.0f - m)));
}

// x0 + sigma_next*(x - x0)/sigma in fp32, one rounding per op as written
__device__ __forceinline__ float euler_fp32(float x, float x0, float sigma, float sigma_next) {
  const float t1 = x - x0;
  const float t2 = sigma_next * t1;
  return x0 + __fdiv_rn(t2, sigma);
}

// The step's Euler update; sigma_next <= 0 (the last step) returns x0 itself in the fp32 form.
__device__ __forceinline__ float euler_update(float x, float x0, float sigma, float sigma_next, int flags) {
  // fp32_euler=False (generate.py:748): every op of x0 + s'*(x - x0)/s materialises a bf16 array
  if (flags & LTXK_STEP_BF16_EULER) return x0 + rbf(__fdiv_rn(rbf(sigma_next * rbf(x - x0)), sigma));
  if (sigma_next > 0.f) return euler_fp32(x, x0, sigma, sigma_next);
  return x0;
}

// GUIDER == 0, plain CFG: the combine runs in velocity space, v = r(v+ + r((cfg-1) * r(v+ - v-))) (vn == NULL: v = v+), and
// STG pushes v away from the perturbed forward's velocity vq, v = r(v + r(stg * r(v+ - vq))), before x0; `rec` is not read.
// LTXK_GUIDER_CFG_STAR / LTXK_GUIDER_APG: the guider's delta d and the STG term in x0 space, with f and a | c of the record.
template <int GUIDER, bool STG>
__global__ void step_tail_kernel(const bf16* __restrict__ vp, const bf16* __restrict__ vn, const bf16* __restrict__ vq,
                                 const bf16* __restrict__ lat, bf16* __restrict__ out, const bf16* __restrict__ clean,
                                 const float* __restrict__ mask, const float* __restrict__ rec, int B, int C, int S,
                                 float cfg, float stg, float eta, int clamp, float sigma, float sigma_next,
                                 const float* __restrict__ sig_dev, int flags) {
  if (sig_dev) {            // graph replay: the two scalars live in device memory
    sigma = sig_dev[0];
    sigma_next = sig_dev[1];
  }
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = blockIdx.y, b = blockIdx.z;
  if (s >= S) return;
  float f = 1.f, coef = 0.f;
  if constexpr (GUIDER != 0) {
    f = rec[(size_t)b * REC + 4];
    coef = rec[(size_t)b * REC + 5];
  }
  const float k = cfg - 1.0f;
  const size_t tokoff = ((size_t)b * S + s) * C + cg * 8;
  const bf16x8 pv = *(const bf16x8*)(vp + tokoff);
  bf16x8 nv = pv;
  if (GUIDER != 0 || vn) nv = *(const bf16x8*)(vn + tokoff);
  bf16x8 qv;
  if constexpr (STG) qv = *(const bf16x8*)(vq + tokoff);
  float m = 1.f;
  if (mask) m = mask[(size_t)b * S + s];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const size_t li = ((size_t)b * C + cg * 8 + j) * S + s;
    const float x = (float)lat[li];
    float x0;
    if constexpr (GUIDER == 0) {
      float v = (float)pv[j];
      if (vn) v = rbf(v + rbf(k * rbf(v - (float)nv[j])));
      if constexpr (STG) v = rbf(v + rbf(stg * rbf((float)pv[j] - (float)qv[j])));
      x0 = denoised(x, sigma, v);
    } else {
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
      x0 = rbf(p + d);
      if constexpr (STG) x0 = rbf(x0 + rbf(stg * rbf(p - denoised(x, sigma, (float)qv[j]))));
    }
    if (mask) x0 = mask_blend(x0, (float)clean[li], m);
    out[li] = (bf16)euler_update(x, x0, sigma, sigma_next, flags);
  }
}

// The eager loop's Euler update alone (ltxk_euler_step): always the fp32 form, whatever the sign of sigma_next.
__global__ void euler_kernel(const bf16* __restrict__ x, const bf16* __restrict__ x0, bf16* __restrict__ out,
                             int64_t n8, float sigma, float sigma_next) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n8) return;
  const bf16x8 a = *(const bf16x8*)(x + idx * 8);
  const bf16x8 d = *(const bf16x8*)(x0 + idx * 8);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)euler_fp32((float)a[j], (float)d[j], sigma, sigma_next);
  *(bf16x8*)(out + idx * 8) = o;
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

// What any of the entries below was asked for: ltxk_guider_args holds every field of ltxk_step_args, and guider 0 is plain CFG.
struct StepTail : ltxk_guider_args {
  bool sums;                  // ltxk_guidance_sums: nothing is written to `out`
};

static StepTail plain_tail(const ltxk_step_args& a) {
  StepTail t{};
  t.v_pos = a.v_pos, t.v_neg = a.v_neg, t.v_pert = a.v_pert, t.latent = a.latent, t.out = a.out;
  t.clean = a.clean, t.mask = a.mask, t.sigmas_dev = a.sigmas_dev;
  t.B = a.B, t.C = a.C, t.S = a.S;
  t.cfg_scale = a.cfg_scale, t.stg_scale = a.stg_scale, t.sigma = a.sigma, t.sigma_next = a.sigma_next;
  t.flags = a.flags;
  return t;
}

static int check_step_tail(const StepTail& t, const char* name) {
  LTXK_CHECK_ARG(t.v_pos && t.latent && (t.out || t.sums) && t.B > 0 && t.S > 0 && t.C > 0 && t.C % 8 == 0, "%s: bad arguments", name);
  LTXK_CHECK_ARG(t.B <= 65535 && t.C / 8 <= 65535, "%s: B and C/8 must fit a grid dimension (65535)", name);
  LTXK_CHECK_ARG((((uintptr_t)t.v_pos | (uintptr_t)t.v_neg | (uintptr_t)t.v_pert) & 15) == 0,
                 "%s: the token tensors must be 16-byte aligned", name);
  LTXK_CHECK_ARG((t.clean == nullptr) == (t.mask == nullptr), "%s: clean and mask must both be set or both NULL", name);
  LTXK_CHECK_ARG(t.sigmas_dev != nullptr || t.sigma > 0.f, "%s: sigma must be > 0", name);
  if (t.guider == 0) return LTXK_OK;
  LTXK_CHECK_ARG(t.v_neg != nullptr, "%s: null v_neg (the guiders compare the positive with the negative prediction)", name);
  LTXK_CHECK_ARG(t.record != nullptr, "%s: null record", name);
  LTXK_CHECK_ARG(isfinite(t.eta), "%s: eta must be finite", name);
  LTXK_CHECK_ARG(t.norm_threshold >= 0.f && isfinite(t.norm_threshold), "%s: norm_threshold must be finite and >= 0", name);
  return LTXK_OK;
}

template <int GUIDER, bool STG>
static void launch_instance(const StepTail& t, hipStream_t st) {
  hipLaunchKernelGGL((step_tail_kernel<GUIDER, STG>), dim3((t.S + 63) / 64, t.C / 8, t.B), dim3(64), 0, st,
                     (const bf16*)t.v_pos, (const bf16*)t.v_neg, (const bf16*)t.v_pert, (const bf16*)t.latent, (bf16*)t.out,
                     (const bf16*)t.clean, t.mask, (const float*)t.record, (int)t.B, (int)t.C, (int)t.S, t.cfg_scale, t.stg_scale,
                     t.eta, (int)(t.norm_threshold > 0.f), t.sigma, t.sigma_next, t.sigmas_dev, (int)t.flags);
}

// One launch: the instance is picked by the guider and by whether there is a perturbed velocity (v_pert NULL: no STG term).
static void launch_step_tail(const StepTail& t, hipStream_t st) {
  const bool stg = t.v_pert != nullptr;
  if (t.guider == LTXK_GUIDER_CFG_STAR) {
    if (stg) launch_instance<LTXK_GUIDER_CFG_STAR, true>(t, st); else launch_instance<LTXK_GUIDER_CFG_STAR, false>(t, st);
  } else if (t.guider == LTXK_GUIDER_APG) {
    if (stg) launch_instance<LTXK_GUIDER_APG, true>(t, st); else launch_instance<LTXK_GUIDER_APG, false>(t, st);
  } else {
    if (stg) launch_instance<0, true>(t, st); else launch_instance<0, false>(t, st);
  }
}

static int run_step_tail(const StepTail& t, void* stream, const char* name) {
  if (int rc = check_step_tail(t, name)) return rc;
  launch_step_tail(t, (hipStream_t)stream);
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}

static inline int64_t partials_per_sample(int32_t C, int32_t S) { return (int64_t)(C / 8) * ((S + 63) / 64); }

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_euler_step(const void* latent, const void* denoised, void* out, int64_t n,
                               float sigma, float sigma_next, void* stream) {
  LTXK_CHECK_ARG(latent && denoised && out && n > 0 && n % 8 == 0, "ltxk_euler_step: n must be a positive multiple of 8");
  LTXK_CHECK_ARG(sigma > 0.f, "ltxk_euler_step: sigma must be > 0");
  const int64_t n8 = n / 8;
  hipLaunchKernelGGL(euler_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)latent, (const bf16*)denoised, (bf16*)out, n8, sigma, sigma_next);
  LTXK_CHECK_LAUNCH("ltxk_euler_step");
  return LTXK_OK;
}

extern "C" int ltxk_cfg_euler_step(const void* v_pos, const void* v_neg, const void* latent, void* out,
                                   const void* clean, const float* mask, int32_t B, int32_t C, int32_t S,
                                   float cfg_scale, float sigma, float sigma_next, int32_t flags, void* stream) {
  const ltxk_step_args a = {v_pos, v_neg, nullptr, latent, out, clean, mask, nullptr, B, C, S, cfg_scale, 0.f, sigma, sigma_next, flags};
  return run_step_tail(plain_tail(a), stream, "ltxk_cfg_euler_step");
}

extern "C" int ltxk_cfg_euler_step_dev(const void* v_pos, const void* v_neg, const void* latent, void* out,
                                       const void* clean, const float* mask, int32_t B, int32_t C, int32_t S,
                                       float cfg_scale, const float* sigmas_dev, int32_t flags, void* stream) {
  LTXK_CHECK_ARG(sigmas_dev != nullptr, "ltxk_cfg_euler_step_dev: null sigmas_dev");
  const ltxk_step_args a = {v_pos, v_neg, nullptr, latent, out, clean, mask, sigmas_dev, B, C, S, cfg_scale, 0.f, 1.f, 0.f, flags};
  return run_step_tail(plain_tail(a), stream, "ltxk_cfg_euler_step_dev");
}

extern "C" int ltxk_guided_euler_step(const ltxk_step_args* a, void* stream) {
  LTXK_CHECK_ARG(a != nullptr, "ltxk_guided_euler_step: null args");
  return run_step_tail(plain_tail(*a), stream, "ltxk_guided_euler_step");
}

// guider id 0 is refused here: plain CFG is the three entries above
static int check_guider_id(const ltxk_guider_args* a, const char* name) {
  LTXK_CHECK_ARG(a != nullptr, "%s: null args", name);
  LTXK_CHECK_ARG(a->guider == LTXK_GUIDER_CFG_STAR || a->guider == LTXK_GUIDER_APG,
                 "%s: unknown guider %d (LTXK_GUIDER_CFG_STAR or LTXK_GUIDER_APG)", name, (int)a->guider);
  return LTXK_OK;
}

extern "C" int ltxk_guider_euler_step(const ltxk_guider_args* a, void* stream) {
  if (int rc = check_guider_id(a, "ltxk_guider_euler_step")) return rc;
  return run_step_tail(StepTail{*a, false}, stream, "ltxk_guider_euler_step");
}

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
  if (int rc = check_guider_id(a, name)) return rc;
  if (int rc = check_step_tail(StepTail{*a, true}, name)) return rc;
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
