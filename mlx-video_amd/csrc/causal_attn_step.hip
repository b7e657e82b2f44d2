// One query position per batch row against a per-layer KV cache (include/ltxk.h, "Gemma-3 decoding"): the attention of a
// KV-cached decode step, the shape ltxk_causal_attn (Tq == Tk) does not take.  A memory-bound read of the live cache, so K and
// V^T go straight from global memory to the MFMA operand registers (no LDS staging); LDS only carries the four waves' partials.
//
// Launch 1, one workgroup of 4 waves per (batch row, KV head, 256-key slice s = keys [256 s, 256 s + 256)); wave w owns the
// 64-key tile 256 s + 64 w.  The Hq/Hkv <= 16 query heads of the KV head are the columns of the 16-wide B operand, so the
// head's cache is read once for its whole group: in attn_tile.h's operand map "query row c" is query head c of the group,
// and every K and V^T fragment is one 16-byte global load.
// Key `step` is the new token: its K row is read from k_new and its V^T column from v_new, never from the cache, and the wave
// whose tile holds `step` stores both into the cache (the append).  Nobody else in the launch touches that row / column.
// A tile wholly outside [max(row_start, step - window + 1), step] is not fetched: its partial is (M = none, l = 0, O = 0).
// Each wave leaves (M, l, O^T) of its tile in LDS; the workgroup merges the four in ascending order into the slice's partial
// (M, l, O[256]) fp32.  Launch 2 merges the slices in ascending order and divides.  M is an integer in the exp2 domain (the
// ceil of the maximum over the visible keys), so every rescale 2^(M_part - M) is exact; which keys form a partial is a
// function of `step` (and the host's window) only, never of B, the cache capacity or what else the launch holds.  No atomics.
#include "attn_tile.h"

namespace ltxk {

constexpr int CS_DH = 256;                       // head dim
constexpr int CS_SLICE = 4 * AT_BK;              // keys per workgroup, one tile per wave
constexpr int CS_PART = 2 + CS_DH;               // floats of one partial: M, l, O[256]
constexpr int CS_LDS = 4 * (2 * 16 + 16 * CS_DH) * 4;      // per wave: M[16], l[16], O[16][256]

// The first slice a launch covers: slices wholly below the window hold no visible key for any row_start.
__host__ __device__ __forceinline__ int cs_first_slice(int step, int window) {
  return window > 0 && step - window + 1 > 0 ? (step - window + 1) / CS_SLICE : 0;
}

// sum over the parts, ascending, of part * 2^(M_part - M); every factor a power of two (0 for a part without a visible key)
__device__ __forceinline__ float cs_rescale(float m_part, float m) { return __builtin_amdgcn_exp2f(m_part - m); }

// DEV (ltxk_causal_attn_dev_step): `step` is *step_dev, and s0 / nslices are derived from it here; the grid holds `gslices`
// slices per (batch row, KV head), sized by the host for max_step, and a workgroup past the step's own count - or any
// workgroup when *step_dev lies outside [0, max_step] - leaves here, block-uniformly, ahead of every load, store and barrier.
// The host form passes gslices == nslices and takes the same path from there on.
template <bool DEV>
__global__ __launch_bounds__(256) void causal_attn_step_kernel(
    const bf16* __restrict__ q, int ldq, const bf16* __restrict__ k_new, int ldkn, const bf16* __restrict__ v_new, int ldvn,
    bf16* k_cache, int ldk, bf16* vt_cache, int ldvt, const int32_t* __restrict__ row_start, float* __restrict__ partials,
    int Hq, int Hkv, int cap, int step, const int32_t* __restrict__ step_dev, int max_step, int window, int s0, int nslices,
    int gslices, float cl2e) {
  if constexpr (DEV) {
    step = *step_dev;
    if (step < 0 || step > max_step) return;
    s0 = cs_first_slice(step, window);
    nslices = step / CS_SLICE + 1 - s0;
    if ((int)(blockIdx.x % (unsigned)gslices) >= nslices) return;
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm_m = (float*)smem;                    // [4][16]
  float* sm_l = sm_m + 64;                       // [4][16]
  float* sm_o = sm_l + 64;                       // [4][16][256]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int G = Hq / Hkv;
  const int si = (int)(blockIdx.x % (unsigned)gslices);
  const int bk = (int)(blockIdx.x / (unsigned)gslices);
  const int b = bk / Hkv, hk = bk - b * Hkv;
  const int kt = (s0 + si) * CS_SLICE + wave * AT_BK;          // this wave's first key
  int rs = row_start[b];
  rs = rs < 0 ? 0 : rs;
  int klo = rs;
  if (window > 0) klo = max(klo, step - window + 1);
  const bool has_step = step >= kt && step < kt + AT_BK;       // wave-uniform
  const bool live = kt <= step && kt + AT_BK - 1 >= klo;       // wave-uniform: the tile holds a visible key

  bf16* kbase = k_cache + (size_t)b * cap * ldk + (size_t)hk * CS_DH;
  bf16* vbase = vt_cache + ((size_t)b * Hkv + hk) * CS_DH * ldvt;
  const bf16* knew = k_new + (size_t)b * ldkn + (size_t)hk * CS_DH;
  const bf16* vnew = v_new + (size_t)b * ldvn + (size_t)hk * CS_DH;

  if (has_step) {                                // the append: K row `step` (32 lanes x 16 bytes), V^T column `step`
    if (lane < 32) *(bf16x8*)(kbase + (size_t)step * ldk + lane * 8) = *(const bf16x8*)(knew + lane * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = i * 64 + lane;
      vbase[(size_t)d * ldvt + step] = vnew[d];
    }
  }

  float m_tile = AT_NONE, l_tile = 0.f;
  f32x4 o[16];
  at_zero(o);

  if (live) {
    // ---- operands: K and V^T fragments straight from the cache, the group's query heads as B columns ----
    bf16x8 kf[4][8], vf[16][2], qf[8];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const int key = kt + at_keymap(kb, c);                   // < cap: kt <= step < cap, both multiples of 64 apart
      const bf16* kp = (key == step ? knew : kbase + (size_t)key * ldk) + g * 8;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) kf[kb][ks] = *(const bf16x8*)(kp + ks * 32);
    }
#pragma unroll
    for (int db = 0; db < 16; ++db) {
      const bf16* vp = vbase + (size_t)(db * 16 + c) * ldvt + kt + g * 8;
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) vf[db][kc] = *(const bf16x8*)(vp + kc * 32);
    }
    {
      const int h = hk * G + (c < G ? c : G - 1);              // columns past the group repeat its last head; never stored
      const bf16* qp = q + (size_t)b * ldq + (size_t)h * CS_DH + g * 8;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 32);
    }
    if (has_step) {                              // column `step` of V^T comes from v_new: one element of one lane group's chunk
      const int off = step - kt, kc_s = off >> 5, g_s = (off >> 3) & 3, e_s = off & 7;
      if (g == g_s) {
#pragma unroll
        for (int db = 0; db < 16; ++db) {
          const bf16 nv = vnew[db * 16 + c];
#pragma unroll
          for (int kc = 0; kc < 2; ++kc)
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (kc == kc_s && e == e_s) vf[db][kc][e] = nv;
        }
      }
    }
    // ---- the tile, with no running state; key j is visible iff row_start <= j <= step and (no window or step - j < window):
    // every head of the group sees the same keys.  (& not &&: seen in the assembly only - with & hipcc keeps the instruction
    // order the hand-written loop had, all 32 S^T MFMAs and then the score reads; with && it reads the first score blocks back
    // between them) ----
    f32x4 s[4];
    at_scores<CS_DH>(s, qf, [&](int kb, int ks) { return kf[kb][ks]; });
    const unsigned vis = at_mask(s, kt, g, cl2e, m_tile, [&](int key) { return (key >= klo) & (key <= step); });
    bf16x8 pb[2];
    l_tile = lane_xor32_sum(lane_xor16_sum(at_probs(s, vis, cl2e, m_tile, pb)));
    at_pv<CS_DH>(o, pb, [&](int db, int kc) { return vf[db][kc]; });
  }

  // ---- the wave's partial to LDS ----
  if (g == 0) { sm_m[wave * 16 + c] = m_tile; sm_l[wave * 16 + c] = l_tile; }
  {
    float* op = sm_o + (size_t)(wave * 16 + c) * CS_DH + 4 * g;
#pragma unroll
    for (int db = 0; db < 16; ++db) *(f32x4*)(op + db * 16) = o[db];
  }
  __syncthreads();

  // ---- merge the four tiles in ascending order: thread = channel, one head of the group at a time ----
  for (int qh = 0; qh < G; ++qh) {
    float m = AT_NONE;
#pragma unroll
    for (int w = 0; w < 4; ++w) m = fmaxf(m, sm_m[w * 16 + qh]);
    float l = 0.f, acc = 0.f;
    if (m > -1e29f) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float a = cs_rescale(sm_m[w * 16 + qh], m);
        l += sm_l[w * 16 + qh] * a;
        acc += sm_o[(size_t)(w * 16 + qh) * CS_DH + tid] * a;
      }
    }
    float* part = partials + (((size_t)b * Hq + hk * G + qh) * nslices + si) * CS_PART;
    if (tid == 0) { part[0] = m; part[1] = l; }
    part[2 + tid] = acc;
  }
}

// Launch 2: one workgroup per (batch row, query head), thread = channel; the slices merged in ascending order, then O / l.
template <bool DEV>
__global__ __launch_bounds__(256) void causal_attn_step_combine_kernel(const float* __restrict__ partials, bf16* __restrict__ out,
                                                                         int ldo, int Hq, int nslices, const int32_t* __restrict__ step_dev,
                                                                         int max_step, int window) {
  if constexpr (DEV) {                           // the device count of slices; a step out of range stores nothing
    const int step = *step_dev;
    if (step < 0 || step > max_step) return;
    nslices = step / CS_SLICE + 1 - cs_first_slice(step, window);
  }
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)Hq), h = (int)(blockIdx.x % (unsigned)Hq);
  const float* part = partials + ((size_t)b * Hq + h) * nslices * CS_PART;
  float m = AT_NONE;
  for (int s = 0; s < nslices; ++s) m = fmaxf(m, part[(size_t)s * CS_PART]);
  float l = 0.f, acc = 0.f;
  if (m > -1e29f) {
    for (int s = 0; s < nslices; ++s) {
      const float* ps = part + (size_t)s * CS_PART;
      const float a = cs_rescale(ps[0], m);
      l += ps[1] * a;
      acc += ps[2 + tid] * a;
    }
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  out[(size_t)b * ldo + (size_t)h * CS_DH + tid] = l > 0.f ? (bf16)(acc * inv) : (bf16)0.f;
}

}  // namespace ltxk

using namespace ltxk;

// The checks both entries share, and the two launches.  DEV: `step` is max_step, which sizes the grid and the partials.
template <bool DEV>
static int causal_attn_step_launch(const char* who, const void* q, int32_t ldq, const void* k_new, int32_t ldkn, const void* v_new, int32_t ldvn,
                                   void* k_cache, int32_t ldk, void* vt_cache, int32_t ldvt, void* out, int32_t ldo,
                                   const int32_t* row_start, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t step,
                                   const int32_t* step_dev, int32_t window, float scale, float* partials, int64_t partials_floats,
                                   void* stream) {
  LTXK_CHECK_ARG(q && k_new && v_new && k_cache && vt_cache && out && row_start && partials, "%s: null pointer", who);
  LTXK_CHECK_ARG(!DEV || (step_dev && ((uintptr_t)step_dev & 3) == 0), "%s: step: null or misaligned pointer", who);
  LTXK_CHECK_ARG(B > 0 && Hq > 0 && Hkv > 0 && cap > 0, "%s: bad dims B=%d Hq=%d Hkv=%d cap=%d", who, B, Hq, Hkv, cap);
  LTXK_CHECK_ARG(Hq % Hkv == 0 && Hq / Hkv <= 16, "%s: Hq=%d must be a multiple of Hkv=%d, at most 16 times it", who, Hq, Hkv);
  LTXK_CHECK_ARG(cap % AT_BK == 0, "%s: cap=%d must be a multiple of %d", who, cap, AT_BK);
  LTXK_CHECK_ARG(step >= 0 && step < cap, "%s: %s=%d must lie in [0, cap=%d)", who, DEV ? "max_step" : "step", step, cap);
  LTXK_CHECK_ARG(scale > 0.f, "%s: scale must be positive", who);
  LTXK_CHECK_ARG(window >= 0, "%s: window=%d must be 0 (none) or a positive count", who, window);
  LTXK_CHECK_ARG((int64_t)Hq * CS_DH <= INT32_MAX && ldq >= Hq * CS_DH && ldo >= Hq * CS_DH && ldkn >= Hkv * CS_DH &&
                     ldvn >= Hkv * CS_DH && ldk >= Hkv * CS_DH,
                 "%s: row strides must be >= Hq*256 (q, out) and >= Hkv*256 (k_new, v_new, k_cache)", who);
  LTXK_CHECK_ARG(ldq % 8 == 0 && ldkn % 8 == 0 && ldvn % 8 == 0 && ldk % 8 == 0 && ldo % 8 == 0, "%s: row strides must be multiples of 8", who);
  LTXK_CHECK_ARG(ldvt >= cap && ldvt % 8 == 0, "%s: ldvt=%d must be >= cap=%d and a multiple of 8", who, ldvt, cap);
  LTXK_CHECK_ARG((((uintptr_t)q | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)vt_cache | (uintptr_t)out |
                   (uintptr_t)partials) & 15) == 0 && ((uintptr_t)row_start & 3) == 0,
                 "%s: q, k_new, v_new, k_cache, vt_cache, out, partials must be 16-byte aligned", who);
  const int s0 = DEV ? 0 : cs_first_slice(step, window);
  int nslices = step / CS_SLICE + 1 - s0;
  const int reach = (window + CS_SLICE - 2) / CS_SLICE + 1;                  // the most slices a window of keys can touch
  if (DEV && window > 0 && reach < nslices) nslices = reach;
  const int64_t need = (int64_t)B * Hq * nslices * CS_PART;
  LTXK_CHECK_ARG(partials_floats >= need, "%s: partials holds %lld floats, %lld needed (B*Hq*slices*258)", who,
                 (long long)partials_floats, (long long)need);
  LTXK_CHECK_ARG((int64_t)B * Hkv * nslices <= INT32_MAX, "%s: too many workgroups", who);
  static std::atomic<uint64_t> attr_set{0};
  const int rc = ensure_dyn_lds((const void*)causal_attn_step_kernel<DEV>, CS_LDS, attr_set, who);
  if (rc != LTXK_OK) return rc;
  hipLaunchKernelGGL(causal_attn_step_kernel<DEV>, dim3((unsigned)(B * Hkv * nslices)), dim3(256), CS_LDS, (hipStream_t)stream,
                     (const bf16*)q, ldq, (const bf16*)k_new, ldkn, (const bf16*)v_new, ldvn, (bf16*)k_cache, ldk, (bf16*)vt_cache, ldvt,
                     row_start, partials, Hq, Hkv, cap, step, step_dev, step, window, s0, nslices, nslices, scale * 1.4426950408889634f);
  LTXK_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(causal_attn_step_combine_kernel<DEV>, dim3((unsigned)(B * Hq)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)partials, (bf16*)out, ldo, Hq, nslices, step_dev, step, window);
  LTXK_CHECK_LAUNCH(who);
  return LTXK_OK;
}

extern "C" int ltxk_causal_attn_step(const void* q, int32_t ldq, const void* k_new, int32_t ldkn, const void* v_new, int32_t ldvn,
                                     void* k_cache, int32_t ldk, void* vt_cache, int32_t ldvt, void* out, int32_t ldo,
                                     const int32_t* row_start, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t step,
                                     int32_t window, float scale, float* partials, int64_t partials_floats, void* stream) {
  return causal_attn_step_launch<false>("ltxk_causal_attn_step", q, ldq, k_new, ldkn, v_new, ldvn, k_cache, ldk, vt_cache, ldvt, out, ldo,
                                        row_start, B, Hq, Hkv, cap, step, nullptr, window, scale, partials, partials_floats, stream);
}

extern "C" int ltxk_causal_attn_dev_step(const void* q, int32_t ldq, const void* k_new, int32_t ldkn, const void* v_new, int32_t ldvn,
                                         void* k_cache, int32_t ldk, void* vt_cache, int32_t ldvt, void* out, int32_t ldo,
                                         const int32_t* row_start, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, const int32_t* step,
                                         int32_t max_step, int32_t window, float scale, float* partials, int64_t partials_floats,
                                         void* stream) {
  return causal_attn_step_launch<true>("ltxk_causal_attn_dev_step", q, ldq, k_new, ldkn, v_new, ldvn, k_cache, ldk, vt_cache, ldvt, out, ldo,
                                       row_start, B, Hq, Hkv, cap, max_step, step, window, scale, partials, partials_floats, stream);
}
