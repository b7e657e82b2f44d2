// Row kernels of the text paths, all memory-bound, run once per prompt.
//   Text stage (include/ltxk.h, "Text stage"): the masked per-layer statistics and normalisation of the stacked hidden states
//   (text_encoder.py:591-639), and the row kernels of the Embeddings1DConnector (text_encoder.py:271-587) at widths the DiT's
//   row kernels do not take (D = 3840 = 7.5 x 512, H = 30).
//   Gemma-3 text encoder (include/ltxk.h, "Gemma-3 text encoder"): the scaled embedding gather, Gemma's (1 + w) RMSNorm with the
//   decoder layer's post-norm residual add, the per-head q/k norm + rotate-half RoPE at head dim 256, and the gate * up product
//   of the GeGLU feed-forward.
// Conventions: every access is a 16-byte vector, contiguous across a wave; a row is reduced by one wave (one group of 16 lanes
// for a head) in a fixed order that depends on its width only; nothing uses a floating-point atomic, so every result is a
// function of the arguments alone; each result is rounded to bf16 once with the arithmetic in front of it in fp32.
#include "common.h"
#include "rows.h"
#include <math.h>

namespace ltxk {

// ---------------------------------------------------------------------------------------
// Masked per-(batch, layer) sum / min / max, two stages of fixed shape.
// Stage 1: STATS_P workgroups per (batch, layer) pair, whatever the launch holds.  Workgroup p owns the valid rows
// [p*rpw, (p+1)*rpw), rpw = ceil(count / STATS_P), as one flat list of 16-byte chunks; thread i takes chunks i, i+256, ...
// and keeps EIGHT running sums (one per element slot of the chunk), so a slot sums ceil(rpw * D/8 / 256) terms - 30 at
// count = 1024, D = 3840 - before the fixed trees: 8 slots -> 1 (3 levels), 64 lanes -> 1 (6), 4 waves -> 1 (2).
// Stage 2: one wave per pair sums the STATS_P partials by butterfly (6 levels).  The longest chain of additions a term
// goes through is therefore ceil(rpw * D/8 / 256) + 17, which is what bounds the error of the sum (tests/test_text_stage_gpu.py).
// ---------------------------------------------------------------------------------------
constexpr int STATS_P = 64;
constexpr int STATS_THREADS = 256;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// the valid rows of batch row b, clamped into [0, T) so that a bad table cannot send a load out of the tensor
__device__ __forceinline__ void valid_rows(const int32_t* row_start, const int32_t* row_count, int b, int T, int& start, int& count) {
  start = row_start[b];
  count = row_count[b];
  if (start < 0) start = 0;
  if (start > T) start = T;
  if (count < 0) count = 0;
  if (count > T - start) count = T - start;
}

__global__ __launch_bounds__(STATS_THREADS) void layer_stats_partial_kernel(
    const bf16* __restrict__ x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
    const int32_t* __restrict__ row_start, const int32_t* __restrict__ row_count, int L, int T, int D,
    float* __restrict__ partials) {
  const int pair = blockIdx.y;              // b * L + l
  const int b = pair / L, l = pair - b * L;
  const int p = blockIdx.x;
  int start, count;
  valid_rows(row_start, row_count, b, T, start, count);
  const int rpw = (count + STATS_P - 1) / STATS_P;
  const int r0 = p * rpw;
  const int r1 = min(count, r0 + rpw);
  const int cpr = D >> 3;                                         // 16-byte chunks per row
  const int nchunk = r1 > r0 ? (r1 - r0) * cpr : 0;
  const bf16* base = x + (int64_t)l * layer_stride + (int64_t)b * batch_stride + (int64_t)(start + r0) * row_stride;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  float mn = INFINITY, mx = -INFINITY;
  // four loads in flight per thread; the chunks are still summed in ascending order
  for (int c0 = threadIdx.x; c0 < nchunk; c0 += 4 * STATS_THREADS) {
    bf16x8 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q * STATS_THREADS;
      if (c < nchunk) {
        const int r = c / cpr, cc = c - r * cpr;
        v[q] = *(const bf16x8*)(base + (int64_t)r * row_stride + cc * 8);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (c0 + q * STATS_THREADS < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = (float)v[q][j];
          s[j] += f;
          mn = fminf(mn, f);
          mx = fmaxf(mx, f);
        }
      }
    }
  }
  float sum = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  sum = wave_sum(sum);
  mn = wave_min(mn);
  mx = wave_max(mx);
  __shared__ float red[3][STATS_THREADS / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = sum; red[1][wave] = mn; red[2][wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = partials + (size_t)pair * 3 * STATS_P;
    out[p] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[STATS_P + p] = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
    out[2 * STATS_P + p] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
  }
}

// one wave per pair; a pair without valid rows gets {0, 0, 0}
__global__ __launch_bounds__(64) void layer_stats_final_kernel(const float* __restrict__ partials, const int32_t* __restrict__ row_start,
                                                               const int32_t* __restrict__ row_count, int L, int T,
                                                               float* __restrict__ stats) {
  static_assert(STATS_P == 64, "one partial per lane");
  const int pair = blockIdx.x;
  const int lane = threadIdx.x;
  int start, count;
  valid_rows(row_start, row_count, pair / L, T, start, count);
  const float* in = partials + (size_t)pair * 3 * STATS_P;
  const float sum = wave_sum(in[lane]);
  const float mn = wave_min(in[STATS_P + lane]);
  const float mx = wave_max(in[2 * STATS_P + lane]);
  if (lane == 0) {
    stats[(size_t)pair * 3 + 0] = count > 0 ? sum : 0.f;
    stats[(size_t)pair * 3 + 1] = count > 0 ? mn : 0.f;
    stats[(size_t)pair * 3 + 2] = count > 0 ? mx : 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// out[row0[b] + t, l*D + d] = bf16(8 * (x[l, b, start_b + t, d] - mean) / (range + 1e-6)) for the valid rows only.
// One workgroup per (compact row, layer): a D-wide piece of the input row in, the same piece of the output row out.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layer_norm_compact_kernel(
    const bf16* __restrict__ x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
    const int32_t* __restrict__ row_start, const int32_t* __restrict__ row_count, const int32_t* __restrict__ row0,
    const float* __restrict__ stats, bf16* __restrict__ out, int64_t ldo, int L, int B, int T, int D, int rows) {
  const int r = blockIdx.x, l = blockIdx.y;
  if (r >= rows) return;
  int b = -1, start = 0, count = 0;
  for (int i = 0; i < B; ++i) {
    int st, cn;
    valid_rows(row_start, row_count, i, T, st, cn);
    const int o = row0[i];
    if (r >= o && r < o + cn) { b = i; start = st; count = cn; }
  }
  if (b < 0) return;
  const int t = r - row0[b];
  const float* st = stats + ((size_t)b * L + l) * 3;
  const float mean = st[0] / ((float)((int64_t)count * D) + 1e-6f);
  const float den = (st[2] - st[1]) + 1e-6f;
  const bf16* xr = x + (int64_t)l * layer_stride + (int64_t)b * batch_stride + (int64_t)(start + t) * row_stride;
  bf16* yr = out + (int64_t)r * ldo + (int64_t)l * D;
  for (int c = threadIdx.x * 8; c < D; c += 256 * 8) {
    const bf16x8 v = *(const bf16x8*)(xr + c);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)((8.0f * ((float)v[j] - mean)) / den);
    *(bf16x8*)(yr + c) = o;
  }
}

// ---------------------------------------------------------------------------------------
// RMSNorm of rows of any width D % 8 == 0 (D <= 8192): one wave per row, ROWS_PER_WG rows per workgroup, the row in registers.
// The sum of squares: a lane adds its elements in ascending order, then the wave's butterfly.
//   HAS_W = false (ltxk_rmsnorm_rows): y = bf16(x * rstd)
//   HAS_W = true (ltxk_rmsnorm_weight_rows): y = bf16(x * rstd * (1 + w)), or bf16(resid + rbf(x * rstd * (1 + w))) with a residual
//   (a test that is uniform over the launch).
// One body, two instances: each keeps the registers and the load schedule of its own form.
// ---------------------------------------------------------------------------------------
constexpr int ROWS_MAXC = 16;   // 16-byte chunks per lane: 64 lanes x 16 x 8 = 8192 elements
constexpr int ROWS_PER_WG = 4;

template <bool HAS_W>
__global__ __launch_bounds__(64 * ROWS_PER_WG) void rmsnorm_rows_kernel(
    const bf16* __restrict__ x, int ldx, const bf16* __restrict__ w, const bf16* resid, int ldr, bf16* y, int ldy, int M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16* xr = x + (size_t)row * ldx;
  const int cpr = D >> 3;
  bf16x8 v[ROWS_MAXC];
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS_MAXC; ++i) {
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
  const bf16* rr = HAS_W && resid ? resid + (size_t)row * ldr : nullptr;
#pragma unroll
  for (int i = 0; i < ROWS_MAXC; ++i) {
    const int c = i * 64 + lane;
    if (c < cpr) {
      bf16x8 o;
      if constexpr (!HAS_W) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)v[i][j] * rstd);
      } else {
        const bf16x8 wv = *(const bf16x8*)(w + c * 8);
        if (rr) {
          const bf16x8 rv = *(const bf16x8*)(rr + c * 8);          // read before the store: y may be resid
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)rv[j] + rbf(norm_w<true>((float)v[i][j], rstd, (float)wv[j])));
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (bf16)norm_w<true>((float)v[i][j], rstd, (float)wv[j]);
        }
      }
      *(bf16x8*)(yr + c * 8) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Exact GELU in place: x * (1 + erf(x / sqrt 2)) / 2 = (x / 2) * erfc(-x / sqrt 2).  The erfc form has no cancellation on the
// negative side, where 1 + erf(x / sqrt 2) loses every digit below x ~ -5.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf_f(float x) { return (0.5f * x) * erfcf(-0.70710678118654752440f * x); }

__global__ void gelu_erf_kernel(bf16* __restrict__ x, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i + 8 <= n) {
    bf16x8 v = *(const bf16x8*)(x + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16)gelu_erf_f((float)v[j]);
    *(bf16x8*)(x + i) = v;
  } else {
    for (int64_t k = i; k < n; ++k) x[k] = (bf16)gelu_erf_f((float)x[k]);
  }
}

// ---------------------------------------------------------------------------------------
// Connector input: row t < count_b of batch row b is feature row row0_b + t, row t >= count_b is registers[t % R].
// ---------------------------------------------------------------------------------------
__global__ void connector_assemble_kernel(const bf16* __restrict__ feat, int ldf, const bf16* __restrict__ reg,
                                          const int32_t* __restrict__ row0, const int32_t* __restrict__ row_count, bf16* __restrict__ out,
                                          int B, int T, int D, int R, int feat_rows) {
  const int cpr = D >> 3;
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (int64_t)B * T * cpr) return;
  const int64_t row = c / cpr;
  const int cc = (int)(c - row * cpr) * 8;
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  const int count = row_count[b];
  const int fr = row0[b] + t;
  const bf16* src = (t < count && fr >= 0 && fr < feat_rows) ? feat + (size_t)fr * ldf + cc : reg + (size_t)(t % R) * D + cc;
  *(bf16x8*)(out + (size_t)row * D + cc) = *(const bf16x8*)src;
}

// ---------------------------------------------------------------------------------------
// Gemma-3 text encoder
// ---------------------------------------------------------------------------------------
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

// The same gather over an e4m3fn table: out[m,:] = bf16((fp32(code) * row_scale[id]) * s), both products fp32 in that order, one
// rounding to bf16; row_scale == nullptr: bf16(fp32(code) * s), which is embed_rows_kernel on the table widened to bf16 (every
// e4m3 value is a bf16 value).  A work item is 16 codes: one 16-byte load, v_cvt_pk_f32_fp8, two 16-byte stores.
__global__ void embed_rows_fp8_kernel(const uint8_t* __restrict__ table, const float* __restrict__ row_scale, int V, int D,
                                      const int32_t* __restrict__ ids, bf16* __restrict__ out, int ldo, int M, float s) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int cpr = D >> 4;
  const int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= (int64_t)M * cpr) return;
  const int m = (int)(ci / cpr), cc = (int)(ci - (int64_t)m * cpr) * 16;
  int id = ids[m];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  const u32x4 v = *(const u32x4*)(table + (size_t)id * D + cc);
  const float rs = row_scale ? row_scale[id] : 1.0f;
  bf16x8 o[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], true);
    const float f[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
    for (int e = 0; e < 4; ++e) o[j >> 1][(j & 1) * 4 + e] = (bf16)((row_scale ? f[e] * rs : f[e]) * s);
  }
  *(bf16x8*)(out + (size_t)m * ldo + cc) = o[0];
  *(bf16x8*)(out + (size_t)m * ldo + cc + 8) = o[1];
}

// Per-head RMSNorm (1 + w) + rotate-half RoPE at head dim 256, in place on the first (Hq + Hkv) heads of a row.  A work item
// is 8 elements of a head's first half and their 8 rotation partners 128 columns up; a head is 16 items = one aligned group
// of 16 lanes, which reduces the head's 256 squares itself (16 per lane in ascending order, then the group's butterfly).
// Values and rounding points: rows.h, with Gemma's 1 + w.
// AT (ltxk_headnorm_rope_at): every row takes table row *pos, read from device memory; a position outside [0, T) stores nothing.
constexpr int HEADNORM_DH = 256;

template <bool AT>
__global__ __launch_bounds__(256) void headnorm_rope_kernel(bf16* __restrict__ buf, int ld, int M, int Hq, int Hkv,
                                                            const bf16* __restrict__ qw, const bf16* __restrict__ kw,
                                                            const float* __restrict__ cosb, const float* __restrict__ sinb, int T, float eps,
                                                            const int32_t* __restrict__ pos) {
  const int NH = Hq + Hkv;
  const int64_t heads = (int64_t)M * NH;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hg_raw = gid >> 4;
  int at = 0;
  if constexpr (AT) {
    at = *pos;
    if (at < 0 || at >= T) return;                // uniform over the launch
  }
  const bool live = hg_raw < heads;               // uniform over a group of 16 lanes
  const int64_t hg = live ? hg_raw : heads - 1;
  const int it = (int)(gid & 15);
  const int row = (int)(hg / NH), hh = (int)(hg - (int64_t)row * NH);
  const int t = AT ? at : row % T;
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
  const RopeTab tab = rope_load(cosb, sinb, (size_t)t * 128 + it * 8);
  bf16x8 oa, ob;
  norm_rope<true>(a, b, rstd, wa, wb, true, tab, oa, ob);
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

static int check_layers(const char* who, const void* x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
                        const int32_t* row_start, const int32_t* row_count, int32_t L, int32_t B, int32_t T, int32_t D) {
  LTXK_CHECK_ARG(x && row_start && row_count, "%s: null pointer", who);
  LTXK_CHECK_ARG(L > 0 && B > 0 && T > 0 && D > 0 && D % 8 == 0, "%s: bad dims L=%d B=%d T=%d D=%d (D must be a multiple of 8)", who, L, B, T, D);
  LTXK_CHECK_ARG((int64_t)L * B <= 65535, "%s: L*B = %lld exceeds 65535", who, (long long)L * B);
  LTXK_CHECK_ARG(aligned16(x) && row_stride >= D && row_stride % 8 == 0 && layer_stride % 8 == 0 && batch_stride % 8 == 0 &&
                     layer_stride >= 0 && batch_stride >= 0,
                 "%s: x must be 16-byte aligned with strides that are multiples of 8 elements, row stride >= D", who);
  return LTXK_OK;
}

extern "C" int ltxk_masked_layer_stats(const void* x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
                                       const int32_t* row_start, const int32_t* row_count, int32_t L, int32_t B, int32_t T,
                                       int32_t D, float* partials, float* stats, void* stream) {
  const int rc = check_layers("ltxk_masked_layer_stats", x, layer_stride, batch_stride, row_stride, row_start, row_count, L, B, T, D);
  if (rc != LTXK_OK) return rc;
  LTXK_CHECK_ARG(partials && stats, "ltxk_masked_layer_stats: null partials / stats");
  hipLaunchKernelGGL(layer_stats_partial_kernel, dim3(STATS_P, L * B), dim3(STATS_THREADS), 0, (hipStream_t)stream, (const bf16*)x,
                     layer_stride, batch_stride, row_stride, row_start, row_count, L, T, D, partials);
  LTXK_CHECK_LAUNCH("ltxk_masked_layer_stats");
  hipLaunchKernelGGL(layer_stats_final_kernel, dim3(L * B), dim3(64), 0, (hipStream_t)stream, (const float*)partials, row_start,
                     row_count, L, T, stats);
  LTXK_CHECK_LAUNCH("ltxk_masked_layer_stats");
  return LTXK_OK;
}

extern "C" int ltxk_layer_norm_compact(const void* x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
                                       const int32_t* row_start, const int32_t* row_count, const int32_t* row0, const float* stats,
                                       void* out, int64_t ldo, int32_t L, int32_t B, int32_t T, int32_t D, int32_t rows,
                                       void* stream) {
  const int rc = check_layers("ltxk_layer_norm_compact", x, layer_stride, batch_stride, row_stride, row_start, row_count, L, B, T, D);
  if (rc != LTXK_OK) return rc;
  LTXK_CHECK_ARG(row0 && stats && out && aligned16(out), "ltxk_layer_norm_compact: null row0 / stats / out, or out not 16-byte aligned");
  LTXK_CHECK_ARG(rows >= 0 && (int64_t)rows <= (int64_t)B * T, "ltxk_layer_norm_compact: rows=%d must be in [0, B*T]", rows);
  LTXK_CHECK_ARG(ldo >= (int64_t)L * D && ldo % 8 == 0, "ltxk_layer_norm_compact: ldo=%lld must be >= L*D and a multiple of 8", (long long)ldo);
  if (rows == 0) return LTXK_OK;
  hipLaunchKernelGGL(layer_norm_compact_kernel, dim3(rows, L), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, layer_stride,
                     batch_stride, row_stride, row_start, row_count, row0, stats, (bf16*)out, ldo, L, B, T, D, rows);
  LTXK_CHECK_LAUNCH("ltxk_layer_norm_compact");
  return LTXK_OK;
}

// the launcher of both RMSNorm entry points, after their own argument checks: weight == NULL is the unit-weight instance
static int rmsnorm_rows_launch(const char* who, const void* x, int ldx, const void* weight, const void* resid, int ldr, void* y, int ldy, int M,
                               int D, float eps, void* stream) {
  const dim3 grid((M + ROWS_PER_WG - 1) / ROWS_PER_WG), block(64 * ROWS_PER_WG);
  if (weight)
    hipLaunchKernelGGL(rmsnorm_rows_kernel<true>, grid, block, 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)weight, (const bf16*)resid,
                       ldr, (bf16*)y, ldy, M, D, eps);
  else
    hipLaunchKernelGGL(rmsnorm_rows_kernel<false>, grid, block, 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)nullptr,
                       (const bf16*)nullptr, 0, (bf16*)y, ldy, M, D, eps);
  LTXK_CHECK_LAUNCH(who);
  return LTXK_OK;
}

extern "C" int ltxk_rmsnorm_rows(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t M, int32_t D, float eps, void* stream) {
  LTXK_CHECK_ARG(x && y && M > 0 && D > 0, "ltxk_rmsnorm_rows: bad arguments");
  LTXK_CHECK_ARG(D % 8 == 0 && D <= 512 * ROWS_MAXC, "ltxk_rmsnorm_rows: D=%d must be a multiple of 8, at most %d", D, 512 * ROWS_MAXC);
  LTXK_CHECK_ARG(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y),
                 "ltxk_rmsnorm_rows: row strides must be >= D and multiples of 8, pointers 16-byte aligned");
  return rmsnorm_rows_launch("ltxk_rmsnorm_rows", x, ldx, nullptr, nullptr, 0, y, ldy, M, D, eps, stream);
}

extern "C" int ltxk_gelu_erf(void* x, int64_t n, void* stream) {
  LTXK_CHECK_ARG(x && n > 0 && aligned16(x), "ltxk_gelu_erf: x must be a 16-byte aligned buffer of n > 0 elements");
  const int64_t n8 = (n + 7) / 8;
  LTXK_CHECK_ARG((n8 + 255) / 256 <= (int64_t)INT32_MAX, "ltxk_gelu_erf: n too large");
  hipLaunchKernelGGL(gelu_erf_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (bf16*)x, n);
  LTXK_CHECK_LAUNCH("ltxk_gelu_erf");
  return LTXK_OK;
}

extern "C" int ltxk_connector_assemble(const void* feat, int32_t ldf, const void* registers, const int32_t* row0,
                                       const int32_t* row_count, void* out, int32_t B, int32_t T, int32_t D, int32_t R,
                                       int32_t feat_rows, void* stream) {
  LTXK_CHECK_ARG(registers && row0 && row_count && out && B > 0 && T > 0 && R > 0 && D > 0 && D % 8 == 0, "ltxk_connector_assemble: bad arguments");
  LTXK_CHECK_ARG(feat_rows >= 0 && (feat_rows == 0 || (feat && ldf >= D && ldf % 8 == 0 && aligned16(feat))),
                 "ltxk_connector_assemble: feat must be 16-byte aligned with ldf >= D, a multiple of 8");
  LTXK_CHECK_ARG(aligned16(registers) && aligned16(out), "ltxk_connector_assemble: registers / out must be 16-byte aligned");
  const int64_t chunks = (int64_t)B * T * (D / 8);
  LTXK_CHECK_ARG((chunks + 255) / 256 <= (int64_t)INT32_MAX, "ltxk_connector_assemble: too large");
  hipLaunchKernelGGL(connector_assemble_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)feat, ldf, (const bf16*)registers, row0, row_count, (bf16*)out, B, T, D, R, feat_rows);
  LTXK_CHECK_LAUNCH("ltxk_connector_assemble");
  return LTXK_OK;
}

extern "C" int ltxk_embed_rows(const void* table, int32_t V, int32_t D, const int32_t* ids, void* out, int32_t ldo, int32_t M,
                               float s, void* stream) {
  LTXK_CHECK_ARG(table && ids && out && V > 0 && M > 0 && D > 0, "ltxk_embed_rows: bad arguments");
  LTXK_CHECK_ARG(D % 8 == 0 && D <= 512 * ROWS_MAXC, "ltxk_embed_rows: D=%d must be a multiple of 8, at most %d", D, 512 * ROWS_MAXC);
  LTXK_CHECK_ARG(ldo >= D && ldo % 8 == 0 && aligned16(table) && aligned16(out) && ((uintptr_t)ids & 3) == 0,
                 "ltxk_embed_rows: ldo must be >= D and a multiple of 8, table / out 16-byte aligned");
  const int64_t chunks = (int64_t)M * (D / 8);
  LTXK_CHECK_ARG((chunks + 255) / 256 <= (int64_t)INT32_MAX, "ltxk_embed_rows: too large");
  hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)table, V, D,
                     ids, (bf16*)out, ldo, M, s);
  LTXK_CHECK_LAUNCH("ltxk_embed_rows");
  return LTXK_OK;
}

extern "C" int ltxk_embed_rows_fp8(const void* table, const float* row_scale, int32_t V, int32_t D, const int32_t* ids, void* out,
                                   int32_t ldo, int32_t M, float s, void* stream) {
  LTXK_CHECK_ARG(table && ids && out && V > 0 && M > 0 && D > 0, "ltxk_embed_rows_fp8: bad arguments");
  LTXK_CHECK_ARG(D % 16 == 0, "ltxk_embed_rows_fp8: D=%d must be a multiple of 16", D);
  LTXK_CHECK_ARG(ldo >= D && ldo % 8 == 0 && aligned16(table) && aligned16(out) && ((uintptr_t)ids & 3) == 0 && ((uintptr_t)row_scale & 3) == 0,
                 "ltxk_embed_rows_fp8: ldo must be >= D and a multiple of 8, table / out 16-byte aligned, ids / row_scale 4-byte aligned");
  const int64_t chunks = (int64_t)M * (D / 16);
  LTXK_CHECK_ARG((chunks + 255) / 256 <= (int64_t)INT32_MAX, "ltxk_embed_rows_fp8: too large");
  hipLaunchKernelGGL(embed_rows_fp8_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)table,
                     row_scale, V, D, ids, (bf16*)out, ldo, M, s);
  LTXK_CHECK_LAUNCH("ltxk_embed_rows_fp8");
  return LTXK_OK;
}

extern "C" int ltxk_rmsnorm_weight_rows(const void* x, int32_t ldx, const void* weight, const void* resid, int32_t ldr, void* y,
                                        int32_t ldy, int32_t M, int32_t D, float eps, void* stream) {
  LTXK_CHECK_ARG(x && weight && y && M > 0 && D > 0, "ltxk_rmsnorm_weight_rows: bad arguments");
  LTXK_CHECK_ARG(D % 8 == 0 && D <= 512 * ROWS_MAXC, "ltxk_rmsnorm_weight_rows: D=%d must be a multiple of 8, at most %d", D, 512 * ROWS_MAXC);
  LTXK_CHECK_ARG(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(weight),
                 "ltxk_rmsnorm_weight_rows: row strides must be >= D and multiples of 8, pointers 16-byte aligned");
  LTXK_CHECK_ARG(!resid || (ldr >= D && ldr % 8 == 0 && aligned16(resid)),
                 "ltxk_rmsnorm_weight_rows: resid must be 16-byte aligned with ldr >= D, a multiple of 8");
  return rmsnorm_rows_launch("ltxk_rmsnorm_weight_rows", x, ldx, weight, resid, ldr, y, ldy, M, D, eps, stream);
}

template <bool AT>
static int headnorm_rope_launch(const char* who, void* buf, int32_t ld, int32_t M, int32_t Hq, int32_t Hkv, const void* q_weight,
                                const void* k_weight, const float* cos, const float* sin, int32_t T, const int32_t* pos, float eps, void* stream) {
  LTXK_CHECK_ARG(buf && q_weight && k_weight && cos && sin && M > 0 && T > 0, "%s: bad arguments", who);
  LTXK_CHECK_ARG(!AT || (pos && ((uintptr_t)pos & 3) == 0), "%s: pos: null or misaligned pointer", who);
  LTXK_CHECK_ARG(Hq >= 1 && Hkv >= 1 && (int64_t)(Hq + Hkv) * HEADNORM_DH <= (int64_t)ld, "%s: ld=%d must be >= (Hq + Hkv) * 256, Hq=%d Hkv=%d",
                 who, ld, Hq, Hkv);
  LTXK_CHECK_ARG(ld % 8 == 0 && aligned16(buf) && aligned16(q_weight) && aligned16(k_weight) && aligned16(cos) && aligned16(sin),
                 "%s: ld must be a multiple of 8, pointers 16-byte aligned", who);
  const int64_t groups = ((int64_t)M * (Hq + Hkv) * 16 + 255) / 256;
  LTXK_CHECK_ARG(groups <= (int64_t)INT32_MAX, "%s: too many rows", who);
  hipLaunchKernelGGL(headnorm_rope_kernel<AT>, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, Hq, Hkv,
                     (const bf16*)q_weight, (const bf16*)k_weight, cos, sin, T, eps, pos);
  LTXK_CHECK_LAUNCH(who);
  return LTXK_OK;
}

extern "C" int ltxk_headnorm_rope(void* buf, int32_t ld, int32_t M, int32_t Hq, int32_t Hkv, const void* q_weight, const void* k_weight,
                                  const float* cos, const float* sin, int32_t T, float eps, void* stream) {
  return headnorm_rope_launch<false>("ltxk_headnorm_rope", buf, ld, M, Hq, Hkv, q_weight, k_weight, cos, sin, T, nullptr, eps, stream);
}

extern "C" int ltxk_headnorm_rope_at(void* buf, int32_t ld, int32_t M, int32_t Hq, int32_t Hkv, const void* q_weight, const void* k_weight,
                                     const float* cos, const float* sin, int32_t T, const int32_t* pos, float eps, void* stream) {
  return headnorm_rope_launch<true>("ltxk_headnorm_rope_at", buf, ld, M, Hq, Hkv, q_weight, k_weight, cos, sin, T, pos, eps, stream);
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
