// Text conditioning between a Gemma-3 forward and the DiT context (include/ltxk.h, "Text stage"): the masked per-layer
// statistics and normalisation of the stacked hidden states (text_encoder.py:591-639), and the row kernels of the
// Embeddings1DConnector (text_encoder.py:271-587) at widths the DiT's row kernels do not take (D = 3840 = 7.5 x 512,
// H = 30).  All of it is memory-bound and runs once per prompt: every access is a 16-byte vector, contiguous across
// a wave; nothing here uses a floating-point atomic, so every result is a function of the arguments alone.
#include "common.h"
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
// Unit-weight RMSNorm of rows of any width D % 8 == 0 (D <= 8192): one wave per row, the row held in registers.
// ---------------------------------------------------------------------------------------
constexpr int ROWS_MAXC = 16;   // 16-byte chunks per lane: 64 lanes x 16 x 8 = 8192 elements

__global__ __launch_bounds__(256) void rmsnorm_rows_kernel(const bf16* __restrict__ x, int ldx, bf16* __restrict__ y, int ldy,
                                                           int M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
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
#pragma unroll
  for (int i = 0; i < ROWS_MAXC; ++i) {
    const int c = i * 64 + lane;
    if (c < cpr) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)v[i][j] * rstd);
      *(bf16x8*)(yr + c * 8) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------
// q/k RMSNorm over the full D (weight row per segment) + SPLIT RoPE over each 128-wide head, in place on the q|k buffer,
// any H >= 1.  One wave per (row, segment), the segment held in registers and reduced by the wave itself.  A work item is
// 8 elements of a head's first half and their 8 rotation partners in the second half: 8 items per head, item i of the
// segment goes to lane i % 64 in pass i / 64, so every access is a 16-byte vector and 8 neighbouring lanes cover a
// 128-byte line.  Rounding points are those of ltxk_qknorm_rope.
// ---------------------------------------------------------------------------------------
constexpr int ROPE1D_MAXP = 8;   // 8 passes x 64 items = 64 heads

__global__ __launch_bounds__(256) void qknorm_rope_1d_kernel(bf16* __restrict__ buf, int ld, int M, int D, const bf16* __restrict__ weight,
                                                             const float* __restrict__ cosb, const float* __restrict__ sinb, int T, int H,
                                                             float eps) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= M * 2) return;
  const int row = item >> 1, sgi = item & 1;
  const int t = row % T;
  const int nitem = H * 8;
  bf16* xr = buf + (size_t)row * ld + (size_t)sgi * D;
  const bf16* wr = weight + (size_t)sgi * D;
  bf16x8 a[ROPE1D_MAXP], b[ROPE1D_MAXP];
  float sq = 0.f;
#pragma unroll
  for (int ps = 0; ps < ROPE1D_MAXP; ++ps) {
    const int it = ps * 64 + lane;
    if (it < nitem) {
      const int base = (it >> 3) * 128 + (it & 7) * 8;
      a[ps] = *(const bf16x8*)(xr + base);
      b[ps] = *(const bf16x8*)(xr + base + 64);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float fa = (float)a[ps][j], fb = (float)b[ps][j];
        sq += fa * fa + fb * fb;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int ps = 0; ps < ROPE1D_MAXP; ++ps) {
    const int it = ps * 64 + lane;
    if (it < nitem) {
      const int head = it >> 3, j0 = (it & 7) * 8;
      const int base = head * 128 + j0;
      const bf16x8 wa = *(const bf16x8*)(wr + base);
      const bf16x8 wb = *(const bf16x8*)(wr + base + 64);
      const size_t off = ((size_t)head * T + t) * 64 + j0;
      const f32x4 c0 = *(const f32x4*)(cosb + off), c1 = *(const f32x4*)(cosb + off + 4);
      const f32x4 s0 = *(const f32x4*)(sinb + off), s1 = *(const f32x4*)(sinb + off + 4);
      bf16x8 oa, ob;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x1 = rbf((float)a[ps][j] * rstd * (float)wa[j]);
        const float x2 = rbf((float)b[ps][j] * rstd * (float)wb[j]);
        const float c = j < 4 ? c0[j & 3] : c1[j & 3], sn = j < 4 ? s0[j & 3] : s1[j & 3];
        oa[j] = (bf16)(x1 * c - sn * x2);
        ob[j] = (bf16)(x2 * c + sn * x1);
      }
      *(bf16x8*)(xr + base) = oa;
      *(bf16x8*)(xr + base + 64) = ob;
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

extern "C" int ltxk_rmsnorm_rows(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t M, int32_t D, float eps, void* stream) {
  LTXK_CHECK_ARG(x && y && M > 0 && D > 0, "ltxk_rmsnorm_rows: bad arguments");
  LTXK_CHECK_ARG(D % 8 == 0 && D <= 512 * ROWS_MAXC, "ltxk_rmsnorm_rows: D=%d must be a multiple of 8, at most %d", D, 512 * ROWS_MAXC);
  LTXK_CHECK_ARG(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y),
                 "ltxk_rmsnorm_rows: row strides must be >= D and multiples of 8, pointers 16-byte aligned");
  hipLaunchKernelGGL(rmsnorm_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ldx, (bf16*)y, ldy, M, D, eps);
  LTXK_CHECK_LAUNCH("ltxk_rmsnorm_rows");
  return LTXK_OK;
}

extern "C" int ltxk_qknorm_rope_1d(void* buf, int32_t ld, int32_t M, int32_t D, const void* weight, const float* cos,
                                   const float* sin, int32_t T, int32_t H, float eps, void* stream) {
  LTXK_CHECK_ARG(buf && weight && cos && sin && M > 0 && T > 0, "ltxk_qknorm_rope_1d: bad arguments");
  LTXK_CHECK_ARG(H >= 1 && H <= 8 * ROPE1D_MAXP && D == 128 * H, "ltxk_qknorm_rope_1d: D=%d must be 128*H, 1 <= H=%d <= %d", D, H, 8 * ROPE1D_MAXP);
  LTXK_CHECK_ARG(ld >= 2 * D && ld % 8 == 0 && aligned16(buf) && aligned16(weight) && aligned16(cos) && aligned16(sin),
                 "ltxk_qknorm_rope_1d: ld=%d must be >= 2*D and a multiple of 8, pointers 16-byte aligned", ld);
  LTXK_CHECK_ARG((int64_t)M * 2 <= (int64_t)INT32_MAX, "ltxk_qknorm_rope_1d: too many rows");
  hipLaunchKernelGGL(qknorm_rope_1d_kernel, dim3((2 * M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, D,
                     (const bf16*)weight, cos, sin, T, H, eps);
  LTXK_CHECK_LAUNCH("ltxk_qknorm_rope_1d");
  return LTXK_OK;
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
