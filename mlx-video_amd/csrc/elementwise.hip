// HBM-bound row / elementwise kernels of the DiT step (include/ltxk.h).  All loads/stores are
// 8- or 16-byte vectors; row reductions are wave64 shuffles (one wave per row); every bf16
// rounding point of the reference's op chain is reproduced.
#include "common.h"
#include "rows.h"
#include <math.h>
#include <stdlib.h>

namespace ltxk {

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

constexpr int ROWS_PER_BLOCK = 4;  // one wave per row, 4 waves per workgroup
constexpr int MAX_CHUNKS = 16;     // D <= 16*512 = 8192

// ---------------------------------------------------------------------------------------
// rms_norm / layer_norm (no affine) + AdaLN modulation
// ---------------------------------------------------------------------------------------
// One wave per row.  Tried and measured slower in the step (11.5-14 us -> 18.5 us per launch at M=2560): walking
// several rows per wave with the next row's loads in flight, and requesting the modulation rows up front.
template <bool LAYERNORM>
__global__ __launch_bounds__(256) void norm_modulate_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ y, int M, int D, float eps,
    const bf16* __restrict__ scale, const bf16* __restrict__ shift, int mod_stride,
    const int32_t* __restrict__ mod_row) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16* xr = x + (size_t)row * D;
  const int nch = D >> 9;  // chunks of 512 elements (64 lanes x 8)
  bf16x8 v[MAX_CHUNKS];
  float sum = 0.f, sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAX_CHUNKS; ++i) {
    if (i < nch) {
      v[i] = *(const bf16x8*)(xr + i * 512 + lane * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[i][j];
        sum += f;
        sq += f * f;
      }
    }
  }
  float mean = 0.f, rstd;
  if constexpr (LAYERNORM) {
    mean = wave_sum(sum) / (float)D;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_CHUNKS; ++i)
      if (i < nch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = (float)v[i][j] - mean;
          var += d * d;
        }
      }
    var = wave_sum(var) / (float)D;
    rstd = rsqrtf(var + eps);
  } else {
    rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
  }
  const size_t mrow = scale ? (size_t)(mod_row ? mod_row[row] : 0) * mod_stride : 0;
  bf16* yr = y + (size_t)row * D;
#pragma unroll
  for (int i = 0; i < MAX_CHUNKS; ++i) {
    if (i < nch) {
      const int col = i * 512 + lane * 8;
      bf16x8 o;
      if (scale) {
        const bf16x8 sc = *(const bf16x8*)(scale + mrow + col);
        const bf16x8 sh = *(const bf16x8*)(shift + mrow + col);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float n = rbf(((float)v[i][j] - mean) * rstd);
          const float one_p = rbf(1.0f + (float)sc[j]);
          o[j] = (bf16)(rbf(n * one_p) + (float)sh[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)(((float)v[i][j] - mean) * rstd);
      }
      *(bf16x8*)(yr + col) = o;
    }
  }
}

// rms_norm + modulation when the row's sum of squares is already known (the producing GEMM's `sumsq` output: NP fp32
// partials per row).  With the statistic precomputed nothing ties a row to one wave: a row is cut into WPR pieces of
// 64*EPL elements, one per wave, each a short independent chain {1 partial load + x loads in flight together ->
// 6-step wave sum -> a dozen VALU ops per element -> store}.  The wave-per-row kernel above keeps a 4096-element row
// in one wave (8 KB of loads, then a reduction that waits for all of them, then 64 elements of arithmetic per lane):
// at M=2560 that is 10 waves per CU each running a long serial chain, i.e. latency-bound at ~3 TB/s.
// ONE_PLUS: `scale` already holds bf16(1 + scale) (ltxk_ada_combine's one_plus_mask), saving an add and a rounding
// per element.
template <int CH, bool ONE_PLUS>     // CH = 16-byte chunks per lane
__global__ __launch_bounds__(256) void norm_scale_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ y, int M, int D, float eps, const float* __restrict__ sumsq, int ss_ld, int NP,
    const bf16* __restrict__ scale, const bf16* __restrict__ shift, int mod_stride, const int32_t* __restrict__ mod_row) {
  const int lane = threadIdx.x & 63;
  const int wpr = D / (512 * CH);                                  // waves per row
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = item / wpr, piece = item - row * wpr;
  if (row >= M) return;
  const int col0 = piece * (512 * CH) + lane * 8;
  const bf16* xr = x + (size_t)row * D + col0;
  // Every load of the wave is requested before the reduction, the token -> row index first (it is the oldest load, so the
  // modulation loads that depend on it wait for it alone): one memory latency in the chain - two with a row map - not three.
  const size_t mrow = scale ? (size_t)(mod_row ? mod_row[row] : 0) * mod_stride : 0;
  bf16x8 v[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) v[i] = *(const bf16x8*)(xr + i * 512);
  const float ss0 = lane < NP ? sumsq[(size_t)row * ss_ld + lane] : 0.f;
  bf16x8 scv[CH], shv[CH];
  if (scale) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      scv[i] = *(const bf16x8*)(scale + mrow + col0 + i * 512);
      shv[i] = *(const bf16x8*)(shift + mrow + col0 + i * 512);
    }
  }
  float ss = ss0;
  for (int i = lane + 64; i < NP; i += 64) ss += sumsq[(size_t)row * ss_ld + i];
  const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
  bf16* yr = y + (size_t)row * D + col0;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    bf16x8 o;
    if (scale) {
      const bf16x8 sc = scv[i];
      const bf16x8 sh = shv[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float n = rbf((float)v[i][j] * rstd);
        const float one_p = ONE_PLUS ? (float)sc[j] : rbf(1.0f + (float)sc[j]);
        o[j] = (bf16)(rbf(n * one_p) + (float)sh[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)v[i][j] * rstd);
    }
    *(bf16x8*)(yr + i * 512) = o;
  }
}

// One normalisation pass, two modulations (ltxk_rmsnorm_modulate2: the cross-modal section of the AudioVideo block reads
// each residual stream once and modulates it for the a2v and for the v2a attention).  n = rbf(x * rstd) is formed once per
// element and feeds both outputs; every rounding point is that of the single-output kernels above, so y0 / y1 carry the bits
// of two launches of them.  SS: the row statistic is the carried partials and the row is cut into pieces as in
// norm_scale_kernel (every load - x, the partial, both scale / shift pairs - requested before the reduction); otherwise one
// wave holds the row and reduces it in norm_modulate_kernel's order (per lane: chunk by chunk, element by element).
template <bool ONE_PLUS>
__device__ __forceinline__ bf16x8 modulate8(const float (&n)[8], const bf16x8& sc, const bf16x8& sh) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float one_p = ONE_PLUS ? (float)sc[j] : rbf(1.0f + (float)sc[j]);
    o[j] = (bf16)(rbf(n[j] * one_p) + (float)sh[j]);
  }
  return o;
}

template <int CH, bool ONE_PLUS>
__global__ __launch_bounds__(256) void norm_scale2_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ y0, bf16* __restrict__ y1, int M, int D, float eps,
    const float* __restrict__ sumsq, int ss_ld, int NP, const bf16* __restrict__ scale0, const bf16* __restrict__ shift0,
    const bf16* __restrict__ scale1, const bf16* __restrict__ shift1, int mod_stride, const int32_t* __restrict__ mod_row) {
  const int lane = threadIdx.x & 63;
  const int wpr = D / (512 * CH);
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = item / wpr, piece = item - row * wpr;
  if (row >= M) return;
  const int col0 = piece * (512 * CH) + lane * 8;
  const size_t mrow = (size_t)(mod_row ? mod_row[row] : 0) * mod_stride + col0;
  const size_t xo = (size_t)row * D + col0;
  bf16x8 v[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) v[i] = *(const bf16x8*)(x + xo + i * 512);
  const float ss0 = lane < NP ? sumsq[(size_t)row * ss_ld + lane] : 0.f;
  bf16x8 sc0[CH], sh0[CH], sc1[CH], sh1[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    sc0[i] = *(const bf16x8*)(scale0 + mrow + i * 512);
    sh0[i] = *(const bf16x8*)(shift0 + mrow + i * 512);
    sc1[i] = *(const bf16x8*)(scale1 + mrow + i * 512);
    sh1[i] = *(const bf16x8*)(shift1 + mrow + i * 512);
  }
  float ss = ss0;
  for (int i = lane + 64; i < NP; i += 64) ss += sumsq[(size_t)row * ss_ld + i];
  const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    float n[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) n[j] = rbf((float)v[i][j] * rstd);
    *(bf16x8*)(y0 + xo + i * 512) = modulate8<ONE_PLUS>(n, sc0[i], sh0[i]);
    *(bf16x8*)(y1 + xo + i * 512) = modulate8<ONE_PLUS>(n, sc1[i], sh1[i]);
  }
}

__global__ __launch_bounds__(256) void norm_modulate2_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ y0, bf16* __restrict__ y1, int M, int D, float eps,
    const bf16* __restrict__ scale0, const bf16* __restrict__ shift0, const bf16* __restrict__ scale1,
    const bf16* __restrict__ shift1, int mod_stride, const int32_t* __restrict__ mod_row) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16* xr = x + (size_t)row * D;
  const int nch = D >> 9;
  bf16x8 v[MAX_CHUNKS];
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAX_CHUNKS; ++i) {
    if (i < nch) {
      v[i] = *(const bf16x8*)(xr + i * 512 + lane * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[i][j];
        sq += f * f;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
  const size_t mrow = (size_t)(mod_row ? mod_row[row] : 0) * mod_stride;
  const size_t yo = (size_t)row * D;
#pragma unroll
  for (int i = 0; i < MAX_CHUNKS; ++i) {
    if (i < nch) {
      const int col = i * 512 + lane * 8;
      const bf16x8 sc0 = *(const bf16x8*)(scale0 + mrow + col);
      const bf16x8 sh0 = *(const bf16x8*)(shift0 + mrow + col);
      const bf16x8 sc1 = *(const bf16x8*)(scale1 + mrow + col);
      const bf16x8 sh1 = *(const bf16x8*)(shift1 + mrow + col);
      float n[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) n[j] = rbf((float)v[i][j] * rstd);
      *(bf16x8*)(y0 + yo + col) = modulate8<false>(n, sc0, sh0);
      *(bf16x8*)(y1 + yo + col) = modulate8<false>(n, sc1, sh1);
    }
  }
}

// ---------------------------------------------------------------------------------------
// q/k RMSNorm (full inner dim, learned weight) + SPLIT RoPE, in place; values and rounding points: rows.h.
// One wave per (row, segment), the segment held in registers.  Lane map: a wave pass covers 8 heads; 8 lanes per head;
// lane holds x1 = [j0, j0+8) of the head's first half and x2 = the same offsets of the second half (the rotation
// partners), so every access is a 16-byte vector and each 8-lane group touches whole 128-byte lines.  Lanes past the
// last head idle, so any H <= 8 * MAXP is served: MAXP = 4 is the DiT's instance (ltxk_qknorm_rope), MAXP = 8 takes
// the text connector's H in 33..64 (ltxk_qknorm_rope_1d).  ROPE (= tables given) is a compile-time flag: the chain's
// rotation test folds away, which leaves each pass one straight run of {6 loads, counted waits, arithmetic, 2 stores}.
// ---------------------------------------------------------------------------------------
template <int MAXP, bool ROPE>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(
    bf16* __restrict__ buf, int ld, int M, int nseg, int D, const bf16* __restrict__ weight,
    const float* __restrict__ cosb, const float* __restrict__ sinb, int T, int H, float eps) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (item >= M * nseg) return;
  const int row = item / nseg, sgi = item - row * nseg;
  const int t = row % T;
  const int npass = (H + 7) >> 3;    // 8 heads per pass, dh = 128
  const int hl = lane >> 3;          // head within pass
  const int j0 = (lane & 7) * 8;     // offset within the 64-wide half
  bf16* xr = buf + (size_t)row * ld + (size_t)sgi * D;
  const bf16* wr = weight + (size_t)sgi * D;
  bf16x8 a[MAXP], b[MAXP];
  float sq = 0.f;
#pragma unroll
  for (int ps = 0; ps < MAXP; ++ps)
    if (ps < npass && ps * 8 + hl < H) {
      const int base = (ps * 8 + hl) * 128 + j0;
      a[ps] = *(const bf16x8*)(xr + base);
      b[ps] = *(const bf16x8*)(xr + base + 64);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float fa = (float)a[ps][j], fb = (float)b[ps][j];
        sq += fa * fa + fb * fb;
      }
    }
  const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int ps = 0; ps < MAXP; ++ps)
    if (ps < npass && ps * 8 + hl < H) {
      const int base = (ps * 8 + hl) * 128 + j0;
      const bf16x8 wa = *(const bf16x8*)(wr + base);
      const bf16x8 wb = *(const bf16x8*)(wr + base + 64);
      RopeTab tab = {};
      if constexpr (ROPE) tab = rope_load(cosb, sinb, ((size_t)(ps * 8 + hl) * T + t) * 64 + j0);
      bf16x8 oa, ob;
      norm_rope(a[ps], b[ps], rstd, wa, wb, ROPE, tab, oa, ob);
      *(bf16x8*)(xr + base) = oa;
      *(bf16x8*)(xr + base + 64) = ob;
    }
}

// The same with the row's sum of squares precomputed (GEMM `sumsq` output, NP partials per segment): one wave per
// (row, segment, pass of 8 heads) - 4x the waves of the kernel above at H=32, each 2 + 2 row loads deep.
__global__ __launch_bounds__(256) void qknorm_rope_ss_kernel(
    bf16* __restrict__ buf, int ld, int M, int nseg, int D, const bf16* __restrict__ weight,
    const float* __restrict__ cosb, const float* __restrict__ sinb, int T, int H, float eps,
    const float* __restrict__ sumsq, int ss_ld, int NP, size_t buf_gs, size_t w_gs, size_t ss_gs) {
  // blockIdx.y = group (ltxk_qknorm_grouped_ss: the text k of every block in one launch); a single call has one group
  buf += blockIdx.y * buf_gs;
  weight += blockIdx.y * w_gs;
  sumsq += blockIdx.y * ss_gs;
  const int lane = threadIdx.x & 63;
  const int npass = (H + 7) >> 3;
  const int item = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (item >= M * nseg * npass) return;
  const int ps = item % npass;
  const int rs = item / npass;
  const int row = rs / nseg, sgi = rs - row * nseg;
  const int t = row % T;
  const int hl = lane >> 3, j0 = (lane & 7) * 8;
  const int head = ps * 8 + hl;
  bf16* xr = buf + (size_t)row * ld + (size_t)sgi * D;
  const bf16* wr = weight + (size_t)sgi * D;
  const bool act = head < H;
  const int base = (act ? head : 0) * 128 + j0;
  bf16x8 a, b;
  if (act) {
    a = *(const bf16x8*)(xr + base);
    b = *(const bf16x8*)(xr + base + 64);
  }
  float ss = 0.f;
  for (int i = lane; i < NP; i += 64) ss += sumsq[(size_t)row * ss_ld + sgi * NP + i];
  // weights and the rotation table are requested before the reduction (they do not depend on it)
  bf16x8 wa, wb;
  RopeTab tab;
  if (act) {
    wa = *(const bf16x8*)(wr + base);
    wb = *(const bf16x8*)(wr + base + 64);
    if (cosb) tab = rope_load(cosb, sinb, ((size_t)head * T + t) * 64 + j0);
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
  if (!act) return;
  bf16x8 oa, ob;
  norm_rope(a, b, rstd, wa, wb, cosb != nullptr, tab, oa, ob);
  *(bf16x8*)(xr + base) = oa;
  *(bf16x8*)(xr + base + 64) = ob;
}

// The same chain at head dim 64 (the audio transformer: 32 heads x 64): a head's halves are 32 wide, the rotation partner of
// channel j is j + 32 and the tables are (H, T, 32).  One wave per (row, segment); 4 lanes per head, 16 heads per pass, two
// passes: H <= 32.  The row statistic is the precomputed partials (`sumsq`, D/64 = H per segment) where given, else the
// wave reduces the row it holds.
template <bool ROPE>
__global__ __launch_bounds__(256) void qknorm_rope_dh64_kernel(
    bf16* __restrict__ buf, int ld, int M, int nseg, int D, const bf16* __restrict__ weight,
    const float* __restrict__ cosb, const float* __restrict__ sinb, int T, int H, float eps,
    const float* __restrict__ sumsq, int ss_ld) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (item >= M * nseg) return;
  const int row = item / nseg, sgi = item - row * nseg;
  const int t = row % T;
  const int hl = lane >> 2;          // head within pass
  const int j0 = (lane & 3) * 8;     // offset within the 32-wide half
  bf16* xr = buf + (size_t)row * ld + (size_t)sgi * D;
  const bf16* wr = weight + (size_t)sgi * D;
  bf16x8 a[2], b[2];
  float sq = 0.f;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps)
    if (ps * 16 + hl < H) {
      const int base = (ps * 16 + hl) * 64 + j0;
      a[ps] = *(const bf16x8*)(xr + base);
      b[ps] = *(const bf16x8*)(xr + base + 32);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float fa = (float)a[ps][j], fb = (float)b[ps][j];
        sq += fa * fa + fb * fb;
      }
    }
  if (sumsq) sq = lane < H ? sumsq[(size_t)row * ss_ld + sgi * H + lane] : 0.f;
  const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int ps = 0; ps < 2; ++ps)
    if (ps * 16 + hl < H) {
      const int base = (ps * 16 + hl) * 64 + j0;
      const bf16x8 wa = *(const bf16x8*)(wr + base);
      const bf16x8 wb = *(const bf16x8*)(wr + base + 32);
      RopeTab tab = {};
      if constexpr (ROPE) tab = rope_load(cosb, sinb, ((size_t)(ps * 16 + hl) * T + t) * 32 + j0);
      bf16x8 oa, ob;
      norm_rope(a[ps], b[ps], rstd, wa, wb, ROPE, tab, oa, ob);
      *(bf16x8*)(xr + base) = oa;
      *(bf16x8*)(xr + base + 32) = ob;
    }
}

// ---------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------
__global__ void timestep_embed_kernel(const bf16* __restrict__ t, bf16* __restrict__ out, int U, int dim, float mult) {
  const int half = dim >> 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= U * half) return;
  const int u = idx / half, i = idx - u * half;
  const float freq = expf(-9.210340371976184f * (float)i / (float)half);  // -ln(1e4)
  const float arg = rbf((float)t[u] * mult) * freq;   // timestep*1000 stays bf16 (ltx.py:68)
  out[(size_t)u * dim + i] = (bf16)cosf(arg);          // flip_sin_to_cos: cos first
  out[(size_t)u * dim + half + i] = (bf16)sinf(arg);
}

// RoPE table (SPLIT layout): rope.py:419-529.  f < pad: cos=1,sin=0 (front pad, rope.py:504-509);
// else idx=(f-pad)/3, dim=(f-pad)%3; angle = ((mid/max_pos[dim])*2-1) * freq[idx].
__global__ void rope_table_kernel(const float* __restrict__ pos, const float* __restrict__ freq,
                                  float* __restrict__ cosb, float* __restrict__ sinb, int T, int H,
                                  int half_dim, int pad, float mp0, float mp1, float mp2) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= T * half_dim) return;
  const int t = idx / half_dim, f = idx - t * half_dim;
  float c = 1.f, s = 0.f;
  if (f >= pad) {
    const int fi = (f - pad) / 3, d = (f - pad) - fi * 3;
    const float st = pos[((size_t)d * T + t) * 2], en = pos[((size_t)d * T + t) * 2 + 1];
    const float mid = (st + en) / 2.0f;
    const float mp = d == 0 ? mp0 : (d == 1 ? mp1 : mp2);
    const float frac = __fdiv_rn(mid, mp);
    const float ang = (frac * 2.0f - 1.0f) * freq[fi];
    c = cosf(ang);
    s = sinf(ang);
  }
  const int per_head = half_dim / H;
  const int h = f / per_head, j = f - h * per_head;
  const size_t o = ((size_t)h * T + t) * per_head + j;
  cosb[o] = c;
  sinb[o] = s;
}

__global__ void ada_combine_kernel(const bf16* __restrict__ table, const bf16* __restrict__ ada,
                                   bf16* __restrict__ out, int L, int U, int K, int D, unsigned one_plus_mask) {
  // out[l,u,k,d] = bf16(table[l,k,d] + ada[u,k,d]) (+1, rounded again, for the k in one_plus_mask); 8 elements per thread
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t kd8 = (size_t)K * D / 8;
  const size_t total = (size_t)L * U * kd8;
  if (idx >= total) return;
  const size_t e = idx % kd8;
  const size_t lu = idx / kd8;
  const int u = (int)(lu % U), l = (int)(lu / U);
  const bf16x8 a = *(const bf16x8*)(table + ((size_t)l * kd8 + e) * 8);
  const bf16x8 b = *(const bf16x8*)(ada + ((size_t)u * kd8 + e) * 8);
  const bool op = (one_plus_mask >> (unsigned)((e * 8) / D)) & 1u;
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = rbf((float)a[j] + (float)b[j]);
    o[j] = (bf16)(op ? 1.0f + v : v);
  }
  *(bf16x8*)(out + idx * 8) = o;
}

__global__ void silu_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int64_t n8) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n8) return;
  const bf16x8 v = *(const bf16x8*)(x + idx * 8);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = (float)v[j];
    o[j] = (bf16)silu_div(f);
  }
  *(bf16x8*)(y + idx * 8) = o;
}

// (B,C,S) -> (rep*B,S,C): thread = (b, s, 8-channel group); lanes run along s (coalesced reads).
__global__ void latent_to_tokens_kernel(const bf16* __restrict__ lat, bf16* __restrict__ tok,
                                        int B, int C, int S, int rep) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int cg = blockIdx.y, b = blockIdx.z;
  if (s >= S) return;
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = lat[((size_t)b * C + cg * 8 + j) * S + s];
  for (int r = 0; r < rep; ++r)
    *(bf16x8*)(tok + (((size_t)(r * B + b)) * S + s) * C + cg * 8) = v;
}

// One wave.  Row *step of the per-step scalar tables -> the buffers the step's kernels read; *step += 1.
__global__ void step_scalars_kernel(const bf16* __restrict__ ts_all, const float* __restrict__ sig_all,
                                    int32_t* __restrict__ step, bf16* __restrict__ ts, float* __restrict__ sig,
                                    int U, int n_steps) {
  int s = *step;
  s = s < n_steps ? s : n_steps - 1;
  __syncthreads();
  for (int i = threadIdx.x; i < U; i += blockDim.x) ts[i] = ts_all[(size_t)s * U + i];
  if (threadIdx.x < 2) sig[threadIdx.x] = sig_all[2 * s + threadIdx.x];
  if (threadIdx.x == 0) *step = s + 1;
}

// Value passthrough of a skipped self-attention (STG): out[(b*T+t)*ldo + c] = vt[(b*D+c)*ldvt + t] for every batch row b
// whose bit is set in row_mask - the V^T buffer the q|k|v GEMM wrote, transposed back to the token-major rows the
// out-projection reads.  A 64(t) x 64(c) tile per workgroup through LDS: 16-byte global loads along t (8 tokens of one
// channel), 16-byte global stores along c (8 channels of one token).  The LDS row holds 66 bf16 (33 dwords) so that a
// wave's transposed reads - 8 channel groups x 8 tokens, one bf16 each - fall into distinct banks.
constexpr int VP_TILE = 64, VP_LD = VP_TILE + 2;

__global__ __launch_bounds__(256) void value_passthrough_kernel(const bf16* __restrict__ vt, int ldvt, bf16* __restrict__ out,
                                                                int ldo, int D, int T, uint64_t row_mask) {
  const int b = blockIdx.z;
  if (!((row_mask >> b) & 1ull)) return;
  __shared__ uint32_t tile[VP_TILE * VP_LD / 2];
  const int t0 = blockIdx.x * VP_TILE, c0 = blockIdx.y * VP_TILE;
  const int tid = threadIdx.x;
  const bf16* src = vt + ((size_t)b * D + c0) * ldvt + t0;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int chunk = tid + it * 256;          // 64 channels x 8 chunks of 8 tokens
    const int c = chunk >> 3, tc = (chunk & 7) * 8;
    // t0 + tc < T <= ldvt and both multiples of 8: the 16 bytes lie inside the padded row
    if (t0 + tc < T) {
      const uint4 v = *(const uint4*)(src + (size_t)c * ldvt + tc);
      uint32_t* d = tile + (c * VP_LD + tc) / 2;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  }
  __syncthreads();
  const unsigned short* t16 = (const unsigned short*)tile;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int item = tid + it * 256;           // 64 tokens x 8 channel groups; a wave covers 8 tokens x all 8 groups
    const int cg = item & 7, t = item >> 3;
    if (t0 + t >= T) continue;
    unsigned short h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = t16[(cg * 8 + j) * VP_LD + t];
    uint4 o;
    o.x = h[0] | ((uint32_t)h[1] << 16); o.y = h[2] | ((uint32_t)h[3] << 16);
    o.z = h[4] | ((uint32_t)h[5] << 16); o.w = h[6] | ((uint32_t)h[7] << 16);
    *(uint4*)(out + ((size_t)b * T + t0 + t) * ldo + c0 + cg * 8) = o;
  }
}

// ---------------------------------------------------------------------------------------
// Row quantiser of the fp8 x fp8 GEMMs (ltxk_quant_rows_fp8): bf16 rows -> OCP e4m3fn bytes + one fp32 scale per row.
//   amax = max |x| ; scale = max(amax, 2^-64) / 448 ; q = e4m3_rne_sat(fp32(x) / scale)     (IEEE fp32 divisions)
// One workgroup per row: every thread loads its 16-byte chunks (chunk c of the row to thread c % 256: whole 4-KiB lines per
// instruction), the row maximum goes through a wave butterfly (v_permlane32/16_swap, then DPP row rotates) and four LDS words,
// and the second sweep runs over the registers (CH chunks per thread, K <= 2048 * CH); CH = 0 re-reads the row instead.
// ---------------------------------------------------------------------------------------
template <int OFF>
__device__ __forceinline__ float lane_butterfly_max(float v) {
  if constexpr (OFF == 32) return lane_xor32_max(v);
  else if constexpr (OFF == 16) return lane_xor16_max(v);
  else {
    const int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + OFF, 0xf, 0xf, false);      // row_ror:OFF
    return vmax(v, __int_as_float(r));
  }
}

__device__ __forceinline__ float absmax8(const bf16x8& v, float m) {
#pragma unroll
  for (int j = 0; j < 8; ++j) m = vmax(m, __builtin_fabsf((float)v[j]));
  return m;
}

__device__ __forceinline__ u32x2_t quant8(const bf16x8& v, float scale) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = __builtin_amdgcn_fmed3f((float)v[j] / scale, -448.f, 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return u32x2_t{(unsigned)lo, (unsigned)hi};
}

template <int CH>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const bf16* __restrict__ x, int lda, uint8_t* __restrict__ q, int ldq,
                                                             float* __restrict__ a_scale, int K) {
  __shared__ float wmax[4];
  const int tid = threadIdx.x, row = blockIdx.x;
  const bf16* xr = x + (size_t)row * lda;
  uint8_t* qr = q + (size_t)row * ldq;
  const int nch = K >> 3;
  bf16x8 v[CH > 0 ? CH : 1];
  float amax = 0.f;
  if constexpr (CH > 0) {
#pragma unroll
    for (int i = 0; i < CH; ++i)
      if (i * 256 + tid < nch) v[i] = *(const bf16x8*)(xr + (size_t)(i * 256 + tid) * 8);
#pragma unroll
    for (int i = 0; i < CH; ++i)
      if (i * 256 + tid < nch) amax = absmax8(v[i], amax);
  } else {
    for (int c = tid; c < nch; c += 256) amax = absmax8(*(const bf16x8*)(xr + (size_t)c * 8), amax);
  }
  amax = lane_butterfly_max<32>(amax);
  amax = lane_butterfly_max<16>(amax);
  amax = lane_butterfly_max<8>(amax);
  amax = lane_butterfly_max<4>(amax);
  amax = lane_butterfly_max<2>(amax);
  amax = lane_butterfly_max<1>(amax);
  if ((tid & 63) == 0) wmax[tid >> 6] = amax;
  __syncthreads();
  amax = vmax(vmax(wmax[0], wmax[1]), vmax(wmax[2], wmax[3]));
  const float scale = vmax(amax, 0x1p-64f) / 448.0f;
  if (tid == 0) a_scale[row] = scale;
  if constexpr (CH > 0) {
#pragma unroll
    for (int i = 0; i < CH; ++i)
      if (i * 256 + tid < nch) *(u32x2_t*)(qr + (size_t)(i * 256 + tid) * 8) = quant8(v[i], scale);
  } else {
    for (int c = tid; c < nch; c += 256) *(u32x2_t*)(qr + (size_t)c * 8) = quant8(*(const bf16x8*)(xr + (size_t)c * 8), scale);
  }
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_quant_rows_fp8(const void* x, int32_t lda, void* q, int32_t ldq, float* a_scale, int32_t M, int32_t K,
                                   void* stream) {
  const char* name = "ltxk_quant_rows_fp8";
  LTXK_CHECK_ARG(x && q && a_scale && M > 0 && K > 0, "%s: null/empty input", name);
  LTXK_CHECK_ARG(K % 8 == 0 && lda >= K && lda % 8 == 0 && ldq >= K && ldq % 8 == 0, "%s: K=%d, lda=%d, ldq=%d must be multiples of 8, strides >= K", name, K, lda, ldq);
  LTXK_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 7) == 0 && ((uintptr_t)a_scale & 3) == 0,
                 "%s: x must be 16-byte, q 8-byte, a_scale 4-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const bf16* xb = (const bf16*)x;
  uint8_t* qb = (uint8_t*)q;
  if (K <= 2048) hipLaunchKernelGGL(quant_rows_fp8_kernel<1>, dim3(M), dim3(256), 0, st, xb, (int)lda, qb, (int)ldq, a_scale, (int)K);
  else if (K <= 4096) hipLaunchKernelGGL(quant_rows_fp8_kernel<2>, dim3(M), dim3(256), 0, st, xb, (int)lda, qb, (int)ldq, a_scale, (int)K);
  else if (K <= 8192) hipLaunchKernelGGL(quant_rows_fp8_kernel<4>, dim3(M), dim3(256), 0, st, xb, (int)lda, qb, (int)ldq, a_scale, (int)K);
  else if (K <= 16384) hipLaunchKernelGGL(quant_rows_fp8_kernel<8>, dim3(M), dim3(256), 0, st, xb, (int)lda, qb, (int)ldq, a_scale, (int)K);
  else hipLaunchKernelGGL(quant_rows_fp8_kernel<0>, dim3(M), dim3(256), 0, st, xb, (int)lda, qb, (int)ldq, a_scale, (int)K);
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}

extern "C" int ltxk_step_scalars(const void* ts_all, const float* sig_all, int32_t* step, void* ts, float* sig,
                                 int32_t U, int32_t n_steps, void* stream) {
  LTXK_CHECK_ARG(ts_all && sig_all && step && ts && sig && U > 0 && n_steps > 0, "ltxk_step_scalars: bad arguments");
  hipLaunchKernelGGL(step_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const bf16*)ts_all, sig_all, step,
                     (bf16*)ts, sig, U, n_steps);
  LTXK_CHECK_LAUNCH("ltxk_step_scalars");
  return LTXK_OK;
}

template <int CH>
static void norm_scale_launch(bool one_plus, dim3 grid, hipStream_t st, const bf16* x, bf16* y, int M, int D, float eps,
                              const float* ss, int ss_ld, int np, const bf16* sc, const bf16* sh, int ms, const int32_t* mr) {
  if (one_plus) hipLaunchKernelGGL((norm_scale_kernel<CH, true>), grid, dim3(256), 0, st, x, y, M, D, eps, ss, ss_ld, np, sc, sh, ms, mr);
  else hipLaunchKernelGGL((norm_scale_kernel<CH, false>), grid, dim3(256), 0, st, x, y, M, D, eps, ss, ss_ld, np, sc, sh, ms, mr);
}

extern "C" int ltxk_rmsnorm_modulate_ss(const void* x, void* y, int32_t M, int32_t D, float eps, const float* sumsq,
                                        int32_t sumsq_ld, int32_t sumsq_n, const void* scale, const void* shift,
                                        int32_t mod_stride, const int32_t* mod_row, int32_t flags, void* stream) {
  const char* name = "ltxk_rmsnorm_modulate_ss";
  LTXK_CHECK_ARG(x && y && sumsq && M > 0, "%s: null/empty input", name);
  LTXK_CHECK_ARG(D % 512 == 0 && D > 0, "%s: D=%d must be a multiple of 512", name, D);
  LTXK_CHECK_ARG(sumsq_n > 0 && sumsq_ld >= sumsq_n, "%s: bad sumsq_n/sumsq_ld", name);
  LTXK_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift must both be set or both NULL", name);
  LTXK_CHECK_ARG(!scale || mod_stride % 8 == 0, "%s: mod_stride must be a multiple of 8", name);
  // 16-byte chunks per lane: 2 (rows cut into 1024-element pieces) when D allows, else 1
  const int ch_env = LTXK_AB_INT("LTXK_NORM_CH", 0);
  int ch = (D % 1024 == 0) ? 2 : 1;
  if ((ch_env == 1 || ch_env == 2 || ch_env == 4 || ch_env == 8) && D % (512 * ch_env) == 0) ch = ch_env;
  const int wpr = D / (512 * ch);
  const dim3 grid((unsigned)(((long long)M * wpr + 3) / 4));
  const bool op = (flags & LTXK_NORM_SCALE_IS_ONE_PLUS) != 0;
  hipStream_t st = (hipStream_t)stream;
  switch (ch) {
    case 1: norm_scale_launch<1>(op, grid, st, (const bf16*)x, (bf16*)y, M, D, eps, sumsq, sumsq_ld, sumsq_n, (const bf16*)scale, (const bf16*)shift, mod_stride, mod_row); break;
    case 2: norm_scale_launch<2>(op, grid, st, (const bf16*)x, (bf16*)y, M, D, eps, sumsq, sumsq_ld, sumsq_n, (const bf16*)scale, (const bf16*)shift, mod_stride, mod_row); break;
    case 4: norm_scale_launch<4>(op, grid, st, (const bf16*)x, (bf16*)y, M, D, eps, sumsq, sumsq_ld, sumsq_n, (const bf16*)scale, (const bf16*)shift, mod_stride, mod_row); break;
    default: norm_scale_launch<8>(op, grid, st, (const bf16*)x, (bf16*)y, M, D, eps, sumsq, sumsq_ld, sumsq_n, (const bf16*)scale, (const bf16*)shift, mod_stride, mod_row); break;
  }
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}

template <int CH>
static void norm_scale2_launch(bool one_plus, dim3 grid, hipStream_t st, const bf16* x, bf16* y0, bf16* y1, int M, int D, float eps,
                               const float* ss, int ss_ld, int np, const bf16* sc0, const bf16* sh0, const bf16* sc1, const bf16* sh1,
                               int ms, const int32_t* mr) {
  if (one_plus) hipLaunchKernelGGL((norm_scale2_kernel<CH, true>), grid, dim3(256), 0, st, x, y0, y1, M, D, eps, ss, ss_ld, np, sc0, sh0, sc1, sh1, ms, mr);
  else hipLaunchKernelGGL((norm_scale2_kernel<CH, false>), grid, dim3(256), 0, st, x, y0, y1, M, D, eps, ss, ss_ld, np, sc0, sh0, sc1, sh1, ms, mr);
}

extern "C" int ltxk_rmsnorm_modulate2(const void* x, void* y0, void* y1, int32_t M, int32_t D, float eps, const float* sumsq,
                                      int32_t sumsq_ld, int32_t sumsq_n, const void* scale0, const void* shift0,
                                      const void* scale1, const void* shift1, int32_t mod_stride, const int32_t* mod_row,
                                      int32_t flags, void* stream) {
  const char* name = "ltxk_rmsnorm_modulate2";
  LTXK_CHECK_ARG(x && y0 && y1 && y0 != y1 && M > 0, "%s: null/empty input, or one buffer for both outputs", name);
  LTXK_CHECK_ARG(D % 512 == 0 && D > 0 && D <= 512 * MAX_CHUNKS, "%s: D=%d must be a multiple of 512, <= %d", name, D, 512 * MAX_CHUNKS);
  LTXK_CHECK_ARG(scale0 && shift0 && scale1 && shift1, "%s: both (scale, shift) pairs are required", name);
  LTXK_CHECK_ARG(mod_stride >= 0 && mod_stride % 8 == 0, "%s: mod_stride must be a multiple of 8", name);
  LTXK_CHECK_ARG((((uintptr_t)x | (uintptr_t)y0 | (uintptr_t)y1 | (uintptr_t)scale0 | (uintptr_t)shift0 | (uintptr_t)scale1 | (uintptr_t)shift1) & 15) == 0,
                 "%s: x, the outputs and the modulation tables must be 16-byte aligned", name);
  LTXK_CHECK_ARG(!sumsq || (sumsq_n > 0 && sumsq_ld >= sumsq_n), "%s: bad sumsq_n/sumsq_ld", name);
  const bool op = (flags & LTXK_NORM_SCALE_IS_ONE_PLUS) != 0;
  LTXK_CHECK_ARG(sumsq || !op, "%s: LTXK_NORM_SCALE_IS_ONE_PLUS needs sumsq", name);
  hipStream_t st = (hipStream_t)stream;
  const bf16 *xb = (const bf16*)x, *sc0 = (const bf16*)scale0, *sh0 = (const bf16*)shift0, *sc1 = (const bf16*)scale1, *sh1 = (const bf16*)shift1;
  if (sumsq) {
    // rows cut into 1024-element pieces (two 16-byte chunks per lane) when D allows, else 512: as ltxk_rmsnorm_modulate_ss
    const int ch = (D % 1024 == 0) ? 2 : 1;
    const dim3 grid((unsigned)(((long long)M * (D / (512 * ch)) + 3) / 4));
    if (ch == 2) norm_scale2_launch<2>(op, grid, st, xb, (bf16*)y0, (bf16*)y1, M, D, eps, sumsq, sumsq_ld, sumsq_n, sc0, sh0, sc1, sh1, mod_stride, mod_row);
    else norm_scale2_launch<1>(op, grid, st, xb, (bf16*)y0, (bf16*)y1, M, D, eps, sumsq, sumsq_ld, sumsq_n, sc0, sh0, sc1, sh1, mod_stride, mod_row);
  } else {
    hipLaunchKernelGGL(norm_modulate2_kernel, dim3((M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(256), 0, st, xb, (bf16*)y0, (bf16*)y1,
                       M, D, eps, sc0, sh0, sc1, sh1, mod_stride, mod_row);
  }
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}

static int norm_modulate_launch(bool ln, const void* x, void* y, int32_t M, int32_t D, float eps,
                                const void* scale, const void* shift, int32_t mod_stride,
                                const int32_t* mod_row, void* stream, const char* name) {
  LTXK_CHECK_ARG(x && y && M > 0, "%s: null/empty input", name);
  LTXK_CHECK_ARG(D % 512 == 0 && D <= 512 * MAX_CHUNKS, "%s: D=%d must be a multiple of 512, <= %d", name, D, 512 * MAX_CHUNKS);
  LTXK_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift must both be set or both NULL", name);
  LTXK_CHECK_ARG(!scale || mod_stride % 8 == 0, "%s: mod_stride must be a multiple of 8", name);
  const dim3 grid((M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (ln)
    hipLaunchKernelGGL(norm_modulate_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)y, M, D, eps,
                       (const bf16*)scale, (const bf16*)shift, mod_stride, mod_row);
  else
    hipLaunchKernelGGL(norm_modulate_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)y, M, D, eps,
                       (const bf16*)scale, (const bf16*)shift, mod_stride, mod_row);
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}

extern "C" int ltxk_rmsnorm_modulate(const void* x, void* y, int32_t M, int32_t D, float eps,
                                     const void* scale, const void* shift, int32_t mod_stride,
                                     const int32_t* mod_row, void* stream) {
  return norm_modulate_launch(false, x, y, M, D, eps, scale, shift, mod_stride, mod_row, stream, "ltxk_rmsnorm_modulate");
}

extern "C" int ltxk_layernorm_modulate(const void* x, void* y, int32_t M, int32_t D, float eps,
                                       const void* scale, const void* shift, int32_t mod_stride,
                                       const int32_t* mod_row, void* stream) {
  return norm_modulate_launch(true, x, y, M, D, eps, scale, shift, mod_stride, mod_row, stream, "ltxk_layernorm_modulate");
}

extern "C" int ltxk_qknorm_rope_ss(void* buf, int32_t ld, int32_t M, int32_t nseg, int32_t D,
                                   const void* weight, const float* cos, const float* sin,
                                   int32_t T, int32_t H, float eps, const float* sumsq, int32_t sumsq_ld, void* stream) {
  LTXK_CHECK_ARG(buf && weight && sumsq && M > 0 && nseg > 0, "ltxk_qknorm_rope_ss: null/empty input");
  LTXK_CHECK_ARG(D == H * 128 && H % 4 == 0, "ltxk_qknorm_rope_ss: need D == H*128, H %% 4 == 0 (D=%d H=%d)", D, H);
  LTXK_CHECK_ARG(ld >= nseg * D && ld % 8 == 0 && ((uintptr_t)buf & 15) == 0, "ltxk_qknorm_rope_ss: ld=%d must be >= nseg*D and a multiple of 8, buf 16-byte aligned", ld);
  LTXK_CHECK_ARG((cos == nullptr) == (sin == nullptr), "ltxk_qknorm_rope_ss: cos and sin must both be set or both NULL");
  LTXK_CHECK_ARG(T > 0 && sumsq_ld >= nseg * (D / 64), "ltxk_qknorm_rope_ss: T must be > 0, sumsq_ld >= nseg*D/64");
  const int npass = (H + 7) / 8;
  const long long items = (long long)M * nseg * npass;
  hipLaunchKernelGGL(qknorm_rope_ss_kernel, dim3((unsigned)((items + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream,
                     (bf16*)buf, ld, M, nseg, D, (const bf16*)weight, cos, sin, T, H, eps, sumsq, sumsq_ld, D / 64, (size_t)0, (size_t)0, (size_t)0);
  LTXK_CHECK_LAUNCH("ltxk_qknorm_rope_ss");
  return LTXK_OK;
}

extern "C" int ltxk_qknorm_grouped_ss(void* buf, int64_t buf_gstride, int32_t ld, int32_t G, int32_t M, int32_t D,
                                      const void* weight, int32_t H, float eps, const float* sumsq, int64_t sumsq_gstride,
                                      int32_t sumsq_ld, void* stream) {
  LTXK_CHECK_ARG(buf && weight && sumsq && M > 0 && G > 0 && G <= 65535, "ltxk_qknorm_grouped_ss: null/empty input (G=%d M=%d)", G, M);
  LTXK_CHECK_ARG(D == H * 128 && H % 4 == 0, "ltxk_qknorm_grouped_ss: need D == H*128, H %% 4 == 0 (D=%d H=%d)", D, H);
  LTXK_CHECK_ARG(ld >= D && ld % 8 == 0 && ((uintptr_t)buf & 15) == 0 && buf_gstride % 8 == 0, "ltxk_qknorm_grouped_ss: ld=%d must be >= D and a multiple of 8, buf 16-byte aligned, group stride a multiple of 8", ld);
  LTXK_CHECK_ARG(sumsq_ld >= D / 64, "ltxk_qknorm_grouped_ss: sumsq_ld >= D/64");
  LTXK_CHECK_ARG(G == 1 || (buf_gstride >= (int64_t)(M - 1) * ld + D && sumsq_gstride >= (int64_t)(M - 1) * sumsq_ld + D / 64),
                 "ltxk_qknorm_grouped_ss: a group stride is smaller than one group");
  const int npass = (H + 7) / 8;
  const long long items = (long long)M * npass;
  hipLaunchKernelGGL(qknorm_rope_ss_kernel, dim3((unsigned)((items + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), (unsigned)G), dim3(256), 0,
                     (hipStream_t)stream, (bf16*)buf, ld, M, 1, D, (const bf16*)weight, (const float*)nullptr, (const float*)nullptr, 1, H, eps,
                     sumsq, sumsq_ld, D / 64, (size_t)buf_gstride, (size_t)D, (size_t)sumsq_gstride);
  LTXK_CHECK_LAUNCH("ltxk_qknorm_grouped_ss");
  return LTXK_OK;
}

extern "C" int ltxk_qknorm_rope(void* buf, int32_t ld, int32_t M, int32_t nseg, int32_t D,
                                const void* weight, const float* cos, const float* sin,
                                int32_t T, int32_t H, float eps, void* stream) {
  LTXK_CHECK_ARG(buf && weight && M > 0 && nseg > 0, "ltxk_qknorm_rope: null/empty input");
  LTXK_CHECK_ARG(D == H * 128 && H % 4 == 0 && H <= 32, "ltxk_qknorm_rope: need D == H*128, H %% 4 == 0, H <= 32 (D=%d H=%d)", D, H);
  LTXK_CHECK_ARG(ld >= nseg * D && ld % 8 == 0 && ((uintptr_t)buf & 15) == 0, "ltxk_qknorm_rope: ld=%d must be >= nseg*D and a multiple of 8, buf 16-byte aligned", ld);
  LTXK_CHECK_ARG((cos == nullptr) == (sin == nullptr), "ltxk_qknorm_rope: cos and sin must both be set or both NULL");
  LTXK_CHECK_ARG(T > 0, "ltxk_qknorm_rope: T must be > 0");
  const dim3 grid((M * nseg + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (cos)
    hipLaunchKernelGGL((qknorm_rope_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, nseg, D, (const bf16*)weight, cos, sin, T, H, eps);
  else
    hipLaunchKernelGGL((qknorm_rope_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, nseg, D, (const bf16*)weight, cos, sin, T, H, eps);
  LTXK_CHECK_LAUNCH("ltxk_qknorm_rope");
  return LTXK_OK;
}

extern "C" int ltxk_qknorm_rope_dh64(void* buf, int32_t ld, int32_t M, int32_t nseg, int32_t D,
                                     const void* weight, const float* cos, const float* sin,
                                     int32_t T, int32_t H, float eps, const float* sumsq, int32_t sumsq_ld, void* stream) {
  LTXK_CHECK_ARG(buf && weight && M > 0 && nseg > 0, "ltxk_qknorm_rope_dh64: null/empty input");
  LTXK_CHECK_ARG(H >= 1 && H <= 32 && D == H * 64, "ltxk_qknorm_rope_dh64: need D == H*64, 1 <= H <= 32 (D=%d H=%d)", D, H);
  LTXK_CHECK_ARG((int64_t)nseg * D <= ld && ld % 8 == 0 && (((uintptr_t)buf | (uintptr_t)weight) & 15) == 0,
                 "ltxk_qknorm_rope_dh64: ld=%d must be >= nseg*D and a multiple of 8, buf and weight 16-byte aligned", ld);
  LTXK_CHECK_ARG((cos == nullptr) == (sin == nullptr) && (((uintptr_t)cos | (uintptr_t)sin) & 15) == 0,
                 "ltxk_qknorm_rope_dh64: cos and sin must both be set (16-byte aligned) or both NULL");
  LTXK_CHECK_ARG(T > 0 && (sumsq == nullptr || sumsq_ld >= nseg * H), "ltxk_qknorm_rope_dh64: T must be > 0, sumsq_ld >= nseg*D/64");
  LTXK_CHECK_ARG((int64_t)M * nseg <= (int64_t)INT32_MAX, "ltxk_qknorm_rope_dh64: too many rows");
  const dim3 grid((unsigned)(((int64_t)M * nseg + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
  if (cos)
    hipLaunchKernelGGL((qknorm_rope_dh64_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, nseg, D, (const bf16*)weight, cos, sin, T, H, eps, sumsq, sumsq_ld);
  else
    hipLaunchKernelGGL((qknorm_rope_dh64_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, nseg, D, (const bf16*)weight, cos, sin, T, H, eps, sumsq, sumsq_ld);
  LTXK_CHECK_LAUNCH("ltxk_qknorm_rope_dh64");
  return LTXK_OK;
}

// the text connector's entry to the same kernel: q|k of one row side by side (nseg = 2), any 1 <= H <= 64, tables required
extern "C" int ltxk_qknorm_rope_1d(void* buf, int32_t ld, int32_t M, int32_t D, const void* weight, const float* cos,
                                   const float* sin, int32_t T, int32_t H, float eps, void* stream) {
  LTXK_CHECK_ARG(buf && weight && cos && sin && M > 0 && T > 0, "ltxk_qknorm_rope_1d: bad arguments");
  LTXK_CHECK_ARG(H >= 1 && H <= 64 && D == 128 * H, "ltxk_qknorm_rope_1d: D=%d must be 128*H, 1 <= H=%d <= %d", D, H, 64);
  LTXK_CHECK_ARG(ld >= 2 * D && ld % 8 == 0 && ((uintptr_t)buf & 15) == 0 && ((uintptr_t)weight & 15) == 0 && ((uintptr_t)cos & 15) == 0 &&
                     ((uintptr_t)sin & 15) == 0,
                 "ltxk_qknorm_rope_1d: ld=%d must be >= 2*D and a multiple of 8, pointers 16-byte aligned", ld);
  LTXK_CHECK_ARG((int64_t)M * 2 <= (int64_t)INT32_MAX, "ltxk_qknorm_rope_1d: too many rows");
  const dim3 grid((2 * M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (H <= 32)
    hipLaunchKernelGGL((qknorm_rope_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, 2, D, (const bf16*)weight, cos, sin, T, H, eps);
  else
    hipLaunchKernelGGL((qknorm_rope_kernel<8, true>), grid, dim3(256), 0, (hipStream_t)stream, (bf16*)buf, ld, M, 2, D, (const bf16*)weight, cos, sin, T, H, eps);
  LTXK_CHECK_LAUNCH("ltxk_qknorm_rope_1d");
  return LTXK_OK;
}

extern "C" int ltxk_rope_table(const float* positions, const float* freq, float* cos, float* sin,
                               int32_t T, int32_t H, int32_t dim, int32_t n_freq, const float* max_pos,
                               void* stream) {
  LTXK_CHECK_ARG(positions && freq && cos && sin && max_pos, "ltxk_rope_table: null pointer");
  LTXK_CHECK_ARG(T > 0 && H > 0 && dim % (2 * H) == 0, "ltxk_rope_table: bad dims");
  const int half_dim = dim / 2;
  const int pad = half_dim - 3 * n_freq;
  LTXK_CHECK_ARG(pad >= 0, "ltxk_rope_table: 3*n_freq exceeds dim/2");
  const int total = T * half_dim;
  hipLaunchKernelGGL(rope_table_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     positions, freq, cos, sin, T, H, half_dim, pad, max_pos[0], max_pos[1], max_pos[2]);
  LTXK_CHECK_LAUNCH("ltxk_rope_table");
  return LTXK_OK;
}

extern "C" int ltxk_timestep_embed(const void* t, void* out, int32_t U, int32_t dim, float mult, void* stream) {
  LTXK_CHECK_ARG(t && out && U > 0 && dim > 0 && dim % 2 == 0, "ltxk_timestep_embed: bad arguments");
  const int total = U * (dim / 2);
  hipLaunchKernelGGL(timestep_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)t, (bf16*)out, U, dim, mult);
  LTXK_CHECK_LAUNCH("ltxk_timestep_embed");
  return LTXK_OK;
}

extern "C" int ltxk_ada_combine(const void* table, const void* ada, void* out, int32_t L, int32_t U,
                                int32_t K, int32_t D, uint32_t one_plus_mask, void* stream) {
  LTXK_CHECK_ARG(table && ada && out && L > 0 && U > 0 && K > 0 && K <= 32 && D > 0 && D % 8 == 0, "ltxk_ada_combine: bad arguments");
  const size_t total = (size_t)L * U * K * D / 8;
  hipLaunchKernelGGL(ada_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)table, (const bf16*)ada, (bf16*)out, L, U, K, D, one_plus_mask);
  LTXK_CHECK_LAUNCH("ltxk_ada_combine");
  return LTXK_OK;
}

extern "C" int ltxk_silu(const void* x, void* y, int64_t n, void* stream) {
  LTXK_CHECK_ARG(x && y && n > 0 && n % 8 == 0, "ltxk_silu: n must be a positive multiple of 8");
  const int64_t n8 = n / 8;
  hipLaunchKernelGGL(silu_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)x, (bf16*)y, n8);
  LTXK_CHECK_LAUNCH("ltxk_silu");
  return LTXK_OK;
}

extern "C" int ltxk_latent_to_tokens(const void* latent, void* tokens, int32_t B, int32_t C, int32_t S,
                                     int32_t rep, void* stream) {
  LTXK_CHECK_ARG(latent && tokens && B > 0 && S > 0 && C > 0 && C % 8 == 0 && rep >= 1, "ltxk_latent_to_tokens: bad arguments");
  hipLaunchKernelGGL(latent_to_tokens_kernel, dim3((S + 63) / 64, C / 8, B), dim3(64), 0, (hipStream_t)stream,
                     (const bf16*)latent, (bf16*)tokens, B, C, S, rep);
  LTXK_CHECK_LAUNCH("ltxk_latent_to_tokens");
  return LTXK_OK;
}

extern "C" int ltxk_attn_value_passthrough(const void* vt, int32_t ldvt, void* out, int32_t ldo, int32_t B, int32_t D, int32_t T,
                                           uint64_t row_mask, void* stream) {
  LTXK_CHECK_ARG(vt && out && B > 0 && B <= 64 && T > 0 && D > 0 && D % 128 == 0,
                 "ltxk_attn_value_passthrough: bad arguments (B in [1,64], T > 0, D a multiple of 128)");
  LTXK_CHECK_ARG(ldvt >= T && ldvt % 8 == 0 && ldo >= D && ldo % 8 == 0,
                 "ltxk_attn_value_passthrough: ldvt must be >= T, ldo >= D, both multiples of 8");
  LTXK_CHECK_ARG(((uintptr_t)vt & 15) == 0 && ((uintptr_t)out & 15) == 0, "ltxk_attn_value_passthrough: vt/out must be 16-byte aligned");
  if (B < 64) row_mask &= (1ull << B) - 1;
  if (row_mask == 0) return LTXK_OK;
  hipLaunchKernelGGL(value_passthrough_kernel, dim3((T + VP_TILE - 1) / VP_TILE, D / VP_TILE, B), dim3(256), 0,
                     (hipStream_t)stream, (const bf16*)vt, (int)ldvt, (bf16*)out, (int)ldo, (int)D, (int)T, row_mask);
  LTXK_CHECK_LAUNCH("ltxk_attn_value_passthrough");
  return LTXK_OK;
}
