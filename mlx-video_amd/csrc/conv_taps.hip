// Stride-1 convolution over the frames of a channels-last volume as an implicit GEMM on MFMA: ltxk_conv_taps_bf16.
// Replaces the causal 3x3 nn.Conv2d of the audio VAE decoder (audio_vae/causal_conv_2d.py) and the dilated nn.Conv1d /
// polyphase-packed nn.ConvTranspose1d of the vocoder (audio_vae/vocoder.py; time is H, W = 1).
//
//   y[r, co] = bias[co] + sum_{tap = (i, j), ci} x[r + (i*dil_h - pad_top) * W + (j - pad_left), ci] * w[co, tap, ci]
//   M = B*D*H*W rows, N = Cout, K = kh*kw*Cin walked tap-major in 64-wide steps: the LDS ring and MFMA loop of the Linear
//   GEMM (gemm_core.h), the row gather of conv3d.hip - a tap outside the row's own (H, W) frame reads the caller's zero
//   page, no padded copy exists - and the values of epilogue.h (taps_value / taps_leaky / taps_tanh).
// The tap offset is not separable into a table as in conv3d.hip (kh up to 16, any dilation): per K-step a lane derives its tap's
// (dh, dw) once, a piece adds its row's (h, w) and compares - a handful of VALU ops per 1-KiB piece, under 32+ MFMAs.
// Cin = 32 (the vocoder's last stage): a 64-wide K-step holds two taps, the lane's 16-byte chunk picks which (chunks 0-3 the even
// tap, 4-7 the odd one), so the tap is a per-lane value in every form.  With an odd tap count K = ntaps * 32 ends in the
// middle of the last K-step: its upper half reads the zero page on BOTH operand sides (the weight row ends there).
#include "gemm_core.h"
#include "epilogue.h"
#include <utility>

namespace ltxk {

struct TapsParams {
  const bf16 *x, *w, *bias, *zero, *resid, *a1, *a2;
  bf16 *out, *act_out;
  float* out_f32;
  int H, W, Cin, Cout, M, K;
  int kw, dil, pad_top, pad_left, ntaps;
  int cpb, c32;         // K-steps per tap (Cin / 64; 1 at Cin = 32, where a K-step is two taps)
  int RT, CT;
  int n_mean;
  float slope;
  float* slab;          // split-K: fp32 partial slabs [S][M][Cp], Cp = Cout rounded up to 4
  int S, kper, Cp;
};

// ---- guarded 4-column accesses of an (M, Cout) tensor at (row offset, column n < Cout): one vector access where Cout % 4 == 0
// (then n + 3 < Cout), element accesses clipped to Cout otherwise ----
__device__ __forceinline__ bf16x4 taps_ld4(const bf16* p, size_t row, int n, int Cout) {
  bf16x4 v = {};
  if (!p) return v;
  if ((Cout & 3) == 0) return *(const bf16x4*)(p + row + n);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (n + j < Cout) v[j] = p[row + n + j];
  return v;
}
__device__ __forceinline__ void taps_st4(bf16* p, size_t row, int n, int Cout, bf16x4 v) {
  if ((Cout & 3) == 0) { *(bf16x4*)(p + row + n) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (n + j < Cout) p[row + n + j] = v[j];
}
__device__ __forceinline__ void taps_st4(float* p, size_t row, int n, int Cout, f32x4 v) {
  if ((Cout & 3) == 0) { *(f32x4*)(p + row + n) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (n + j < Cout) p[row + n + j] = v[j];
}

template <int TT, int WN, bool SPLIT>
__global__ __launch_bounds__(GEMM_THREADS) void conv_taps_kernel(TapsParams p) {
  using G = GemmGeom<TT, WN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  int tile, slice = 0;
  if constexpr (SPLIT) {
    tile = blockIdx.x / p.S;
    slice = blockIdx.x - tile * p.S;
  } else {
    // XCD-aware order as in conv3d.hip: each XCD takes a contiguous run of tiles (neighbours share their halo rows in its L2)
    const int nt_all = p.RT * p.CT, q = nt_all >> 3, r = nt_all & 7;
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    tile = x * q + (x < r ? x : r) + j;
  }
  const int ct = tile % p.CT, rt = tile / p.CT;
  const int m0 = rt * G::BM, n0 = ct * G::BN;
  const int nq = (lane >> 4) * 4;

  // ---- bias first: older than every LDS-DMA piece, so the counted vmcnt waits below cover it (as conv3d.hip's kw kernel).
  // Element loads clipped to Cout: Cout may be 2. ----
  // Sixteen 2-byte loads into registers of their own: packing them here would wait for them in front of the first DMA.
  unsigned braw[4][4] = {};
  if constexpr (!SPLIT) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = n0 + wn * 64 + nt * 16 + nq;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int nn = n + j < p.Cout ? n + j : p.Cout - 1;
        braw[nt][j] = *opaque_gptr<unsigned short>((const unsigned short*)p.bias + nn);
      }
    }
  }

  const int lrow = lane >> 3;
  const int chunk = (lane & 7) ^ lrow;
  const bf16* wptr[G::W_PER_WAVE];
#pragma unroll
  for (int i = 0; i < G::W_PER_WAVE; ++i) {
    int r = n0 + (wave * G::W_PER_WAVE + i) * 8 + lrow;
    r = r < p.Cout ? r : p.Cout - 1;
    wptr[i] = p.w + (size_t)r * p.K + chunk * 8;
  }
  // uniform piece count per wave (see gemm.hip): waves past A_REM re-issue their last A piece
  const int nA = G::A_BASE + (wave < G::A_REM ? 1 : 0);
  const int a0 = wave * G::A_BASE + (wave < G::A_REM ? wave : G::A_REM);
  const unsigned rowB = (unsigned)p.Cin * 2u;
  int vh[G::MAXA], vw[G::MAXA], adst[G::MAXA];
  unsigned roff[G::MAXA];                                   // byte offset of the piece's own row (volume < 4 GiB, checked on the host)
#pragma unroll
  for (int i = 0; i < G::MAXA; ++i) {
    const int pi = nA > 0 ? a0 + (i < nA ? i : nA - 1) : G::A_PIECES - 1;
    int r = m0 + pi * 8 + lrow;
    r = r < p.M ? r : p.M - 1;
    roff[i] = (unsigned)r * rowB;
    vw[i] = r % p.W;
    vh[i] = (r / p.W) % p.H;
    adst[i] = G::W_STAGE_BYTES + (pi < G::A_PIECES ? pi : G::A_PIECES - 1) * 1024;
  }
  constexpr int PER_STAGE = G::W_PER_WAVE + G::MAXA;
  static_assert(PER_STAGE <= 7, "vmcnt immediates assume <= 7 pieces per stage");
  const char* zsrc = (const char*)p.zero + chunk * 16;
  const char* xb = (const char*)p.x;

  // this workgroup's K-step range [kbeg, nk) (the whole K unless split)
  const int nk_all = (p.K + GEMM_BK - 1) / GEMM_BK;
  const int kbeg = SPLIT ? slice * p.kper : 0;
  int nk = SPLIT ? kbeg + p.kper : nk_all;
  nk = nk < nk_all ? nk : nk_all;

  // per-lane source state of the prefetch stream's K-step
  int ptap = kbeg / p.cpb, pcb = kbeg - ptap * p.cpb;
  int dh_l, dw_l, delta_l;
  bool zt_l, wz_l;
  auto set_step = [&](int kt) __attribute__((always_inline)) {
    const int tap = p.c32 ? 2 * kt + (chunk >> 2) : ptap;
    const int coff = p.c32 ? (chunk & 3) * 16 : pcb * 128 + chunk * 16;
    const int ti = p.kw == 3 ? (tap * 43691) >> 17 : tap;       // tap / 3 (exact below 2^15)
    const int tj = tap - ti * p.kw;
    dh_l = ti * p.dil - p.pad_top;
    dw_l = tj - p.pad_left;
    delta_l = (dh_l * p.W + dw_l) * (int)rowB + coff;
    zt_l = tap >= p.ntaps;
    wz_l = kt * GEMM_BK + chunk * 8 >= p.K;
  };
  auto advance = [&]() __attribute__((always_inline)) {
    ++pcb;
    if (pcb == p.cpb) { pcb = 0; ++ptap; }
  };
  // i-th LDS-DMA piece of this wave for K-step kt (the one set_step last saw) into ring slot s
  auto issue_piece = [&](int i, int kt, int s) __attribute__((always_inline)) {
    char* base = smem + s * G::STAGE_BYTES;
    if (i < G::W_PER_WAVE) {
      const char* src = wz_l ? zsrc : (const char*)(wptr[i < G::W_PER_WAVE ? i : 0] + kt * GEMM_BK);
      glds16(src, base + (wave * G::W_PER_WAVE + i) * 1024);
    } else if (i < PER_STAGE) {
      const int j = i - G::W_PER_WAVE < G::MAXA ? i - G::W_PER_WAVE : 0;
      const int h = vh[j] + dh_l, w = vw[j] + dw_l;
      const bool z = zt_l || (unsigned)h >= (unsigned)p.H || (unsigned)w >= (unsigned)p.W;
      const char* src = z ? zsrc : xb + (size_t)(roff[j] + (unsigned)delta_l);
      glds16(src, base + adst[j]);
    }
  };

  f32x4 acc[TT][4];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[tt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: stages kbeg and, where it exists, kbeg + 1
  set_step(kbeg);
#pragma unroll
  for (int i = 0; i < PER_STAGE; ++i) issue_piece(i, kbeg, 0);
  if (kbeg + 1 < nk) {
    advance();
    set_step(kbeg + 1);
#pragma unroll
    for (int i = 0; i < PER_STAGE; ++i) issue_piece(i, kbeg + 1, 1);
  }
  int s = 0;
  MmaPipe<TT, WN, false> pipe;
  pipe.init();
  // MODE 0: steady state (requests K-step kt + 2); 1: next-to-last (nothing left to request); 2: last (nothing younger than
  // its own stage is in flight)
  auto kstep = [&](int kt, auto mode_c) __attribute__((always_inline)) {
    constexpr int MODE = decltype(mode_c)::value;
    if constexpr (MODE == 2) wait_keep_and_barrier<0>();
    else wait_keep_and_barrier<PER_STAGE>();
    int s2 = s + 2;
    s2 = s2 >= 3 ? s2 - 3 : s2;
    if constexpr (MODE == 0) {
      advance();
      set_step(kt + 2);
    }
    pipe.step(smem + s * G::STAGE_BYTES, wm, wn, lane, acc, [&](int i) {
      if constexpr (MODE == 0) issue_piece(i, kt + 2, s2);
    });
    s = s + 1 == 3 ? 0 : s + 1;
  };
  for (int kt = kbeg; kt < nk - 2; ++kt) kstep(kt, IntC<0>{});
  if (nk - kbeg >= 2) kstep(nk - 2, IntC<1>{});
  kstep(nk - 1, IntC<2>{});
  pipe.finish(acc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (!SPLIT) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(braw[nt][j]));      // never dead, never dropped (see gemm.hip)
  }
  bf16x4 bpre[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) bpre[nt][j] = __builtin_bit_cast(bf16, (unsigned short)braw[nt][j]);

  // epilogue: acc[tt][nt][j]: row = lane & 15, co = 4 * (lane >> 4) + j.  Rows past M and columns past Cout are never stored.
  if constexpr (SPLIT) {
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const int m = m0 + wm * TT * 16 + tt * 16 + (lane & 15);
      if (m >= p.M) continue;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wn * 64 + nt * 16 + nq;
        if (n >= p.Cout) continue;
        *(f32x4*)(p.slab + ((size_t)slice * p.M + m) * p.Cp + n) = acc[tt][nt];   // n + 3 < Cp
      }
    }
  } else {
    if (p.out_f32) {
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int m = m0 + wm * TT * 16 + tt * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int n = n0 + wn * 64 + nt * 16 + nq;
          if (n >= p.Cout) continue;
          taps_st4(p.out_f32, (size_t)m * p.Cout, n, p.Cout, taps_tanh(acc[tt][nt], bpre[nt]));
        }
      }
      return;
    }
    // bf16 outputs of whole 8-column groups go through a wave-private LDS line image and leave as whole lines (epilogue.h)
    const bool wide = (p.Cout & 7) == 0;
    const LineImage<128, TT * 16> img{smem + wave * (TT * 16 * 128), lane};
    if (wide) __syncthreads();
    // y replaces the accumulators: both outputs follow from it
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const int m = m0 + wm * TT * 16 + tt * 16 + (lane & 15);
      if (m >= p.M) continue;
      const size_t row = (size_t)m * p.Cout;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wn * 64 + nt * 16 + nq;
        if (n >= p.Cout) continue;
        float y[4];
        taps_value(acc[tt][nt], bpre[nt], p.resid != nullptr, taps_ld4(p.resid, row, n, p.Cout), p.n_mean,
                   taps_ld4(p.a1, row, n, p.Cout), taps_ld4(p.a2, row, n, p.Cout), y);
        acc[tt][nt] = f32x4{y[0], y[1], y[2], y[3]};
      }
    }
    auto store_all = [&](bf16* dst, bool leaky) __attribute__((always_inline)) {
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int m = m0 + wm * TT * 16 + tt * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int n = n0 + wn * 64 + nt * 16 + nq;
          if (n >= p.Cout) continue;
          const float y[4] = {acc[tt][nt][0], acc[tt][nt][1], acc[tt][nt][2], acc[tt][nt][3]};
          const bf16x4 o = leaky ? taps_leaky(y, p.slope) : to_bf16x4(y);
          if (wide) img.put(tt * 16 + (lane & 15), nt, o);
          else taps_st4(dst, (size_t)m * p.Cout, n, p.Cout, o);
        }
      }
      if (wide) img.flush(dst, p.Cout, m0 + wm * TT * 16, n0 + wn * 64, p.M, p.Cout);
    };
    if (p.out) store_all(p.out, false);
    if (p.act_out) store_all(p.act_out, true);
  }
}

// split-K finalize: the slabs summed in slice order (deterministic), then the epilogue of the single pass; one thread per 4 columns
__global__ void conv_taps_finalize_kernel(TapsParams p) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = p.Cp / 4;
  if (idx >= (size_t)p.M * q) return;
  const int m = (int)(idx / q), n = (int)(idx - (size_t)m * q) * 4;
  const f32x4 a = sum_slices(p.slab + idx * 4, (size_t)p.M * p.Cp, p.S);
  bf16x4 bs;
#pragma unroll
  for (int j = 0; j < 4; ++j) bs[j] = p.bias[n + j < p.Cout ? n + j : p.Cout - 1];
  const size_t row = (size_t)m * p.Cout;
  if (p.out_f32) {
    taps_st4(p.out_f32, row, n, p.Cout, taps_tanh(a, bs));
    return;
  }
  float y[4];
  taps_value(a, bs, p.resid != nullptr, taps_ld4(p.resid, row, n, p.Cout), p.n_mean, taps_ld4(p.a1, row, n, p.Cout),
             taps_ld4(p.a2, row, n, p.Cout), y);
  if (p.out) taps_st4(p.out, row, n, p.Cout, to_bf16x4(y));
  if (p.act_out) taps_st4(p.act_out, row, n, p.Cout, taps_leaky(y, p.slope));
}

// The launch form of one ltxk_conv_taps_bf16 call: the argument checks, then tile / split-K slices.  ltxk_conv_taps_bf16
// launches what this decides and ltxk_conv_taps_plan reports it, so the two cannot drift apart.
struct TapsForm {
  struct ltxk_conv3d_plan plan;
  int M, K, Cp;
};

static int taps_form(const ltxk_conv_taps_args* a, TapsForm& f) {
  const char* who = "ltxk_conv_taps_bf16";
  LTXK_CHECK_ARG(a != nullptr, "%s: null args", who);
  LTXK_CHECK_ARG(a->struct_bytes == (int)sizeof(ltxk_conv_taps_args), "%s: struct_bytes = %d, this build's ltxk_conv_taps_args has %d",
                 who, a->struct_bytes, (int)sizeof(ltxk_conv_taps_args));
  LTXK_CHECK_ARG(a->x && a->w && a->bias && a->zero_page, "%s: null x/w/bias/zero_page", who);
  LTXK_CHECK_ARG(a->B > 0 && a->D > 0 && a->H > 0 && a->W > 0, "%s: bad volume %dx%dx%dx%d", who, a->B, a->D, a->H, a->W);
  LTXK_CHECK_ARG(a->Cin == 32 || (a->Cin > 0 && a->Cin % 64 == 0), "%s: Cin=%d must be 32 or a multiple of 64 (pad channels with zeros)", who, a->Cin);
  LTXK_CHECK_ARG(a->Cout >= 1, "%s: Cout=%d must be at least 1", who, a->Cout);
  LTXK_CHECK_ARG(a->kh >= 1 && a->kh <= 16 && (a->kw == 1 || a->kw == 3) && a->dil_h >= 1 && a->dil_h <= 8,
                 "%s: kernel %dx%d dilation %d: needs kh in [1,16], kw 1 or 3, dil_h in [1,8]", who, a->kh, a->kw, a->dil_h);
  LTXK_CHECK_ARG(a->pad_top >= 0 && a->pad_bottom >= 0 && a->pad_top + a->pad_bottom == (a->kh - 1) * a->dil_h,
                 "%s: pad_top + pad_bottom = %d + %d must be (kh-1)*dil_h = %d", who, a->pad_top, a->pad_bottom, (a->kh - 1) * a->dil_h);
  LTXK_CHECK_ARG(a->pad_left >= 0 && a->pad_right >= 0 && a->pad_left + a->pad_right == a->kw - 1,
                 "%s: pad_left + pad_right = %d + %d must be kw-1 = %d", who, a->pad_left, a->pad_right, a->kw - 1);
  const long long M = (long long)a->B * a->D * a->H * a->W;
  LTXK_CHECK_ARG(M < (1ll << 31) && M * a->Cin * 2 < (1ll << 32) && M * a->Cout < (1ll << 40), "%s: input volume must be < 4 GiB (32-bit tile offsets)", who);
  if (a->out_f32) {
    LTXK_CHECK_ARG(!a->out && !a->act_out && !a->resid && a->n_mean == 0 && !a->mean_a1 && !a->mean_a2,
                   "%s: the tanh form (out_f32) takes no resid / mean / out / act_out", who);
  } else {
    LTXK_CHECK_ARG(a->out || a->act_out, "%s: no output (out, act_out and out_f32 all NULL)", who);
    LTXK_CHECK_ARG(a->n_mean == 0 || a->n_mean == 2 || a->n_mean == 3, "%s: n_mean=%d must be 0, 2 or 3", who, a->n_mean);
    LTXK_CHECK_ARG((a->n_mean >= 2) == (a->mean_a1 != nullptr) && (a->n_mean == 3) == (a->mean_a2 != nullptr),
                   "%s: n_mean=%d does not match mean_a1 / mean_a2", who, a->n_mean);
  }
  LTXK_CHECK_ARG((((uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->zero_page) & 15) == 0, "%s: x / w / zero_page must be 16-byte aligned", who);
  const uintptr_t rows = (uintptr_t)a->out | (uintptr_t)a->act_out | (uintptr_t)a->resid | (uintptr_t)a->mean_a1 | (uintptr_t)a->mean_a2;
  const int row_align = a->Cout % 8 == 0 ? 16 : a->Cout % 4 == 0 ? 8 : 2;
  LTXK_CHECK_ARG((rows & (row_align - 1)) == 0 && ((uintptr_t)a->bias & 1) == 0, "%s: misaligned bf16 row tensor (Cout=%d needs %d bytes)", who, a->Cout, row_align);
  LTXK_CHECK_ARG(((uintptr_t)a->out_f32 & (a->Cout % 4 == 0 ? 15 : 3)) == 0, "%s: misaligned out_f32", who);
  float* ws = (float*)a->workspace;
  const size_t wsb = ws ? (size_t)a->workspace_bytes : 0;
  LTXK_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
  f.M = (int)M;
  f.K = a->kh * a->kw * a->Cin;
  f.Cp = (a->Cout + 3) & ~3;
  struct ltxk_conv3d_plan& pl = f.plan;
  pl = {};
  pl.kernel = LTXK_CONV_KERNEL_TAPS;
  pl.tile_rows = 256;
  pl.tile_cols = a->Cout > 64 ? 128 : 64;      // 256x64: the 32- and 64-channel stages and conv_post waste fewer MFMA columns
  pl.row_tiles = (int)((M + pl.tile_rows - 1) / pl.tile_rows);
  pl.col_tiles = (a->Cout + pl.tile_cols - 1) / pl.tile_cols;
  const int nk = (f.K + GEMM_BK - 1) / GEMM_BK;
  pl.slices = 1;
  pl.ksteps = nk;
  // split K when the tile grid leaves most of the 256 CUs idle (the vocoder's first stages are a few hundred rows):
  // S slices of >= 8 K-steps, fp32 slabs in the caller's workspace
  const long tiles = (long)pl.row_tiles * pl.col_tiles;
  int S = 1;
  if (ws && tiles <= 128) {
    S = (int)(256 / tiles);
    if (S > nk / 8) S = nk / 8;
    const size_t per = (size_t)M * f.Cp * sizeof(float);
    if ((size_t)S * per > wsb) S = (int)(wsb / per);
    if (S > 16) S = 16;
  }
  if (S >= 2) {
    pl.ksteps = (nk + S - 1) / S;
    pl.slices = (nk + pl.ksteps - 1) / pl.ksteps;                    // drop empty trailing slices
  }
  return LTXK_OK;
}

template <int TT, int WN>
static int taps_launch(TapsParams p, const TapsForm& f, hipStream_t stream) {
  using G = GemmGeom<TT, WN>;
  const struct ltxk_conv3d_plan& pl = f.plan;
  p.RT = pl.row_tiles;
  p.CT = pl.col_tiles;
  if (pl.slices >= 2) {
    auto kern = conv_taps_kernel<TT, WN, true>;
    static std::atomic<uint64_t> attr_set{0};
    const int rc = ensure_dyn_lds((const void*)kern, G::LDS_BYTES, attr_set, "ltxk_conv_taps_bf16");
    if (rc != LTXK_OK) return rc;
    p.S = pl.slices; p.kper = pl.ksteps;
    hipLaunchKernelGGL(kern, dim3(p.RT * p.CT * p.S), dim3(GEMM_THREADS), G::LDS_BYTES, stream, p);
    LTXK_CHECK_LAUNCH("ltxk_conv_taps_bf16(split-K)");
    const size_t total = (size_t)p.M * (p.Cp / 4);
    hipLaunchKernelGGL(conv_taps_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p);
    LTXK_CHECK_LAUNCH("ltxk_conv_taps_bf16(finalize)");
    return LTXK_OK;
  }
  auto kern = conv_taps_kernel<TT, WN, false>;
  static std::atomic<uint64_t> attr_set{0};
  const int rc = ensure_dyn_lds((const void*)kern, G::LDS_BYTES, attr_set, "ltxk_conv_taps_bf16");
  if (rc != LTXK_OK) return rc;
  p.slab = nullptr; p.S = 1; p.kper = pl.ksteps;
  hipLaunchKernelGGL(kern, dim3(p.RT * p.CT), dim3(GEMM_THREADS), G::LDS_BYTES, stream, p);
  LTXK_CHECK_LAUNCH("ltxk_conv_taps_bf16");
  return LTXK_OK;
}

}  // namespace ltxk

extern "C" int ltxk_conv_taps_plan(const ltxk_conv_taps_args* a, struct ltxk_conv3d_plan* plan) {
  using namespace ltxk;
  LTXK_CHECK_ARG(plan != nullptr, "ltxk_conv_taps_plan: null plan");
  TapsForm f;
  const int rc = taps_form(a, f);
  if (rc == LTXK_OK) *plan = f.plan;
  return rc;
}

extern "C" int ltxk_conv_taps_bf16(const ltxk_conv_taps_args* a, void* stream) {
  using namespace ltxk;
  TapsForm f;
  const int rc = taps_form(a, f);
  if (rc != LTXK_OK) return rc;
  TapsParams p;
  p.x = (const bf16*)a->x; p.w = (const bf16*)a->w; p.bias = (const bf16*)a->bias; p.zero = (const bf16*)a->zero_page;
  p.resid = (const bf16*)a->resid; p.a1 = (const bf16*)a->mean_a1; p.a2 = (const bf16*)a->mean_a2;
  p.out = (bf16*)a->out; p.act_out = (bf16*)a->act_out; p.out_f32 = a->out_f32;
  p.H = a->H; p.W = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.M = f.M; p.K = f.K;
  p.kw = a->kw; p.dil = a->dil_h; p.pad_top = a->pad_top; p.pad_left = a->pad_left; p.ntaps = a->kh * a->kw;
  p.c32 = a->Cin == 32; p.cpb = p.c32 ? 1 : a->Cin / 64;
  p.RT = p.CT = 0;
  p.n_mean = a->n_mean; p.slope = a->slope;
  p.slab = (float*)a->workspace; p.S = 1; p.kper = 0; p.Cp = f.Cp;
  hipStream_t st = (hipStream_t)stream;
  return f.plan.tile_cols == 128 ? taps_launch<4, 2>(p, f, st) : taps_launch<2, 1>(p, f, st);
}
