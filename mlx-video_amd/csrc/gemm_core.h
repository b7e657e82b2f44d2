// MFMA GEMM main loop shared by the dense (Linear) and implicit (conv3d) kernels.
// (What follows the loop - accumulators to stored bf16 - is shared the same way in epilogue.h.)
//
//   C[m,n] = sum_k A[m,k] * W[n,k]          A rows and W rows are both k-contiguous bf16
//
// Geometry (gfx950, wave64): one workgroup = 8 waves = WM (rows) x WN (cols), WM*WN = 8;
// tile BM x BN x 64 with BM = 16*TT*WM, BN = 16*NT*WN; per wave TT x NT MFMA tiles of
// v_mfma_f32_16x16x32_bf16.  (TT=5, WN=4, NT=4): 160x256, the Linear layers at M=2560;
// (TT=4, WN=2, NT=4): 256x128, the 128-channel convolutions; (TT=5, WN=4, NT=2): 160x128 with 80x32 per wave, the
// Linear layers whose 256-column tiling leaves CUs idle (M=1280, N=4096: exactly 256 tiles; round 4).
// Staging: global_load_lds_dwordx4 (LDS-DMA, no VGPR round trip) into a 3-deep LDS ring; one
// raw s_barrier per K-step, counted vmcnt so that two K-steps stay in flight across it.
// LDS image: 128-byte rows ([row][64 bf16]) with the 16-byte chunk index XOR-swizzled by
// (row & 7): the DMA destination is lane-linear, so the permutation is applied to the per-lane
// SOURCE address and again on the ds_read_b128 fragment reads (conflict-free for the 16x16x32
// operand map).
// W8 (weight-fp8) forms: the W half of a stage holds e4m3 bytes, 64-byte rows ([row][64 fp8]); the A half is unchanged.  A
// 1-KiB LDS-DMA piece is then 16 rows x 64 B (half as many W pieces per wave), and a lane's fragment is the 8 consecutive
// bytes of the 8 k-positions its bf16x8 holds in the bf16 form, read with ds_read_b64 and widened in registers by four
// v_cvt_scalef32_pk_bf16_fp8 (scale 1.0: every e4m3 value is a bf16 value) in front of the first MFMA group that uses it:
// the MFMAs, their operands and their order are those of the bf16 form.  ds_read_b64 banks over 256 B = four 64-byte rows
// and conflicts inside a 32-lane half, which reads 16 rows x two 8-byte chunks: rows r, r+4, r+8, r+12 share 16 banks, so
// the 16-byte chunk index (0..3) is XOR-swizzled by ((row >> 2) & 3) - each of the four rows then owns its own 16 bytes of
// the shared banks for every k-quarter.  The swizzle unit is the DMA's 16 bytes, so it is again applied to the per-lane
// source address.
// W8A8 (fp8 x fp8) forms: a K-step is 128 k and BOTH halves of a stage hold e4m3 bytes in 128-byte rows ([row][128 fp8]) - the
// byte geometry, LDS-DMA pieces, swizzle and counted waits of the bf16 stage.  One v_mfma_scale_f32_16x16x128_f8f6f4 (both
// formats e4m3, both block scales the E8M0 code of 1.0) per 16x16 tile and K-step takes 32 bytes per lane and operand: lane l
// reads the two 16-byte chunks (l >> 4) and 4 + (l >> 4) of row (l & 15) - exactly the two ds_read_b128 the bf16 form issues for
// its K-sub-steps 0 and 1, at the same swizzled addresses, so they are conflict-free by the same bank rule.  The lane therefore
// holds k = 16g..16g+15 and 64+16g..64+16g+15 (g = l >> 4) of the 128, not the instruction's nominal 32g..32g+31: the sum over
// k is order-free and the A and W fragments use the same assignment (MmaPipe8).
#pragma once
#include "common.h"

namespace ltxk {

template <int V> struct IntC { static constexpr int value = V; };

// A global pointer the optimiser cannot see through (an empty asm: no instruction, no wait): `load(c ? a : dummy)` used
// only when c holds otherwise gets unfolded into a load under `if (c)`, which breaks a counted-vmcnt prologue that
// assumes a fixed number of loads per lane (gemm.hip).
// (The pointer comes back as an explicit global-address-space pointer: a generic one would turn the load into flat_load,
// which hipcc waits for with vmcnt(0).)
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* opaque_gptr(const T* p) {
  uintptr_t u = (uintptr_t)p;
  asm volatile("" : "+v"(u));
  return (const __attribute__((address_space(1))) T*)u;
}

constexpr int GEMM_BK = 64;
constexpr int GEMM_THREADS = 512;

template <int TT, int WN, int NT = 4, bool W8 = false>
struct GemmGeom {
  static constexpr int WM = 8 / WN;
  static constexpr int BM = 16 * TT * WM;
  static constexpr int BN = 16 * NT * WN;
  static_assert(BN % 64 == 0, "whole 1-KiB W pieces per wave");
  static constexpr int W_ROW_BYTES = W8 ? GEMM_BK : GEMM_BK * 2;
  static constexpr int W_PIECES = BN * W_ROW_BYTES / 1024;   // 1 KiB pieces (8 rows x 128 B; fp8: 16 rows x 64 B)
  static_assert(W_PIECES % 8 == 0, "the same number of W pieces for every wave");
  static constexpr int W_PER_WAVE = W_PIECES / 8;
  static constexpr int W_STAGE_BYTES = BN * W_ROW_BYTES;
  static constexpr int A_PIECES = BM / 8;
  static constexpr int A_BASE = A_PIECES / 8;      // pieces per wave (floor)
  static constexpr int A_REM = A_PIECES % 8;       // first A_REM waves take one more
  static constexpr int MAXA = A_BASE + (A_REM ? 1 : 0);
  static constexpr int STAGE_BYTES = W_STAGE_BYTES + BM * GEMM_BK * 2;
  static constexpr int STAGES = 3;
  static constexpr int LDS_BYTES = STAGES * STAGE_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS ring exceeds 160 KiB");
};

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Each XCD owns a band
// of CT/8 column tiles and walks it in patches of 8 row tiles x 4 column tiles per 32-workgroup round: the round then
// pulls 8 A panels + 4 W panels through that XCD's L2 (against 16 + 2 for "all row tiles x 2 columns": -25 % of the
// L2->fabric reads, and the chip is power-limited in these launches - the first form of this patch order was worth
// < 1 % on FF1 in round 1, the 16x16 case below 0.8 % of the whole block in round 2).  Column bands that are not a
// multiple of 4 wide (q|k|v: 6) finish with a 2-column strip.  Placement affects speed only.
__device__ __forceinline__ void map_tile(int bid, int RT, int CT, int& rt, int& ct) {
  if ((CT & 15) == 0) {
    const int xcd = bid & 7, idx = bid >> 3;
    const int cpx = CT >> 3;                 // column tiles owned by this XCD
    if (cpx == 2 && RT == 16) {
      // 16 x 16 tiles = ONE round (FF2, out, q2, o2 at M=2560, N=4096): two XCDs share a 4-column group, one row half each
      rt = (xcd & 1) * 8 + (idx >> 2);
      ct = (xcd >> 1) * 4 + (idx & 3);
    } else if ((RT & 7) == 0) {
      const int full = (cpx >> 2) * 4 * RT;  // tiles of the band's whole 4-column groups
      if (idx < full) {
        const int per_cg = 4 * RT;           // workgroups per column group (all row tiles)
        const int cg = idx / per_cg, j = idx - cg * per_cg;
        const int rg = j >> 5, k = j & 31;   // row group of 8, position inside the 8x4 patch
        rt = rg * 8 + (k >> 2);
        ct = xcd * cpx + cg * 4 + (k & 3);
      } else {
        const int remc = cpx & 3, j = idx - full;      // the remaining 1-3 columns, all row tiles
        rt = j / remc;
        ct = xcd * cpx + (cpx >> 2) * 4 + (j - rt * remc);
      }
    } else {
      const int pair = idx / (2 * RT), j = idx - pair * 2 * RT;
      rt = j >> 1;
      ct = xcd * cpx + pair * 2 + (j & 1);
    }
  } else {
    rt = bid % RT;
    ct = bid / RT;
  }
}

// Wait until this wave's loads of the current K-step have landed, leaving `keep` younger
// LDS-DMA instructions (the next K-step's) in flight, then rendezvous.
template <int KEEP>
__device__ __forceinline__ void wait_keep_and_barrier() {
  static_assert(KEEP >= 0 && KEEP <= 63, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(KEEP) : "memory");
}

__device__ __forceinline__ void wait_stage_and_barrier(int keep) {
  switch (keep) {
    case 0: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
  }
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn bytes -> the bf16x8 with the same values in the same order (exact: e4m3 is a subset of bf16)
__device__ __forceinline__ bf16x8 fp8x8_to_bf16x8(u32x2 v) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[0], 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[0], 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[1], 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[1], 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// Byte offset, inside a lane's 64-byte fp8 W row, of its fragment of K-sub-step ks (the swizzle of the header comment)
__device__ __forceinline__ int w8_koff(int lane, int ks) {
  return ((ks * 4 + (lane >> 4)) ^ (((lane >> 2) & 3) << 1)) << 3;
}

// Operand roles.  SWAP=false: acc tile = D[n (4 regs)][row (lane&15)]  (W is the MFMA A operand), so a lane
// holds 4 consecutive output columns of one row: 8-byte row-major stores.  SWAP=true: acc tile =
// D[row (4 regs)][n (lane&15)]: 4 consecutive rows of one column, used for the transposed (V^T) output.
// Software-pipelined K-step: the 2*TT MFMA groups (4 MFMAs each: one A-row fragment x 4 W
// fragments) run in a fixed order pinned by sched_barrier; fragment ds_read_b128s are issued two
// groups ahead of their use, and this wave's LDS-DMA pieces of the stage two K-steps ahead are
// sprinkled one (or PPG) per group instead of being issued as a burst in front of the MFMAs — the
// DMA issue cost (~60-180 cycles per 1-KiB piece) then hides under the matrix pipe.
// issue(i): launch this wave's i-th LDS-DMA piece of the prefetched stage (no-op for i >= count).
template <int TT, int WN, bool SWAP, int NT = 4, bool W8 = false, class IssueFn>
__device__ __forceinline__ void mma_stage_pipelined(const char* st, int wm, int wn, int lane,
                                                    f32x4 (&acc)[TT][NT], IssueFn&& issue) {
  using G = GemmGeom<TT, WN, NT, W8>;
  constexpr int NG = 2 * TT;                                   // MFMA groups per K-step
  constexpr int MAXP = G::W_PER_WAVE + G::MAXA;                // LDS-DMA pieces per wave per stage
  constexpr int PPG = (MAXP + NG - 1) / NG;
  const char* wb = st + (wn * 16 * NT + (lane & 15)) * G::W_ROW_BYTES;
  const char* ab = st + G::W_STAGE_BYTES + (wm * TT * 16) * 128 + (lane & 15) * 128;
  const int koff0 = (((lane >> 4)) ^ (lane & 7)) << 4;
  const int koff1 = (((4 + (lane >> 4))) ^ (lane & 7)) << 4;
  const int kw0 = w8_koff(lane, 0), kw1 = w8_koff(lane, 1);
  bf16x8 wf[2][NT], af[2][TT];
  u32x2 wraw[2][NT];                  // W8: the fragments as read, widened into wf in front of their first MFMA group
  // flat read order: W0[0..NT-1], A0[0..TT-1], W1[0..NT-1], A1[0..TT-1]
  auto rd = [&](int idx) {
    // idx is a compile-time constant after unrolling
    const int ks = idx / (NT + TT), r = idx % (NT + TT);
    const int ko = ks ? koff1 : koff0;
    if (r < NT) {
      if constexpr (W8) wraw[ks][r] = *(const u32x2*)(wb + r * 1024 + (ks ? kw1 : kw0));
      else wf[ks][r] = *(const bf16x8*)(wb + r * 2048 + ko);
    } else af[ks][r - NT] = *(const bf16x8*)(ab + (r - NT) * 2048 + ko);
  };
  constexpr int TOTAL = 2 * (NT + TT);
  auto need = [](int g) { return (g / TT) * (NT + TT) + NT + (g % TT) + 1; };
  int issued = 0;
#pragma unroll
  for (int i = 0; i < TOTAL; ++i)
    if (i < need(1 < NG ? 1 : 0)) { rd(i); issued = i + 1; }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int target = need(g + 2 < NG ? g + 2 : NG - 1);
#pragma unroll
    for (int i = 0; i < TOTAL; ++i)
      if (i >= issued && i < target) rd(i);
    issued = target > issued ? target : issued;
#pragma unroll
    for (int q = 0; q < PPG; ++q) issue(g * PPG + q);
    const int ks = g / TT, tt = g % TT;
    if constexpr (W8) {
      if (tt == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[ks][nt] = fp8x8_to_bf16x8(wraw[ks][nt]);
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      acc[tt][nt] = SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][tt], wf[ks][nt], acc[tt][nt], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][nt], af[ks][tt], acc[tt][nt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Rotated software pipeline: like mma_stage_pipelined, but the last two MFMA groups of every
// K-step are deferred until AFTER the next K-step's barrier (their operands are already in
// registers), so they execute while the first fragment reads of the new stage are in flight: the
// LDS cold start after each barrier (all 8 waves reading at once) no longer idles the matrix pipe.
// Requires TT >= 2 (both deferred groups then share the ks=1 W fragments).
// Fragment reads run this many MFMA groups ahead of their use.  1, not 2 (round 2, interleaved A/B on one box,
// profiles/r02_gemm_prefetch_depth_ab.log): the N=4096 launches 85.5 -> 79.7 us (bias) / 89.7 -> 85.2 us (gate+residual),
// FF2 299 -> 290 us, the whole block -1.1 %, the VAE decode -0.7 %; 3 is slower than 2.  With two waves per SIMD the
// other wave covers an LDS read that is one group (64 matrix-pipe cycles) ahead, and the shorter lead leaves fewer
// reads queued in front of each barrier.
#ifndef LTXK_PREFETCH_GROUPS
#define LTXK_PREFETCH_GROUPS 1
#endif
// DG = number of trailing MFMA groups of a K-step that are deferred past the next barrier (2 <= DG <= TT:
// all deferred groups use the ks=1 W fragments).  DG=2 hides the LDS cold start; DG=TT additionally puts a
// wave half a K-step out of phase with a DG=2 wave — used for waves 4-7, the SIMD partners of waves 0-3, so
// that the two waves of a SIMD do not hit their LDS-read bursts, DMA issues and MFMA-dense stretches together.
template <int TT, int WN, bool SWAP, int DG = 2, int NT = 4, bool W8 = false>
struct MmaPipe {
  using G = GemmGeom<TT, WN, NT, W8>;
  static constexpr int PD = LTXK_PREFETCH_GROUPS;   // fragment reads run PD MFMA groups ahead of their use
  static constexpr int NG = 2 * TT;
  static constexpr int MAXP = G::W_PER_WAVE + G::MAXA;
#ifdef LTXK_DMA_PER_GROUP
  static constexpr int PPG = LTXK_DMA_PER_GROUP;                // A/B: bunch the stage's LDS-DMA pieces into the first groups
#else
  static constexpr int PPG = (MAXP + NG - 1) / NG;
#endif
  static constexpr int TOTAL = 2 * (NT + TT);
  static_assert(TT >= 2 && DG >= 2 && DG <= TT, "deferred groups must all lie in the ks=1 half");
  // fragment registers persist across K-steps: after step() wf[1][*] and af[1][TT-DG..TT-1] hold the operands
  // of the deferred groups; the next step() consumes them before overwriting them.
  bf16x8 wf[2][NT], af[2][TT];
  // W8: the W fragments as read (8 fp8 bytes), widened into wf[ks] in front of the first MFMA group of K-sub-step ks; the
  // groups deferred past the barrier then find bf16 operands in wf[1] exactly as in the bf16 form
  u32x2 wraw[2][W8 ? NT : 1];

  __device__ __forceinline__ void widen(int ks) {
#pragma unroll
    for (int nt = 0; nt < (W8 ? NT : 0); ++nt) wf[ks][nt] = fp8x8_to_bf16x8(wraw[ks][nt]);
  }

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) wf[1][i][j] = (bf16)0.f;
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) af[1][i][j] = (bf16)0.f;
  }

  static __device__ __forceinline__ void group(const bf16x8& a, const bf16x8 (&w)[NT], f32x4 (&acc)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      acc[nt] = SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w[nt], acc[nt], 0, 0, 0)
                     : __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[nt], a, acc[nt], 0, 0, 0);
  }

  template <class IssueFn>
  __device__ __forceinline__ void step(const char* st, int wm, int wn, int lane, f32x4 (&acc)[TT][NT], IssueFn&& issue) {
    const char* wb = st + (wn * 16 * NT + (lane & 15)) * G::W_ROW_BYTES;
    const char* ab = st + G::W_STAGE_BYTES + (wm * TT * 16) * 128 + (lane & 15) * 128;
    const int koff0 = (((lane >> 4)) ^ (lane & 7)) << 4;
    const int koff1 = (((4 + (lane >> 4))) ^ (lane & 7)) << 4;
    const int kw0 = w8_koff(lane, 0), kw1 = w8_koff(lane, 1);
    auto rd = [&](int idx) {
      const int ks = idx / (NT + TT), r = idx % (NT + TT);
      const int ko = ks ? koff1 : koff0;
#ifdef LTXK_PROBE_FEWER_LDS_READS      // energy probe only (WRONG results): the ks=1 fragments are copies of the ks=0 ones
      if (ks == 1) { if (r < NT) wf[1][r] = wf[0][r]; else af[1][r - NT] = af[0][r - NT]; return; }
#endif
      if (r < NT) {
        if constexpr (W8) wraw[ks][r < NT ? r : 0] = *(const u32x2*)(wb + r * 1024 + (ks ? kw1 : kw0));
        else wf[ks][r] = *(const bf16x8*)(wb + r * 2048 + ko);
      } else af[ks][r - NT] = *(const bf16x8*)(ab + (r - NT) * 2048 + ko);
    };
    // reads needed by real group g of THIS stage (flat order W0, A0[*], W1, A1[*]); g >= NG: everything
    auto need = [](int g) { return g < 0 ? 0 : (g >= NG ? TOTAL : (g / TT) * (NT + TT) + NT + (g % TT) + 1); };
    int issued = 0;
    // virtual groups: the DG groups deferred from the previous K-step (operands already in registers)
#pragma unroll
    for (int v = 0; v < DG; ++v) {
      int target = need(v - DG + PD);
      if (target > NT + TT) target = NT + TT;        // the ks=1 registers still feed the deferred groups
#pragma unroll
      for (int i = 0; i < TOTAL; ++i)
        if (i >= issued && i < target) rd(i);
      issued = target > issued ? target : issued;
#pragma unroll
      for (int q = 0; q < PPG; ++q) issue(v * PPG + q);
      group(af[1][TT - DG + v], wf[1], acc[TT - DG + v]);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int g = 0; g < NG - DG; ++g) {
      const int target = need(g + PD);
#pragma unroll
      for (int i = 0; i < TOTAL; ++i)
        if (i >= issued && i < target) rd(i);
      issued = target > issued ? target : issued;
#pragma unroll
      for (int q = 0; q < PPG; ++q) issue((g + DG) * PPG + q);
      if constexpr (W8) {
        if (g % TT == 0) widen(g / TT);
      }
      group(af[g / TT][g % TT], wf[g / TT], acc[g % TT]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // operands of the groups deferred to the next step must leave this stage's LDS slot before the barrier
#pragma unroll
    for (int i = 0; i < TOTAL; ++i)
      if (i >= issued) rd(i);
    if constexpr (W8 && DG == TT) widen(1);            // no real group of this step used the ks=1 fragments
  }

  __device__ __forceinline__ void finish(f32x4 (&acc)[TT][NT]) {
#pragma unroll
    for (int v = 0; v < DG; ++v) group(af[1][TT - DG + v], wf[1], acc[TT - DG + v]);
  }
};

// ---- fp8 x fp8 (W8A8): the 160-row family on v_mfma_scale_f32_16x16x128_f8f6f4 ------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int GEMM_BK8 = 128;                       // k per K-step of the fp8 x fp8 forms (128-byte rows)
constexpr int E8M0_ONE_X4 = 0x7f7f7f7f;             // block scale 1.0 in every byte, whichever one op_sel picks

// The rotated pipeline of MmaPipe for one MFMA per tile and K-step: a K-step is TT groups of NT MFMAs (one A-row fragment x NT W
// fragments), each MFMA twice as long as a 16x16x32 bf16 one, so the step spends the matrix-pipe cycles of the bf16 step's 2*TT
// groups.  Every group uses ALL W fragments, so only ONE group (the last) is deferred past the next barrier: it runs on the
// previous stage's W registers while the new stage's first A fragment is in flight, and the W fragments are re-read behind it.
// A fragments are read one group ahead of their use.  The stage's LDS-DMA pieces are spread over the TT groups.  TT = 1 has
// nothing to defer: read, issue, multiply.
template <int TT, bool SWAP, int NT = 4>
struct MmaPipe8 {
  using G = GemmGeom<TT, 4, NT, false>;             // 128-byte rows in both halves: the bf16 stage's geometry
  static constexpr int DG = TT >= 2 ? 1 : 0;
  static constexpr int MAXP = G::W_PER_WAVE + G::MAXA;
  static constexpr int PPG = (MAXP + TT - 1) / TT;
  i32x8 wf[NT], af[TT];

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) wf[i][j] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) af[TT - 1][j] = 0;
  }

  static __device__ __forceinline__ void group(const i32x8& a, const i32x8 (&w)[NT], f32x4 (&acc)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      acc[nt] = SWAP ? __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, w[nt], acc[nt], 0, 0, 0, E8M0_ONE_X4, 0, E8M0_ONE_X4)
                     : __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w[nt], a, acc[nt], 0, 0, 0, E8M0_ONE_X4, 0, E8M0_ONE_X4);
  }

  template <class IssueFn>
  __device__ __forceinline__ void step(const char* st, int wm, int wn, int lane, f32x4 (&acc)[TT][NT], IssueFn&& issue) {
    const char* wb = st + (wn * 16 * NT + (lane & 15)) * 128;
    const char* ab = st + G::W_STAGE_BYTES + (wm * TT * 16 + (lane & 15)) * 128;
    const int koff0 = (((lane >> 4)) ^ (lane & 7)) << 4;
    const int koff1 = (((4 + (lane >> 4))) ^ (lane & 7)) << 4;
    auto frag = [&](const char* row) {
      const i32x4 lo = *(const i32x4*)(row + koff0), hi = *(const i32x4*)(row + koff1);
      return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    if constexpr (DG) {
      af[0] = frag(ab);
#pragma unroll
      for (int q = 0; q < PPG; ++q) issue(q);
      group(af[TT - 1], wf, acc[TT - 1]);              // deferred from the previous K-step (step 0: zeros)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[nt] = frag(wb + nt * 2048);
#pragma unroll
      for (int g = 0; g < TT - 1; ++g) {
        af[g + 1] = frag(ab + (g + 1) * 2048);         // (the last one feeds the group deferred to the next step)
#pragma unroll
        for (int q = 0; q < PPG; ++q) issue((g + 1) * PPG + q);
        group(af[g], wf, acc[g]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[nt] = frag(wb + nt * 2048);
      af[0] = frag(ab);
#pragma unroll
      for (int q = 0; q < PPG; ++q) issue(q);
      group(af[0], wf, acc[0]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  __device__ __forceinline__ void finish(f32x4 (&acc)[TT][NT]) {
    if constexpr (DG) group(af[TT - 1], wf, acc[TT - 1]);
  }
};

// ---- MXFP4 x MXFP4: the 160-row family on the same instruction with e2m1 operands (cbsz = blgp = 4) --------------------------
// A K-step is 256 k: both halves of a stage hold code bytes in 128-byte rows, so loader, ring and swizzle are again those of the
// bf16 stage.  An fp4 operand of v_mfma_scale_f32_16x16x128_f8f6f4 is 16 bytes per lane, and in the instruction's own k assignment
// lane l holds k = 32g..32g+31 (g = l >> 4) of row (l & 15): one OCP scale block, whose e8m0 byte the lane passes as its scale
// operand (byte 0 of the register, op_sel 0).  A K-step is two such MFMAs per 16x16 tile (K-sub-steps ks = 0, 1 = the row's bytes
// 0-63 and 64-127), and sub-step ks reads the 16-byte chunk 4*ks + g of row (l & 15): chunk for chunk the two ds_read_b128 of the
// bf16 form's K-sub-steps, at the same swizzled addresses (chunk ^ (row & 7)).  Bank rule: row r reads the 16 bytes at
// 128 r + 16 (c ^ (r & 7)) for its chunk c; modulo the 256 bytes of the 64 banks that is slot 8 (r & 1) + (c ^ (r & 7)) of sixteen
// 16-byte slots.  ds_read_b128 is served in four groups of 16 lanes that are NOT contiguous: {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same two shifted by 32 (MI355X_MICROARCH.md).  The first holds rows 0-3 and 12-15 at chunk
// c = 4 ks (g = 0) and rows 4-11 at chunk c + 1 = c ^ 1 (g = 1): the eight rows at chunk c have eight different r & 7, so they take
// eight different slots (the four even r & 7 in slots 0-7, the four odd ones in 8-15), and the eight rows at c ^ 1 take, half by
// half, exactly the other four - 16 lanes on 16 different slots, no conflict.  The second group is the same with the roles of the
// row sets exchanged, the last two with chunks c + 2, c + 3.  These are address for address the reads of the bf16 form, whose
// rule this restates; nothing new is swizzled.  Unlike MmaPipe8 the reads follow the nominal k assignment: its k = 16g..,
// 64+16g.. form would split a lane across two scale blocks.
//
// Scale bytes go from memory straight to registers, a K-step ahead: a lane loads the 8 bytes (the K-step's 8 blocks) of each of
// its NT W rows and TT A rows, and one v_perm_b32 per row keeps its two - block g of sub-step 0 in byte 0, of sub-step 1 in byte 1,
// which op_sel 0 / 1 then pick.  The loads are inline asm, so hipcc inserts no wait of its own for them (it does not count the
// LDS-DMA pieces and would drain them: vmcnt(0) at the first use); they are issued right after a K-step's barrier, in front of
// that step's LDS-DMA pieces, retired by a counted vmcnt at the END of the same step (everything issued behind them may stay in
// flight), and only then - through an empty asm that the values pass through - handed to the next step: no register holding an
// in-flight load is ever copied or read.
// This rests on the register allocator: between request() and settle() it must neither spill nor move nxt[] (the compiler does
// not know the registers are being written).  Nothing enforces that.  It holds in the build this was written against - the one
// instance with scratch (160 x 256, gate + residual) spills residual-band values, not these - and the exact-data tests fail if
// it ever does not; after a change of compiler or flags, re-read the assembly of the instances that reach 254-256 VGPRs.
__device__ __forceinline__ u32x2 gload8_untracked(const uint8_t* base, unsigned off) {
  u32x2 v;
  asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(v) : "v"(off), "s"(base) : "memory");
  return v;
}

template <int TT, int NT>
struct MxScales {
  static constexpr int NS = NT + TT;
  const uint8_t *wbase, *abase;       // the two scale panels (uniform)
  unsigned off[NS];                   // byte offset of this lane's row in its panel: W tiles 0..NT-1, then A tiles 0..TT-1
  unsigned sel;                       // v_perm_b32 selector: bytes g and 4 + g of a row's 8, then zeros
  unsigned cur[NS];                   // the scale operands of the K-step being multiplied
  u32x2 nxt[NS];                      // the 8 block scales per row of the next one, as loaded

  __device__ __forceinline__ void request(int kt) {
    const uint8_t* wb = wbase + (size_t)kt * 8;
    const uint8_t* ab = abase + (size_t)kt * 8;
#pragma unroll
    for (int i = 0; i < NS; ++i) nxt[i] = gload8_untracked(i < NT ? wb : ab, off[i]);
  }
  // after a wait that retired the requests
  __device__ __forceinline__ void landed() {
#pragma unroll
    for (int i = 0; i < NS; ++i) asm volatile("" : "+v"(nxt[i]));
  }
  __device__ __forceinline__ void take() {
    landed();
#pragma unroll
    for (int i = 0; i < NS; ++i) cur[i] = __builtin_amdgcn_perm(nxt[i][1], nxt[i][0], sel);
  }
  template <int KEEP>
  __device__ __forceinline__ void settle() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KEEP) : "memory");
    landed();
  }
};
struct NoScales {};

// One K-step: 2 * TT groups of NT MFMAs in the flat order of mma_stage_pipelined (W0, A0[*], W1, A1[*]), fragment reads two
// groups ahead of their use, the stage's LDS-DMA pieces spread over the groups.  Nothing is deferred past the barrier.
template <int TT, bool SWAP, int NT = 4>
struct MmaPipe4 {
  using G = GemmGeom<TT, 4, NT, false>;             // 128-byte rows in both halves: the bf16 stage's geometry
  static constexpr int NG = 2 * TT;
  static constexpr int MAXP = G::W_PER_WAVE + G::MAXA;
  static constexpr int PPG = (MAXP + NG - 1) / NG;
  static constexpr int TOTAL = 2 * (NT + TT);

  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ void finish(f32x4 (&)[TT][NT]) {}

  static __device__ __forceinline__ i32x8 widen(const i32x4& v) { return i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0}; }

  template <class IssueFn>
  __device__ __forceinline__ void step(const char* st, int wm, int wn, int lane, f32x4 (&acc)[TT][NT], IssueFn&& issue,
                                       const MxScales<TT, NT>& sc) {
    const char* wb = st + (wn * 16 * NT + (lane & 15)) * 128;
    const char* ab = st + G::W_STAGE_BYTES + (wm * TT * 16 + (lane & 15)) * 128;
    const int koff[2] = {(((lane >> 4)) ^ (lane & 7)) << 4, (((4 + (lane >> 4))) ^ (lane & 7)) << 4};
    i32x4 wf[2][NT], af[2][TT];
    auto rd = [&](int idx) {
      const int ks = idx / (NT + TT), r = idx % (NT + TT);
      if (r < NT) wf[ks][r] = *(const i32x4*)(wb + r * 2048 + koff[ks]);
      else af[ks][r - NT] = *(const i32x4*)(ab + (r - NT) * 2048 + koff[ks]);
    };
    auto need = [](int g) { return (g / TT) * (NT + TT) + NT + (g % TT) + 1; };
    int issued = 0;
#pragma unroll
    for (int i = 0; i < TOTAL; ++i)
      if (i < need(1 < NG ? 1 : 0)) { rd(i); issued = i + 1; }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int target = need(g + 2 < NG ? g + 2 : NG - 1);
#pragma unroll
      for (int i = 0; i < TOTAL; ++i)
        if (i >= issued && i < target) rd(i);
      issued = target > issued ? target : issued;
#pragma unroll
      for (int q = 0; q < PPG; ++q) issue(g * PPG + q);
      const int ks = g / TT, tt = g % TT;
      const int sa = (int)sc.cur[NT + tt];
      const i32x8 a = widen(af[ks][tt]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int sw = (int)sc.cur[nt];
        const i32x8 w = widen(wf[ks][nt]);
        // (op_sel = ks: byte ks of the scale registers; an immediate, hence the two spellings)
        if (SWAP) acc[tt][nt] = ks ? __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, w, acc[tt][nt], 4, 4, 1, sa, 1, sw)
                                   : __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, w, acc[tt][nt], 4, 4, 0, sa, 0, sw);
        else acc[tt][nt] = ks ? __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, acc[tt][nt], 4, 4, 1, sw, 1, sa)
                              : __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, acc[tt][nt], 4, 4, 0, sw, 0, sa);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
};

}  // namespace ltxk
