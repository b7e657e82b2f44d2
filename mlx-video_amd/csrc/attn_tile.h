// One 64-key attention tile on v_mfma_f32_16x16x32_bf16: the arithmetic and the rounding points that attn64.hip,
// causal_attn.hip and causal_attn_step.hip share (the tests' float64 bounds rest on them), in pieces that keep no state
// and decide nothing: how operands reach the MFMA, which keys are visible, the grid and the addresses are each kernel's.
//
// Operand map (the one of fa_body16 in attention.hip; g = lane >> 4, c = lane & 15), head dim DH:
//   S^T block kb (16 keys) = K(kb) . Q^T over DH/32 k-steps of 32 channels:
//     A = K fragment : lane (c,g) holds key row keymap(kb, c), channels 32ks + 8g .. +7
//     B = Q fragment : lane (c,g) holds query row c, the same channels
//     D : lane (c,g) register j = S^T[key keymap(kb, 4g + j)][query c]
//   keymap(kb, r) = 32 (kb >> 1) + 8 (r >> 2) + 4 (kb & 1) + (r & 3): the 8 scores a lane holds of blocks 2kc, 2kc+1 are the
//   8 CONTIGUOUS keys 32kc + 8g .. +7 - exactly the k-slots of its B operand in
//   O^T block db (16 channels) += V^T(db, kc) . P^T(kc), A = V^T fragment: lane (c,g) holds channel 16db + c, keys 32kc + 8g .. +7,
//   so P goes from the softmax to the matrix pipe in registers.
//   D : lane (c,g) register j = O^T[channel 16db + 4g + j][query c] - four consecutive channels of one output row per lane.
// LDS images (the kernels that stage a tile, workgroups of 256 threads, DH = 64 or 256): K rows of 2 DH bytes with 16-byte
// chunk ch at position ch ^ at_kswz<DH>(c) for row = keymap(kb, c) - c itself in the 32-chunk rows of DH = 256, c >> 1 in the
// 8-chunk rows of DH = 64; V^T rows of 128 B with chunk ch at ch ^ ((d >> 1) & 7).  The 16 lanes of a fragment read differ
// in bank group.
//
// Softmax: the "flash" rounding points of ltxk_flash_attn.  The row offset M is an INTEGER in the exp2 domain, the ceil of
// the maximum over the VISIBLE keys seen so far (raised whenever a tile exceeds it: no deferral), so every rescale
// 2^(M_old - M) is exact and bf16(P) does not depend on the tiling.  A key that is not visible takes no part in the maximum
// and its P is the constant 0, not exp2 of a large negative number: a row that has met no visible key keeps M = AT_NONE,
// l = 0, O = 0, and what V^T holds in that key's column does not matter as long as it is finite.
#pragma once
#include "common.h"

namespace ltxk {

constexpr int AT_BK = 64;                        // keys per tile
constexpr float AT_NONE = -1e30f;                // "no visible key yet"; every real offset is > -1e29

__device__ __forceinline__ constexpr int at_keymap(int kb, int r) { return 32 * (kb >> 1) + 8 * (r >> 2) + 4 * (kb & 1) + (r & 3); }

template <int N>
__device__ __forceinline__ void at_zero(f32x4 (&o)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[n][j] = 0.f;
}

// ---- the swizzled LDS image of a tile: K [64][DH] at sk, V^T [DH][64] at sv, DH/32 chunks of each per thread of 256 ----
template <int DH>
__device__ __forceinline__ int at_kswz(int c) {
  static_assert(DH == 64 || DH == 256, "the two staged head dims: the swizzle is not derived for another row width");
  return DH == 256 ? c : c >> 1;
}
__device__ __forceinline__ int at_keyrow_c(int row) { return 4 * ((row >> 3) & 3) + (row & 3); }      // c of row = keymap(kb, c)

// this thread's chunks of K rows key0 .. key0 + 63; a row past the sequence is a copy of row Tk - 1, for the caller to mask
template <int DH>
__device__ __forceinline__ void at_fetch_k(bf16x8 (&kr)[DH / 32], const bf16* kbase, int ldk, int key0, int Tk, int tid) {
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    const int id = i * 256 + tid, row = id / (DH / 8), ch = id % (DH / 8);
    int key = key0 + row;
    key = key < Tk ? key : Tk - 1;
    kr[i] = *(const bf16x8*)(kbase + (size_t)key * ldk + ch * 8);
  }
}

// kr as fetched above; vr[i] = chunk ch = id & 7 (keys key0 + 8ch .. +7) of V^T channel row d = id >> 3, id = 256 i + tid
template <int DH>
__device__ __forceinline__ void at_stage(char* sk, char* sv, const bf16x8 (&kr)[DH / 32], const bf16x8 (&vr)[DH / 32], int tid) {
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    const int id = i * 256 + tid, row = id / (DH / 8), ch = id % (DH / 8);
    *(bf16x8*)(sk + row * (2 * DH) + ((ch ^ at_kswz<DH>(at_keyrow_c(row))) << 4)) = kr[i];
  }
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    const int id = i * 256 + tid, d = id >> 3, ch = id & 7;
    *(bf16x8*)(sv + d * 128 + ((ch ^ ((d >> 1) & 7)) << 4)) = vr[i];
  }
}

template <int DH>
__device__ __forceinline__ bf16x8 at_kfrag_lds(const char* sk, int kb, int ks, int c, int g) {
  return *(const bf16x8*)(sk + at_keymap(kb, c) * (2 * DH) + (((4 * ks + g) ^ at_kswz<DH>(c)) << 4));
}
__device__ __forceinline__ bf16x8 at_vfrag_lds(const char* sv, int db, int kc, int c, int g) {
  const int d = db * 16 + c;
  return *(const bf16x8*)(sv + d * 128 + (((4 * kc + g) ^ ((d >> 1) & 7)) << 4));
}

// ---- S^T = K . Q^T: kfrag(kb, ks) is the A fragment of key block kb, k-step ks ----
template <int DH, class KFrag>
__device__ __forceinline__ void at_scores(f32x4 (&s)[4], const bf16x8 (&qf)[DH / 32], KFrag kfrag) {
  at_zero(s);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int ks = 0; ks < DH / 32; ++ks) s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kb, ks), qf[ks], s[kb], 0, 0, 0);
}

// ---- mask: bit 4kb + j of the result says that visible(key of s[kb][j]); m_tile = the tile's row offset, the ceil of the
// maximum of c * score over the row's visible keys (registers x the four lane groups g), AT_NONE when it has none ----
template <class Visible>
__device__ __forceinline__ unsigned at_mask(const f32x4 (&s)[4], int key0, int g, float c, float& m_tile, Visible visible) {
  unsigned vis = 0;
  float mx = AT_NONE;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (visible(key0 + 8 * g + at_keymap(kb, j))) {            // at_keymap(kb, 4g + j)
        vis |= 1u << (kb * 4 + j);
        mx = fmaxf(mx, s[kb][j]);
      }
  float mxc = mx > -1e29f ? mx * c : AT_NONE;
  mxc = lane_xor32_max(lane_xor16_max(mxc));
  m_tile = mxc > -1e29f ? __builtin_ceilf(mxc) : AT_NONE;
  return vis;
}

// ---- P = exp2(c s - M) where visible, the constant 0 where not, as bf16 in the B operand's k-slots; returns this lane's
// sum of the un-rounded P ----
__device__ __forceinline__ float at_probs(const f32x4 (&s)[4], unsigned vis, float c, float M, bf16x8 (&pb)[2]) {
  float psum = 0.f;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float e = (vis >> (kb * 4 + j)) & 1u ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][j], c, -M)) : 0.f;
      psum += e;
      pb[kb >> 1][(kb & 1) * 4 + j] = (bf16)e;
    }
  return psum;
}

// ---- online softmax over a walk of tiles: raise the running offset to the tile's, rescale l and O^T, add the tile's P ----
template <int NB>
__device__ __forceinline__ void at_online(const f32x4 (&s)[4], unsigned vis, float m_tile, float c, float& m_run, float& l_run,
                                          f32x4 (&o)[NB], bf16x8 (&pb)[2]) {
  const float m_new = m_tile > -1e29f ? fmaxf(m_run, m_tile) : m_run;
  if (__any(m_new != m_run)) {
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);        // a power of two, 0 from AT_NONE, 1 where nothing moved
    l_run *= alpha;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[db][j] *= alpha;
    m_run = m_new;
  }
  l_run += at_probs(s, vis, c, m_run, pb);
}

// ---- O^T += V^T . P^T: vfrag(db, kc) is the A fragment of channel block db, 32-key chunk kc ----
template <int DH, class VFrag>
__device__ __forceinline__ void at_pv(f32x4 (&o)[DH / 16], const bf16x8 (&pb)[2], VFrag vfrag) {
#pragma unroll
  for (int db = 0; db < DH / 16; ++db)
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfrag(db, kc), pb[kc], o[db], 0, 0, 0);
}

}  // namespace ltxk
