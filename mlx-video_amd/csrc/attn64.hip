// Unmasked attention at head dim 64 (include/ltxk.h, ltxk_flash_attn_dh64): the attention of the audio transformer
// (32 heads x 64) and of the cross-modal attentions, which ltxk_flash_attn (dh = 128) does not take.  At the audio shapes
// (T = 126 tokens, Tk <= 1024) the launch is latency-bound, so the structure is causal_attn.hip's - the plainest that is
// correct on v_mfma_f32_16x16x32_bf16 - with one addition: the next key tile's global loads are requested before the
// current tile's products, so they fly under them.  (A ring of four tiles in flight with a double-buffered LDS image and one
// barrier per tile measured the same at all three profiled shapes - the per-tile time is the wave's own dependent chain of
// LDS reads, MFMAs and 16 v_exp_f32, not the loads - and was taken out again, as was issuing the next tile's scores ahead
// of the softmax, which measured slower: DESIGN.md 5n.)
//
// One workgroup of 4 waves per (batch, head, 64-row query tile); wave w owns query rows 16w .. 16w+15 and walks every
// 64-key tile.  Per tile the four waves stage K (64 x 64, 8 KiB) and V^T (64 x 64, 8 KiB) in LDS through registers, one
// buffer, two barriers.  Keys are never split across waves or workgroups and there is one launch form: a (batch, head)'s
// bits depend on its own data, Tq and Tk only - not on B, H or the grid.
//
// Operand map: the one causal_attn.hip documents (g = lane >> 4, c = lane & 15), at two 32-channel k-steps and four
// 16-channel output blocks:
//   S^T block kb (16 keys) = K(kb) . Q^T:  A = K fragment, lane (c,g) holds key row keymap(kb, c), channels 32ks + 8g .. +7;
//     B = Q fragment, lane (c,g) holds query row c, the same channels; D register j = S^T[key keymap(kb, 4g + j)][query c].
//   keymap makes the 8 scores a lane holds of blocks 2kc, 2kc+1 the 8 contiguous keys 32kc + 8g .. +7 - the k-slots of its
//   B operand in O^T block db (16 channels) += V^T(db, kc) . P^T(kc), so P stays in registers.
//   D register j = O^T[channel 16db + 4g + j][query c]: four consecutive channels of one output row per lane.
// LDS images: rows of 128 B (8 chunks of 16 B); K row r keeps chunk ch at ch ^ (2 ((r >> 3) & 3) + ((r >> 1) & 1)), which is
// c >> 1 for r = keymap(kb, c); V^T row d keeps chunk ch at ch ^ ((d >> 1) & 7), c >> 1 for d = 16db + c: the 16 lanes of a
// fragment read differ in (row parity, chunk position), i.e. in bank group.
//
// Softmax: the "flash" rounding points of ltxk_flash_attn.  The row offset M is an INTEGER in the exp2 domain, the ceil of
// the running maximum over the keys < Tk seen so far, so bf16(P) does not depend on the tiling.  A key >= Tk takes no part
// in the maximum and its P is the constant 0 (V^T pad columns may hold any finite value).
//
// Addresses: a K row past Tk is a copy of row Tk - 1 and a Q row past Tq a copy of row Tq - 1 (both masked), V^T chunks stay
// below ldvt >= Tk rounded up to 64: no load leaves its tensor.  Rows >= Tq are not stored.
#include "common.h"

namespace ltxk {

constexpr int A64_DH = 64;                        // head dim
constexpr int A64_BQ = 64;                        // query rows per workgroup (16 per wave)
constexpr int A64_BK = 64;                        // keys per tile
constexpr int A64_K_BYTES = A64_BK * A64_DH * 2;  // 8 KiB
constexpr int A64_V_BYTES = A64_DH * A64_BK * 2;  // 8 KiB
constexpr float A64_NONE = -1e30f;                // "no key yet"

struct A64Params {
  const bf16* q; const bf16* k; const bf16* vt; bf16* out;
  int ldq, ldk, ldvt, ldo;
  int B, H, Tq, Tk, QT;
  float c;                                        // scale * log2(e)
};

__device__ __forceinline__ constexpr int a64_keymap(int kb, int r) { return 32 * (kb >> 1) + 8 * (r >> 2) + 4 * (kb & 1) + (r & 3); }
__device__ __forceinline__ int a64_kswz(int row) { return 2 * ((row >> 3) & 3) + ((row >> 1) & 1); }

// the two 16-byte chunks of K and of V^T that this thread stages of key tile t
__device__ __forceinline__ void a64_fetch(const bf16* kbase, const bf16* vbase, int ldk, int ldvt, int Tk, int t, int tid,
                                          bf16x8 (&kr)[2], bf16x8 (&vr)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = i * 256 + tid, row = id >> 3, ch = id & 7;
    int key = t * A64_BK + row;
    key = key < Tk ? key : Tk - 1;                // rows past the sequence: a copy of the last row, masked in the softmax
    kr[i] = *(const bf16x8*)(kbase + (size_t)key * ldk + ch * 8);
    vr[i] = *(const bf16x8*)(vbase + (size_t)row * ldvt + t * A64_BK + ch * 8);      // ldvt >= 64 * tiles: inside the row
  }
}

__global__ __launch_bounds__(256) void flash_attn_dh64_kernel(A64Params p) {
  __shared__ __attribute__((aligned(16))) char smem[A64_K_BYTES + A64_V_BYTES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int BH = p.B * p.H;
  const int qt = (int)(blockIdx.x / (unsigned)BH);
  const int bh = (int)(blockIdx.x % (unsigned)BH);
  const int b = bh / p.H, h = bh - b * p.H;
  const int Tq = p.Tq, Tk = p.Tk;
  const int NT = (Tk + A64_BK - 1) / A64_BK;

  const int qi = qt * A64_BQ + 16 * wave + c;     // this lane's query row
  bf16x8 qf[2];
  {
    const int qrow = qi < Tq ? qi : Tq - 1;
    const bf16* qp = p.q + ((size_t)b * Tq + qrow) * p.ldq + (size_t)h * A64_DH + g * 8;
    qf[0] = *(const bf16x8*)qp;
    qf[1] = *(const bf16x8*)(qp + 32);
  }
  const bf16* kbase = p.k + (size_t)b * Tk * p.ldk + (size_t)h * A64_DH;
  const bf16* vbase = p.vt + ((size_t)b * p.H + h) * A64_DH * p.ldvt;
  char* sk = smem;
  char* sv = smem + A64_K_BYTES;

  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[db][j] = 0.f;
  float mc_run = A64_NONE, l_run = 0.f;

  bf16x8 kr[2], vr[2];
  a64_fetch(kbase, vbase, p.ldk, p.ldvt, Tk, 0, tid, kr, vr);
  for (int t = 0; t < NT; ++t) {
    __syncthreads();                              // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int id = i * 256 + tid, row = id >> 3, ch = id & 7;
      *(bf16x8*)(sk + row * 128 + ((ch ^ a64_kswz(row)) << 4)) = kr[i];
      *(bf16x8*)(sv + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)) = vr[i];
    }
    __syncthreads();
    if (t + 1 < NT) a64_fetch(kbase, vbase, p.ldk, p.ldvt, Tk, t + 1, tid, kr, vr);      // in flight under the products below

    // ---- S^T = K . Q^T ----
    f32x4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[kb][j] = 0.f;
      const int row = a64_keymap(kb, c);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(sk + row * 128 + (((4 * ks + g) ^ (c >> 1)) << 4));
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[kb], 0, 0, 0);
      }
    }
    // ---- keys >= Tk: out of the maximum, P = 0 ----
    unsigned vis = 0;
    float mx = A64_NONE;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = t * A64_BK + 32 * (kb >> 1) + 8 * g + 4 * (kb & 1) + j;          // a64_keymap(kb, 4g + j)
        if (key < Tk) { vis |= 1u << (kb * 4 + j); mx = fmaxf(mx, s[kb][j]); }
      }
    // ---- online softmax: the key axis is registers x the four lane groups g ----
    float mxc = mx > -1e29f ? mx * p.c : A64_NONE;
    mxc = lane_xor32_max(lane_xor16_max(mxc));
    const float m_new = mxc > -1e29f ? fmaxf(mc_run, __builtin_ceilf(mxc)) : mc_run;
    if (__any(m_new != mc_run)) {
      const float alpha = __builtin_amdgcn_exp2f(mc_run - m_new);       // a power of two, 0 from A64_NONE, 1 where nothing moved
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[db][j] *= alpha;
      mc_run = m_new;
    }
    bf16x8 pb[2];
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = (vis >> (kb * 4 + j)) & 1u ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][j], p.c, -mc_run)) : 0.f;
        psum += e;
        pb[kb >> 1][(kb & 1) * 4 + j] = (bf16)e;
      }
    l_run += psum;
    // ---- O^T += V^T . P^T ----
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const char* vrow = sv + (db * 16 + c) * 128;
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const bf16x8 vf = *(const bf16x8*)(vrow + (((4 * kc + g) ^ (c >> 1)) << 4));
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[kc], o[db], 0, 0, 0);
      }
    }
  }

  // ---- O = O^T / l (Tk > 0: every row has met a key, l > 0) ----
  const float l_tot = lane_xor32_sum(lane_xor16_sum(l_run));
  if (qi < Tq) {
    bf16* orow = p.out + ((size_t)b * Tq + qi) * p.ldo + (size_t)h * A64_DH + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      bf16x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (bf16)(o[db][j] / l_tot);
      *(bf16x4*)(orow + db * 16) = v;
    }
  }
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_flash_attn_dh64(const ltxk_attn_args* a, void* stream) {
  LTXK_CHECK_ARG(a != nullptr, "ltxk_flash_attn_dh64: null args");
  const int32_t ldq = a->ldq, ldk = a->ldk, ldvt = a->ldvt, ldo = a->ldo, B = a->B, H = a->H, Tq = a->Tq, Tk = a->Tk;
  LTXK_CHECK_ARG(a->q && a->k && a->vt && a->out, "ltxk_flash_attn_dh64: null pointer");
  LTXK_CHECK_ARG(B > 0 && H > 0 && Tq > 0 && Tk > 0, "ltxk_flash_attn_dh64: bad dims");
  LTXK_CHECK_ARG(a->scale > 0.f, "ltxk_flash_attn_dh64: scale must be positive");
  LTXK_CHECK_ARG(a->q_sumsq == nullptr, "ltxk_flash_attn_dh64: no fused query preparation at head dim 64 (q_sumsq must be NULL)");
  LTXK_CHECK_ARG((int64_t)H * A64_DH <= INT32_MAX && ldq >= H * A64_DH && ldk >= H * A64_DH && ldo >= H * A64_DH, "ltxk_flash_attn_dh64: row strides < H*64");
  LTXK_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldo % 8 == 0, "ltxk_flash_attn_dh64: row strides must be multiples of 8");
  const int64_t tk_pad = ((int64_t)Tk + A64_BK - 1) / A64_BK * A64_BK;
  LTXK_CHECK_ARG(ldvt >= tk_pad && ldvt % 8 == 0, "ltxk_flash_attn_dh64: ldvt=%d must be >= %lld (Tk rounded up to 64) and a multiple of 8", ldvt, (long long)tk_pad);
  LTXK_CHECK_ARG((((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->vt | (uintptr_t)a->out) & 15) == 0, "ltxk_flash_attn_dh64: misaligned pointer");
  const int QT = (Tq + A64_BQ - 1) / A64_BQ;
  LTXK_CHECK_ARG((int64_t)QT * B * H <= INT32_MAX, "ltxk_flash_attn_dh64: too many query tiles");
  A64Params p;
  p.q = (const bf16*)a->q; p.k = (const bf16*)a->k; p.vt = (const bf16*)a->vt; p.out = (bf16*)a->out;
  p.ldq = ldq; p.ldk = ldk; p.ldvt = ldvt; p.ldo = ldo;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk; p.QT = QT;
  p.c = a->scale * 1.4426950408889634f;
  hipLaunchKernelGGL(flash_attn_dh64_kernel, dim3((unsigned)(QT * B * H)), dim3(256), 0, (hipStream_t)stream, p);
  LTXK_CHECK_LAUNCH("ltxk_flash_attn_dh64");
  return LTXK_OK;
}
