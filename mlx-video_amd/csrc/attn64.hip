// Unmasked attention at head dim 64 (include/ltxk.h, ltxk_flash_attn_dh64): the attention of the audio transformer
// (32 heads x 64) and of the cross-modal attentions, which ltxk_flash_attn (dh = 128) does not take.  At the audio shapes
// (T = 126 tokens, Tk <= 1024) the launch is latency-bound, so the structure is causal_attn.hip's - the plainest walk of
// attn_tile.h's tile - with one addition: the next key tile's global loads are requested before the current tile's
// products, so they fly under them.  (A ring of four tiles in flight with a double-buffered LDS image and one barrier per
// tile measured the same at all three profiled shapes - the per-tile time is the wave's own dependent chain of LDS reads,
// MFMAs and 16 v_exp_f32, not the loads - and was taken out again, as was issuing the next tile's scores ahead of the
// softmax, which measured slower: DESIGN.md 5n.)
//
// One workgroup of 4 waves per (batch, head, 64-row query tile); wave w owns query rows 16w .. 16w+15 and walks every
// 64-key tile.  Per tile the four waves stage K (64 x 64, 8 KiB) and V^T (64 x 64, 8 KiB) in LDS through registers, one
// buffer, two barriers.  Keys are never split across waves or workgroups and there is one launch form: a (batch, head)'s
// bits depend on its own data, Tq and Tk only - not on B, H or the grid.
//
// Mask: a key >= Tk is not visible (V^T pad columns may hold any finite value).
//
// Addresses: a K row past Tk is a copy of row Tk - 1 and a Q row past Tq a copy of row Tq - 1 (both masked), V^T chunks stay
// below ldvt >= Tk rounded up to 64: no load leaves its tensor.  Rows >= Tq are not stored.
#include "attn_tile.h"

namespace ltxk {

constexpr int A64_DH = 64;                        // head dim
constexpr int A64_BQ = 64;                        // query rows per workgroup (16 per wave)
constexpr int A64_K_BYTES = AT_BK * A64_DH * 2;   // 8 KiB
constexpr int A64_V_BYTES = A64_DH * AT_BK * 2;   // 8 KiB

struct A64Params {
  const bf16* q; const bf16* k; const bf16* vt; bf16* out;
  int ldq, ldk, ldvt, ldo;
  int B, H, Tq, Tk, QT;
  float c;                                        // scale * log2(e)
};

// the two 16-byte chunks of K and of V^T that this thread stages of key tile t
__device__ __forceinline__ void a64_fetch(const bf16* kbase, const bf16* vbase, int ldk, int ldvt, int Tk, int t, int tid,
                                          bf16x8 (&kr)[2], bf16x8 (&vr)[2]) {
  at_fetch_k<A64_DH>(kr, kbase, ldk, t * AT_BK, Tk, tid);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = i * 256 + tid, d = id >> 3, ch = id & 7;
    vr[i] = *(const bf16x8*)(vbase + (size_t)d * ldvt + t * AT_BK + ch * 8);         // ldvt >= 64 * tiles: inside the row
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
  const int NT = (Tk + AT_BK - 1) / AT_BK;

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
  at_zero(o);
  float mc_run = AT_NONE, l_run = 0.f;

  bf16x8 kr[2], vr[2];
  a64_fetch(kbase, vbase, p.ldk, p.ldvt, Tk, 0, tid, kr, vr);
  for (int t = 0; t < NT; ++t) {
    __syncthreads();                              // the previous tile's readers are done
    at_stage<A64_DH>(sk, sv, kr, vr, tid);
    __syncthreads();
    if (t + 1 < NT) a64_fetch(kbase, vbase, p.ldk, p.ldvt, Tk, t + 1, tid, kr, vr);      // in flight under the products below

    f32x4 s[4];
    at_scores<A64_DH>(s, qf, [&](int kb, int ks) { return at_kfrag_lds<A64_DH>(sk, kb, ks, c, g); });
    float m_tile;
    const unsigned vis = at_mask(s, t * AT_BK, g, p.c, m_tile, [&](int key) { return key < Tk; });
    bf16x8 pb[2];
    at_online(s, vis, m_tile, p.c, mc_run, l_run, o, pb);
    at_pv<A64_DH>(o, pb, [&](int db, int kc) { return at_vfrag_lds(sv, db, kc, c, g); });
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
  const int64_t tk_pad = ((int64_t)Tk + AT_BK - 1) / AT_BK * AT_BK;
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
