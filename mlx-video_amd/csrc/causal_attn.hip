// Causal, left-padding-aware, grouped-query attention at head dim 256 (include/ltxk.h, "Gemma-3 text encoder"): the one
// attention shape of a Gemma-3 forward, which ltxk_flash_attn (dh = 128, no mask, one K/V head per query head) does not take.
// It runs once per prompt (T <= 1024, 48 layers), so the structure is the plainest walk of attn_tile.h's tile; none of
// fa_body16's pipelining is ported.
//
// One workgroup of 4 waves per (batch, query head, 64-row query tile); wave w owns query rows 16w .. 16w+15 and walks the
// 64-key tiles [t0, t1] that hold a visible key for some row of the tile - tiles wholly below row_start / the window or above
// the tile's last row are never fetched, and a query tile wholly inside the padding only stores zeros.  Per tile the four waves
// stage K (64 x 256, 32 KiB) and V^T (256 x 64, 32 KiB) in LDS through registers, one buffer, two barriers: two workgroups
// share a CU's 160 KiB, so one's loads run under the other's MFMAs.  Keys are never split across workgroups or waves: a
// row's sums depend on (row_start, window, T) and its own head's data only.
//
// Mask: key j is visible to query i iff row_start <= j <= i and (no window or i - j < window); a row whose window starts in
// a later tile has met no visible key yet.  The Q fragments stay in registers for the whole kernel; every K and V^T
// fragment is one ds_read_b128.
#include "attn_tile.h"

namespace ltxk {

constexpr int CA_DH = 256;                       // head dim
constexpr int CA_BQ = 64;                        // query rows per workgroup (16 per wave)
constexpr int CA_K_BYTES = AT_BK * CA_DH * 2;    // 32 KiB
constexpr int CA_V_BYTES = CA_DH * AT_BK * 2;    // 32 KiB
constexpr int CA_LDS = CA_K_BYTES + CA_V_BYTES;

struct CaParams {
  const bf16* q; const bf16* k; const bf16* vt; bf16* out;
  const int32_t* row_start;
  int ldq, ldk, ldvt, ldo;
  int B, Hq, Hkv, T, window, QT;
  float c;                                       // scale * log2(e)
};

// Two waves per SIMD = two workgroups per CU: without the hint the compiler takes 224 VGPRs + 80 AGPRs and one workgroup owns the
// CU; with it 223 VGPRs, no AGPRs, nothing spilled.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void causal_attn_kernel(CaParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  // the last (longest) query tiles of every (batch, head) first
  const int BH = p.B * p.Hq;
  const int qt = p.QT - 1 - (int)(blockIdx.x / (unsigned)BH);
  const int bh = (int)(blockIdx.x % (unsigned)BH);
  const int b = bh / p.Hq, h = bh - b * p.Hq;
  const int hk = h / (p.Hq / p.Hkv);
  const int T = p.T;
  int rs = p.row_start[b];
  rs = rs < 0 ? 0 : (rs > T ? T : rs);
  const int q0 = qt * CA_BQ;
  const int q1 = min(q0 + CA_BQ - 1, T - 1);
  bf16* obase = p.out + (size_t)b * T * p.ldo + (size_t)h * CA_DH;

  if (q1 < rs) {                                 // the whole tile is padding: zero rows, nothing read
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (bf16)0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int id = i * 256 + tid, row = q0 + (id >> 5), ch = id & 31;
      if (row < T) *(bf16x8*)(obase + (size_t)row * p.ldo + ch * 8) = z;
    }
    return;
  }
  // key tiles that hold a visible key of some valid row of this query tile
  const int qlo = max(q0, rs);
  int klo = rs;
  if (p.window > 0) klo = max(klo, qlo - p.window + 1);
  const int t0 = klo / AT_BK, t1 = q1 / AT_BK;

  const int qi = q0 + 16 * wave + c;             // this lane's query row
  bf16x8 qf[8];
  {
    const int qrow = qi < T ? qi : T - 1;
    const bf16* qp = p.q + ((size_t)b * T + qrow) * p.ldq + (size_t)h * CA_DH + g * 8;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 32);
  }
  const bf16* kbase = p.k + (size_t)b * T * p.ldk + (size_t)hk * CA_DH;
  const bf16* vbase = p.vt + ((size_t)b * p.Hkv + hk) * CA_DH * p.ldvt;
  char* sk = smem;
  char* sv = smem + CA_K_BYTES;

  f32x4 o[16];
  at_zero(o);
  float mc_run = AT_NONE, l_run = 0.f;

  for (int t = t0; t <= t1; ++t) {
    // ---- stage the tile: 2048 16-byte chunks of K and of V^T, 8 + 8 per thread ----
    bf16x8 kr[8], vr[8];
    at_fetch_k<CA_DH>(kr, kbase, p.ldk, t * AT_BK, T, tid);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int id = i * 256 + tid, d = id >> 3, ch = id & 7;
      const int col = t * AT_BK + ch * 8;
      if (col < p.ldvt) vr[i] = *(const bf16x8*)(vbase + (size_t)d * p.ldvt + col);      // ldvt % 8 == 0: the chunk is inside the row
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) vr[i][j] = (bf16)0.f;
      }
    }
    __syncthreads();                             // the previous tile's readers are done
    at_stage<CA_DH>(sk, sv, kr, vr, tid);
    __syncthreads();

    f32x4 s[4];
    at_scores<CA_DH>(s, qf, [&](int kb, int ks) { return at_kfrag_lds<CA_DH>(sk, kb, ks, c, g); });
    float m_tile;
    const unsigned vis = at_mask(s, t * AT_BK, g, p.c, m_tile, [&](int key) {
      return key >= rs && key <= qi && qi < T && (p.window == 0 || qi - key < p.window);
    });
    bf16x8 pb[2];
    at_online(s, vis, m_tile, p.c, mc_run, l_run, o, pb);
    at_pv<CA_DH>(o, pb, [&](int db, int kc) { return at_vfrag_lds(sv, db, kc, c, g); });
  }

  // ---- O = O^T / l; a row without a visible key (a padded query row) is all zeros ----
  const float l_tot = lane_xor32_sum(lane_xor16_sum(l_run));
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  if (qi < T) {
    bf16* orow = obase + (size_t)qi * p.ldo + 4 * g;
#pragma unroll
    for (int db = 0; db < 16; ++db) {
      bf16x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = l_tot > 0.f ? (bf16)(o[db][j] * inv) : (bf16)0.f;
      *(bf16x4*)(orow + db * 16) = v;
    }
  }
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_causal_attn_args_sizeof(void) { return (int)sizeof(ltxk_causal_attn_args); }

extern "C" int ltxk_causal_attn(const ltxk_causal_attn_args* a, void* stream) {
  LTXK_CHECK_ARG(a != nullptr, "ltxk_causal_attn: null args");
  LTXK_CHECK_ARG(a->q && a->k && a->vt && a->out && a->row_start, "ltxk_causal_attn: null pointer");
  const int32_t B = a->B, Hq = a->Hq, Hkv = a->Hkv, T = a->T;
  LTXK_CHECK_ARG(B > 0 && Hq > 0 && Hkv > 0 && T > 0, "ltxk_causal_attn: bad dims B=%d Hq=%d Hkv=%d T=%d", B, Hq, Hkv, T);
  LTXK_CHECK_ARG(Hq % Hkv == 0, "ltxk_causal_attn: Hq=%d must be a multiple of Hkv=%d", Hq, Hkv);
  LTXK_CHECK_ARG(a->scale > 0.f, "ltxk_causal_attn: scale must be positive");
  LTXK_CHECK_ARG(a->window >= 0, "ltxk_causal_attn: window=%d must be 0 (none) or a positive count", a->window);
  LTXK_CHECK_ARG((int64_t)Hq * CA_DH <= INT32_MAX && a->ldq >= Hq * CA_DH && a->ldo >= Hq * CA_DH && a->ldk >= Hkv * CA_DH,
                 "ltxk_causal_attn: row strides must be >= Hq*256 (q, out) and >= Hkv*256 (k)");
  LTXK_CHECK_ARG(a->ldq % 8 == 0 && a->ldk % 8 == 0 && a->ldo % 8 == 0, "ltxk_causal_attn: row strides must be multiples of 8");
  LTXK_CHECK_ARG(a->ldvt >= T && a->ldvt % 8 == 0, "ltxk_causal_attn: ldvt=%d must be >= T=%d and a multiple of 8", a->ldvt, T);
  LTXK_CHECK_ARG((((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->vt | (uintptr_t)a->out) & 15) == 0 && ((uintptr_t)a->row_start & 3) == 0,
                 "ltxk_causal_attn: q, k, vt, out must be 16-byte aligned");
  const int QT = (T + CA_BQ - 1) / CA_BQ;
  LTXK_CHECK_ARG((int64_t)QT * B * Hq <= INT32_MAX, "ltxk_causal_attn: too many query tiles");
  CaParams p;
  p.q = (const bf16*)a->q; p.k = (const bf16*)a->k; p.vt = (const bf16*)a->vt; p.out = (bf16*)a->out;
  p.row_start = a->row_start;
  p.ldq = a->ldq; p.ldk = a->ldk; p.ldvt = a->ldvt; p.ldo = a->ldo;
  p.B = B; p.Hq = Hq; p.Hkv = Hkv; p.T = T; p.window = a->window; p.QT = QT;
  p.c = a->scale * 1.4426950408889634f;
  static std::atomic<uint64_t> attr_set{0};
  const int rc = ensure_dyn_lds((const void*)causal_attn_kernel, CA_LDS, attr_set, "ltxk_causal_attn");
  if (rc != LTXK_OK) return rc;
  hipLaunchKernelGGL(causal_attn_kernel, dim3((unsigned)(QT * B * Hq)), dim3(256), CA_LDS, (hipStream_t)stream, p);
  LTXK_CHECK_LAUNCH("ltxk_causal_attn");
  return LTXK_OK;
}
