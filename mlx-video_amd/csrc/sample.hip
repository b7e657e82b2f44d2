// Token sampling of a KV-cached decode step on the device (include/ltxk.h, "Gemma-3 decoding: sampling"): the repetition
// penalty, then argmax or an inverse-CDF draw from softmax(l' / temperature), and the decode state's bookkeeping - what
// gemma.sample_tokens and the host loop around it do per token, without the logits leaving the device.
//
// A row of V bf16 logits is cut into chunks of SP_CHUNK = 2048 elements (a function of V only), a chunk into 256 threads
// of 8 consecutive elements.  Three launches, each ordered behind the one before it by the stream; no atomics and nobody waits
// for another workgroup:
//   1. sp_max_kernel,  grid (chunks, B): l' of the chunk, its maximum and the smallest index that holds it.
//   2. sp_sum_kernel,  grid (chunks, B), temperature > 0 only: the row maximum from launch 1's partials, p = exp(l'/T - m),
//      and the chunk's sum - DEFINED as the inclusive prefix of its last element under sp_scan, so that launch 3 recomputes it
//      to the bit.
//   3. sp_pick_kernel, grid (B): merges the partials in ascending chunk order (one thread, cum[c] = cum[c-1] + sum[c]),
//      S = cum[last], target = u * S, the first chunk with cum[c] > target, then rescans that one chunk for the smallest v with
//      p_v > 0 and cum[c-1] + prefix(v) > target; if rounding leaves none, the largest v with p_v > 0.  Then the bookkeeping.
//   4. sp_advance_kernel, one thread: ctl = {n + 1, pos + 1, rows not done}.  A launch of its own because every workgroup of
//      1-3, and the position readers of the step in between, read the old value.
// The longest sequential fp32 addition chain behind a prefix sum (the tests' `depth`, tests/ref_gemma_sample.py):
//   SAMPLE_DEPTH_BASE = 17 inside a chunk (7 in the thread, 6 levels of the lane scan, 2 wave offsets, thread base, element)
//   plus one per chunk for the ascending merge: depth(V) = 17 + ceil(V / 2048), 146 at V = 262208.
// The token is a function of the row's logits, its context, temperature, penalty and its uniform: nothing here reads B, another
// row or the grid.  n = ctl[0] outside [0, n_max): every launch leaves before its first store.
#include "common.h"

namespace ltxk {

constexpr int SP_THREADS = 256;
constexpr int SP_CHUNK = SP_THREADS * 8;
constexpr int SP_MAX_CTX = 64;
constexpr int SP_MAX_EOS = 8;
constexpr int SP_MAX_CHUNKS = 1024;              // sp_pick_kernel keeps a row's chunk sums in LDS
constexpr int SP_NONE = 0x7fffffff;

// The penalised context of row b into LDS: the last min(rep_ctx, hist_len[b]) ids of history[b].  Returns their count.
__device__ __forceinline__ int sp_load_ctx(const int32_t* __restrict__ history, const int32_t* __restrict__ hist_len, int b, int hcap,
                                           int rep_ctx, float penalty, int* ctx) {
  int hl = hist_len[b];
  hl = hl < 0 ? 0 : (hl > hcap ? hcap : hl);
  const int nctx = penalty == 1.0f ? 0 : (rep_ctx < hl ? rep_ctx : hl);
  if ((int)threadIdx.x < nctx) ctx[threadIdx.x] = history[(size_t)b * hcap + hl - nctx + threadIdx.x];
  __syncthreads();
  return nctx;
}

// l' of the thread's 8 elements [base, base + 8): the bf16 logits widened, an id of the context penalised ONCE however often it
// occurs there (l < 0 ? l * penalty : l / penalty; IEEE multiply, correctly rounded divide).  false past the row's end.
__device__ __forceinline__ bool sp_load(const bf16* __restrict__ row, int V, int base, const int* ctx, int nctx, float penalty, float l[8]) {
  const bool valid = base < V;                   // V % 8 == 0: a thread's 8 elements are inside or outside together
  if (valid) {
    const bf16x8 x = *(const bf16x8*)(row + base);
#pragma unroll
    for (int j = 0; j < 8; ++j) l[j] = (float)x[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) l[j] = -INFINITY;
  }
  unsigned hit = 0;
  for (int i = 0; i < nctx; ++i) {
    const unsigned d = (unsigned)(ctx[i] - base);
    if (d < 8u) hit |= 1u << d;
  }
  if (hit && valid) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if ((hit >> j) & 1u) l[j] = l[j] < 0.f ? l[j] * penalty : l[j] / penalty;
  }
  return valid;
}

// (value, index) with the larger value, on a tie the smaller index
__device__ __forceinline__ void sp_better(float& m, int& a, float m2, int a2) {
  if (m2 > m || (m2 == m && a2 < a)) { m = m2; a = a2; }
}

// the workgroup's best (value, index); every thread returns it.  red_f / red_i: 4 floats / ints of LDS
__device__ __forceinline__ void sp_wg_best(float& m, int& a, float* red_f, int* red_i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sp_better(m, a, __shfl_xor(m, d, 64), __shfl_xor(a, d, 64));
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red_f[wave] = m; red_i[wave] = a; }
  __syncthreads();
  m = red_f[0]; a = red_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) sp_better(m, a, red_f[w], red_i[w]);
}

// max l' of the row from launch 1's partials (a maximum: the order does not matter)
__device__ __forceinline__ float sp_row_max(const float* __restrict__ pmax, int nchunks, float* red_f, int* red_i) {
  float m = -INFINITY;
  int a = SP_NONE;
  for (int c = threadIdx.x; c < nchunks; c += SP_THREADS) sp_better(m, a, pmax[c], c);
  sp_wg_best(m, a, red_f, red_i);
  return m;
}

// The chunk's inclusive prefix sums, incl[j] = prefix of the thread's element j: 7 additions in the thread, the inclusive lane
// scan of the thread totals (6 levels), the waves' totals added in ascending order, base = wave offset + lanes before, and
// incl[j] = base + local[j].  wsum: 4 floats of LDS.
__device__ __forceinline__ void sp_scan(const float p[8], float incl[8], float* wsum) {
  float loc[8];
  loc[0] = p[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) loc[j] = loc[j - 1] + p[j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float x = loc[7];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  const float before = __shfl_up(x, 1, 64);      // the lanes below this one (lane 0: none)
  __syncthreads();
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  float off = 0.f;                              // (p >= 0: an addition of 0 is exact, so wave 0 / lane 0 need no case of their own)
  if (wave >= 1) off += wsum[0];
  if (wave >= 2) off += wsum[1];
  if (wave >= 3) off += wsum[2];
  const float base = off + (lane == 0 ? 0.f : before);
#pragma unroll
  for (int j = 0; j < 8; ++j) incl[j] = base + loc[j];
}

__device__ __forceinline__ bool sp_idle(const int32_t* __restrict__ ctl, int n_max, int& n) {
  n = ctl[0];
  return n < 0 || n >= n_max;
}

__global__ __launch_bounds__(SP_THREADS) void sp_max_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks,
                                                            const int32_t* __restrict__ ctl, int n_max,
                                                            const int32_t* __restrict__ history, const int32_t* __restrict__ hist_len,
                                                            int hcap, int rep_ctx, float penalty, float* __restrict__ pmax,
                                                            int32_t* __restrict__ parg) {
  __shared__ int ctx[SP_MAX_CTX];
  __shared__ float red_f[4];
  __shared__ int red_i[4];
  int n;
  if (sp_idle(ctl, n_max, n)) return;
  const int c = blockIdx.x, b = blockIdx.y;
  const int nctx = sp_load_ctx(history, hist_len, b, hcap, rep_ctx, penalty, ctx);
  const int base = c * SP_CHUNK + (int)threadIdx.x * 8;
  float l[8];
  const bool valid = sp_load(logits + (size_t)b * ld, V, base, ctx, nctx, penalty, l);
  float m = -INFINITY;
  int a = SP_NONE;
  if (valid) {
    m = l[0]; a = base;
#pragma unroll
    for (int j = 1; j < 8; ++j)
      if (l[j] > m) { m = l[j]; a = base + j; }
  }
  sp_wg_best(m, a, red_f, red_i);
  if (threadIdx.x == 0) { pmax[(size_t)b * nchunks + c] = m; parg[(size_t)b * nchunks + c] = a; }
}

// p of the thread's elements: exp(l'/T - m), 0 past the row's end
__device__ __forceinline__ void sp_probs(const float l[8], bool valid, float temperature, float m, float p[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = valid ? expf(l[j] / temperature - m) : 0.f;
}

__global__ __launch_bounds__(SP_THREADS) void sp_sum_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks,
                                                            const int32_t* __restrict__ ctl, int n_max,
                                                            const int32_t* __restrict__ history, const int32_t* __restrict__ hist_len,
                                                            int hcap, int rep_ctx, float penalty, float temperature,
                                                            const float* __restrict__ pmax, float* __restrict__ psum) {
  __shared__ int ctx[SP_MAX_CTX];
  __shared__ float red_f[4];
  __shared__ int red_i[4];
  int n;
  if (sp_idle(ctl, n_max, n)) return;
  const int c = blockIdx.x, b = blockIdx.y;
  const int nctx = sp_load_ctx(history, hist_len, b, hcap, rep_ctx, penalty, ctx);
  const float m = sp_row_max(pmax + (size_t)b * nchunks, nchunks, red_f, red_i) / temperature;     // max of l'/T: the division is monotone
  const int base = c * SP_CHUNK + (int)threadIdx.x * 8;
  float l[8], p[8], incl[8];
  const bool valid = sp_load(logits + (size_t)b * ld, V, base, ctx, nctx, penalty, l);
  sp_probs(l, valid, temperature, m, p);
  sp_scan(p, incl, red_f);
  if (threadIdx.x == SP_THREADS - 1) psum[(size_t)b * nchunks + c] = incl[7];
}

__global__ __launch_bounds__(SP_THREADS) void sp_pick_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks, int B,
                                                             const int32_t* __restrict__ ctl, int n_max, int32_t* __restrict__ done,
                                                             int32_t* __restrict__ next_ids, int32_t* __restrict__ history,
                                                             int32_t* __restrict__ hist_len, int hcap, int rep_ctx,
                                                             int32_t* __restrict__ tokens_out, const int32_t* __restrict__ eos, int n_eos,
                                                             const float* __restrict__ uniforms, float penalty, float temperature,
                                                             const float* __restrict__ pmax, const int32_t* __restrict__ parg,
                                                             const float* __restrict__ psum) {
  __shared__ int ctx[SP_MAX_CTX];
  __shared__ float red_f[4];
  __shared__ int red_i[4];
  __shared__ float sums[SP_MAX_CHUNKS];
  __shared__ float sel_f[2];                     // cum[c_sel - 1], target
  __shared__ int sel_c;
  int n;
  if (sp_idle(ctl, n_max, n)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  pmax += (size_t)b * nchunks; parg += (size_t)b * nchunks; psum += (size_t)b * nchunks;
  int tok;
  if (temperature == 0.f) {                      // the smallest v with l'_v = max l'
    float m = -INFINITY;
    int a = SP_NONE;
    for (int c = tid; c < nchunks; c += SP_THREADS) sp_better(m, a, pmax[c], parg[c]);
    sp_wg_best(m, a, red_f, red_i);
    tok = a;
  } else {
    const int nctx = sp_load_ctx(history, hist_len, b, hcap, rep_ctx, penalty, ctx);
    const float m = sp_row_max(pmax, nchunks, red_f, red_i) / temperature;
    for (int c = tid; c < nchunks; c += SP_THREADS) sums[c] = psum[c];
    __syncthreads();
    if (tid == 0) {                              // the ascending merge: one chain of nchunks - 1 additions
      float S = 0.f;
      for (int c = 0; c < nchunks; ++c) S += sums[c];
      const float target = uniforms[(size_t)n * B + b] * S;
      float cum = 0.f, below = 0.f;
      int c_sel = -1, c_last = 0;
      for (int c = 0; c < nchunks; ++c) {
        const float prev = cum;
        cum += sums[c];
        if (sums[c] > 0.f) c_last = c;
        if (c_sel < 0 && cum > target) { c_sel = c; below = prev; }
      }
      if (c_sel < 0) {                           // rounding left no chunk: the last one that holds a p > 0, and nothing exceeds
        sel_c = c_last; sel_f[0] = 0.f; sel_f[1] = INFINITY;
      } else {
        sel_c = c_sel; sel_f[0] = below; sel_f[1] = target;
      }
    }
    __syncthreads();
    const int c = sel_c;
    const float below = sel_f[0], target = sel_f[1];
    const int base = c * SP_CHUNK + tid * 8;
    float l[8], p[8], incl[8];
    const bool valid = sp_load(logits + (size_t)b * ld, V, base, ctx, nctx, penalty, l);
    sp_probs(l, valid, temperature, m, p);
    sp_scan(p, incl, red_f);
    int first = SP_NONE, last = -1;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
      if (p[j] > 0.f) {
        if (last < 0) last = base + j;
        if (below + incl[j] > target) first = base + j;
      }
    }
    // the smallest `first` and the largest `last` of the workgroup (equal values: sp_wg_best keeps the smaller index)
    float same = 0.f;
    sp_wg_best(same, first, red_f, red_i);
    int neg_last = -last;
    sp_wg_best(same, neg_last, red_f, red_i);
    tok = first != SP_NONE ? first : -neg_last;
  }
  tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);  // (a row of NaNs has no maximum: the id stays one embed_rows may gather)
  __syncthreads();                               // every read of history[b] above is done
  if (tid == 0) {
    if (done[b]) {
      tokens_out[(size_t)b * n_max + n] = -1;    // a finished row keeps feeding next_ids[b], as the host loop does
    } else {
      tokens_out[(size_t)b * n_max + n] = tok;
      next_ids[b] = tok;
      const int hl = hist_len[b];
      if (hl >= 0 && hl < hcap) { history[(size_t)b * hcap + hl] = tok; hist_len[b] = hl + 1; }
      int fin = 0;
      for (int i = 0; i < n_eos; ++i) fin |= eos[i] == tok;
      done[b] = fin;
    }
  }
}

__global__ void sp_advance_kernel(int32_t* __restrict__ ctl, int n_max, const int32_t* __restrict__ done, int B) {
  if (threadIdx.x != 0) return;
  const int n = ctl[0];
  if (n < 0 || n >= n_max) return;
  int live = 0;
  for (int b = 0; b < B; ++b) live += done[b] == 0;
  const int pos = ctl[1];
  ctl[0] = n + 1; ctl[1] = pos + 1; ctl[2] = live;
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_sample_rows(const ltxk_sample_args* a, void* stream) {
  const char* who = "ltxk_sample_rows";
  LTXK_CHECK_ARG(a && a->struct_bytes == (int32_t)sizeof(ltxk_sample_args), "%s: struct_bytes does not match this build's ltxk_sample_args (%d)",
                 who, (int)sizeof(ltxk_sample_args));
  LTXK_CHECK_ARG((a->flags & ~(LTXK_SAMPLE_DRAW | LTXK_SAMPLE_ADVANCE)) == 0 && a->flags != 0, "%s: flags=%d must be DRAW, ADVANCE or both", who, a->flags);
  LTXK_CHECK_ARG(a->ctl && a->done && ((uintptr_t)a->ctl & 3) == 0 && ((uintptr_t)a->done & 3) == 0, "%s: ctl / done: null or misaligned pointer", who);
  LTXK_CHECK_ARG(a->B >= 1 && a->B <= 8 && a->n_max >= 1, "%s: B=%d must lie in [1, 8], n_max=%d must be positive", who, a->B, a->n_max);
  hipStream_t s = (hipStream_t)stream;
  if (a->flags & LTXK_SAMPLE_DRAW) {
    LTXK_CHECK_ARG(a->logits && a->next_ids && a->history && a->hist_len && a->tokens_out && a->workspace, "%s: null pointer", who);
    LTXK_CHECK_ARG(a->V >= 8 && a->V % 8 == 0 && a->ld >= a->V && a->ld % 8 == 0 && ((uintptr_t)a->logits & 15) == 0,
                   "%s: V=%d must be a positive multiple of 8, ld=%d >= V a multiple of 8, logits 16-byte aligned", who, a->V, a->ld);
    const int nchunks = (a->V + SP_CHUNK - 1) / SP_CHUNK;
    LTXK_CHECK_ARG(nchunks <= SP_MAX_CHUNKS, "%s: V=%d is more than %d chunks of %d", who, a->V, SP_MAX_CHUNKS, SP_CHUNK);
    LTXK_CHECK_ARG(a->hist_cap >= 1 && a->rep_ctx >= 0 && a->rep_ctx <= SP_MAX_CTX, "%s: hist_cap=%d must be positive, rep_ctx=%d in [0, %d]", who,
                   a->hist_cap, a->rep_ctx, SP_MAX_CTX);
    LTXK_CHECK_ARG(a->n_eos >= 0 && a->n_eos <= SP_MAX_EOS && (a->n_eos == 0 || a->eos), "%s: n_eos=%d must lie in [0, %d], with eos", who, a->n_eos, SP_MAX_EOS);
    LTXK_CHECK_ARG(a->temperature >= 0.f && a->temperature < INFINITY && a->penalty > 0.f && a->penalty < INFINITY,
                   "%s: temperature must be >= 0 and penalty positive, both finite", who);
    LTXK_CHECK_ARG(a->temperature == 0.f || a->uniforms, "%s: temperature > 0 needs uniforms", who);
    LTXK_CHECK_ARG((((uintptr_t)a->next_ids | (uintptr_t)a->history | (uintptr_t)a->hist_len | (uintptr_t)a->tokens_out | (uintptr_t)a->eos |
                     (uintptr_t)a->uniforms | (uintptr_t)a->workspace) & 3) == 0, "%s: misaligned pointer", who);
    const int64_t need = (int64_t)3 * a->B * nchunks * 4;
    LTXK_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace holds %lld bytes, %lld needed (3 * B * chunks * 4)", who,
                   (long long)a->workspace_bytes, (long long)need);
    float* pmax = (float*)a->workspace;
    int32_t* parg = (int32_t*)(pmax + (size_t)a->B * nchunks);
    float* psum = (float*)(parg + (size_t)a->B * nchunks);
    const bf16* lg = (const bf16*)a->logits;
    hipLaunchKernelGGL(sp_max_kernel, dim3(nchunks, a->B), dim3(SP_THREADS), 0, s, lg, a->ld, a->V, nchunks, a->ctl, a->n_max, a->history,
                       a->hist_len, a->hist_cap, a->rep_ctx, a->penalty, pmax, parg);
    LTXK_CHECK_LAUNCH(who);
    if (a->temperature != 0.f) {
      hipLaunchKernelGGL(sp_sum_kernel, dim3(nchunks, a->B), dim3(SP_THREADS), 0, s, lg, a->ld, a->V, nchunks, a->ctl, a->n_max, a->history,
                         a->hist_len, a->hist_cap, a->rep_ctx, a->penalty, a->temperature, pmax, psum);
      LTXK_CHECK_LAUNCH(who);
    }
    hipLaunchKernelGGL(sp_pick_kernel, dim3(a->B), dim3(SP_THREADS), 0, s, lg, a->ld, a->V, nchunks, a->B, a->ctl, a->n_max, a->done, a->next_ids,
                       a->history, a->hist_len, a->hist_cap, a->rep_ctx, a->tokens_out, a->eos, a->n_eos, a->uniforms, a->penalty,
                       a->temperature, pmax, parg, psum);
    LTXK_CHECK_LAUNCH(who);
  }
  if (a->flags & LTXK_SAMPLE_ADVANCE) {
    hipLaunchKernelGGL(sp_advance_kernel, dim3(1), dim3(64), 0, s, a->ctl, a->n_max, a->done, a->B);
    LTXK_CHECK_LAUNCH(who);
  }
  return LTXK_OK;
}
