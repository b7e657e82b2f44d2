/*
 * ltxk.h — C ABI of libltxk.so: the MI355X (gfx950) kernels behind the LTX-2 denoise step
 * (DiT forward + step algebra) and the causal-3D-conv video VAE.
 *
 * The reference (CharafChnioune/mlx-video) has no FFI of its own; its seams are Python
 * callables that hand every numeric op to MLX built-ins.  Each entry point below replaces
 * one of those MLX call sites (file:line relative to the reference root).  Host code that
 * sits where LTXModel.__call__ (mlx_video/models/ltx/ltx.py:459), LTX2VideoDecoder.__call__
 * (video_vae/decoder.py:361) and VideoEncoder.__call__ (video_vae/video_vae.py:321) sit
 * calls these through ctypes.
 *
 * Conventions
 *   - the caller owns every buffer; the library never allocates, frees or retains memory;
 *   - all pointers are device pointers unless noted; activations/weights are bf16,
 *     side tables fp32, indices int32;
 *   - token tensors are row-major (tokens, dim); volumes are channels-last (B,D,H,W,C);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and re-entrant across streams and threads;
 *   - no state influences a result or a launch form: both are functions of the arguments and of
 *     the current device alone.  The only process-wide state is one idempotent bit per (kernel,
 *     device), "the dynamic-LDS attribute of this kernel is set", and the thread-local error string;
 *   - returns 0 on success, a negative LTXK_E* code on error; ltxk_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.
 */
#ifndef LTXK_H
#define LTXK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTXK_VERSION 412

#define LTXK_OK 0
#define LTXK_EINVAL (-1)   /* bad argument (shape / alignment / null pointer) */
#define LTXK_ELAUNCH (-2)  /* HIP launch error */

int ltxk_version(void);
const char* ltxk_last_error(void);
/* sizeof the argument structs in THIS build: 0 = ltxk_gemm_args, 1 = ltxk_conv3d_args, 2 = ltxk_attn_args,
 * 3 = struct ltxk_gemm_plan, 4 = ltxk_step_args; anything else returns -1;
 * lets a foreign-language binding verify its struct layout before the first call.        */
int ltxk_abi_sizeof(int which);

/* ---------------------------------------------------------------------------------------
 * GEMM with fused epilogue: replaces nn.Linear (mlx x@W.T+b) at attention.py:123-126,142,
 * feed_forward.py:35-40, adaln.py:46,134-138, text_projection.py, ltx.py:130,455.
 * out = epi(A[M,K] @ W[N,K]^T + bias[N]); fp32 accumulate on MFMA; bf16 rounding is applied
 * at every point where the reference materialises a bf16 array.
 * ------------------------------------------------------------------------------------- */
enum {
  LTXK_EPI_BIAS = 0,          /* y = bf16(acc + b)                                        */
  LTXK_EPI_BIAS_GELU = 1,     /* bf16(gelu_tanh(y))          feed_forward.py:12           */
  LTXK_EPI_BIAS_SILU = 2,     /* bf16(y*sigmoid(y))          adaln.py:136                 */
  LTXK_EPI_BIAS_GATE_RES = 3, /* bf16(res + bf16(y*gate))    transformer.py:254,347       */
  LTXK_EPI_BIAS_RES = 4,      /* bf16(res + y)               transformer.py:257           */
  LTXK_EPI_SCALE_RES = 5      /* bf16(res + bf16(alpha*acc)) LoRA merge W += s*(B@A), lora.py:94-127 */
};

typedef struct ltxk_gemm_args {
  const void* A;        /* (M,K) bf16, row stride lda elements                            */
  const void* W;        /* (N,K) bf16, row-major (nn.Linear weight layout)                */
  const void* bias;     /* (N) bf16 or NULL                                               */
  void* out;            /* (M,N) bf16 row stride ldo; or see out_tokens_per_batch         */
  const void* resid;    /* (M,N) bf16 row stride ldr, for *_RES epilogues                 */
  const void* gate;     /* gate value for row m, col n: gate[gate_row[m]*gate_stride + n] */
  const int32_t* gate_row; /* (M) int32 or NULL (=> row 0)                                */
  int32_t M, N, K;
  int32_t lda, ldo, ldr, gate_stride;
  int32_t epilogue;
  /* >0: write the output transposed per batch: row m = b*T + t goes to
   * out[(b*N + n)*ldo + t]   (used for V^T so that attention reads V k-contiguous)       */
  int32_t out_tokens_per_batch;
  float alpha;          /* LTXK_EPI_SCALE_RES only                                        */
  /* Split output (n_split > 0, a multiple of 256; EPI_BIAS): columns [0,n_split) go row-major to `out` (ldo), columns
   * [n_split,N) transposed per batch to out2[(b*(N-n_split) + n-n_split)*ldo2 + t] with T = out_tokens_per_batch.
   * One launch then produces q|k row-major and V^T (attention.py:123-125 as one GEMM over the packed to_q|to_k|to_v
   * panel), or the text-side k and V^T.                                                   */
  void* out2;
  int32_t n_split, ldo2;
  /* Optional (row-major columns only): sumsq[m*sumsq_ld + n/64] = sum over the 64-column block of the squares of the
   * bf16 values stored for row m (fp32, fixed summation order).  Lets the consumer of this output (rms_norm,
   * utils.py:398-400; q/k RMSNorm, attention.py:129-131) take its row statistic without re-reading the row.   */
  float* sumsq;
  int32_t sumsq_ld;
  /* Optional caller-owned scratch (16-byte aligned, fp32), reused by every call on the stream.  With it, a launch whose
   * row count gives the chip too few workgroups to stream the weight panel (small M: low-resolution / distilled stage-1
   * steps, ltx.py:459-506 at config 1's geometry) runs as split-K: every K slice parks its fp32 accumulator tile here
   * (slices x M x N x 4 bytes; fewer slices if the scratch is smaller) and a second launch sums the slices in slice order
   * and applies the epilogue - deterministic, one rounding of the fp32 sum.  NULL: never split.                        */
  void* workspace;
  int64_t workspace_bytes;
} ltxk_gemm_args;

int ltxk_gemm_bf16(const ltxk_gemm_args* args, void* stream);

/* The launch form ltxk_gemm_bf16 takes for `args`, decided without launching anything (host only: pointers are checked for
 * NULL / alignment, never read).  ltxk_gemm_bf16 decides its form by the same host function, so a plan and a launch of the
 * same arguments cannot disagree; the same argument checks run and return the same error codes.
 * Only the split-K form sums a row's products in an order that depends on M (through its slice count): single-pass and
 * big-tile launches give a row the same bits whatever M is.  A caller that needs bits independent of how many rows share
 * the launch passes no workspace.                                                                                      */
enum { LTXK_GEMM_FORM_SINGLE = 0, LTXK_GEMM_FORM_BIG = 1, LTXK_GEMM_FORM_SPLITK = 2 };
struct ltxk_gemm_plan {   /* a struct tag only: the name is also the function's */
  int32_t form;                 /* LTXK_GEMM_FORM_*                                                                */
  int32_t tile_rows, tile_cols; /* workgroup tile                                                                  */
  int32_t row_tiles, col_tiles; /* tiles over M and over N                                                         */
  int32_t slices;               /* K slices (1 unless split-K)                                                     */
  int32_t ksteps;               /* 64-wide K-steps per slice; the last slice may have fewer                        */
};

int ltxk_gemm_plan(const ltxk_gemm_args* args, struct ltxk_gemm_plan* plan);

/* The same GEMM over an FP8 weight panel (W8A16): args->W is (N,K) OCP e4m3fn BYTES, row-major, 16-byte aligned; everything
 * else in `args` means what it means to ltxk_gemm_bf16, and the same argument checks return the same error codes.  The
 * panel is staged as fp8 (half the weight bytes from memory and through LDS) and widened to bf16 in registers in front of
 * the same v_mfma_f32_16x16x32_bf16 with the same K order; every e4m3 value is a bf16 value, so with w_scale == NULL the
 * outputs (out, out2, sumsq) equal those of ltxk_gemm_bf16 on the panel converted to bf16, bit for bit.  No bf16 copy of
 * the panel is made anywhere.
 * w_scale: (N) fp32 per-output-channel factors, 4-byte aligned, or NULL.  Applied as acc[n] * w_scale[n] on the fp32
 * accumulator before the bias (in the split-K form: on the summed slices); NULL: no multiply at all.
 * Launch forms: the single-pass 160-row family and split-K.  ltxk_gemm_w8_plan reports the form by the host rules of
 * ltxk_gemm_plan, except that a call the bf16 entry would run on the big tile is planned SINGLE: the split-K decision,
 * slice count and ksteps are those of the bf16 call with the same M, N, K and workspace.                                 */
int ltxk_gemm_w8(const ltxk_gemm_args* args, const float* w_scale, void* stream);
int ltxk_gemm_w8_plan(const ltxk_gemm_args* args, struct ltxk_gemm_plan* plan);

/* The same GEMM with FP8 activations too (W8A8, opt-in): args->A is (M,K) OCP e4m3fn BYTES with row stride lda in BYTES (pointer
 * and lda 16-byte aligned), args->W an e4m3fn panel as for ltxk_gemm_w8; K must be a multiple of 128 (LTXK_EINVAL otherwise).
 * Both operands are staged as fp8 and multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 (both formats e4m3, both block scales
 * 1.0) into the fp32 accumulators of the bf16 kernel; then acc * a_scale[m], then * w_scale[n] if given, then the bias and
 * the epilogue of ltxk_gemm_bf16 (every epilogue, the transposed and split outputs and sumsq are the shared code).
 * a_scale: (M) fp32 per-row factors, required (ltxk_quant_rows_fp8 writes them); w_scale: (N) fp32 or NULL.
 * Launch forms: the single-pass 160-row family only (every tile height, both tile widths); args->workspace is ignored, so a
 * row's bits never depend on M.  ltxk_gemm_w8a8_plan reports SINGLE with that tile and ksteps = K / 128.  There is no
 * split-K, big-tile or grouped W8A8 form: small-M launches are weight streams that gain nothing from fp8 arithmetic (callers
 * keep ltxk_gemm_w8 there), the other two are follow-ups.                                                                 */
int ltxk_gemm_w8a8(const ltxk_gemm_args* args, const float* a_scale, const float* w_scale, void* stream);
int ltxk_gemm_w8a8_plan(const ltxk_gemm_args* args, struct ltxk_gemm_plan* plan);

/* The same GEMM with both operands in OCP MXFP4 (opt-in): out = epilogue(sum_k a[m,k] * w[n,k]) with
 * a[m,k] = e2m1(codeA[m,k]) * 2^(EA[m, k/32] - 127) and w likewise.  args->A: (M, K/2) code bytes, element 2i in the low nibble of
 * byte i, row stride lda in BYTES (pointer and lda 16-byte aligned, lda >= K/2) - what ltxk_quant_rows_mxfp4 writes; args->W: the
 * (N, K/2) code bytes of weights.quantize_mxfp4, rows contiguous, 16-byte aligned - the panel ltxk_gemv_w4 reads, no re-packing.
 * a_block_scales (M, K/32) and w_block_scales (N, K/32): the e8m0 bytes with their row strides in bytes; pointers and strides
 * 8-byte aligned, strides >= K/32, both required.  args->K counts k (elements) and must be a multiple of LTXK_MXFP4_KSTEP = 256;
 * N % 8 == 0; anything else is LTXK_EINVAL and nothing is launched.
 * One v_mfma_scale_f32_16x16x128_f8f6f4 with both formats e2m1 per 16x16 tile and 128 k: a lane's 16 bytes are 32 consecutive k =
 * one scale block, and the block's e8m0 byte is the lane's scale operand - the e8m0 scales are the only scales, no fp32 multiply
 * follows.  Then the bias and the epilogue of ltxk_gemm_bf16 (every epilogue, the transposed and split outputs and sumsq are the
 * shared code).  Scale byte 255 is NaN, as the format defines it; the project's quantisers never write it.
 * Launch forms: the single-pass 160-row family only (every tile height, both tile widths); args->workspace is ignored and a row's
 * bits depend neither on M nor on the tile.  ltxk_gemm_mxfp4_plan reports SINGLE with that tile and ksteps = K / 256.  There is
 * no split-K, big-tile or grouped form.                                                                                      */
#define LTXK_MXFP4_KSTEP 256
int ltxk_gemm_mxfp4(const ltxk_gemm_args* args, const uint8_t* a_block_scales, int32_t ld_a_scales,
                    const uint8_t* w_block_scales, int32_t ld_w_scales, void* stream);
int ltxk_gemm_mxfp4_plan(const ltxk_gemm_args* args, struct ltxk_gemm_plan* plan);

/* Row quantiser in front of ltxk_gemm_mxfp4: x (M,K) bf16 with row stride lda (elements) -> codes (M, K/2) bytes with row stride
 * ldq (bytes) and block_scales (M, K/32) e8m0 bytes with row stride lds (bytes), in the layout and arithmetic of
 * weights.quantize_mxfp4, bit for bit.  Per row and 32 consecutive k: E = clamp(floor(log2 amax) - 2, -127, 127) + 127, a zero block
 * 127, never 255; element = nearest e2m1 magnitude of x / 2^(E-127), ties to the even 3-bit index, saturating at +-6, sign bit
 * kept (-0 stays -0); element 2i in the low nibble.  Inputs must be finite.  K % 32 == 0; x and lda 16-byte, codes and ldq
 * 16-byte, scales and lds 1-byte aligned (the GEMM wants them 8-byte aligned).  No atomics; a row's bits depend on that row only. */
int ltxk_quant_rows_mxfp4(const void* x, int32_t lda, void* codes, int32_t ldq, uint8_t* block_scales, int32_t lds,
                          int32_t M, int32_t K, void* stream);

/* The weight stream of a decode step: out[m,n] = r(acc * w_scale[n] + bias[n]), acc = A[m,:] . W[n,:] in fp32, for
 * 1 <= M <= 8 rows.  `args` as for ltxk_gemm_w8 (W: (N,K) e4m3fn bytes, 16-byte aligned; A: (M,K) bf16, 16-byte aligned, lda a
 * multiple of 8; out (M,N) bf16 with row stride ldo; bias (N) bf16 or NULL; w_scale (N) fp32 or NULL = no multiply) with
 * K % 16 == 0, any N >= 1, LTXK_EPI_BIAS only, and resid, gate, gate_row, out2, n_split, out_tokens_per_batch, sumsq and
 * workspace all zero: anything else is LTXK_EINVAL.  One launch (csrc/gemv.hip): W goes from memory straight to registers in
 * 16-byte loads, the rows of A are staged once per workgroup in LDS, a wave reduces a row of W - per lane fp32 FMAs over its
 * k in ascending order into an even-k and an odd-k accumulator, their sum, then the wave's butterfly - and applies the scale
 * and the bias as two fp32 operations.  No atomics, no K slices: the bits of out[m,n] are a function of row m of A, row n of
 * W, w_scale[n] and bias[n] alone, whatever M, N and the other rows are.  (The summation order differs from the MFMA forms',
 * so the result equals ltxk_gemm_w8's within the rounding bound, not bit for bit.)                                        */
int ltxk_gemv_w8(const ltxk_gemm_args* args, const float* w_scale, void* stream);

/* The same weight stream on an OCP MXFP4 panel: out[m,n] = r(A[m,:] . w[n,:] + bias[n]) in fp32 with
 * w[n,k] = e2m1(code[n,k]) * 2^(E[n, k/32] - 127), for 1 <= M <= 8 rows.  args->W: the (N, K/2) code bytes, element 2i in the low
 * nibble of byte i (torch.float4_e2m1fn_x2's order), 16-byte aligned; w_block_scales: the (N, K/32) e8m0 bytes, row-contiguous,
 * 4-byte aligned (E = 255 is NaN, as the format defines it; the project's quantiser never writes it).  A, out and bias as for
 * ltxk_gemv_w8; K >= 32 and K % 32 == 0, any N >= 1, LTXK_EPI_BIAS only, and resid, gate, gate_row, out2, n_split,
 * out_tokens_per_batch, sumsq and workspace all zero: anything else is LTXK_EINVAL.  One launch (csrc/gemv4.hip): a lane's
 * 16-byte load is 32 codes = one scale block, widened two at a time by v_cvt_scalef32_pk_f32_fp4 with the block's scale (exact),
 * then per lane fp32 FMAs over its k in ascending order into an even-k and an odd-k accumulator, their sum, the wave's
 * butterfly, the bias as one fp32 add, one rounding to bf16.  No atomics, no K slices: the bits of out[m,n] are a function of
 * row m of A, row n of the codes, its scale row and bias[n] alone, whatever M, N and the other rows are.                  */
int ltxk_gemv_w4(const ltxk_gemm_args* args, const uint8_t* w_block_scales, void* stream);

/* Row quantiser in front of ltxk_gemm_w8a8: x (M,K) bf16 with row stride lda -> q (M,K) e4m3fn bytes with row stride ldq
 * (bytes) and a_scale (M) fp32.  Per row, no special cases: amax = max|x|; scale = max(amax, 2^-64) / 448 in fp32 (correctly
 * rounded); q = e4m3 round-to-nearest-even, saturating, of fp32(x) / scale (IEEE fp32 division).  A zero row gives code 0.
 * Inputs must be finite.  K, lda, ldq multiples of 8; x 16-byte, q 8-byte aligned (the GEMM wants q and ldq 16-byte aligned). */
int ltxk_quant_rows_fp8(const void* x, int32_t lda, void* q, int32_t ldq, float* a_scale, int32_t M, int32_t K, void* stream);

/* Grouped GEMM: G problems that share A, M, N, K and the split output layout, as ONE persistent launch of 256-column big
 * tiles - the text k | V^T projections of every transformer block (attention.py:123-125 on the text side), none of which
 * depends on the token stream.  Group g computes exactly what
 *   ltxk_gemm_bf16{A, W[g], bias[g], out + g*out_gstride, out2 + g*out2_gstride, sumsq + g*sumsq_gstride, n_split, EPI_BIAS}
 * computes without a workspace, bit for bit (same K order, same MFMA, same rounding points, same sumsq order).
 * Per-group operands: W and bias are DEVICE arrays of G device pointers (weights stay wherever they live; the table is read
 * by the kernel, never by the host, so every W[g] must be 16-byte aligned and every bias[g] 8-byte aligned on the caller's
 * word); the outputs are one buffer each with a group stride in ELEMENTS.
 * Launch form: min(tiles, CUs) workgroups, each walking the static list t = workgroup, workgroup + grid, ... of the G x row
 * tiles x column tiles (groups in order, the single launch's XCD-aware tile order inside a group).  Tiles are independent:
 * no counter, no hand-over between workgroups.  Rows beyond the last whole row tile run on a shorter tile body.
 * Needs n_split > 0 (a multiple of 256), N a multiple of 256, K a multiple of 64, EPI_BIAS.                              */
typedef struct ltxk_gemm_grouped_args {
  const void* A;             /* (M,K) bf16, row stride lda; shared by every group                  */
  const void* const* W;      /* device array of G pointers to (N,K) bf16 row-major panels          */
  const void* const* bias;   /* device array of G pointers to (N) bf16, or NULL: no bias           */
  void* out;                 /* group g: (M,n_split) bf16 row stride ldo at out + g*out_gstride    */
  void* out2;                /* group g: (B,N-n_split,ldo2) bf16 at out2 + g*out2_gstride          */
  float* sumsq;              /* group g: (M,sumsq_ld) fp32 at sumsq + g*sumsq_gstride, or NULL     */
  int64_t out_gstride, out2_gstride, sumsq_gstride;   /* in elements                               */
  int32_t G, M, N, K;
  int32_t lda, ldo, ldo2, sumsq_ld;
  int32_t n_split, out_tokens_per_batch;
} ltxk_gemm_grouped_args;

int ltxk_gemm_bf16_grouped(const ltxk_gemm_grouped_args* args, void* stream);
/* sizeof(ltxk_gemm_grouped_args) in this build (the struct has an entry of its own; the index list above is closed).     */
int ltxk_gemm_grouped_args_sizeof(void);

/* The tiling ltxk_gemm_bf16_grouped takes (host only, nothing is launched or read).  tile_rows: 320 or 256; rem_rows: the
 * height of the body that runs the rows left after the whole row tiles (0: none; 128, 256 or tile_rows).                 */
struct ltxk_gemm_grouped_plan {
  int32_t tile_rows, rem_rows;
  int32_t row_tiles, col_tiles;  /* per group, the remainder row tile included                      */
  int32_t tiles;                 /* G * row_tiles * col_tiles                                        */
};
int ltxk_gemm_grouped_plan(const ltxk_gemm_grouped_args* args, struct ltxk_gemm_grouped_plan* plan);

/* ---------------------------------------------------------------------------------------
 * Fused attention: replaces mx.fast.scaled_dot_product_attention (attention.py:47) incl. the
 * (B,T,H*dh)<->(B,H,T,dh) reshapes (attention.py:24-33,50-51).  dh must be 128.  No mask
 * (context_mask=None on this path, generate.py:800).
 *   q  : (B,Tq,H*128) bf16 row stride ldq        k : (B,Tk,H*128) bf16 row stride ldk
 *   vt : (B,H*128,ldvt) bf16 = V transposed, ldvt >= Tk rounded up to 64, multiple of 8, pad columns finite
 *   out: (B,Tq,H*128) bf16 row stride ldo
 * q, k, vt, out 16-byte aligned; ldq, ldk, ldo multiples of 8; scale > 0.
 * Rounding points (oracle/dit.py::sdpa, "flash" policy): S = q.k^T in fp32; P = exp2(fma(S, scale*log2 e, -M)) with M an
 * INTEGER row offset, so bf16(P) does not depend on the tiling; l = sum P in fp32; O = bf16((bf16(P) @ V) / l).
 * ------------------------------------------------------------------------------------- */
enum {
  /* Launches of fewer than 1.25 rounds of 128-row query tiles: the tiles of the short last round of workgroups are normally
   * split over two workgroups that halve the keys and merge (O, M, l): faster, but those rows then sum their keys in another
   * order than in a launch whose grid has no short round.  With this flag the result for a (batch, head) does not depend on
   * how many share a launch.  Larger launches run a mixed grid of 192- and 128-row tiles that never splits keys: they have
   * the flag's bits with or without it.                                                                                  */
  LTXK_ATTN_NO_TAIL_SPLIT = 1
};
typedef struct ltxk_attn_args {
  const void* q; const void* k; const void* vt; void* out;
  int32_t ldq, ldk, ldvt, ldo;
  int32_t B, H, Tq, Tk;
  float scale;
  /* Optional fused query preparation (attention.py:129-136).  With q_sumsq set, `q` holds the RAW to_q projection
   * and the kernel applies, to its Q fragments in registers, q_norm (RMSNorm over all H*128 channels jointly, learned
   * weight) and - if cos/sin are given - the SPLIT rotation of rope.py:109-172, with the rounding points of
   * ltxk_qknorm_rope.  q_sumsq: (B*Tq, q_sumsq_ld) fp32, the first q_sumsq_n = H*128/64 entries of a row are the sums
   * of squares of its 64-column blocks (the `sumsq` output of ltxk_gemm_bf16).  cos/sin: (H,Tq,64) fp32.           */
  const float* q_sumsq;
  int32_t q_sumsq_ld, q_sumsq_n;
  const void* q_norm_weight;   /* (H*128) bf16 */
  const float* cos;
  const float* sin;
  float eps;
  int32_t flags;               /* LTXK_ATTN_* */
} ltxk_attn_args;

int ltxk_flash_attn(const ltxk_attn_args* args, void* stream);

/* The launch form ltxk_flash_attn takes for `args` on a device of `cus` compute units, decided without launching anything
 * (host only: pointers are checked for NULL / alignment, never read; cus <= 0 is LTXK_EINVAL).  ltxk_flash_attn decides its form
 * by the same host function with the current device's CU count, so a plan and a launch of the same arguments cannot disagree;
 * the same argument checks run and return the same error codes.
 * KERNEL_128: 128-row query tiles; split_tiles of them (those of the short last round of 2 * cus workgroups) halve their keys
 * over two workgroups each - the one form whose rows sum their keys in another order.  KERNEL_MIX: per (batch, head) tiles_192
 * tiles of 192 rows followed by tiles_128 of 128 rows, never split.                                                        */
enum { LTXK_ATTN_KERNEL_128 = 0, LTXK_ATTN_KERNEL_MIX = 1 };
struct ltxk_flash_attn_plan {   /* a struct tag only: the name is also the function's */
  int32_t kernel;          /* LTXK_ATTN_KERNEL_*                                              */
  int32_t mfma_k;          /* 16; 32 only in the A/B build with LTXK_FA_MFMA=32               */
  int32_t tiles_192;       /* per (batch, head): 192-row tiles (0 for KERNEL_128)             */
  int32_t tiles_128;       /* per (batch, head): 128-row tiles                                */
  int32_t whole_workgroups;/* workgroups that run a whole tile                                */
  int32_t split_tiles;     /* tiles whose keys are halved over two workgroups (0 for MIX)     */
  int32_t workgroups;      /* grid size = whole_workgroups + 2 * split_tiles                  */
  int32_t xcd_order;       /* 1: the XCD-aware tile order                                     */
};
int ltxk_flash_attn_plan(const ltxk_attn_args* args, int32_t cus, struct ltxk_flash_attn_plan* plan);
/* sizeof(struct ltxk_flash_attn_plan) in this build (an entry of its own: the ltxk_abi_sizeof index list is closed).     */
int ltxk_flash_attn_plan_sizeof(void);

/* The same without query preparation (positional form kept for existing bindings).       */
int ltxk_flash_attn_bf16(const void* q, int32_t ldq, const void* k, int32_t ldk,
                         const void* vt, int32_t ldvt, void* out, int32_t ldo,
                         int32_t B, int32_t H, int32_t Tq, int32_t Tk, float scale,
                         void* stream);

/* ltxk_flash_attn at head dim 64 (the audio transformer, 32 heads x 64: ltx.py AudioOnly; also the head dim of the
 * cross-modal attentions).  The same struct read at dh = 64: q, k, out (B,T,H*64); vt (B,H*64,ldvt), ldvt >= Tk rounded up
 * to 64; the alignment and stride rules and the "flash" rounding points above, word for word.  No fused query preparation:
 * q_sumsq != NULL is LTXK_EINVAL (q_norm_weight, cos, sin, eps and flags are not read).  One launch form: 64-row query
 * tiles x whole key range per workgroup, keys never split, so a (batch, head)'s bits do not depend on B, H or the grid.
 * Keys >= Tk get P = 0 and take no part in the row maximum (V^T pad columns may hold any finite value); rows >= Tq are
 * not stored; no load leaves q, k or vt as sized above.                                                                  */
int ltxk_flash_attn_dh64(const ltxk_attn_args* args, void* stream);

/* ---------------------------------------------------------------------------------------
 * rms_norm (weight 1) + AdaLN modulation: utils.py:398-400 + transformer.py:253,258,346.
 *   y = bf16(bf16(bf16(rms(x)) * bf16(1+scale)) + shift); scale/shift NULL => plain rms_norm.
 *   scale/shift value for row m, col d: p[mod_row[m]*mod_stride + d].
 * ------------------------------------------------------------------------------------- */
int ltxk_rmsnorm_modulate(const void* x, void* y, int32_t M, int32_t D, float eps,
                          const void* scale, const void* shift, int32_t mod_stride,
                          const int32_t* mod_row, void* stream);

/* The same when the rows' sums of squares are already known: sumsq (M, sumsq_ld) fp32, row statistic = the sum of
 * the first sumsq_n entries (ltxk_gemm_bf16's `sumsq` output for the GEMM that produced x).  The row is then not
 * re-read for its statistic and is split over several waves.  flags & LTXK_NORM_SCALE_IS_ONE_PLUS: `scale` already
 * holds bf16(1+scale) (ltxk_ada_combine's one_plus_mask).                                 */
enum { LTXK_NORM_SCALE_IS_ONE_PLUS = 1 };
int ltxk_rmsnorm_modulate_ss(const void* x, void* y, int32_t M, int32_t D, float eps, const float* sumsq,
                             int32_t sumsq_ld, int32_t sumsq_n, const void* scale, const void* shift,
                             int32_t mod_stride, const int32_t* mod_row, int32_t flags, void* stream);

/* One normalisation pass, two modulations (the cross-modal section of the AudioVideo block, transformer.py:282-283,
 * 315-316, 329-330): y0 = modulate(rms(x), scale0, shift0), y1 = modulate(rms(x), scale1, shift1), x read once.  Both
 * pairs are required and share mod_stride / mod_row; y0 != y1, neither aliases x.  sumsq != NULL: the carried statistic,
 * as ltxk_rmsnorm_modulate_ss reads it (sumsq_ld, sumsq_n); NULL: the kernel reduces the row itself, as
 * ltxk_rmsnorm_modulate does.  flags & LTXK_NORM_SCALE_IS_ONE_PLUS (needs sumsq) holds for both scales.  D a multiple of
 * 512, <= 8192; every pointer but sumsq / mod_row 16-byte aligned.  Each output carries the bits of the single-output
 * entry called with the same operands.                                                                                  */
int ltxk_rmsnorm_modulate2(const void* x, void* y0, void* y1, int32_t M, int32_t D, float eps, const float* sumsq,
                           int32_t sumsq_ld, int32_t sumsq_n, const void* scale0, const void* shift0,
                           const void* scale1, const void* shift1, int32_t mod_stride, const int32_t* mod_row,
                           int32_t flags, void* stream);

/* LayerNorm(affine=False) + modulation of the output head: ltx.py:432-457.               */
int ltxk_layernorm_modulate(const void* x, void* y, int32_t M, int32_t D, float eps,
                            const void* scale, const void* shift, int32_t mod_stride,
                            const int32_t* mod_row, void* stream);

/* ---------------------------------------------------------------------------------------
 * q/k RMSNorm over the whole inner dim (all heads jointly, learned weight) + SPLIT RoPE:
 * attention.py:96-97,129-136 + rope.py:109-172.  In place on `nseg` column segments of
 * width D of each row of buf (self-attn: q|k packed => nseg=2).
 *   weight: (nseg,D) bf16.  cos/sin: (H,T,dh/2) fp32 or NULL (no rope: cross-attention).
 *   row m belongs to token t = m % T.
 * ------------------------------------------------------------------------------------- */
int ltxk_qknorm_rope(void* buf, int32_t ld, int32_t M, int32_t nseg, int32_t D,
                     const void* weight, const float* cos, const float* sin,
                     int32_t T, int32_t H, float eps, void* stream);

/* The same with the per-row sums of squares precomputed: sumsq[m*sumsq_ld + seg*(D/64) + i], i < D/64
 * (ltxk_gemm_bf16's `sumsq` output of the projection that wrote buf).                     */
int ltxk_qknorm_rope_ss(void* buf, int32_t ld, int32_t M, int32_t nseg, int32_t D,
                        const void* weight, const float* cos, const float* sin,
                        int32_t T, int32_t H, float eps, const float* sumsq, int32_t sumsq_ld, void* stream);

/* The same chain at head dim 64: D == H*64, 1 <= H <= 32, cos/sin (H,T,32) fp32 or NULL, the rotation partner of channel j
 * of a head is j + 32.  sumsq as for ltxk_qknorm_rope_ss (D/64 = H partials per segment), or NULL: the kernel then reduces
 * the row itself.  buf, weight, cos, sin 16-byte aligned.                                   */
int ltxk_qknorm_rope_dh64(void* buf, int32_t ld, int32_t M, int32_t nseg, int32_t D,
                          const void* weight, const float* cos, const float* sin,
                          int32_t T, int32_t H, float eps, const float* sumsq, int32_t sumsq_ld, void* stream);

/* The q/k RMSNorm above without rotation over G stacked buffers in one launch (the text-side k of every block): group g is
 * the (M,D) rows at buf + g*buf_gstride (row stride ld) with weight row g of the (G,D) table and the statistics at
 * sumsq + g*sumsq_gstride; strides in elements.  Same bits as G calls of the single-buffer form with nseg = 1, no cos/sin. */
int ltxk_qknorm_grouped_ss(void* buf, int64_t buf_gstride, int32_t ld, int32_t G, int32_t M, int32_t D,
                           const void* weight, int32_t H, float eps, const float* sumsq, int64_t sumsq_gstride,
                           int32_t sumsq_ld, void* stream);

/* Sinusoidal timestep projection: utils.py:486-526 (flip_sin_to_cos, shift 0), applied to
 * bf16(t*mult) (ltx.py:68: timestep*timestep_scale_multiplier stays in the model dtype).
 * t: (U) bf16 timesteps; out: (U,dim) bf16.                                              */
int ltxk_timestep_embed(const void* t, void* out, int32_t U, int32_t dim, float mult, void* stream);

/* SPLIT-layout RoPE table, fp32: rope.py:419-529 (_precompute_freqs_cis_double_precision with
 * use_middle_indices_grid).  positions: (3,T,2) fp32 [start,end); freq: (n_freq) fp32 =
 * theta^linspace(0,1,n_freq)*pi/2 (host table, rope.py:449-450); max_pos: 3 HOST floats.
 * cos/sin out: (H,T,dim/2/H) fp32; the first dim/2-3*n_freq entries are cos=1,sin=0.     */
int ltxk_rope_table(const float* positions, const float* freq, float* cos, float* sin,
                    int32_t T, int32_t H, int32_t dim, int32_t n_freq, const float* max_pos,
                    void* stream);

/* out[l,u,k,:] = bf16(table[l,k,:] + ada[u,k,:]): transformer.py:135-177, ltx.py:440-447.  For the k whose bit is set
 * in one_plus_mask the stored value is bf16(1 + that) - the `(1 + scale)` factor of transformer.py:253,346, which is
 * the same for every token that shares the row.                                           */
int ltxk_ada_combine(const void* table, const void* ada, void* out, int32_t L, int32_t U,
                     int32_t K, int32_t D, uint32_t one_plus_mask, void* stream);

/* Elementwise bf16 SiLU (adaln.py:45).                                                   */
int ltxk_silu(const void* x, void* y, int64_t n, void* stream);

/* (B,C,S) channels-first latent -> (B,S,C) tokens, optionally replicated `rep` times on the
 * batch axis (cfg_batch): generate.py:1236,1239-1241.  Bit-exact index map.              */
int ltxk_latent_to_tokens(const void* latent, void* tokens, int32_t B, int32_t C, int32_t S,
                          int32_t rep, void* stream);

/* One denoise-step tail: CFG combine + token->latent transpose + x0 + mask blend + Euler:
 * generate.py:1255,1283-1301 (compiled: 1160-1174), utils.py:404-440, latent.py:180-196.
 *   v_pos/v_neg: (B,S,C) bf16 velocities (v_neg NULL => no CFG)
 *   latent/out : (B,C,S) bf16;  clean: (B,C,S) bf16 or NULL;  mask: (B,S) float or NULL
 *   x0  = bf16(x - sigma*v);  x0 = x0*m + clean*(1-m);  out = bf16(x0 + sigma_next*(x-x0)/sigma)
 *   sigma_next <= 0 => out = x0.
 *   flags & LTXK_STEP_BF16_EULER: the Euler update runs op by op in bf16, the reference's
 *   fp32_euler=False / LTX_FP32_EULER=0 compiled step (generate.py:741-748):
 *   out = bf16(x0 + bf16(bf16(sigma_next * bf16(x - x0)) / sigma)).
 * Every step-tail entry (this one, _dev, ltxk_guided_euler_step, ltxk_guider_euler_step) runs one host check and one kernel
 * family (csrc/step_tail.hip).  LTXK_EINVAL from each of them: NULL v_pos / latent / out, B, C or S <= 0, C % 8 != 0, B or C/8
 * above 65535 (they are grid dimensions), a token tensor (v_pos, v_neg, v_pert) that is not 16-byte aligned, clean without
 * mask or mask without clean, sigma <= 0 without sigmas_dev.                                */
enum { LTXK_STEP_BF16_EULER = 1 };
int ltxk_cfg_euler_step(const void* v_pos, const void* v_neg, const void* latent, void* out,
                        const void* clean, const float* mask, int32_t B, int32_t C, int32_t S,
                        float cfg_scale, float sigma, float sigma_next, int32_t flags, void* stream);

/* Same step tail with {sigma, sigma_next} read from DEVICE memory (2 floats): lets one captured
 * hipGraph of the whole denoise step be replayed for every step of the schedule.           */
int ltxk_cfg_euler_step_dev(const void* v_pos, const void* v_neg, const void* latent, void* out,
                            const void* clean, const float* mask, int32_t B, int32_t C, int32_t S,
                            float cfg_scale, const float* sigmas_dev, int32_t flags, void* stream);

/* The step tail with spatio-temporal guidance (STG): a third velocity v_pert (B,S,C) - the forward of the positive
 * prompt with the video self-attention of chosen blocks skipped (ltxk_attn_value_passthrough) - pushes the guided
 * velocity away from it, in velocity space, before x0:
 *   g = v_neg ? bf16(v_pos + bf16((cfg_scale-1) * bf16(v_pos - v_neg))) : v_pos       (exactly the CFG combine above)
 *   v = bf16(g + bf16(stg_scale * bf16(v_pos - v_pert)))
 * then x0, mask blend and Euler exactly as ltxk_cfg_euler_step.  x0 = x - sigma*v is affine in v with coefficients that
 * sum to one, so this is cond + CFGGuider.delta + STGGuider.delta of the x0-space guiders (guiders.py) in exact
 * arithmetic.  sigmas_dev != NULL: {sigma, sigma_next} are read from device memory (as ltxk_cfg_euler_step_dev).
 * v_pert == NULL: the very launch ltxk_cfg_euler_step(_dev) makes (stg_scale ignored).                           */
typedef struct ltxk_step_args {
  const void* v_pos;          /* (B,S,C) bf16, 16-byte aligned                                     */
  const void* v_neg;          /* (B,S,C) bf16, 16-byte aligned, or NULL (no CFG)                   */
  const void* v_pert;         /* (B,S,C) bf16, 16-byte aligned, or NULL (no STG)                   */
  const void* latent;         /* (B,C,S) bf16                                                      */
  void* out;                  /* (B,C,S) bf16; may be `latent`                                     */
  const void* clean;          /* (B,C,S) bf16 or NULL                                              */
  const float* mask;          /* (B,S) fp32 or NULL (with clean)                                   */
  const float* sigmas_dev;    /* 2 fp32 in device memory, or NULL: use sigma / sigma_next          */
  int32_t B, C, S;
  float cfg_scale, stg_scale, sigma, sigma_next;
  int32_t flags;              /* LTXK_STEP_*                                                       */
} ltxk_step_args;

int ltxk_guided_euler_step(const ltxk_step_args* args, void* stream);

/* CFG* and APG: the two x0-space guiders of ltx_core/components/guiders.py that need a global reduction
 * (CFGStarRescalingGuider :14-43, LtxAPGGuider :57-76).  With r(.) = round to bf16 (every array-valued op of the reference
 * materialises a bf16 array), p = r(x - sigma*v_pos), n = r(x - sigma*v_neg), k = cfg_scale - 1 (fp32), sums per batch
 * sample over all C*S elements (masked tokens included), each summand the bf16-rounded product, a sum used as r(sum):
 *   CFG_STAR: a = r(r(S r(p*n)) / r(r(S r(n*n)) + 1e-8));                       d = r(k * r(p - r(a*n)))
 *   APG:      g = r(p - n);  norm_threshold > 0 only: nrm = r(sqrt(r(r(S r(g*g)) + 1e-8))), f = min(1, r(norm_threshold/nrm)),
 *             g = r(g*f);    c = r(r(S r(g*p)) / r(r(S r(p*p)) + 1e-8));  par = r(c*p);
 *                                                                               d = r(k * r(r(par*eta) + r(g - par)))
 *   x0 = r(p + d);  with v_pert (STG): x0 = r(x0 + r(stg_scale * r(p - r(x - sigma*v_pert))));
 * then mask blend, Euler, sigma_next <= 0 and LTXK_STEP_BF16_EULER exactly as ltxk_cfg_euler_step.
 *
 * A step is ltxk_guidance_sums (the reductions -> `record`, in device memory) followed by ltxk_guider_euler_step (the tail,
 * which reads the derived scalars from `record`); the host never reads a sum, so both are captured in a step graph.
 * record: LTXK_GUIDER_RECORD_FLOATS fp32 per sample, every one written by each ltxk_guidance_sums call:
 *   CFG_STAR  [0] S r(p*n)  [1] S r(n*n)  [2] 0         [3] 0    [4] 1                    [5] a   [6..7] 0
 *   APG       [0] S r(g*g)  [1] S r(g*p)  [2] S r(p*p)  [3] nrm  [4] f                    [5] c   [6..7] 0
 *             ([0] and [3] are 0 and f is 1 when norm_threshold == 0; [0] sums g before the clamp, [1] after it)
 * Sums are deterministic: no atomics; one fp32 partial per wave (8 serial terms per lane, then the wave butterfly) and a
 * float64 combine per sample in an order that depends on (C, S) only - not on B, the device or the launch path - so sample
 * b of a batch has the bits of the same sample launched alone.  Each raw sum is within 1e-5 * S|term| of the exact sum.
 * CFG_STAR and APG without the clamp make one reduction pass (2 launches), APG with norm_threshold > 0 two (the second
 * reads f from the record).  workspace: ltxk_guidance_sums_workspace_bytes(B, C, S) bytes, caller-owned, contents
 * irrelevant on entry.  ltxk_guidance_sums reads v_pos, v_neg, latent, sigma | sigmas_dev[0], guider, norm_threshold.
 * LTXK_EINVAL: what every step-tail entry refuses (see ltxk_cfg_euler_step; ltxk_guidance_sums needs no `out`), and an
 * unknown guider id (plain CFG is ltxk_cfg_euler_step), eta not finite, norm_threshold < 0 or not finite, NULL v_neg, NULL
 * record, a workspace too small.                                                                                          */
enum { LTXK_GUIDER_CFG_STAR = 1, LTXK_GUIDER_APG = 2 };
#define LTXK_GUIDER_RECORD_FLOATS 8
typedef struct ltxk_guider_args {
  const void* v_pos;          /* (B,S,C) bf16, 16-byte aligned                                     */
  const void* v_neg;          /* (B,S,C) bf16, 16-byte aligned; required                           */
  const void* v_pert;         /* (B,S,C) bf16 or NULL (no STG); tail only                          */
  const void* latent;         /* (B,C,S) bf16                                                      */
  void* out;                  /* (B,C,S) bf16; may be `latent`; tail only                          */
  const void* clean;          /* (B,C,S) bf16 or NULL; tail only                                   */
  const float* mask;          /* (B,S) fp32 or NULL (with clean); tail only                        */
  const float* sigmas_dev;    /* 2 fp32 in device memory, or NULL: use sigma / sigma_next          */
  float* record;              /* (B, LTXK_GUIDER_RECORD_FLOATS) fp32: written by the sums, read by the tail */
  void* workspace;            /* sums only                                                         */
  int64_t workspace_bytes;
  int32_t B, C, S;
  int32_t guider;             /* LTXK_GUIDER_*                                                     */
  float cfg_scale, stg_scale, sigma, sigma_next;
  float eta, norm_threshold;  /* APG: weight of the parallel component; norm clamp (0: none)       */
  int32_t flags;              /* LTXK_STEP_*                                                       */
} ltxk_guider_args;
/* sizeof(ltxk_guider_args) in this build (an entry of its own: the ltxk_abi_sizeof index list is closed).               */
int ltxk_guider_args_sizeof(void);
int64_t ltxk_guidance_sums_workspace_bytes(int32_t B, int32_t C, int32_t S);   /* -1 on bad arguments                 */
int ltxk_guidance_sums(const ltxk_guider_args* args, void* stream);
int ltxk_guider_euler_step(const ltxk_guider_args* args, void* stream);

/* The value passthrough of a skipped video self-attention (STG, perturbations.py SKIP_VIDEO_SELF_ATTN): for every batch
 * row b whose bit is set in row_mask, out[(b*T+t)*ldo + c] = vt[(b*D+c)*ldvt + t] for t < T, c < D - the V^T buffer of
 * the q|k|v GEMM (ltxk_gemm_bf16 split output) transposed back to the token-major rows the out-projection reads, a
 * bit-exact copy.  Rows whose bit is clear are not touched.  B <= 64; D a multiple of 128; ldvt >= T and ldo >= D,
 * both multiples of 8; vt and out 16-byte aligned.                                       */
int ltxk_attn_value_passthrough(const void* vt, int32_t ldvt, void* out, int32_t ldo, int32_t B, int32_t D, int32_t T,
                                uint64_t row_mask, void* stream);

/* Per-step scalars of a replayed step graph: with s = min(*step, n_steps-1), copies ts_all[s,:] (U bf16
 * timestep values = bf16(sigma_s)*mask, generate.py:1084,1237) to ts and sig_all[s,:] ({sigma, sigma_next}
 * fp32) to sig, then stores *step = s+1.  As the first node of a captured denoise step it lets the whole
 * schedule run as graph replays with no host->device traffic between steps.               */
int ltxk_step_scalars(const void* ts_all, const float* sig_all, int32_t* step, void* ts, float* sig,
                      int32_t U, int32_t n_steps, void* stream);

/* Euler update alone (eager path, generate.py:1293-1301, with un-rounded float sigmas):
 * out = bf16(x0 + sigma_next*(x - x0)/sigma) in fp32; n elements, any layout.             */
int ltxk_euler_step(const void* latent, const void* denoised, void* out, int64_t n,
                    float sigma, float sigma_next, void* stream);

/* ---------------------------------------------------------------------------------------
 * Text stage: from the hidden states of a Gemma-3 forward to the DiT's context.  norm_and_concat_hidden_states
 * (text_encoder.py:591-639) and the row operations of Embeddings1DConnector (text_encoder.py:271-587) at widths the
 * DiT's row kernels do not take (D = 3840, H = 30).  The GEMMs and the attention of the connector are ltxk_gemm_bf16
 * and ltxk_flash_attn.  The Gemma-3 forward that produces the hidden states is the next section.
 *
 * The layer stack is ONE base pointer with explicit strides (in elements): element (l, b, t, d) of the L hidden states
 * is x[l*layer_stride + b*batch_stride + t*row_stride + d].  A caller that holds the layers as separately allocated
 * tensors stacks them first.  x 16-byte aligned; D and every stride a multiple of 8; L*B <= 65535.
 * Batch row b's valid tokens are the rows [row_start[b], row_start[b] + row_count[b]) (device int32 arrays; left padding:
 * row_start = T - row_count); a range that leaves [0, T) is clipped to it.  Rows outside are never read.
 * ------------------------------------------------------------------------------------- */

/* stats[(b*L + l)*3 + {0,1,2}] = fp32 {sum, min, max} over the valid rows x D of layer l, batch row b.  min and max are
 * exact.  Two launches of fixed shape, no floating-point atomics: 64 workgroups per (b, l) each reduce a contiguous run of
 * ceil(count/64) rows (8 running sums per thread, then fixed trees), one wave per (b, l) then sums the 64 partials; a
 * term passes through at most ceil(ceil(count/64) * D/8 / 256) + 17 additions (47 at count = 1024, D = 3840), and the
 * result of a (b, l) pair does not depend on what else the launch holds.  row_count[b] == 0 writes {0, 0, 0}.
 * partials: caller-owned scratch of L*B*192 floats.                                        */
int ltxk_masked_layer_stats(const void* x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
                            const int32_t* row_start, const int32_t* row_count, int32_t L, int32_t B, int32_t T,
                            int32_t D, float* partials, float* stats, void* stream);

/* out[(row0[b] + t)*ldo + l*D + d] = bf16(8 * (x[l,b,row_start[b]+t,d] - mean) / ((max - min) + 1e-6)) for t < row_count[b],
 * mean = sum / (row_count[b]*D + 1e-6), with `stats` as written by ltxk_masked_layer_stats: all in fp32, one rounding to
 * bf16 at the store.  The matrix is compact - `rows` = sum of the counts, row0 (B) their exclusive prefix sums (device
 * int32) - and LAYER-major: column l*D + d, where the reference's concatenation is d*L + l; the aggregate_embed panel
 * that multiplies it has its K axis permuted to match, once, when it is loaded.  Padded rows are neither read nor
 * written (the reference zeroes them and then replaces them by registers).  ldo >= L*D, a multiple of 8.              */
int ltxk_layer_norm_compact(const void* x, int64_t layer_stride, int64_t batch_stride, int64_t row_stride,
                            const int32_t* row_start, const int32_t* row_count, const int32_t* row0, const float* stats,
                            void* out, int64_t ldo, int32_t L, int32_t B, int32_t T, int32_t D, int32_t rows,
                            void* stream);

/* rms_norm with unit weight (utils.py:398-400) for rows of any width D % 8 == 0, D <= 8192: y = bf16(x * rsqrt(mean(x^2) + eps)),
 * one pass with the row in registers.  x (M,D) row stride ldx, y (M,D) row stride ldy (y may be x).  One kernel body
 * with ltxk_rmsnorm_weight_rows: the bits of that entry point with a zero weight and no residual.                          */
int ltxk_rmsnorm_rows(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t M, int32_t D, float eps, void* stream);

/* ltxk_qknorm_rope for any head count: in place on the q | k halves (columns [0,D) and [D,2D)) of buf (M, ld >= 2D):
 * RMSNorm over the full D with weight row 0 / 1 of `weight` (2,D) bf16, then the SPLIT rotation over each 128-wide head
 * with cos/sin (H,T,64) fp32, row m at position m % T (text_encoder.py:308-363).  D == 128*H, 1 <= H <= 64; the kernel
 * reduces the row itself.  One kernel with ltxk_qknorm_rope (nseg = 2): the same bits where both take H.  Columns past 2D
 * are not touched.                                                                                                     */
int ltxk_qknorm_rope_1d(void* buf, int32_t ld, int32_t M, int32_t D, const void* weight, const float* cos,
                        const float* sin, int32_t T, int32_t H, float eps, void* stream);

/* In-place exact GELU (nn.gelu, text_encoder.py:388): x = bf16(x * (1 + erf(x / sqrt 2)) / 2) evaluated in fp32 as
 * (x/2) * erfc(-x / sqrt 2), which keeps its relative accuracy on the negative side.  n elements, x 16-byte aligned.  */
int ltxk_gelu_erf(void* x, int64_t n, void* stream);

/* The connector's input (text_encoder.py:510-563): out (B,T,D); row t < row_count[b] is row row0[b] + t of the compact
 * feature matrix feat (feat_rows, ldf), row t >= row_count[b] is registers[t % R] (registers (R,D) bf16): the valid tokens
 * moved to the front, the learnable registers tiled over the sequence behind them.  Bit-exact copies.                 */
int ltxk_connector_assemble(const void* feat, int32_t ldf, const void* registers, const int32_t* row0,
                            const int32_t* row_count, void* out, int32_t B, int32_t T, int32_t D, int32_t R,
                            int32_t feat_rows, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gemma-3 text encoder: token ids to the L+1 hidden states the text stage above consumes.  The reference wraps mlx_vlm's
 * Gemma3Model (text_encoder.py:47-152: embedding scale :107, left padding and the combined causal-and-padding mask :58-81,
 * the list [embeddings, h_1 .. h_{L-1}, norm(h_L)] :110-148); the layer itself is the Gemma-3 definition (transformers'
 * Gemma3TextModel).  The no-bias Linears are ltxk_gemm_bf16; what follows are the four row operations and the attention
 * that the library had no kernel for.  r(.) = one rounding to bf16 with fp32 arithmetic in front of it.  Row kernels take
 * any D % 8 == 0, D <= 8192, hold the row in registers, reduce in a fixed order that depends on the row's width only and
 * use no atomics; pointers 16-byte aligned, row strides multiples of 8.
 * ------------------------------------------------------------------------------------- */

/* out[m,:] = r(table[ids[m],:] * s): the embedding gather with Gemma's scale, s = bf16(sqrt(D)) passed as a float (62.0 at
 * D = 3840; text_encoder.py:107 rounds the scale to bf16 first).  table (V,D) bf16 contiguous, ids (M) DEVICE int32,
 * out (M,D) row stride ldo.  The kernel cannot report an error for device data: an id outside [0, V) reads row 0 / V-1;
 * a caller that needs the range checked checks its host copy.                                                          */
int ltxk_embed_rows(const void* table, int32_t V, int32_t D, const int32_t* ids, void* out, int32_t ldo, int32_t M,
                    float s, void* stream);

/* The same gather over an e4m3fn table (V,D), D % 16 == 0: out[m,:] = r((fp32(code) * row_scale[id]) * s), both products
 * in fp32 in that order; row_scale (V) fp32 or NULL - then out[m,:] = r(fp32(code) * s), which equals ltxk_embed_rows on the
 * table converted to bf16 bit for bit.  Gemma-3 ties the output head to this table, so one per-row scale serves the gather
 * (row = token) and the logits GEMM (row = output channel: its w_scale).                                                 */
int ltxk_embed_rows_fp8(const void* table, const float* row_scale, int32_t V, int32_t D, const int32_t* ids, void* out,
                        int32_t ldo, int32_t M, float s, void* stream);

/* Gemma RMSNorm (Gemma3RMSNorm): n = r(x * rsqrt(mean(x^2) + eps) * (1 + w)), w (D) bf16 widened so that 1 + w is formed in
 * fp32.  resid == NULL: y = n.  Otherwise y = r(resid + n), the decoder layer's post-norm-then-add (n is a bf16 tensor in
 * the model, so it is rounded before the add); y may be resid, and y may be x.  x (M,D) stride ldx, resid stride ldr,
 * y stride ldy.  The sum of squares: each lane adds its elements in ascending order, then the wave's butterfly.       */
int ltxk_rmsnorm_weight_rows(const void* x, int32_t ldx, const void* weight, const void* resid, int32_t ldr, void* y,
                             int32_t ldy, int32_t M, int32_t D, float eps, void* stream);

/* q_norm / k_norm + RoPE, in place on the first (Hq + Hkv) * 256 columns of buf (M, ld): the q | k part of the fused q|k|v
 * projection, head hh < Hq a query head (q_weight), the next Hkv key heads (k_weight); weights (256) bf16.  Per 256-wide head:
 *   x' = r(x * rsqrt(mean(x^2) + eps) * (1 + w)), then the rotate-half rotation on the pairs (i, i + 128), i < 128:
 *   o1 = r(x1' * c - x2' * s), o2 = r(x2' * c + x1' * s), c = cos[t*128 + i], s = sin[t*128 + i], t = m % T.
 * cos / sin: (T,128) fp32.  The position of a row is its index in the PADDED sequence, 0 .. T-1, whatever the attention
 * mask - what the reference's nn.RoPE call (offset 0) and transformers' default position_ids both do.  The caller builds the
 * tables (float64 on the host, rounded to bf16 and widened; one pair for the local base, one for the global base with its
 * linear position scaling).  Columns past (Hq + Hkv) * 256 are not touched.                                           */
int ltxk_headnorm_rope(void* buf, int32_t ld, int32_t M, int32_t Hq, int32_t Hkv, const void* q_weight, const void* k_weight,
                       const float* cos, const float* sin, int32_t T, float eps, void* stream);

/* GeGLU: out[m,f] = r(r(gelu_tanh(g[m,f])) * u[m,f]) for gu = [g | u] (M, 2F) row stride ld, the output of one GEMM over the
 * stacked gate | up panel; out (M,F) row stride ldo, and out may be gu with ldo == ld (the product then replaces g).
 * gelu_tanh(x) = x / (1 + exp(-2 sqrt(2/pi) (x + 0.044715 x^3))) in fp32, which keeps its relative accuracy on the
 * negative side; F % 8 == 0.                                                                                          */
int ltxk_geglu_tanh(const void* gu, int32_t ld, void* out, int32_t ldo, int32_t M, int32_t F, void* stream);

/* Causal, left-padding-aware, grouped-query attention, head dim 256.
 *   q  : (B,T,Hq*256)  bf16 row stride ldq          k : (B,T,Hkv*256) bf16 row stride ldk
 *   vt : (B,Hkv*256,ldvt) bf16 = V transposed, exactly as ltxk_gemm_bf16's split output writes it (n_split = (Hq+Hkv)*256
 *        gives q | k row-major and V^T in one launch); ldvt >= T, a multiple of 8; columns >= T are read in whole 16-byte
 *        chunks and must be finite
 *   out: (B,T,Hq*256) bf16 row stride ldo
 * Hq % Hkv == 0; query head h reads K/V head h / (Hq/Hkv).  row_start (B) DEVICE int32, the text stage's convention: the
 * valid tokens of batch row b are [row_start[b], T) (clipped into [0, T]).  window: 0 = none, else a positive count.
 * Key j is visible to query i iff  row_start[b] <= j <= i  and  (window == 0 or i - j < window).
 * Rounding points are ltxk_flash_attn's ("flash" policy) over the visible keys: S = q.k^T in fp32; P = exp2(fma(S, scale*log2 e,
 * -M)) with M an integer row offset (the ceil of the running maximum over visible keys); l = sum P in fp32;
 * O = r((bf16(P) @ V) / l).  A masked key contributes P = 0 exactly (its K row may hold anything, its V row anything finite).
 * A query row i < row_start[b] has no visible key and gets an all-zero output row (no NaN, no division by l = 0).
 * Key tiles wholly outside the visible range of a 64-row query tile are not fetched, and a query tile wholly in the
 * padding only stores zeros.  Keys are never split across workgroups: the bits of a (batch, head) depend on its own
 * data, row_start[b], window and T, not on what else the launch holds.                                                */
typedef struct ltxk_causal_attn_args {
  const void* q; const void* k; const void* vt; void* out;
  const int32_t* row_start;
  int32_t ldq, ldk, ldvt, ldo;
  int32_t B, Hq, Hkv, T;
  int32_t window;
  float scale;
} ltxk_causal_attn_args;

int ltxk_causal_attn(const ltxk_causal_attn_args* args, void* stream);
/* sizeof(ltxk_causal_attn_args) in this build (an entry of its own: the ltxk_abi_sizeof index list is closed).          */
int ltxk_causal_attn_args_sizeof(void);

/* Gemma-3 decoding: ltxk_causal_attn for ONE query position per batch row against a per-layer KV cache, with the append fused.
 * The cache is held in ltxk_causal_attn's own operand layouts at T = cap, so a prefill writes it with the encoder's launches:
 *   k_cache : (B,cap,Hkv*256) bf16 row stride ldk          vt_cache : (B,Hkv*256,ldvt >= cap) bf16 = V transposed
 *   cap % 64 == 0; cache positions > step are read in whole tiles and must be finite (a zero-initialised cache).
 *   q      : (B,Hq*256) bf16 row stride ldq, the step's normed and rotated query
 *   k_new  : (B,Hkv*256) row stride ldkn, the step's key after norm and RoPE;  v_new : (B,Hkv*256) row stride ldvn, its value
 *   out    : (B,Hq*256) row stride ldo
 *   row_start (B) DEVICE int32 as above; step: host int, 0 <= step < cap, the new token's position in the padded sequence.
 * Key j is visible iff  row_start[b] <= j <= step  and  (window == 0 or step - j < window).  Key `step` is read from k_new /
 * v_new, never from the cache, and the launch stores k_new into K row `step` and v_new into V^T column `step` (the append;
 * the one wave whose keys hold `step` stores it and no other reads that position).  Every other cache element is left as it
 * was.  row_start[b] > step: an all-zero output row (no NaN); the append still happens.  Hq % Hkv == 0 and Hq/Hkv <= 16: the
 * query heads of one KV head are the 16-wide operand's columns, so a KV head's cache is read once for its group.
 * Rounding points: the "flash" policy above.  Keys are split across workgroups: slice s = keys [256 s, 256 s + 256), one
 * 64-key tile per wave; S in fp32, P = exp2(fma(S, scale*log2 e, -M)) with M the ceil of the tile's maximum over its visible
 * keys, l = sum P in fp32, O = bf16(P) @ V in fp32.  The four tiles of a slice, then the slices, are merged in ascending order:
 * M = max M_i, l = sum l_i 2^(M_i - M), O = sum O_i 2^(M_i - M) - M is an integer, so every factor is an exact power of two -
 * and out = r(O * (1/l)).  A tile wholly outside the visible range is not fetched.  The slices of a launch are
 * [s0, step/256] with s0 = max(0, step - window + 1) / 256 for a window, else 0: a function of step (and window) only, so
 * the bits of a (batch row, head) do not depend on B, on cap or on what else the launch holds.  No atomics; the merge of the
 * slices is a second small launch, as ltxk_gemm_bf16's split-K combine.
 * partials: caller-owned fp32 scratch of >= B * Hq * (step/256 + 1 - s0) * 258 floats ((M, l, O[256]) per batch row, head and
 * slice; B * Hq * ceil(cap/256) * 258 serves every step), 16-byte aligned; partials_floats is its size.                  */
int ltxk_causal_attn_step(const void* q, int32_t ldq, const void* k_new, int32_t ldkn, const void* v_new, int32_t ldvn,
                          void* k_cache, int32_t ldk, void* vt_cache, int32_t ldvt, void* out, int32_t ldo,
                          const int32_t* row_start, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t step,
                          int32_t window, float scale, float* partials, int64_t partials_floats, void* stream);

/* The same step with its position in DEVICE memory, so that a decode step can be recorded once and replayed: the kernel body of
 * ltxk_causal_attn_step (one template), `step` read from *step.  s0, the slice count and the partials' indexing are derived
 * inside the kernel from *step; the grid is sized on the host for max_step (0 <= max_step < cap): min(max_step/256 + 1,
 * (window + 254)/256 + 1) slices under a window - the slices a window can never reach are not launched - else max_step/256 + 1.
 * A workgroup whose slice is past the step's own count leaves before any load or store (a block-uniform exit ahead of the
 * barrier), and the combine launch loops to the device count.  *step outside [0, max_step]: nothing is loaded from or stored
 * to the cache or partials, and out is left as it was.  For *step == step the bits of out, of the appended K row and V^T
 * column and of the live partials equal ltxk_causal_attn_step's, whatever max_step >= step is.
 * partials: >= B * Hq * (that slice count) * 258 floats.                                                                */
int ltxk_causal_attn_dev_step(const void* q, int32_t ldq, const void* k_new, int32_t ldkn, const void* v_new, int32_t ldvn,
                              void* k_cache, int32_t ldk, void* vt_cache, int32_t ldvt, void* out, int32_t ldo,
                              const int32_t* row_start, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, const int32_t* step,
                              int32_t max_step, int32_t window, float scale, float* partials, int64_t partials_floats,
                              void* stream);

/* ltxk_headnorm_rope for rows that all sit at ONE position held in device memory: every one of the M rows takes table row
 * *pos of cos / sin (T,128).  The bits equal ltxk_headnorm_rope on the tables' row *pos with T = 1 (the rotation is the one
 * definition both share).  *pos outside [0, T): no store.                                                               */
int ltxk_headnorm_rope_at(void* buf, int32_t ld, int32_t M, int32_t Hq, int32_t Hkv, const void* q_weight, const void* k_weight,
                          const float* cos, const float* sin, int32_t T, const int32_t* pos, float eps, void* stream);

/* Gemma-3 decoding: sampling on the device.  One token per row of the logits GEMM's own output, logits (B,V) bf16 row stride
 * ld, 1 <= B <= 8, V % 8 == 0, widened to fp32 in registers (no fp32 copy is made), against a caller-owned decode state, all
 * DEVICE int32 unless noted:
 *   ctl = {n, pos, live}: the draw index, the cache position at which the token drawn now will be fed, the rows not finished;
 *   done (B), next_ids (B), history (B,hist_cap) with hist_len (B), tokens_out (B,n_max), eos (n_eos <= 8),
 *   uniforms (n_max,B) fp32 in [0,1).
 * Per row b, n = ctl[0]:
 *   penalty     ctx = the last min(rep_ctx, hist_len[b]) ids of history[b] (rep_ctx <= 64), as a SET: for v in ctx
 *               l'_v = l_v < 0 ? l_v * penalty : l_v / penalty in fp32 (IEEE multiply, correctly rounded divide); every other
 *               l'_v = l_v.  penalty == 1 or an empty ctx touches nothing.
 *   choice      temperature == 0: t = the smallest v with l'_v = max l'.  Otherwise z_v = l'_v / temperature, m = max z,
 *               p_v = exp(z_v - m), S = sum p, target = uniforms[n,b] * S, t = the smallest v with p_v > 0 whose inclusive
 *               prefix sum exceeds target; if rounding leaves none, the largest v with p_v > 0.  Sums run over chunks of 2048
 *               elements (a function of V only) merged in ascending order; the longest sequential fp32 addition chain is
 *               17 + ceil(V/2048).  t is a function of the row's logits, ctx, temperature, penalty and uniform alone.
 *   bookkeeping done[b]: tokens_out[b,n] = -1, next_ids[b] and history[b] stay (a finished row keeps feeding its last token).
 *               Otherwise tokens_out[b,n] = next_ids[b] = t, history[b,hist_len[b]++] = t (dropped once hist_cap is full),
 *               done[b] = t in eos.
 * flags: LTXK_SAMPLE_DRAW runs the above; LTXK_SAMPLE_ADVANCE sets ctl = {n + 1, pos + 1, rows not done} in a launch of its
 * own, which must follow every reader of the old value - a decode step draws first, feeds the token at ctl's pos and
 * advances last; both flags: a draw followed at once by the advance.  n outside [0, n_max): no store anywhere.
 * No atomics and no workgroup waits on another: chunk partials (maximum and argmax, then sums) are merged by later launches.
 * workspace: >= 3 * B * ceil(V/2048) * 4 bytes, 4-byte aligned.  struct_bytes = sizeof(ltxk_sample_args), checked.       */
enum { LTXK_SAMPLE_DRAW = 1, LTXK_SAMPLE_ADVANCE = 2 };

typedef struct {
  int32_t struct_bytes;
  int32_t B, V, ld, n_max, hist_cap, rep_ctx, n_eos, flags;
  float temperature, penalty;
  const void* logits;
  int32_t* ctl;
  int32_t* done;
  int32_t* next_ids;
  int32_t* history;
  int32_t* hist_len;
  int32_t* tokens_out;
  const int32_t* eos;
  const float* uniforms;
  void* workspace;
  int64_t workspace_bytes;
} ltxk_sample_args;

int ltxk_sample_rows(const ltxk_sample_args* args, void* stream);

/* ---------------------------------------------------------------------------------------
 * Step cache (csrc/step_cache.hip): the device side of a timestep-aware step cache of the denoise loop
 * ------------------------------------------------------------------------------------- */
/* ltxk_step_cache_probe: cur, prev (rows, D) bf16, contiguous, 16-byte aligned, not overlapping (checked), D % 8 == 0.  One pass reads both
 * once and writes prev <- cur (a copy of the bytes); sums[0] = S_d = sum |f32(cur) - f32(prev)| (each difference rounded once,
 * to fp32) and sums[1] = S_p = sum |f32(prev)| over the OLD prev, fp32, DEVICE.  Summation order, a function of rows * D alone
 * (not of the grid, the device or timing): chunks of 8192 consecutive elements, inside a chunk 256 threads of four 8-element
 * vectors (vector 256 * k + t of the chunk, k ascending, elements ascending, one chain from 0), the wave butterfly 32 .. 1,
 * the four wave totals in ascending order; the chunk partials go through `workspace` and a second launch adds them in
 * ascending chunk order.  The longest sequential fp32 addition chain is ltxk_step_cache_depth = 40 + ceil(rows * D / 8192) - 1.
 * No atomics and no workgroup waits on another.  flags: LTXK_PROBE_INIT = the copy alone; sums and workspace are not
 * touched (and may be null).  workspace: >= ltxk_step_cache_workspace_bytes(rows, D) = 2 * chunks * 4 bytes, 4-byte aligned,
 * contents irrelevant on entry.  The two size functions return -1 on rows < 1, D < 8, D % 8 != 0 or rows * D > 2^35.   */
enum { LTXK_PROBE_INIT = 1 };
int64_t ltxk_step_cache_workspace_bytes(int64_t rows, int32_t D);
int32_t ltxk_step_cache_depth(int64_t rows, int32_t D);
int ltxk_step_cache_probe(const void* cur, void* prev, int64_t rows, int32_t D, int32_t flags, float* sums, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* The residual of a computed step and its reuse, n bf16 elements each, n % 8 == 0, 16-byte aligned, not overlapping (checked), in place:
 *   ltxk_residual_store:  r <- rbf(f32(x) - f32(r))     (r holds the copy of x taken in front of block 0 on entry)
 *   ltxk_residual_apply:  x <- rbf(f32(x) + f32(r))
 * rbf: round to nearest even to bf16.                                                                                   */
int ltxk_residual_store(const void* x, void* r, int64_t n, void* stream);
int ltxk_residual_apply(void* x, const void* r, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------
 * Video VAE (volumes are channels-last (B,D,H,W,C) bf16; a row = one voxel)
 * ------------------------------------------------------------------------------------- */
enum { LTXK_PAD_ZEROS = 0, LTXK_PAD_REFLECT = 1 };

typedef struct ltxk_conv3d_args {
  const void* x;         /* (B,D,H,W,Cin) bf16, Cin % 64 == 0                              */
  const void* w;         /* (Cout,3,3,3,Cin) bf16 (MLX layout, decoder.py:708-710)         */
  const void* bias;      /* (Cout) bf16                                                    */
  void* out;             /* (B,D,H,W,Cout) bf16                                            */
  const void* resid;     /* optional (B,D,H,W,Cout): out = bf16(conv + resid) (decoder.py:180) */
  const void* zero_page; /* >= 128 zero bytes in device memory (zero-padding source)       */
  int32_t B, D, H, W, Cin, Cout;
  int32_t causal;        /* temporal halo: 1 = 2x first frame; 0 = first + last (convolution.py:126-137);
                          * 2 = zeros on both sides (plain Conv3d padding=1 of the latent upsampler, upsampler.py:6-62) */
  int32_t pad_mode;      /* spatial halo: LTXK_PAD_ZEROS | LTXK_PAD_REFLECT (convolution.py:143-157) */
  /* optional caller-owned fp32 scratch for split-K on small volumes (the decoder's 1024/512-channel stages
   * have too few voxels to fill 256 CUs): S*M*Cout*4 bytes are used if they fit; NULL disables split-K.
   * Partial slabs are written with plain stores and summed in slice order, so results are deterministic. */
  void* workspace;
  int64_t workspace_bytes;
  /* temporal taps: 0 or 3 = the 3x3x3 kernel; 1 = a per-frame 3x3 kernel, w = (Cout,3,3,Cin) (the latent
   * upsampler's nn.Conv2d applied frame by frame, upsampler.py:64-99): only the centre temporal tap exists,
   * K = 9*Cin instead of 27*Cin.  A voxel then reads its own frame alone, whatever `causal` says.      */
  int32_t taps_d;
  /* Optional fused PixelNorm (+ AdaLN modulation) + SiLU of the OUTPUT row (decoder.py:136-180: the pixel_norm / scale /
   * shift / SiLU that follows every conv of a res block; utils.py:477-483):
   *   act_out[v,:] = silu?( modulate?( pixel_norm(y[v,:], act_eps) ) ),  y = this conv's bf16 output row (bias, residual),
   * with the rounding points of ltxk_pixelnorm_act.  Needs Cout == 128 or 256 (the tile then holds whole voxel rows; the
   * row statistic is reduced inside the tile).  act_out == NULL: off.  `out` may be NULL when act_out is set (a conv whose
   * raw output nothing else reads).  act_scale / act_shift: (B,Cout) bf16 or both NULL; act_rows_per_batch = D*H*W. */
  void* act_out;
  const void* act_scale;
  const void* act_shift;
  float act_eps;
  int32_t act_silu;
} ltxk_conv3d_args;

/* nn.Conv3d 3x3x3 stride 1 inside CausalConv3d (convolution.py:78-222) as implicit GEMM.   */
int ltxk_conv3d_k3_bf16(const ltxk_conv3d_args* args, void* stream);

/* The launch form ltxk_conv3d_k3_bf16 takes for `args`, decided without launching anything (host only: pointers are checked
 * for NULL / alignment, never read).  ltxk_conv3d_k3_bf16 decides its form by the same host function, so a plan and a launch
 * of the same arguments cannot disagree; the same argument checks run and return the same error codes.
 * Every form computes a row's sum with the same rounding points; the kw-reuse kernel and the split-K slices walk K in another
 * order than the per-tap single pass.  A tail launch gives its rows the bits of the main tile.                            */
enum { LTXK_CONV_KERNEL_PER_TAP = 0, LTXK_CONV_KERNEL_KW = 1, LTXK_CONV_KERNEL_TAPS = 2 /* ltxk_conv_taps_bf16 */ };
struct ltxk_conv3d_plan {   /* a struct tag only: the name is also the function's */
  int32_t kernel;               /* LTXK_CONV_KERNEL_*: one A tile per tap, or one A panel per (kd, kh) shared by the 3 kw taps */
  int32_t tile_rows, tile_cols; /* workgroup tile of the main launch: 256 x 128 or 160 x 256 (kw: 256 x 128)             */
  int32_t row_tiles, col_tiles; /* tiles of the main launch over the voxel rows and over Cout                            */
  int32_t slices;               /* K slices (1 unless split-K: fp32 slabs in the workspace + a finalize launch)          */
  int32_t ksteps;               /* K-steps per slice, the last slice may have fewer; per-tap: 64 channels of one tap
                                 * (taps * Cin/64 in all), kw: 32 channels of the 3 kw taps of one (kd, kh) (9 * Cin/32)   */
  /* The rows past the last whole round of 256 workgroups run as a second launch of lower tiles (128 rows for the 256-row
   * tile, 96 for the 160-row tile) over rows [tail_m_base, M); the main launch then covers row_tiles * tile_rows rows.
   * All three are 0 when there is no tail launch.                                                                       */
  int32_t tail_tile_rows, tail_m_base, tail_row_tiles;
  int32_t fused_act;            /* 1: the PixelNorm / modulation / SiLU epilogue runs (act_out set)                      */
};
int ltxk_conv3d_plan(const ltxk_conv3d_args* args, struct ltxk_conv3d_plan* plan);
/* sizeof(struct ltxk_conv3d_plan) in this build (an entry of its own: the ltxk_abi_sizeof index list is closed).          */
int ltxk_conv3d_plan_sizeof(void);

/* ---------------------------------------------------------------------------------------
 * Audio VAE decoder and vocoder: a stride-1 convolution over the frames of a channels-last volume as implicit GEMM.
 * Replaces the causal 3x3 nn.Conv2d of the audio decoder (audio_vae/causal_conv_2d.py, resnet.py, upsample.py) and the
 * dilated nn.Conv1d / polyphase-packed nn.ConvTranspose1d of the vocoder (audio_vae/vocoder.py; time is H, W = 1).
 * Every one of the B*D frames is an (H,W) image of its own: no tap reads across a frame or batch boundary.
 *
 *   y[b,d,h,w,co] = bias[co] + sum_{i<kh, j<kw, ci} x[b,d, h + i*dil_h - pad_top, w + j - pad_left, ci] * w[co,i,j,ci]
 *
 * with terms outside the frame zero (they read zero_page; no padded copy exists) and the output extent the input's:
 * pad_top + pad_bottom == (kh-1)*dil_h, pad_left + pad_right == kw-1.  kh <= 16, kw in {1,3}, dil_h <= 8, Cin 32 or a multiple
 * of 64 (at 32 a 64-wide K-step spans two taps; with an odd tap count the last half step reads zero_page on both operand
 * sides), any Cout >= 1 (only valid columns are stored), M = B*D*H*W >= 1.
 * One epilogue, rounding in this order (acc fp32):
 *   1. y = bf16(acc + bias)
 *   2. resid:           y = bf16(y + resid)
 *   3. n_mean = 2 | 3:  y = bf16((y + mean_a1 [+ mean_a2]) / n_mean), summed in fp32 in that order
 *   4. out = y                                        (optional)
 *   5. act_out = max(y, bf16(y * slope))              (optional; leaky ReLU as resnet.py:15-17 writes it)
 *   6. out_f32 = tanhf(acc + bias), fp32, unrounded   (conv_post + tanh; excludes 2-5)
 * Small launches split K as ltxk_conv3d_k3_bf16 does: fp32 slabs [slice][M][round_up(Cout,4)] in the workspace, a finalize
 * launch that sums in slice order and runs the same epilogue.  No atomics: bits depend on the arguments alone.             */
typedef struct ltxk_conv_taps_args {
  int32_t struct_bytes;   /* sizeof(ltxk_conv_taps_args) of the caller's build; checked                                  */
  int32_t B, D, H, W, Cin, Cout;
  int32_t kh, kw, dil_h;
  int32_t pad_top, pad_bottom, pad_left, pad_right;
  int32_t n_mean;         /* 0, or 2 / 3 with mean_a1 [/ mean_a2]                                                        */
  float slope;            /* of act_out                                                                                  */
  const void* x;          /* (B,D,H,W,Cin) bf16, 16-byte aligned                                                         */
  const void* w;          /* (Cout,kh,kw,Cin) bf16, 16-byte aligned                                                      */
  const void* bias;       /* (Cout) bf16                                                                                 */
  const void* zero_page;  /* >= 128 zero bytes, 16-byte aligned                                                          */
  const void* resid;      /* (M,Cout) bf16 or NULL                                                                       */
  const void* mean_a1;    /* (M,Cout) bf16, n_mean >= 2                                                                  */
  const void* mean_a2;    /* (M,Cout) bf16, n_mean == 3                                                                  */
  void* out;              /* (M,Cout) bf16 or NULL                                                                       */
  void* act_out;          /* (M,Cout) bf16 or NULL                                                                       */
  float* out_f32;         /* (M,Cout) fp32 or NULL: the tanh form                                                        */
  void* workspace;        /* fp32 split-K scratch or NULL (no split-K)                                                   */
  int64_t workspace_bytes;
} ltxk_conv_taps_args;

int ltxk_conv_taps_bf16(const ltxk_conv_taps_args* args, void* stream);
/* The launch form of ltxk_conv_taps_bf16 for `args`, by the host function the launch uses: kernel = LTXK_CONV_KERNEL_TAPS,
 * tile 256 x 128 (Cout > 64) or 256 x 64, ksteps = 64-wide K-steps per slice (ceil(kh*kw*Cin / 64) in all), no tail launch,
 * fused_act = 0 (that field speaks of the PixelNorm epilogue).                                                          */
int ltxk_conv_taps_plan(const ltxk_conv_taps_args* args, struct ltxk_conv3d_plan* plan);

/* pixel_norm over channels [+ (1+scale)+shift per (batch,channel)] [+ SiLU]: decoder.py:136-180,
 * 415-437; utils.py:477-483.  x,y: (V,C) rows = voxels, C in {64..2048, power of two}.
 * scale/shift: (B,C) bf16 or NULL; rows_per_batch = D*H*W.                                 */
int ltxk_pixelnorm_act(const void* x, void* y, int64_t V, int32_t C, float eps, const void* scale,
                       const void* shift, int64_t rows_per_batch, int32_t apply_silu, void* stream);

/* DepthToSpaceUpsample tail (sampling.py:143-197): conv (B,D,H,W,8*Co) -> out (B,2D-1,2H,2W,Co),
 * channel (c,st,sh,sw), first output frame dropped, plus the residual d2s(xin) tiled over
 * channels (xin (B,D,H,W,Ci) or NULL).                                                     */
int ltxk_d2s_add(const void* conv, const void* xin, void* out, int32_t B, int32_t D, int32_t H, int32_t W,
                 int32_t Co, int32_t Ci, void* stream);

/* SpaceToDepthDownsample tail (sampling.py:53-103): conv (B,Dp,Hp,Wp,Cc) and the (front-frame
 * duplicated) input xpad (B,Dp,Hp,Wp,Cx) -> out (B,Dp/st,Hp/sh,Wp/sw,Cc*st*sh*sw) =
 * s2d(conv) + group-mean_G(s2d(xpad)), G = Cx/Cc.                                          */
int ltxk_s2d_skip(const void* conv, const void* xpad, void* out, int32_t B, int32_t Dp, int32_t Hp,
                  int32_t Wp, int32_t Cc, int32_t Cx, int32_t st, int32_t sh, int32_t sw, int32_t G,
                  void* stream);

/* latents (B,C,S) channels-first -> (B,S,C) channels-last with fp32 x*std+mean (decoder.py:349-355);
 * noise != NULL: the timestep-conditioned decoder's blend noise*s + (1-s)*x first (decoder.py:381-385). */
int ltxk_latent_denorm_cl(const void* latent, const void* noise, float noise_scale, const void* mean,
                          const void* std, void* out, int32_t B, int32_t C, int64_t S, void* stream);

/* (B,S,ldx>=C) channels-last -> (B,C,S) channels-first with fp32 (x-mean)/std (ops.py:94-109). */
int ltxk_latent_norm_cf(const void* x, int32_t ldx, const void* mean, const void* std, void* out,
                        int32_t B, int32_t C, int64_t S, void* stream);

/* conv_out (B,D,H,W,C*P*P) channels-last -> unpatchify (ops.py:47-80, channel order (c,p_w,p_h))
 * -> video (B,C,D,H*P,W*P) channels-first.  Bit-exact index map.                           */
int ltxk_unpatchify_cf(const void* x, void* out, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C,
                       int32_t P, void* stream);

/* video (B,C,D,H,W) -> patchify (ops.py:9-44) -> (B,D,H/P,W/P,Cpad) channels-last, channels
 * beyond C*P*P zero (pads 48 -> 64 for the first encoder convolution).                     */
int ltxk_patchify_cl(const void* video, void* out, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W,
                     int32_t P, int32_t Cpad, void* stream);

/* video (B,C,F,H,W) bf16 in [-1,1] -> uint8 frames (B,F,H,W,C): generate.py:3894-3898.     */
int ltxk_to_uint8(const void* x, void* out, int32_t B, int32_t C, int32_t F, int32_t H, int32_t W,
                  void* stream);

/* Area resize of conditioning frames, DOWNscaling only: cv2.resize(frame, (OW,OH), interpolation=cv2.INTER_AREA) on float
 * frames (prepare_video_for_encoding, utils.py:699-705; OpenCV resizeArea_: destination pixel d averages the source
 * interval [d*scale,(d+1)*scale) with fractional end weights, horizontal pass then vertical pass in fp32).
 * x: `planes` contiguous (H,W) planes, fp32 (x_is_f32 != 0) or bf16; out: planes x (OH,OW) bf16.  Linear, so it may be
 * applied to frames already mapped to [-1,1].                                               */
int ltxk_resize_area(const void* x, int32_t x_is_f32, void* out, int64_t planes, int32_t H, int32_t W,
                     int32_t OH, int32_t OW, void* stream);

/* GroupNorm over (D*H*W, C/G) per (batch, group) in fp32 + affine [+ residual] [+ SiLU]:
 * upsampler.py:65-98,160-174.  x,out (B,V,C) bf16 channels-last, gamma/beta (C) bf16.
 *   y = bf16((x-mean)/sqrt(var+eps)*gamma+beta); if resid: y = bf16(y+resid); if silu: bf16(silu(y)) */
int ltxk_groupnorm_act(const void* x, void* out, const void* gamma, const void* beta, const void* resid,
                       int32_t B, int64_t V, int32_t C, int32_t G, float eps, int32_t apply_silu,
                       void* stream);

/* Tiled-decode blending (tiling.py:399-447): acc[b,c,t0+t,h0+y,w0+x] += tile[b,c,t,y,x]*m,
 * wsum[b,t0+t,h0+y,w0+x] += m with m = mt[t]*mh[y]*mw[x]; tile (B,C,Tt,Th,Tw) bf16 of which the
 * leading (at,ah,aw) box is used; acc (B,C,F,H,W) / wsum (B,F,H,W) fp32.                    */
int ltxk_tile_blend_accum(const void* tile, int32_t Tt, int32_t Th, int32_t Tw, int32_t at, int32_t ah,
                          int32_t aw, const float* mt, const float* mh, const float* mw, float* acc,
                          float* wsum, int32_t B, int32_t C, int32_t F, int32_t H, int32_t W, int32_t t0,
                          int32_t h0, int32_t w0, void* stream);

/* out = bf16(acc / max(wsum, 1e-8)) (tiling.py:492-509); S = F*H*W.                         */
int ltxk_tile_blend_finalize(const float* acc, const float* wsum, void* out, int32_t B, int32_t C,
                             int64_t S, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTXK_H */
