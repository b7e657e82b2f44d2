// Row quantiser in front of ltxk_gemm_mxfp4 (ltxk_quant_rows_mxfp4, include/ltxk.h): bf16 rows -> OCP MXFP4 code bytes + one
// e8m0 scale byte per 32 consecutive k, bit for bit what weights.quantize_mxfp4 gives for the same matrix.
//
// Integer arithmetic on the bf16 bit patterns throughout, so neither the fp32 denormal mode nor a conversion instruction's
// rounding of ties, saturation or subnormals enters (v_cvt_scalef32_pk_fp4_bf16 exists; its behaviour at those inputs is not
// documented where this project could check it, and the definition here is the Python one):
//   mag   = bits & 0x7fff                      (orders like |x|)
//   E     = amax_mag == 0 ? 127 : max((amax_mag >> 7) - 2, 0)
//           (the exponent field is floor(log2 amax) + 127 for normal numbers; subnormal and the two lowest binades clamp at 0;
//            the largest field, 254, gives 252: byte 255 cannot appear)
//   P     = the bf16 pattern of |x| * 2^127:  mag + (127 << 7) for normal x, pattern(float(mag)) - (6 << 7) for subnormal x
//           (mag * 2^-133 * 2^127 = mag * 2^-6) - a 7-bit significand either way, exact
//   xb    = P - (E << 7)                       = the pattern of |x| / 2^(E-127) whenever that is a normal number; smaller and
//           negative values mean "below 2^-126", which is below every midpoint
//   index = number of midpoints 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0 (as bf16 patterns) that xb passes, a tie passing when the
//           upper index is even; xb < 8.0 always (x / scale < 8), so 7 = 6.0 is the saturation
// (tests/test_mxfp4_dit_cpu.py holds a transcription of this rule - the same midpoint patterns, the same > / >= pattern - to
// quantize_mxfp4 over every finite bf16 pattern: change the two together.)
// Four lanes share a block: each loads 16 bytes (8 elements), the block maximum is two lane exchanges, each lane stores its 4
// code bytes and the first of the four the scale byte.  One workgroup per row; no LDS, no atomics.
#include "common.h"

namespace ltxk {

typedef unsigned u32x4_q __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned e2m1_code(unsigned h, int E) {
  const int mag = (int)(h & 0x7fffu);
  const int P = mag >= 0x80 ? mag + (127 << 7) : (int)(__float_as_uint((float)mag) >> 16) - (6 << 7);
  const int xb = P - (E << 7);
  const unsigned idx = (unsigned)(xb > 0x3E80) + (unsigned)(xb >= 0x3F40) + (unsigned)(xb > 0x3FA0) + (unsigned)(xb >= 0x3FE0) +
                       (unsigned)(xb > 0x4020) + (unsigned)(xb >= 0x4060) + (unsigned)(xb > 0x40A0);
  return idx | ((h >> 12) & 8u);
}

__global__ __launch_bounds__(256) void quant_rows_mxfp4_kernel(const uint16_t* __restrict__ x, int lda, uint8_t* __restrict__ q, int ldq,
                                                               uint8_t* __restrict__ sc, int lds, int K) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const uint16_t* xr = x + row * lda;
  uint8_t* qr = q + row * ldq;
  uint8_t* sr = sc + row * lds;
  const int nch = K >> 3;                      // 8-element chunks; a multiple of 4, so the four lanes of a block stay together
  for (int c = tid; c < nch; c += 256) {
    const u32x4_q v = *(const u32x4_q*)(xr + (size_t)c * 8);
    int amax = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lo = (int)(v[j] & 0x7fffu), hi = (int)((v[j] >> 16) & 0x7fffu);
      amax = amax > lo ? amax : lo;
      amax = amax > hi ? amax : hi;
    }
    int o = __shfl_xor(amax, 1);
    amax = amax > o ? amax : o;
    o = __shfl_xor(amax, 2);
    amax = amax > o ? amax : o;
    int E = (amax >> 7) - 2;
    E = amax == 0 ? 127 : (E > 0 ? E : 0);
    unsigned codes = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      codes |= e2m1_code(v[j] & 0xffffu, E) << (8 * j);
      codes |= e2m1_code(v[j] >> 16, E) << (8 * j + 4);
    }
    *(unsigned*)(qr + (size_t)c * 4) = codes;
    if ((c & 3) == 0) sr[c >> 2] = (uint8_t)E;
  }
}

}  // namespace ltxk

using namespace ltxk;

extern "C" int ltxk_quant_rows_mxfp4(const void* x, int32_t lda, void* codes, int32_t ldq, uint8_t* block_scales, int32_t lds,
                                     int32_t M, int32_t K, void* stream) {
  const char* name = "ltxk_quant_rows_mxfp4";
  LTXK_CHECK_ARG(x && codes && block_scales && M > 0 && K > 0, "%s: null/empty input", name);
  LTXK_CHECK_ARG(K % 32 == 0, "%s: K=%d must be a multiple of 32", name, K);
  LTXK_CHECK_ARG(lda >= K && lda % 8 == 0 && ldq >= K / 2 && ldq % 16 == 0 && lds >= K / 32,
                 "%s: lda=%d (>= K, multiple of 8), ldq=%d (>= K/2, multiple of 16), lds=%d (>= K/32)", name, lda, ldq, lds);
  LTXK_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & 15) == 0, "%s: x and codes must be 16-byte aligned", name);
  hipLaunchKernelGGL(quant_rows_mxfp4_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (int)lda,
                     (uint8_t*)codes, (int)ldq, block_scales, (int)lds, (int)K);
  LTXK_CHECK_LAUNCH(name);
  return LTXK_OK;
}
