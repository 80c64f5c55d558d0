// OCP MXFP8 (e4m3 elements, one e8m0 scale per 32 consecutive elements) for
// the quantising kernels: csrc/mx_quant.hip and the MX output mode of
// csrc/layernorm.hip.  The format is defined in plain torch by
// ops.reference.mx_quantize; docs/KERNELS.md "MXFP8 operands".
//
// Lane map: a lane holds one packet of 8 consecutive bf16 values and packet i
// of a row (or of the flat tensor) sits in lane i % 64 of its wave, so one
// 32-element block is the four packets of a lane quad {4g .. 4g + 3}.  All
// four lanes of a quad must be active together; K % 32 == 0 guarantees it
// wherever a loop bound cuts a wave.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(2))) unsigned int uint2_t;

// The block's scale byte from one lane's packet: s = max(E - 8, 0), E the
// biased exponent field of the quad's largest magnitude.  bf16 magnitudes
// order like their bit patterns, so the maximum is an integer one and two
// cross-lane steps inside the quad finish it.  E <= 255 keeps s <= 247: the
// NaN scale 255 never appears, whatever the input.
__device__ __forceinline__ int mx_block_scale(short8_t v) {
  int m = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = max(m, (int)v[j] & 0x7fff);
  m = max(m, __shfl_xor(m, 1, WAVE));
  m = max(m, __shfl_xor(m, 2, WAVE));
  return max((m >> 7) - 8, 0);
}

// q = e4m3fn(clamp(x * 2^(127 - s), -448, 448)) for the 8 values of a packet,
// element j in byte j of the 8 returned bytes.  The multiplier's exponent
// field is 254 - s >= 7, a normal f32, and the product is exact unless it
// underflows far below e4m3's half-ulp at zero.  The clamp comes first
// because a scaled magnitude reaches (448, 512) whenever the block maximum's
// mantissa is above 1.75; the convert is gfx950's OCP e4m3fn one, round to
// nearest even with subnormals.
__device__ __forceinline__ uint2_t mx_pack8(short8_t v, int s) {
  union { unsigned int i; float f; } mul;
  mul.i = (unsigned int)(254 - s) << 23;
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = __builtin_fminf(__builtin_fmaxf(bf16_to_f32(v[j]) * mul.f, -448.f),
                           448.f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return uint2_t{(unsigned int)lo, (unsigned int)hi};
}

// Quantise one lane's packet whose first element has offset `elem` in a
// tensor with q [.., K] and s [.., K / 32]: 8 bytes of q per lane, and the
// quad's first lane writes the block's scale byte.
__device__ __forceinline__ void mx_store_packet(short8_t v, long elem,
                                                unsigned char* __restrict__ q,
                                                unsigned char* __restrict__ sc) {
  const int s = mx_block_scale(v);
  *(uint2_t*)(q + elem) = mx_pack8(v, s);
  if ((elem & 31) == 0) sc[elem >> 5] = (unsigned char)s;
}
