// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11) with the Random123 constants, and the dropout mask built on it.
// Host and device compile the same code, so the known-answer vectors can be
// checked without a GPU; tosem2021_amd/ops/reference.py holds the same
// definition in NumPy.
//
// One call covers one 8-element packet (the short8 unit the LayerNorm kernels
// stream):
//   counter = (pkt & 0xffffffff, pkt >> 32, site, call),
//             pkt = (row * D + col) / 8 as a 64-bit value
//   key     = (seed & 0xffffffff, seed >> 32)
// Output word w gives element 2w from its low and element 2w+1 from its high
// 16 bits; an element is kept iff its 16 bits >= thr.  The mask is a function
// of (seed, call, site, element index) alone, never of launch geometry.
#pragma once

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ void philox4x32_10(unsigned (&c)[4],
                                                       unsigned k0,
                                                       unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0];
    const unsigned long long p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (unsigned)p1; c[2] = n2; c[3] = (unsigned)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// What a dropout launch carries: plain kernel arguments.  scale is
// 65536 / (65536 - thr), the inverse of the effective keep rate.
struct LnDrop {
  unsigned seed_lo, seed_hi, call, site, thr;
  float scale;
};

// Keep bits of packet pkt: bit j set = element j of the packet is kept.
__host__ __device__ __forceinline__ unsigned drop_keep8(const LnDrop& dr,
                                                        long pkt) {
  unsigned c[4] = {(unsigned)pkt, (unsigned)((unsigned long long)pkt >> 32),
                   dr.site, dr.call};
  philox4x32_10(c, dr.seed_lo, dr.seed_hi);
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned bits = (c[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    m |= (bits >= dr.thr ? 1u : 0u) << j;
  }
  return m;
}
