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

// ---- attention-probability dropout (flash_attn.hip) --------------------------
// One call covers one 4 x 4 block of the [L, L] probability matrix of one
// (b, h), nb = ceil(L / 4) blocks a side:
//   counter = (blk & 0xffffffff, blk >> 32, site, call),
//             blk = ((b * H + h) * nb + q / 4) * nb + k / 4 as a 64-bit value
//   key     = (seed & 0xffffffff, seed >> 32)
// Output word q & 3 holds row q of the block, its byte k & 3 (byte 0 the
// lowest) element (q, k); the element is kept iff that byte >= thr.  site is
// 0x10000 + layer, above every residual site.  A function of (seed, call,
// layer, b, h, q, k) alone: the three flash kernels hold the scores in two
// transposed register layouts and draw the same bits.
//
// What a launch carries: thr in [1, 255] (0 = no dropout), scale =
// 256 / (256 - thr), the inverse of the effective keep rate.
struct FaDrop {
  unsigned seed_lo, seed_hi, call, site, thr;
  float scale;
};

__host__ __device__ __forceinline__ FaDrop fa_drop_make(
    unsigned long long seed, unsigned call, unsigned site, unsigned thr) {
  return {(unsigned)seed, (unsigned)(seed >> 32), call, site, thr,
          256.0f / (float)(256u - thr)};
}

// The four words of block blk.
__host__ __device__ __forceinline__ void fa_drop_block(const FaDrop& dr,
                                                       unsigned long long blk,
                                                       unsigned (&w)[4]) {
  w[0] = (unsigned)blk; w[1] = (unsigned)(blk >> 32);
  w[2] = dr.site; w[3] = dr.call;
  philox4x32_10(w, dr.seed_lo, dr.seed_hi);
}

// Element (q, k) of the block whose words are w.
__host__ __device__ __forceinline__ bool fa_drop_keep(const FaDrop& dr,
                                                      const unsigned (&w)[4],
                                                      int q, int k) {
  return ((w[q & 3] >> (8 * (k & 3))) & 0xffu) >= dr.thr;
}

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
