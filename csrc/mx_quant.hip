// MXFP8 quantising kernels for gfx950: the operands of the block-scaled GEMM
// (ops.mx_linear).  Inference only.  Format, lane map and the conversion:
// mx.h; the third producer, Add+LayerNorm with MX output, is an output mode
// of the forward kernels in layernorm.hip.
//
// Both kernels here see the tensor as a flat run of 16-byte packets (8 bf16):
// K % 32 == 0 makes every 32-element block four consecutive packets of the
// flat index, whatever the row length, so thread t of the grid takes packet
// t, t + stride, ... and a lane quad always holds one whole block.  The
// packet count is a multiple of 4 and so is the stride: a quad is active or
// idle as a whole.
//
//   mx_quant_rows   x [R, K] bf16 -> q [R, K] e4m3 bytes, s [R, K/32] e8m0
//                   2 B read, 1 + 1/32 B written per element.
//   mx_bias_gelu    the same of bf16(gelu_tanh(h + b)), b [K] bf16: the value
//                   bias_gelu_fwd_kernel stores, rounded to bf16 in registers
//                   by the same expression (gelu_tanh of common.h), then
//                   quantised.

#include "common.h"
#include "launchers.h"
#include "mx.h"
#include <algorithm>

#define MXQ_BLOCK 256
// One packet per thread up to the cap, grid-stride beyond it.
#define MXQ_MAX_GRID 2048

template <bool GELU>
__global__ void __launch_bounds__(MXQ_BLOCK)
mx_quant_kernel(const short* __restrict__ x, const short* __restrict__ b,
                unsigned char* __restrict__ q, unsigned char* __restrict__ sc,
                long n_pkt, int K) {
  const long stride = (long)gridDim.x * MXQ_BLOCK;
  long i = (long)blockIdx.x * MXQ_BLOCK + threadIdx.x;
  // the packet's column, carried along the grid-stride loop in 32 bits: a
  // 64-bit modulo per packet costs more than the GeLU (col, step < K)
  int col = GELU ? (int)(i * 8 % K) : 0;
  const int step = GELU ? (int)(stride * 8 % K) : 0;
  for (; i < n_pkt; i += stride) {
    const long elem = i * 8;
    short8_t v = *(const short8_t*)(x + elem);
    if (GELU) {
      // K % 8 == 0: the packet stays inside one row
      short8_t b8 = *(const short8_t*)(b + col);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = f32_to_bf16(gelu_tanh(bf16_to_f32(v[j]) + bf16_to_f32(b8[j])));
      col += step;
      if (col >= K) col -= K;
    }
    mx_store_packet(v, elem, q, sc);
  }
}

static int mx_quant_grid(long n_pkt) {
  return (int)std::min((n_pkt + MXQ_BLOCK - 1) / MXQ_BLOCK,
                       (long)MXQ_MAX_GRID);
}

extern "C" {

hipError_t mx_quant_rows_launch(const void* x, void* q, void* s, long R, int K,
                                hipStream_t stream) {
  if (R <= 0 || K <= 0 || K % 32) return hipErrorInvalidValue;
  const long n_pkt = R * K / 8;
  mx_quant_kernel<false><<<mx_quant_grid(n_pkt), MXQ_BLOCK, 0, stream>>>(
      (const short*)x, nullptr, (unsigned char*)q, (unsigned char*)s, n_pkt,
      K);
  return hipGetLastError();
}

hipError_t mx_bias_gelu_launch(const void* h, const void* b, void* q, void* s,
                               long R, int K, hipStream_t stream) {
  if (R <= 0 || K <= 0 || K % 32) return hipErrorInvalidValue;
  const long n_pkt = R * K / 8;
  mx_quant_kernel<true><<<mx_quant_grid(n_pkt), MXQ_BLOCK, 0, stream>>>(
      (const short*)h, (const short*)b, (unsigned char*)q, (unsigned char*)s,
      n_pkt, K);
  return hipGetLastError();
}

}  // extern "C"
