// Fused bias + GeLU (tanh) forward/backward, bf16, gfx950.
//
// y = gelu(x + b); bwd recomputes the pre-activation from x,b (no saved
// activation: 1 extra read instead of a [N,Dff] bf16 save — HBM3E-friendly).
// dbias uses deterministic per-block LDS partials + colsum (colsum.hip).
// x: [N, D] bf16 row-major, b: [D] bf16.
//
// Round 2: 4 packets per thread per iteration for memory-level parallelism,
// laid out BLOCK-STRIDED (packet p of thread t at tile + p*BG_BLOCK*8 + t*8)
// so every b128 load instruction stays perfectly dense across the wave —
// the first attempt used 4 CONSECUTIVE packets per thread (64 B lane
// stride), which broke per-instruction coalescing and measured ~15% slower
// than round 1.  Fast path needs the grid stride and the per-packet stride
// (BG_BLOCK*8 = 2048) multiples of D and n % 8 == 0; generic fallback
// otherwise (bias_gelu_grid below rounds the grid accordingly).

#include "common.h"
#include "launchers.h"
#include <algorithm>
#include <numeric>

#define BG_BLOCK 256
#define BG_PK 4                      // packets of 8 bf16 per iteration
#define BG_TILE (BG_BLOCK * 8)       // elements per packet-slab per block

extern "C" {

__global__ void __launch_bounds__(BG_BLOCK)
bias_gelu_fwd_kernel(const short* __restrict__ x, const short* __restrict__ b,
                     short* __restrict__ y, long n_elem, int D) {
  long tile0 = (long)blockIdx.x * (BG_TILE * BG_PK) + threadIdx.x * 8;
  long stride = (long)gridDim.x * (BG_TILE * BG_PK);
  if (stride % D == 0) {
    // per-packet columns are loop-invariant: hoist the bias loads
    float bb[BG_PK * 8];
#pragma unroll
    for (int p = 0; p < BG_PK; ++p) {
      int col = (int)((tile0 + p * BG_TILE) % D);
      short8_t b8 = *(const short8_t*)(b + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) bb[8 * p + j] = bf16_to_f32(b8[j]);
    }
    for (long i = tile0; i < n_elem; i += stride) {
      short8_t v[BG_PK];
      bool ok[BG_PK];
#pragma unroll
      for (int p = 0; p < BG_PK; ++p) {
        ok[p] = i + p * BG_TILE < n_elem;
        v[p] = ok[p] ? *(const short8_t*)(x + i + p * BG_TILE) : short8_t{};
      }
#pragma unroll
      for (int p = 0; p < BG_PK; ++p) {
        if (!ok[p]) continue;
        short8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = f32_to_bf16(gelu_tanh(bf16_to_f32(v[p][j]) + bb[8 * p + j]));
        *(short8_t*)(y + i + p * BG_TILE) = o;
      }
    }
    return;
  }
  // generic path (one packet per iteration, per-packet bias reload)
  long idx0 = ((long)blockIdx.x * BG_BLOCK + threadIdx.x) * 8;
  long gstride = (long)gridDim.x * BG_BLOCK * 8;
  for (long i = idx0; i < n_elem; i += gstride) {
    short8_t v = *(const short8_t*)(x + i);
    int col = (int)(i % D);  // D % 8 == 0 so the packet stays in one row
    short8_t b8 = *(const short8_t*)(b + col);
    short8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f32_to_bf16(gelu_tanh(bf16_to_f32(v[j]) + bf16_to_f32(b8[j])));
    *(short8_t*)(y + i) = o;
  }
}

}  // extern "C" (the template below needs C++ linkage)

// dbias: each thread's per-packet fixed 8-column windows accumulate in
// registers and merge once at the END (not per element) into one per-block
// f32 partial row for the deterministic colsum reduction.
//
// OWNED (D % BG_TILE == 0, i.e. D a multiple of 2048): a column is only
// ever touched by ONE thread of the block, whose packets add to it in
// program order, so the LDS row needs no ordering between threads.
//
// !OWNED, fast path (any other D whose grid stride is a multiple of D):
// threads of different waves share columns (t and t+128 at D=1024), so the
// merge goes through a [BG_PK * BG_TILE] LDS slab instead: every thread
// stores its 32 partials at the block-relative element index they belong
// to, and the thread that owns column c adds the slab entries e0, e0 + D,
// e0 + 2D, ... in ascending order.  Same order on every run, no atomics.
//
// The generic fallback (grid stride not a multiple of D: D >= 16392 with an
// odd factor) still merges per element with LDS atomics.
template <bool OWNED>
__global__ void __launch_bounds__(BG_BLOCK)
bias_gelu_bwd_kernel(const short* __restrict__ dy, const short* __restrict__ x,
                     const short* __restrict__ b, short* __restrict__ dx,
                     float* __restrict__ ws_dbias, long n_elem, int D) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // OWNED and the fallback: [D] block partial; !OWNED fast path: the slab
  float* sdb = (float*)smem;
  long tile0 = (long)blockIdx.x * (BG_TILE * BG_PK) + threadIdx.x * 8;
  long stride = (long)gridDim.x * (BG_TILE * BG_PK);
  const bool fast = stride % D == 0;
  if (OWNED || !fast) {
    for (int i = threadIdx.x; i < D; i += BG_BLOCK) sdb[i] = 0.f;
    __syncthreads();
  }
  if (fast) {
    float acc[BG_PK * 8] = {0.f};
    int cols[BG_PK];
    float bb[BG_PK * 8];
#pragma unroll
    for (int p = 0; p < BG_PK; ++p) {
      cols[p] = (int)((tile0 + p * BG_TILE) % D);
      short8_t b8 = *(const short8_t*)(b + cols[p]);
#pragma unroll
      for (int j = 0; j < 8; ++j) bb[8 * p + j] = bf16_to_f32(b8[j]);
    }
    for (long i = tile0; i < n_elem; i += stride) {
      short8_t vd[BG_PK], vx[BG_PK];
      bool ok[BG_PK];
#pragma unroll
      for (int p = 0; p < BG_PK; ++p) {
        ok[p] = i + p * BG_TILE < n_elem;
        vd[p] = ok[p] ? *(const short8_t*)(dy + i + p * BG_TILE) : short8_t{};
        vx[p] = ok[p] ? *(const short8_t*)(x + i + p * BG_TILE) : short8_t{};
      }
#pragma unroll
      for (int p = 0; p < BG_PK; ++p) {
        if (!ok[p]) continue;
        short8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float g = bf16_to_f32(vd[p][j]);
          float pre = bf16_to_f32(vx[p][j]) + bb[8 * p + j];
          float dpre = g * gelu_tanh_grad(pre);
          o[j] = f32_to_bf16(dpre);
          acc[8 * p + j] += dpre;
        }
        *(short8_t*)(dx + i + p * BG_TILE) = o;
      }
    }
    if (OWNED) {
#pragma unroll
      for (int p = 0; p < BG_PK; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          atomicAdd(&sdb[cols[p] + j], acc[8 * p + j]);
    } else {
#pragma unroll
      for (int p = 0; p < BG_PK; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          sdb[p * BG_TILE + threadIdx.x * 8 + j] = acc[8 * p + j];
      __syncthreads();
      // slab entry e holds the partial of column (off + e) % D
      const int off = (int)((long)blockIdx.x * (BG_TILE * BG_PK) % D);
      float* out = ws_dbias + (long)blockIdx.x * D;
      for (int c = threadIdx.x; c < D; c += BG_BLOCK) {
        float s = 0.f;
        for (int e = (c - off + D) % D; e < BG_TILE * BG_PK; e += D)
          s += sdb[e];
        out[c] = s;
      }
      return;
    }
  } else {
    long idx0 = ((long)blockIdx.x * BG_BLOCK + threadIdx.x) * 8;
    long gstride = (long)gridDim.x * BG_BLOCK * 8;
    for (long i = idx0; i < n_elem; i += gstride) {
      short8_t vd = *(const short8_t*)(dy + i);
      short8_t vx = *(const short8_t*)(x + i);
      int col = (int)(i % D);
      short8_t b8 = *(const short8_t*)(b + col);
      short8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g = bf16_to_f32(vd[j]);
        float pre = bf16_to_f32(vx[j]) + bf16_to_f32(b8[j]);
        float dpre = g * gelu_tanh_grad(pre);
        o[j] = f32_to_bf16(dpre);
        atomicAdd(&sdb[col + j], dpre);
      }
      *(short8_t*)(dx + i) = o;
    }
  }
  __syncthreads();
  float* out = ws_dbias + (long)blockIdx.x * D;
  for (int i = threadIdx.x; i < D; i += BG_BLOCK) out[i] = sdb[i];
}

// Launch geometry, shared by forward and backward: one block per
// BG_BLOCK * BG_PK packets up to `cap`, then rounded UP to a multiple of
// D / gcd(D, BG_TILE * BG_PK) so that the kernels' grid stride
// (grid * BG_TILE * BG_PK elements) is a multiple of D: their fast path, with
// a fixed per-thread column window.  A D whose rounding unit exceeds
// BG_MAX_ROUND_UNIT keeps the unrounded grid and takes the generic path.
// The backward cap is lower because its [grid, D] dbias workspace and the
// column sum over it scale with the grid.
#define BG_FWD_MAX_GRID 4096
#define BG_BWD_MAX_GRID 1024
#define BG_MAX_ROUND_UNIT 2048
static int bias_gelu_grid(long n_elem, int D, long cap) {
  long grid = std::min((n_elem / (BG_PK * 8) + BG_BLOCK - 1) / BG_BLOCK, cap);
  const long unit = D / std::gcd((long)D, (long)(BG_TILE * BG_PK));
  if (unit <= BG_MAX_ROUND_UNIT) grid = (grid + unit - 1) / unit * unit;
  return (int)grid;
}

extern "C" {

hipError_t bias_gelu_fwd_launch(const void* x, const void* b, void* y,
                                long n_elem, int D, hipStream_t s) {
  const int grid = bias_gelu_grid(n_elem, D, BG_FWD_MAX_GRID);
  bias_gelu_fwd_kernel<<<grid, BG_BLOCK, 0, s>>>((const short*)x, (const short*)b,
                                                 (short*)y, n_elem, D);
  return hipGetLastError();
}

hipError_t bias_gelu_bwd_launch(const void* dy, const void* x, const void* b,
                                void* dx, void* ws_dbias, long n_elem, int D,
                                hipStream_t s) {
  const int grid = bias_gelu_grid(n_elem, D, BG_BWD_MAX_GRID);
  // [D] block partial, or the [BG_PK * BG_TILE] merge slab of the !OWNED
  // fast path, whichever the kernel will use
  size_t shm = (size_t)D * sizeof(float);
  if (D % BG_TILE == 0) {
    bias_gelu_bwd_kernel<true><<<grid, BG_BLOCK, shm, s>>>(
        (const short*)dy, (const short*)x, (const short*)b, (short*)dx,
        (float*)ws_dbias, n_elem, D);
  } else {
    if ((long)grid * (BG_TILE * BG_PK) % D == 0)
      shm = (size_t)BG_TILE * BG_PK * sizeof(float);
    bias_gelu_bwd_kernel<false><<<grid, BG_BLOCK, shm, s>>>(
        (const short*)dy, (const short*)x, (const short*)b, (short*)dx,
        (float*)ws_dbias, n_elem, D);
  }
  return hipGetLastError();
}

// One ws_dbias row per block of the backward grid.
int bias_gelu_bwd_ws_rows(long n_elem, int D) {
  return bias_gelu_grid(n_elem, D, BG_BWD_MAX_GRID);
}

}  // extern "C"
