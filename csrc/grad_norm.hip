// Global gradient norm over the FLAT gradient buffer, gfx950: the clip factor
// and the non-finite guard for the fused AdamW step (csrc/adamw.hip).
//
// Two kernels, no atomics, every sum in a fixed order, so the result is
// bitwise identical from launch to launch:
//
//  1. grad_sumsq_kernel: grid-stride, 16 B per lane per load (short8 bf16,
//     2 x float4 f32), two loads in flight per lane.  A lane keeps 8 f32
//     accumulators (one per vector slot) and folds them as a fixed pairwise
//     tree; wave_sum's xor butterfly gives every lane the same wave total;
//     lane 0 of each wave parks it in LDS and thread 0 adds the four in wave
//     order.  One f32 partial per block goes to the workspace.
//  2. clip_state_kernel: ONE block.  Thread t adds partials[t], [t + 256], ...
//     in index order, then the same wave/LDS merge, then thread 0 writes
//     clip_state = {norm, scale, finite, sumsq}.
//
// Which elements a lane, a wave and a block own depends only on (n, grid),
// never on timing, and the stream orders kernel 2 after kernel 1.
//
// Read-only pass: 2 B/elem (bf16) against the AdamW kernel's 48 B/elem.

#include "common.h"
#include "launchers.h"

#define GN_BLOCK 256
#define GN_WAVES (GN_BLOCK / WAVE)
#define GN_MAX_PARTIALS 2048

template <bool GRAD_F32>
__device__ __forceinline__ void gn_accum8(const void* __restrict__ grad,
                                          long i, float (&acc)[8]) {
  if (GRAD_F32) {
    const float* g = (const float*)grad + i;
    float4_t a = *(const float4_t*)g;
    float4_t b = *(const float4_t*)(g + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] += a[j] * a[j];
      acc[4 + j] += b[j] * b[j];
    }
  } else {
    short8_t gs = *(const short8_t*)((const short*)grad + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = bf16_to_f32(gs[j]);
      acc[j] += x * x;
    }
  }
}

// Fixed-order block merge: wave butterfly, then waves 0..3 in order.  Valid
// in thread 0 only.
__device__ __forceinline__ float gn_block_sum(float v, float* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = v;
  __syncthreads();
  float s = lds[0];
#pragma unroll
  for (int w = 1; w < GN_WAVES; ++w) s += lds[w];
  return s;
}

template <bool GRAD_F32>
__global__ void __launch_bounds__(GN_BLOCK)
grad_sumsq_kernel(const void* __restrict__ grad, long n,
                  float* __restrict__ partials) {
  __shared__ float lds[GN_WAVES];
  long i = ((long)blockIdx.x * GN_BLOCK + threadIdx.x) * 8;
  const long stride = (long)gridDim.x * GN_BLOCK * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  // n % 8 == 0 (checked by the binding): i < n means i + 8 <= n
  for (; i + stride < n; i += 2 * stride) {
    gn_accum8<GRAD_F32>(grad, i, acc);
    gn_accum8<GRAD_F32>(grad, i + stride, acc);
  }
  if (i < n) gn_accum8<GRAD_F32>(grad, i, acc);
  float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
            ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  float s = gn_block_sum(v, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(GN_BLOCK)
clip_state_kernel(const float* __restrict__ partials, int n_partials,
                  float grad_scale, float max_norm,
                  float* __restrict__ clip_state) {
  __shared__ float lds[GN_WAVES];
  float v = 0.f;
  for (int k = threadIdx.x; k < n_partials; k += GN_BLOCK) v += partials[k];
  float sumsq = gn_block_sum(v, lds);
  if (threadIdx.x == 0) {
    float norm = grad_scale * sqrtf(sumsq);
    // clip_grad_norm_'s factor; fminf drops a NaN ratio (inf / inf), so a
    // non-finite norm leaves coef at 1 and is reported through `finite`
    float coef = fminf(1.0f, max_norm / (norm + 1e-6f));
    clip_state[0] = norm;
    clip_state[1] = grad_scale * coef;
    clip_state[2] = isfinite(sumsq) ? 1.0f : 0.0f;
    clip_state[3] = sumsq;
  }
}

extern "C" int grad_norm_grid(long n) {
  long blocks = (n / 8 + GN_BLOCK - 1) / GN_BLOCK;
  return (int)(blocks < GN_MAX_PARTIALS ? blocks : GN_MAX_PARTIALS);
}

// partials: f32[grad_norm_grid(n)] workspace; clip_state: f32[4].
extern "C" hipError_t grad_clip_state_launch(const void* grad, int grad_is_f32,
                                             long n, float grad_scale,
                                             float max_norm, void* partials,
                                             void* clip_state, hipStream_t s) {
  int grid = grad_norm_grid(n);
  if (grad_is_f32)
    grad_sumsq_kernel<true><<<grid, GN_BLOCK, 0, s>>>(grad, n,
                                                      (float*)partials);
  else
    grad_sumsq_kernel<false><<<grid, GN_BLOCK, 0, s>>>(grad, n,
                                                       (float*)partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  clip_state_kernel<<<1, GN_BLOCK, 0, s>>>((const float*)partials, grid,
                                           grad_scale, max_norm,
                                           (float*)clip_state);
  return hipGetLastError();
}
