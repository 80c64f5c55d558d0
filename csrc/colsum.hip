// Deterministic column sums for gfx950: the reduction chains behind every
// bias / affine-parameter gradient (LayerNorm dgamma/dbeta/dres_sum,
// bias_gelu dbias, the folded flash qkv bias, bias_grad).
//
//   colsum_launch       [R, D] f32 partials workspace -> [D] f32 or bf16
//   colsum_bf16_launch  [N, D] bf16 matrix            -> [D] bf16
//
// Both split the rows over gridDim.y, keep a fixed summation order (no
// atomics) and own the size of the f32 scratch they need: the bindings ask
// colsum_scratch_rows() / colsum_bf16_scratch_rows().

#include "common.h"
#include "launchers.h"

// Split rows of the first stage, and rows of the middle stage that collapses
// them (both chains share the middle stage).
#define COLSUM_MAX_SPLITS 256
#define COLSUM_BF16_MAX_SPLITS 1024
#define COLSUM_MID 16

extern "C" {

// Column-sum of the [R, D] f32 partials workspace into [D] f32.
// Two-stage split-row reduction: the single-threaded-column version ran 4
// blocks at D=1024 (15.6 ms/step in the baseline profile); this one fills the
// chip with gridDim.y row-splits x float4 columns and stays deterministic.
__global__ void __launch_bounds__(256)
colsum_stage_kernel(const float* __restrict__ ws, float* __restrict__ out,
                    int R, int D, int rows_per_split) {
  int col = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= D) return;
  int r0 = blockIdx.y * rows_per_split;
  int r1 = min(R, r0 + rows_per_split);
  float4_t s = {0.f, 0.f, 0.f, 0.f};
  for (int r = r0; r < r1; ++r) {
    float4_t v = *(const float4_t*)(ws + (long)r * D + col);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += v[j];
  }
  *(float4_t*)(out + (long)blockIdx.y * D + col) = s;
}

// Final stage of the chain for callers that want bf16: the same sum over
// all R rows in the same order, rounded once on the way out, so the
// parameter gradient needs no separate convert launch.
__global__ void __launch_bounds__(256)
colsum_stage_bf16_kernel(const float* __restrict__ ws, short* __restrict__ out,
                         int R, int D) {
  int col = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= D) return;
  float4_t s = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < R; ++r) {
    float4_t v = *(const float4_t*)(ws + (long)r * D + col);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += v[j];
  }
  short4_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32_to_bf16(s[j]);
  *(short4_t*)(out + col) = o;
}

// Bias gradient: column-sum of a [N, D] bf16 matrix -> [D] bf16.
// Two-stage deterministic split-row reduction with f32 accumulation —
// replaces torch's generic reduce_kernel for the projection bias grads
// (~58 us -> ~20 us each at [65536, 1024..3072]).
__global__ void __launch_bounds__(256)
colsum_bf16_stage1_kernel(const short* __restrict__ x,
                          float* __restrict__ scratch, long N, int D,
                          long rows_per_split) {
  int col = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (col >= D) return;
  long r0 = (long)blockIdx.y * rows_per_split;
  long r1 = min(N, r0 + rows_per_split);
  float s[8] = {0.f};
  for (long r = r0; r < r1; ++r) {
    short8_t v = *(const short8_t*)(x + r * D + col);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += bf16_to_f32(v[j]);
  }
  float* out = scratch + (long)blockIdx.y * D + col;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = s[j];
}

__global__ void __launch_bounds__(256)
colsum_bf16_stage2_kernel(const float* __restrict__ scratch,
                          short* __restrict__ out, int splits, int D) {
  int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= D) return;
  float s = 0.f;
  for (int r = 0; r < splits; ++r) s += scratch[(long)r * D + col];
  out[col] = f32_to_bf16(s);
}

// Adaptive splits (round 2): the fixed 64-way split left a [65536, 1024]
// bias grad running on 64 blocks of a 256-CU chip — 452 us/call, which
// was the REAL cause of the round-1 "fused_linear regresses 13.7 ms"
// finding (misattributed to GEMM dispatch).  Stage 1 launches
// ~COLSUM_BF16_MAX_SPLITS blocks; a float4 middle stage collapses the splits
// to COLSUM_MID; the bf16 stage finishes.
int colsum_bf16_scratch_rows(void) {
  return COLSUM_BF16_MAX_SPLITS + COLSUM_MID;
}

hipError_t colsum_bf16_launch(const void* x, void* scratch, void* out,
                              long N, int D, hipStream_t stream) {
  int gx = (D / 8 + 255) / 256;
  int splits = COLSUM_BF16_MAX_SPLITS / gx;
  if (splits > COLSUM_BF16_MAX_SPLITS) splits = COLSUM_BF16_MAX_SPLITS;
  if ((long)splits > N) splits = (int)N;
  long rows_per_split = (N + splits - 1) / splits;
  dim3 g1(gx, splits);
  colsum_bf16_stage1_kernel<<<g1, 256, 0, stream>>>(
      (const short*)x, (float*)scratch, N, D, rows_per_split);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (splits > COLSUM_MID && D % 4 == 0) {
    float* mid = (float*)scratch + (long)COLSUM_BF16_MAX_SPLITS * D;
    int rps2 = (splits + COLSUM_MID - 1) / COLSUM_MID;
    colsum_stage_kernel<<<dim3((D / 4 + 255) / 256, COLSUM_MID), 256, 0,
                          stream>>>((const float*)scratch, mid, splits, D,
                                    rps2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    colsum_bf16_stage2_kernel<<<dim3((D + 255) / 256), 256, 0, stream>>>(
        mid, (short*)out, COLSUM_MID, D);
    return hipGetLastError();
  }
  colsum_bf16_stage2_kernel<<<dim3((D + 255) / 256), 256, 0, stream>>>(
      (const float*)scratch, (short*)out, splits, D);
  return hipGetLastError();
}

// Adaptive split count (round 2): the fixed 64-way split left a D=1024
// reduction at 64 blocks on a 256-CU chip (21.6 us/call in the r2 bench
// profile); pick splits so stage 1 launches ~1024 blocks, then collapse
// with a narrow second stage and a single-split final stage.
//
// One chain reduces several outputs at once: ws is [R, D] with D = n * unit
// (n column slabs side by side).  The split count comes from `split_w`, not
// from D, so a column is summed in the same order whether or not the caller
// appended a further slab: asking for an extra output leaves the others
// bit-identical.  out is [D] f32, or [D] bf16 when out_bf16 is set (the
// final stage rounds on the way out).
int colsum_scratch_rows(void) { return COLSUM_MAX_SPLITS + COLSUM_MID; }

static hipError_t colsum_final(const float* in, void* out, int R, int D,
                               int out_bf16, hipStream_t stream) {
  dim3 grid1((D / 4 + 255) / 256, 1);
  if (out_bf16) {
    colsum_stage_bf16_kernel<<<grid1, 256, 0, stream>>>(in, (short*)out, R, D);
  } else {
    colsum_stage_kernel<<<grid1, 256, 0, stream>>>(in, (float*)out, R, D, R);
  }
  return hipGetLastError();
}

hipError_t colsum_launch(const void* ws, void* scratch, void* out, int R,
                         int D, int split_w, int out_bf16,
                         hipStream_t stream) {
  int gx = (D / 4 + 255) / 256;
  if (R <= COLSUM_MID)
    return colsum_final((const float*)ws, out, R, D, out_bf16, stream);
  int splits = 1024 / ((split_w / 4 + 255) / 256);
  if (splits > COLSUM_MAX_SPLITS) splits = COLSUM_MAX_SPLITS;
  if (splits > R) splits = R;
  int rows_per_split = (R + splits - 1) / splits;
  colsum_stage_kernel<<<dim3(gx, splits), 256, 0, stream>>>(
      (const float*)ws, (float*)scratch, R, D, rows_per_split);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (splits <= COLSUM_MID)
    return colsum_final((const float*)scratch, out, splits, D, out_bf16,
                        stream);
  float* mid = (float*)scratch + (long)COLSUM_MAX_SPLITS * D;
  int rps2 = (splits + COLSUM_MID - 1) / COLSUM_MID;
  colsum_stage_kernel<<<dim3(gx, COLSUM_MID), 256, 0, stream>>>(
      (const float*)scratch, mid, splits, D, rps2);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return colsum_final(mid, out, COLSUM_MID, D, out_bf16, stream);
}

}  // extern "C"
