// Row-wise softmax cross-entropy over a wide vocabulary, gfx950: the token
// loss of masked-LM pretraining (MLTC.mlm_loss).  bf16 logits [N, V], int64
// targets [N], f32 math.  6 B per logit end to end (forward reads the row
// once, backward reads it once and writes the gradient once); no f32 copy of
// the logits exists at any point.
//
// A row is IGNORED when its target is ignore_index or lies outside [0, V):
// its loss is 0, its gradient row is zeros, and the target is never used as
// an index.  (Range validation is the Python side's business; the kernels
// only promise not to touch memory through a bad target.)
//
//  1. ce_fwd_kernel: one 256-thread workgroup per row, grid-stride over rows
//     past the block cap.  Thread t owns the 16-byte packets t, t + 256, ...
//     of the row and keeps an ONLINE (max, sum): per packet the 8 values'
//     maximum joins the running maximum, the running sum is rescaled by
//     exp(old_max - new_max) and the packet's 8 exponentials are added in
//     slot order.  The row is read once.  The 64 lanes of a wave merge their
//     pairs with an xor butterfly (both partners compute the same
//     commutative expression, so every lane ends with the same bits), lane 0
//     of each wave parks its pair in LDS and every thread merges waves
//     0, 1, 2, 3 in that order.  lse = max + log(sum); loss = lse - x[target],
//     the one extra 2-byte read of the row.
//  2. ce_bwd_kernel: same ownership; dlogits = (exp(x - lse) - [j == target])
//     * grow[row] rounded once to bf16.  Every element of dlogits is written,
//     ignored rows as zeros.
//  3. ce_mean_kernel: ONE block.  Thread t adds loss_rows[t], [t + 256], ...
//     in index order and counts its valid rows, then the wave/LDS merge;
//     thread 0 writes {sum / count, 1 / count}, or {0, 0} with no valid row.
//
// No atomics; which elements a lane, a wave and a block own depends only on
// (N, V, grid), so every output is bitwise identical from launch to launch.
// Offsets are long: N * V passes 2^31 bytes at the training shapes.

#include "common.h"
#include "launchers.h"

#define CE_BLOCK 256
#define CE_WAVES (CE_BLOCK / WAVE)
#define CE_SWEEP (CE_BLOCK * 8)   // elements one sweep of the block covers
#define CE_MAX_GRID 2048
// the empty (max, sum) pair: finite, so that exp(max - max) is 1, not NaN
#define CE_NEG -3.0e38f

static int ce_grid(int N) { return N < CE_MAX_GRID ? N : CE_MAX_GRID; }

// (m, s) <- (m, s) merged with one packet of 8 logits
__device__ __forceinline__ void ce_accum8(short8_t x, float& m, float& s) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf16_to_f32(x[j]);
  float pm = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])),
                   fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
  float mn = fmaxf(m, pm);
  s *= __expf(m - mn);
#pragma unroll
  for (int j = 0; j < 8; ++j) s += __expf(f[j] - mn);
  m = mn;
}

// (m, s) <- (m, s) merged with (om, os); commutative bit for bit
__device__ __forceinline__ void ce_merge(float& m, float& s, float om,
                                         float os) {
  float mn = fmaxf(m, om);
  s = s * __expf(m - mn) + os * __expf(om - mn);
  m = mn;
}

// target of a row -> its column, or -1 for an ignored row
__device__ __forceinline__ int ce_target(const long* __restrict__ target,
                                         long row, int V, long ignore_index) {
  long t = target[row];
  return (t == ignore_index || t < 0 || t >= (long)V) ? -1 : (int)t;
}

__global__ void __launch_bounds__(CE_BLOCK)
ce_fwd_kernel(const short* __restrict__ logits,
              const long* __restrict__ target, float* __restrict__ loss_rows,
              float* __restrict__ lse_out, int N, int V, long ignore_index) {
  __shared__ float lds_m[CE_WAVES], lds_s[CE_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  for (long row = blockIdx.x; row < N; row += gridDim.x) {
    const short* xr = logits + row * (long)V;
    float m = CE_NEG, s = 0.f;
    // V % 8 == 0 (checked by the binding): i < V means i + 8 <= V
    int i = threadIdx.x * 8;
    for (; i + CE_SWEEP < V; i += 2 * CE_SWEEP) {
      short8_t a = *(const short8_t*)(xr + i);
      short8_t b = *(const short8_t*)(xr + i + CE_SWEEP);
      ce_accum8(a, m, s);
      ce_accum8(b, m, s);
    }
    if (i < V) ce_accum8(*(const short8_t*)(xr + i), m, s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      ce_merge(m, s, __shfl_xor(m, off, WAVE), __shfl_xor(s, off, WAVE));
    if (lane == 0) { lds_m[wid] = m; lds_s[wid] = s; }
    __syncthreads();
    m = lds_m[0]; s = lds_s[0];
#pragma unroll
    for (int w = 1; w < CE_WAVES; ++w) ce_merge(m, s, lds_m[w], lds_s[w]);
    if (threadIdx.x == 0) {
      float lse = m + logf(s);
      int t = ce_target(target, row, V, ignore_index);
      lse_out[row] = lse;
      loss_rows[row] = t < 0 ? 0.f : lse - bf16_to_f32(xr[t]);
    }
    __syncthreads();    // the next row reuses the LDS slots
  }
}

__device__ __forceinline__ short8_t ce_grad8(short8_t x, int col0, int t,
                                             float lse, float g) {
  short8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float p = __expf(bf16_to_f32(x[j]) - lse);
    o[j] = f32_to_bf16((p - (col0 + j == t ? 1.f : 0.f)) * g);
  }
  return o;
}

__global__ void __launch_bounds__(CE_BLOCK)
ce_bwd_kernel(const short* __restrict__ logits,
              const long* __restrict__ target, const float* __restrict__ lse,
              const float* __restrict__ grow, short* __restrict__ dlogits,
              int N, int V, long ignore_index) {
  for (long row = blockIdx.x; row < N; row += gridDim.x) {
    const short* xr = logits + row * (long)V;
    short* dr = dlogits + row * (long)V;
    const int t = ce_target(target, row, V, ignore_index);
    int i = threadIdx.x * 8;
    if (t < 0) {
      const short8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
      for (; i < V; i += CE_SWEEP) *(short8_t*)(dr + i) = z;
      continue;
    }
    const float l = lse[row], g = grow[row];
    for (; i + CE_SWEEP < V; i += 2 * CE_SWEEP) {
      short8_t a = *(const short8_t*)(xr + i);
      short8_t b = *(const short8_t*)(xr + i + CE_SWEEP);
      *(short8_t*)(dr + i) = ce_grad8(a, i, t, l, g);
      *(short8_t*)(dr + i + CE_SWEEP) = ce_grad8(b, i + CE_SWEEP, t, l, g);
    }
    if (i < V)
      *(short8_t*)(dr + i) = ce_grad8(*(const short8_t*)(xr + i), i, t, l, g);
  }
}

__global__ void __launch_bounds__(CE_BLOCK)
ce_mean_kernel(const float* __restrict__ loss_rows,
               const long* __restrict__ target, float* __restrict__ out,
               int N, int V, long ignore_index) {
  __shared__ float lds_v[CE_WAVES], lds_c[CE_WAVES];
  float v = 0.f, c = 0.f;     // counts stay exact in f32: N < 2^24 per lane
  for (int k = threadIdx.x; k < N; k += CE_BLOCK) {
    v += loss_rows[k];
    c += ce_target(target, k, V, ignore_index) < 0 ? 0.f : 1.f;
  }
  v = wave_sum(v);
  c = wave_sum(c);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    lds_v[threadIdx.x / WAVE] = v;
    lds_c[threadIdx.x / WAVE] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sv = lds_v[0], sc = lds_c[0];
#pragma unroll
    for (int w = 1; w < CE_WAVES; ++w) { sv += lds_v[w]; sc += lds_c[w]; }
    out[0] = sc > 0.f ? sv / sc : 0.f;
    out[1] = sc > 0.f ? 1.0f / sc : 0.f;
  }
}

extern "C" hipError_t ce_fwd_launch(const void* logits, const void* target,
                                    void* loss_rows, void* lse, int N, int V,
                                    long ignore_index, hipStream_t s) {
  if (N == 0) return hipSuccess;
  ce_fwd_kernel<<<ce_grid(N), CE_BLOCK, 0, s>>>(
      (const short*)logits, (const long*)target, (float*)loss_rows,
      (float*)lse, N, V, ignore_index);
  return hipGetLastError();
}

extern "C" hipError_t ce_bwd_launch(const void* logits, const void* target,
                                    const void* lse, const void* grow,
                                    void* dlogits, int N, int V,
                                    long ignore_index, hipStream_t s) {
  if (N == 0) return hipSuccess;
  ce_bwd_kernel<<<ce_grid(N), CE_BLOCK, 0, s>>>(
      (const short*)logits, (const long*)target, (const float*)lse,
      (const float*)grow, (short*)dlogits, N, V, ignore_index);
  return hipGetLastError();
}

extern "C" hipError_t ce_mean_launch(const void* loss_rows, const void* target,
                                     void* out, int N, int V,
                                     long ignore_index, hipStream_t s) {
  ce_mean_kernel<<<1, CE_BLOCK, 0, s>>>((const float*)loss_rows,
                                        (const long*)target, (float*)out, N,
                                        V, ignore_index);
  return hipGetLastError();
}
