// Fused AdamW step over FLAT parameter storage, gfx950.
//
// The trainer flattens every parameter into one contiguous bf16 tensor with a
// matching f32 master copy and f32 m/v states (tosem2021_amd/train.py), so the
// whole optimizer step is ONE bandwidth-bound kernel pass: read g(bf16),
// m,v,master(f32), write m,v,master(f32) + p(bf16) = 26 B/elem read +
// 22 B/elem write.  Decoupled weight decay (AdamW), bias-corrected.
//
// grad may be bf16 (local step) or f32 (set by the DDP reduce path).
//
// Two entry points share one sweep (adamw_sweep), so they cannot drift:
//  * adamw_kernel takes grad_scale by value;
//  * adamw_clipped_kernel reads it from the device-side clip_state written by
//    csrc/grad_norm.hip (scale = grad_scale * clip coefficient) and leaves
//    every buffer untouched when the gradient was not finite.

#include "common.h"
#include "launchers.h"

#define AD_BLOCK 256

// Launch geometry of both entry points: one thread per 4-wide group,
// grid-stride past the cap.
#define AD_MAX_GRID 2048
static int adamw_grid(long n) {
  long blocks = (n / 4 + AD_BLOCK - 1) / AD_BLOCK;
  return (int)(blocks < AD_MAX_GRID ? blocks : AD_MAX_GRID);
}

// One 4-wide group: updates mm, vv, mw in place, returns the bf16 weights.
//
// Every fused multiply-add is written out and contraction is off, so the
// rounding does not depend on how the compiler happens to pair multiplies
// with adds around this call (it paired them differently once the body moved
// into a function).  The forms below are the ones adamw_kernel has always
// compiled to; the one difference between the grad dtypes, which product of
// the v update is fused, is part of that and keeps both bitwise stable.
template <bool GRAD_F32>
__device__ __forceinline__ short4_t adamw_update4(
    const float4_t& gm, float4_t& mm, float4_t& vv, float4_t& mw, float lr,
    float beta1, float beta2, float eps, float wd, float bc1, float bc2,
    float grad_scale) {
#pragma clang fp contract(off)
  short4_t po;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float g = gm[j] * grad_scale;
    float m_ = __builtin_fmaf(1.f - beta1, g, beta1 * mm[j]);
    float gg = (1.f - beta2) * g;
    float v_ = GRAD_F32 ? __builtin_fmaf(g, gg, beta2 * vv[j])
                        : __builtin_fmaf(beta2, vv[j], gg * g);
    float mhat = m_ * bc1;
    float vhat = v_ * bc2;
    float w = mw[j];
    float u = __builtin_fmaf(wd, w, mhat / (sqrtf(vhat) + eps));
    w = __builtin_fmaf(-lr, u, w);
    mm[j] = m_; vv[j] = v_; mw[j] = w;
    po[j] = f32_to_bf16(w);
  }
  return po;
}

template <bool GRAD_F32>
__device__ __forceinline__ void adamw_sweep(
    short* __restrict__ p_bf16, const void* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ master,
    long n, float lr, float beta1, float beta2, float eps, float wd,
    float bc1, float bc2, float grad_scale) {
  long i0 = ((long)blockIdx.x * AD_BLOCK + threadIdx.x) * 4;
  long stride = (long)gridDim.x * AD_BLOCK * 4;
  for (long i = i0; i < n; i += stride) {
    // 4-wide: 16 B f32 / 8 B bf16 per lane per tensor
    float4_t gm, mm, vv, mw;
    mm = *(float4_t*)(m + i);
    vv = *(float4_t*)(v + i);
    mw = *(float4_t*)(master + i);
    if (GRAD_F32) {
      gm = *(const float4_t*)((const float*)grad + i);
    } else {
      short4_t gs = *(const short4_t*)((const short*)grad + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) gm[j] = bf16_to_f32(gs[j]);
    }
    short4_t po = adamw_update4<GRAD_F32>(
        gm, mm, vv, mw, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale);
    *(float4_t*)(m + i) = mm;
    *(float4_t*)(v + i) = vv;
    *(float4_t*)(master + i) = mw;
    *(short4_t*)(p_bf16 + i) = po;
  }
}

template <bool GRAD_F32>
__global__ void __launch_bounds__(AD_BLOCK)
adamw_kernel(short* __restrict__ p_bf16, const void* __restrict__ grad,
             float* __restrict__ m, float* __restrict__ v,
             float* __restrict__ master, long n, float lr, float beta1,
             float beta2, float eps, float wd, float bc1, float bc2,
             float grad_scale) {
  adamw_sweep<GRAD_F32>(p_bf16, grad, m, v, master, n, lr, beta1, beta2, eps,
                        wd, bc1, bc2, grad_scale);
}

// clip_state = {norm, scale, finite, sumsq} (csrc/grad_norm.hip), written by
// an earlier kernel on the same stream.
template <bool GRAD_F32>
__global__ void __launch_bounds__(AD_BLOCK)
adamw_clipped_kernel(short* __restrict__ p_bf16,
                     const void* __restrict__ grad, float* __restrict__ m,
                     float* __restrict__ v, float* __restrict__ master,
                     long n, float lr, float beta1, float beta2, float eps,
                     float wd, float bc1, float bc2,
                     const float* __restrict__ clip_state) {
  if (clip_state[2] == 0.f) return;  // non-finite gradient: skip the step
  adamw_sweep<GRAD_F32>(p_bf16, grad, m, v, master, n, lr, beta1, beta2, eps,
                        wd, bc1, bc2, clip_state[1]);
}

extern "C" hipError_t adamw_launch(void* p_bf16, const void* grad, int grad_is_f32,
                        void* m, void* v, void* master, long n, float lr,
                        float beta1, float beta2, float eps, float wd,
                        int step, float grad_scale, hipStream_t s) {
  const int grid = adamw_grid(n);
  float bc1 = 1.0f / (1.0f - powf(beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf(beta2, (float)step));
  if (grad_is_f32)
    adamw_kernel<true><<<grid, AD_BLOCK, 0, s>>>(
        (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master, n, lr,
        beta1, beta2, eps, wd, bc1, bc2, grad_scale);
  else
    adamw_kernel<false><<<grid, AD_BLOCK, 0, s>>>(
        (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master, n, lr,
        beta1, beta2, eps, wd, bc1, bc2, grad_scale);
  return hipGetLastError();
}

extern "C" hipError_t adamw_clipped_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, long n, float lr, float beta1, float beta2, float eps,
    float wd, int step, const void* clip_state, hipStream_t s) {
  const int grid = adamw_grid(n);
  float bc1 = 1.0f / (1.0f - powf(beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf(beta2, (float)step));
  if (grad_is_f32)
    adamw_clipped_kernel<true><<<grid, AD_BLOCK, 0, s>>>(
        (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master, n, lr,
        beta1, beta2, eps, wd, bc1, bc2, (const float*)clip_state);
  else
    adamw_clipped_kernel<false><<<grid, AD_BLOCK, 0, s>>>(
        (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master, n, lr,
        beta1, beta2, eps, wd, bc1, bc2, (const float*)clip_state);
  return hipGetLastError();
}
