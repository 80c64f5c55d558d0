// Fused AdamW step over FLAT parameter storage, gfx950.
//
// The trainer flattens every parameter into one contiguous bf16 tensor with a
// matching f32 master copy and f32 m/v states (tosem2021_amd/train.py), so the
// whole optimizer step is ONE bandwidth-bound kernel pass: read g(bf16),
// m,v,master(f32), write m,v,master(f32) + p(bf16) = 14 B/elem read +
// 14 B/elem write.  Decoupled weight decay (AdamW), bias-corrected.
//
// grad may be bf16 (local step) or f32 (set by the DDP reduce path).
//
// Four entry points share one update (adamw_update4), so they cannot drift:
//  * adamw_kernel takes grad_scale by value;
//  * adamw_clipped_kernel reads it from the device-side clip_state written by
//    csrc/grad_norm.hip (scale = grad_scale * clip coefficient) and leaves
//    every buffer untouched when the gradient was not finite;
//  * adamw_grouped_kernel and adamw_grouped_clipped_kernel are their twins
//    with a per-element lr and wd looked up in a segment table (parameter
//    groups over the flat buffer): element e of segment s is updated exactly,
//    bit for bit, as adamw_kernel would with lr * seg_lr_mult[s], seg_wd[s].
//
// Each of the four has an EMA form (template flag EMA, the *_ema_launch entry
// points) that also keeps an exponential moving average of the weights:
// ema [n] f32 is read with m, v and master and updated from the new master
// value w as ema = d * ema + (1 - d) * w, 8 B/elem more traffic.  p, m, v and
// master come out as without it, the average never feeds back, and a skipped
// step leaves it untouched too.  With EMA = false nothing of it is compiled.

#include "common.h"
#include "launchers.h"

#define AD_BLOCK 256

// Launch geometry of every entry point: one thread per 4-wide group,
// grid-stride past the cap.
#define AD_MAX_GRID 2048
// Segment table cap: 16 B per entry (end, lr_mult, wd), 16 KB of LDS.
#define AD_MAX_SEGS 1024
static int adamw_grid(long n) {
  long blocks = (n / 4 + AD_BLOCK - 1) / AD_BLOCK;
  return (int)(blocks < AD_MAX_GRID ? blocks : AD_MAX_GRID);
}

// One 4-wide group: updates mm, vv, mw in place, returns the bf16 weights.
// lr and wd are per element; the ungrouped kernels pass a splat.
//
// Every fused multiply-add is written out and contraction is off, so the
// rounding does not depend on how the compiler happens to pair multiplies
// with adds around this call (it paired them differently once the body moved
// into a function).  The forms below are the ones adamw_kernel has always
// compiled to; the one difference between the grad dtypes, which product of
// the v update is fused, is part of that and keeps both bitwise stable.
template <bool GRAD_F32>
__device__ __forceinline__ short4_t adamw_update4(
    const float4_t& gm, float4_t& mm, float4_t& vv, float4_t& mw,
    const float4_t& lr, float beta1, float beta2, float eps,
    const float4_t& wd, float bc1, float bc2, float grad_scale) {
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
    float u = __builtin_fmaf(wd[j], w, mhat / (sqrtf(vhat) + eps));
    w = __builtin_fmaf(-lr[j], u, w);
    mm[j] = m_; vv[j] = v_; mw[j] = w;
    po[j] = f32_to_bf16(w);
  }
  return po;
}

// The 4-wide group at element i, 16 B f32 / 8 B bf16 per lane per tensor, in
// two halves: the loads, and the update with its stores.
template <bool GRAD_F32>
__device__ __forceinline__ void adamw_load4(
    const void* __restrict__ grad, const float* __restrict__ m,
    const float* __restrict__ v, const float* __restrict__ master, long i,
    float4_t& gm, float4_t& mm, float4_t& vv, float4_t& mw) {
  mm = *(const float4_t*)(m + i);
  vv = *(const float4_t*)(v + i);
  mw = *(const float4_t*)(master + i);
  if (GRAD_F32) {
    gm = *(const float4_t*)((const float*)grad + i);
  } else {
    short4_t gs = *(const short4_t*)((const short*)grad + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) gm[j] = bf16_to_f32(gs[j]);
  }
}

// The weight average of one 4-wide group: ema = d * ema + (1 - d) * w with w
// the new master value, as three separately rounded f32 operations (two
// products, one sum; omd = 1.f - d is formed once on the host).  No fused
// multiply-add, so separate f32 tensor ops on the host give the same bits.
__device__ __forceinline__ void adamw_ema4(float4_t& ee, const float4_t& mw,
                                           float d, float omd) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float a = d * ee[j];
    float b = omd * mw[j];
    ee[j] = a + b;
  }
}

template <bool GRAD_F32, bool EMA>
__device__ __forceinline__ void adamw_update_store4(
    short* __restrict__ p_bf16, float* __restrict__ m, float* __restrict__ v,
    float* __restrict__ master, float* __restrict__ ema, long i,
    const float4_t& gm, float4_t& mm, float4_t& vv, float4_t& mw,
    float4_t& ee, const float4_t& lr, float beta1, float beta2, float eps,
    const float4_t& wd, float bc1, float bc2, float grad_scale, float ema_d,
    float ema_omd) {
  short4_t po = adamw_update4<GRAD_F32>(
      gm, mm, vv, mw, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale);
  *(float4_t*)(m + i) = mm;
  *(float4_t*)(v + i) = vv;
  *(float4_t*)(master + i) = mw;
  *(short4_t*)(p_bf16 + i) = po;
  if (EMA) {
    adamw_ema4(ee, mw, ema_d, ema_omd);
    *(float4_t*)(ema + i) = ee;
  }
}

template <bool GRAD_F32, bool EMA>
__device__ __forceinline__ void adamw_sweep(
    short* __restrict__ p_bf16, const void* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ master,
    float* __restrict__ ema, long n, float lr, float beta1, float beta2,
    float eps, float wd, float bc1, float bc2, float grad_scale, float ema_d,
    float ema_omd) {
  long i0 = ((long)blockIdx.x * AD_BLOCK + threadIdx.x) * 4;
  long stride = (long)gridDim.x * AD_BLOCK * 4;
  const float4_t lr4 = {lr, lr, lr, lr}, wd4 = {wd, wd, wd, wd};
  for (long i = i0; i < n; i += stride) {
    float4_t gm, mm, vv, mw, ee;
    adamw_load4<GRAD_F32>(grad, m, v, master, i, gm, mm, vv, mw);
    if (EMA) ee = *(const float4_t*)(ema + i);
    adamw_update_store4<GRAD_F32, EMA>(p_bf16, m, v, master, ema, i, gm, mm,
                                       vv, mw, ee, lr4, beta1, beta2, eps,
                                       wd4, bc1, bc2, grad_scale, ema_d,
                                       ema_omd);
  }
}

// The grouped sweep.  seg_end [S] holds strictly increasing exclusive end
// offsets with seg_end[S - 1] == n (checked on the host before upload);
// element e belongs to the first segment s with e < seg_end[s] and is updated
// with lr * seg_lr_mult[s] and seg_wd[s].  Boundaries fall anywhere, so the
// four elements of a group may lie in up to four segments: the loads and
// stores stay 4-wide and only lr and wd become per element.
//
// The table is staged in LDS once per workgroup.  A lane finds the segment of
// its group's first element by binary search, from the segment it ended the
// previous grid-stride pass in (offsets only grow), and walks forward for
// the other three elements.  Neither the search nor the walk leaves
// [0, S - 1], whatever the table holds.
template <bool GRAD_F32, bool EMA>
__device__ __forceinline__ void adamw_grouped_sweep(
    short* __restrict__ p_bf16, const void* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ master,
    float* __restrict__ ema, long n, float lr, float beta1, float beta2,
    float eps, float bc1, float bc2, const long* __restrict__ seg_end,
    const float* __restrict__ seg_lr_mult, const float* __restrict__ seg_wd,
    int S, float grad_scale, float ema_d, float ema_omd) {
#pragma clang fp contract(off)
  __shared__ long s_end[AD_MAX_SEGS];
  __shared__ float s_mult[AD_MAX_SEGS];
  __shared__ float s_wd[AD_MAX_SEGS];
  for (int t = threadIdx.x; t < S; t += AD_BLOCK) {
    s_end[t] = seg_end[t];
    s_mult[t] = seg_lr_mult[t];
    s_wd[t] = seg_wd[t];
  }
  __syncthreads();
  long i0 = ((long)blockIdx.x * AD_BLOCK + threadIdx.x) * 4;
  long stride = (long)gridDim.x * AD_BLOCK * 4;
  int s = 0;
  for (long i = i0; i < n; i += stride) {
    // the loads go out first: the lookup below touches only LDS and runs
    // while they are in flight
    float4_t gm, mm, vv, mw, ee;
    adamw_load4<GRAD_F32>(grad, m, v, master, i, gm, mm, vv, mw);
    if (EMA) ee = *(const float4_t*)(ema + i);
    int hi = S - 1;
    while (s < hi) {
      int mid = (s + hi) >> 1;
      if (i < s_end[mid]) hi = mid; else s = mid + 1;
    }
    long end = s_end[s];
    float lr_s = lr * s_mult[s];
    float wd_s = s_wd[s];
    float4_t lr4, wd4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      while (i + j >= end && s < S - 1) {
        end = s_end[++s];
        lr_s = lr * s_mult[s];
        wd_s = s_wd[s];
      }
      lr4[j] = lr_s;
      wd4[j] = wd_s;
    }
    adamw_update_store4<GRAD_F32, EMA>(p_bf16, m, v, master, ema, i, gm, mm,
                                       vv, mw, ee, lr4, beta1, beta2, eps,
                                       wd4, bc1, bc2, grad_scale, ema_d,
                                       ema_omd);
  }
}

// The kernels.  EMA = false takes ema = nullptr and ignores it and the two
// decay words.
template <bool GRAD_F32, bool EMA>
__global__ void __launch_bounds__(AD_BLOCK)
adamw_kernel(short* __restrict__ p_bf16, const void* __restrict__ grad,
             float* __restrict__ m, float* __restrict__ v,
             float* __restrict__ master, float* __restrict__ ema, long n,
             float lr, float beta1, float beta2, float eps, float wd,
             float bc1, float bc2, float grad_scale, float ema_d,
             float ema_omd) {
  adamw_sweep<GRAD_F32, EMA>(p_bf16, grad, m, v, master, ema, n, lr, beta1,
                             beta2, eps, wd, bc1, bc2, grad_scale, ema_d,
                             ema_omd);
}

// clip_state = {norm, scale, finite, sumsq} (csrc/grad_norm.hip), written by
// an earlier kernel on the same stream.
template <bool GRAD_F32, bool EMA>
__global__ void __launch_bounds__(AD_BLOCK)
adamw_clipped_kernel(short* __restrict__ p_bf16,
                     const void* __restrict__ grad, float* __restrict__ m,
                     float* __restrict__ v, float* __restrict__ master,
                     float* __restrict__ ema, long n, float lr, float beta1,
                     float beta2, float eps, float wd, float bc1, float bc2,
                     const float* __restrict__ clip_state, float ema_d,
                     float ema_omd) {
  if (clip_state[2] == 0.f) return;  // non-finite gradient: skip the step
  adamw_sweep<GRAD_F32, EMA>(p_bf16, grad, m, v, master, ema, n, lr, beta1,
                             beta2, eps, wd, bc1, bc2, clip_state[1], ema_d,
                             ema_omd);
}

template <bool GRAD_F32, bool EMA>
__global__ void __launch_bounds__(AD_BLOCK)
adamw_grouped_kernel(short* __restrict__ p_bf16,
                     const void* __restrict__ grad, float* __restrict__ m,
                     float* __restrict__ v, float* __restrict__ master,
                     float* __restrict__ ema, long n, float lr, float beta1,
                     float beta2, float eps, float bc1, float bc2,
                     const long* __restrict__ seg_end,
                     const float* __restrict__ seg_lr_mult,
                     const float* __restrict__ seg_wd, int S,
                     float grad_scale, float ema_d, float ema_omd) {
  adamw_grouped_sweep<GRAD_F32, EMA>(p_bf16, grad, m, v, master, ema, n, lr,
                                     beta1, beta2, eps, bc1, bc2, seg_end,
                                     seg_lr_mult, seg_wd, S, grad_scale,
                                     ema_d, ema_omd);
}

template <bool GRAD_F32, bool EMA>
__global__ void __launch_bounds__(AD_BLOCK)
adamw_grouped_clipped_kernel(
    short* __restrict__ p_bf16, const void* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ master,
    float* __restrict__ ema, long n, float lr, float beta1, float beta2,
    float eps, float bc1, float bc2, const long* __restrict__ seg_end,
    const float* __restrict__ seg_lr_mult, const float* __restrict__ seg_wd,
    int S, const float* __restrict__ clip_state, float ema_d, float ema_omd) {
  // uniform over the grid, and ahead of the sweep's barrier
  if (clip_state[2] == 0.f) return;  // non-finite gradient: skip the step
  adamw_grouped_sweep<GRAD_F32, EMA>(p_bf16, grad, m, v, master, ema, n, lr,
                                     beta1, beta2, eps, bc1, bc2, seg_end,
                                     seg_lr_mult, seg_wd, S, clip_state[1],
                                     ema_d, ema_omd);
}

// One launch body per entry point, shared by its plain and its EMA launcher
// (ema == nullptr picks the plain kernels).  1 - d is formed here in f32, the
// value a host recurrence in f32 forms too.
static hipError_t adamw_dispatch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, float wd, int step, float grad_scale,
    hipStream_t s) {
  const int grid = adamw_grid(n);
  float bc1 = 1.0f / (1.0f - powf(beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf(beta2, (float)step));
  const float omd = 1.0f - ema_decay;
#define AD_LAUNCH(G, E)                                                       \
  adamw_kernel<G, E><<<grid, AD_BLOCK, 0, s>>>(                               \
      (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master,             \
      (float*)ema, n, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale,        \
      ema_decay, omd)
  if (ema) {
    if (grad_is_f32) AD_LAUNCH(true, true); else AD_LAUNCH(false, true);
  } else {
    if (grad_is_f32) AD_LAUNCH(true, false); else AD_LAUNCH(false, false);
  }
#undef AD_LAUNCH
  return hipGetLastError();
}

static hipError_t adamw_clipped_dispatch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, float wd, int step, const void* clip_state,
    hipStream_t s) {
  const int grid = adamw_grid(n);
  float bc1 = 1.0f / (1.0f - powf(beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf(beta2, (float)step));
  const float omd = 1.0f - ema_decay;
#define AD_LAUNCH(G, E)                                                       \
  adamw_clipped_kernel<G, E><<<grid, AD_BLOCK, 0, s>>>(                       \
      (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master,             \
      (float*)ema, n, lr, beta1, beta2, eps, wd, bc1, bc2,                    \
      (const float*)clip_state, ema_decay, omd)
  if (ema) {
    if (grad_is_f32) AD_LAUNCH(true, true); else AD_LAUNCH(false, true);
  } else {
    if (grad_is_f32) AD_LAUNCH(true, false); else AD_LAUNCH(false, false);
  }
#undef AD_LAUNCH
  return hipGetLastError();
}

static hipError_t adamw_grouped_dispatch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, int step, const void* seg_end,
    const void* seg_lr_mult, const void* seg_wd, int n_seg, float grad_scale,
    hipStream_t s) {
  if (n_seg < 1 || n_seg > AD_MAX_SEGS) return hipErrorInvalidValue;
  const int grid = adamw_grid(n);
  float bc1 = 1.0f / (1.0f - powf(beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf(beta2, (float)step));
  const float omd = 1.0f - ema_decay;
#define AD_LAUNCH(G, E)                                                       \
  adamw_grouped_kernel<G, E><<<grid, AD_BLOCK, 0, s>>>(                       \
      (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master,             \
      (float*)ema, n, lr, beta1, beta2, eps, bc1, bc2, (const long*)seg_end,  \
      (const float*)seg_lr_mult, (const float*)seg_wd, n_seg, grad_scale,     \
      ema_decay, omd)
  if (ema) {
    if (grad_is_f32) AD_LAUNCH(true, true); else AD_LAUNCH(false, true);
  } else {
    if (grad_is_f32) AD_LAUNCH(true, false); else AD_LAUNCH(false, false);
  }
#undef AD_LAUNCH
  return hipGetLastError();
}

static hipError_t adamw_grouped_clipped_dispatch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, int step, const void* seg_end,
    const void* seg_lr_mult, const void* seg_wd, int n_seg,
    const void* clip_state, hipStream_t s) {
  if (n_seg < 1 || n_seg > AD_MAX_SEGS) return hipErrorInvalidValue;
  const int grid = adamw_grid(n);
  float bc1 = 1.0f / (1.0f - powf(beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf(beta2, (float)step));
  const float omd = 1.0f - ema_decay;
#define AD_LAUNCH(G, E)                                                       \
  adamw_grouped_clipped_kernel<G, E><<<grid, AD_BLOCK, 0, s>>>(               \
      (short*)p_bf16, grad, (float*)m, (float*)v, (float*)master,             \
      (float*)ema, n, lr, beta1, beta2, eps, bc1, bc2, (const long*)seg_end,  \
      (const float*)seg_lr_mult, (const float*)seg_wd, n_seg,                 \
      (const float*)clip_state, ema_decay, omd)
  if (ema) {
    if (grad_is_f32) AD_LAUNCH(true, true); else AD_LAUNCH(false, true);
  } else {
    if (grad_is_f32) AD_LAUNCH(true, false); else AD_LAUNCH(false, false);
  }
#undef AD_LAUNCH
  return hipGetLastError();
}

extern "C" hipError_t adamw_launch(void* p_bf16, const void* grad, int grad_is_f32,
                        void* m, void* v, void* master, long n, float lr,
                        float beta1, float beta2, float eps, float wd,
                        int step, float grad_scale, hipStream_t s) {
  return adamw_dispatch(p_bf16, grad, grad_is_f32, m, v, master, nullptr, 0.f,
                        n, lr, beta1, beta2, eps, wd, step, grad_scale, s);
}

extern "C" hipError_t adamw_clipped_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, long n, float lr, float beta1, float beta2, float eps,
    float wd, int step, const void* clip_state, hipStream_t s) {
  return adamw_clipped_dispatch(p_bf16, grad, grad_is_f32, m, v, master,
                                nullptr, 0.f, n, lr, beta1, beta2, eps, wd,
                                step, clip_state, s);
}

extern "C" hipError_t adamw_grouped_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, long n, float lr, float beta1, float beta2, float eps,
    int step, const void* seg_end, const void* seg_lr_mult,
    const void* seg_wd, int n_seg, float grad_scale, hipStream_t s) {
  return adamw_grouped_dispatch(p_bf16, grad, grad_is_f32, m, v, master,
                                nullptr, 0.f, n, lr, beta1, beta2, eps, step,
                                seg_end, seg_lr_mult, seg_wd, n_seg,
                                grad_scale, s);
}

extern "C" hipError_t adamw_grouped_clipped_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, long n, float lr, float beta1, float beta2, float eps,
    int step, const void* seg_end, const void* seg_lr_mult,
    const void* seg_wd, int n_seg, const void* clip_state, hipStream_t s) {
  return adamw_grouped_clipped_dispatch(p_bf16, grad, grad_is_f32, m, v,
                                        master, nullptr, 0.f, n, lr, beta1,
                                        beta2, eps, step, seg_end,
                                        seg_lr_mult, seg_wd, n_seg,
                                        clip_state, s);
}

// The EMA forms: ema must not be nullptr.
extern "C" hipError_t adamw_ema_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, float wd, int step, float grad_scale,
    hipStream_t s) {
  if (!ema) return hipErrorInvalidValue;
  return adamw_dispatch(p_bf16, grad, grad_is_f32, m, v, master, ema,
                        ema_decay, n, lr, beta1, beta2, eps, wd, step,
                        grad_scale, s);
}

extern "C" hipError_t adamw_clipped_ema_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, float wd, int step, const void* clip_state,
    hipStream_t s) {
  if (!ema) return hipErrorInvalidValue;
  return adamw_clipped_dispatch(p_bf16, grad, grad_is_f32, m, v, master, ema,
                                ema_decay, n, lr, beta1, beta2, eps, wd, step,
                                clip_state, s);
}

extern "C" hipError_t adamw_grouped_ema_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, int step, const void* seg_end,
    const void* seg_lr_mult, const void* seg_wd, int n_seg, float grad_scale,
    hipStream_t s) {
  if (!ema) return hipErrorInvalidValue;
  return adamw_grouped_dispatch(p_bf16, grad, grad_is_f32, m, v, master, ema,
                                ema_decay, n, lr, beta1, beta2, eps, step,
                                seg_end, seg_lr_mult, seg_wd, n_seg,
                                grad_scale, s);
}

extern "C" hipError_t adamw_grouped_clipped_ema_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, int step, const void* seg_end,
    const void* seg_lr_mult, const void* seg_wd, int n_seg,
    const void* clip_state, hipStream_t s) {
  if (!ema) return hipErrorInvalidValue;
  return adamw_grouped_clipped_dispatch(p_bf16, grad, grad_is_f32, m, v,
                                        master, ema, ema_decay, n, lr, beta1,
                                        beta2, eps, step, seg_end,
                                        seg_lr_mult, seg_wd, n_seg,
                                        clip_state, s);
}
