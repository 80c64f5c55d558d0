// The one declaration of every C-linkage launcher and host-side geometry
// query the bindings (ops.cpp) call.  Every kernel file includes this header
// too, so a definition that disagrees with its declaration does not compile.
//
// Conventions: bf16 tensors travel as void*; every tensor is contiguous and
// row-major; "nullptr = none" marks an optional operand.  A kernel file owns
// its launch geometry: no launcher takes a grid, and where the bindings must
// size a workspace from it, the file exports the query next to the launcher.
#pragma once

#include <hip/hip_runtime.h>

extern "C" {

// ---- layernorm.hip ----------------------------------------------------------
// x, y, s_out [N, D] bf16; gamma, beta [D] bf16; mean, rstd [N] f32.
// res (nullptr = none) is added to x first and the sum is written to s_out
// (nullptr exactly when res is).
hipError_t ln_fwd_launch(const void* x, const void* res, const void* gamma,
                         const void* beta, void* y, void* s_out, void* mean,
                         void* rstd, int N, int D, float eps,
                         hipStream_t stream);
// ws is [ln_bwd_ws_rows(N, D), n_out * D] f32, n_out = 2 ([dgamma | dbeta])
// or 3 (+ [dres_sum]); ds_extra (nullptr = none) is [N, D] bf16, added to dx.
hipError_t ln_bwd_launch(const void* dy, const void* x, const void* gamma,
                         const void* mean, const void* rstd,
                         const void* ds_extra, void* dx, void* ws, int n_out,
                         int N, int D, hipStream_t stream);
int ln_bwd_ws_rows(int N, int D);
// Fused residual dropout (philox.h): as ln_fwd_launch with res and s_out
// required, s_out = bf16(x + (keep ? res * scale : 0)); as ln_bwd_launch with
// n_out = 2 and a second output dres [N, D] bf16 = keep ? bf16(v * scale) : 0,
// v the f32 value dx is rounded from.  seed, call, site: the mask's key and
// counter words; thr in [1, 65535]: an element is dropped iff its 16 random
// bits are below thr, scale = 65536 / (65536 - thr).  The backward takes
// D <= ln_drop_bwd_max_d() and sizes ws with ln_bwd_ws_rows.
hipError_t ln_drop_fwd_launch(const void* x, const void* res,
                              const void* gamma, const void* beta, void* y,
                              void* s_out, void* mean, void* rstd, int N,
                              int D, float eps, unsigned long long seed,
                              unsigned call, unsigned site, unsigned thr,
                              hipStream_t stream);
hipError_t ln_drop_bwd_launch(const void* dy, const void* x,
                              const void* gamma, const void* mean,
                              const void* rstd, const void* ds_extra, void* dx,
                              void* dres, void* ws, int N, int D,
                              unsigned long long seed, unsigned call,
                              unsigned site, unsigned thr,
                              hipStream_t stream);
int ln_drop_bwd_max_d(void);
// MX output (inference; mx_quant.hip below for the format): as ln_fwd_launch
// without mean and rstd, and instead of y the MXFP8 form of the bf16 values y
// would hold: q [N, D] e4m3 bytes, scales [N, D / 32] e8m0 bytes.  D % 32 == 0,
// D <= ln_mx_fwd_max_d() (hipErrorInvalidValue otherwise).
hipError_t ln_mx_fwd_launch(const void* x, const void* res, const void* gamma,
                            const void* beta, void* q, void* scales,
                            void* s_out, int N, int D, float eps,
                            hipStream_t stream);
int ln_mx_fwd_max_d(void);

// ---- colsum.hip -------------------------------------------------------------
// ws [R, D] f32 -> out [D] (f32, or bf16 with out_bf16).  scratch is
// [colsum_scratch_rows(), D] f32.  split_w: the width the split count is
// derived from (D, or less when slabs were appended to an existing layout).
hipError_t colsum_launch(const void* ws, void* scratch, void* out, int R,
                         int D, int split_w, int out_bf16,
                         hipStream_t stream);
int colsum_scratch_rows(void);
// x [N, D] bf16 -> out [D] bf16.  scratch is [colsum_bf16_scratch_rows(), D]
// f32.
hipError_t colsum_bf16_launch(const void* x, void* scratch, void* out, long N,
                              int D, hipStream_t stream);
int colsum_bf16_scratch_rows(void);

// ---- bias_gelu.hip ----------------------------------------------------------
// x, y, dy, dx [n_elem / D, D] bf16; b [D] bf16.
hipError_t bias_gelu_fwd_launch(const void* x, const void* b, void* y,
                                long n_elem, int D, hipStream_t stream);
// ws_dbias is [bias_gelu_bwd_ws_rows(n_elem, D), D] f32.
hipError_t bias_gelu_bwd_launch(const void* dy, const void* x, const void* b,
                                void* dx, void* ws_dbias, long n_elem, int D,
                                hipStream_t stream);
int bias_gelu_bwd_ws_rows(long n_elem, int D);

// ---- mx_quant.hip -----------------------------------------------------------
// OCP MXFP8 along K: x, h [R, K] bf16, K % 32 == 0 -> q [R, K] uint8 (e4m3fn
// bytes) and s [R, K / 32] uint8 (e8m0: one power-of-two scale per 32
// consecutive elements), bit for bit ops.reference.mx_quantize of x, or of
// bf16(gelu_tanh(h + b)) with b [K] bf16, the value bias_gelu_fwd_launch
// stores.
hipError_t mx_quant_rows_launch(const void* x, void* q, void* s, long R, int K,
                                hipStream_t stream);
hipError_t mx_bias_gelu_launch(const void* h, const void* b, void* q, void* s,
                               long R, int K, hipStream_t stream);

// ---- softmax.hip ------------------------------------------------------------
// s, p, dp, ds [n_rows, Lk] bf16; mask (nullptr = none) [B, Lk] f32 with
// H_Lq = n_rows / B rows sharing one mask row; lse [n_rows] f32.
hipError_t softmax_fwd_launch(const void* s, const void* mask, void* p,
                              long n_rows, int Lk, int H_Lq, float scale,
                              hipStream_t stream);
hipError_t softmax_bwd_launch(const void* dp, const void* p, void* ds,
                              long n_rows, int Lk, float scale,
                              hipStream_t stream);
hipError_t p_from_lse_launch(const void* s, const void* mask, const void* lse,
                             void* p, long n_rows, int Lk, int H_Lq,
                             float scale, hipStream_t stream);

// ---- adamw.hip, grad_norm.hip -----------------------------------------------
// p_bf16 [n] bf16; grad [n] bf16 or f32; m, v, master [n] f32; n % 4 == 0.
hipError_t adamw_launch(void* p_bf16, const void* grad, int grad_is_f32,
                        void* m, void* v, void* master, long n, float lr,
                        float beta1, float beta2, float eps, float wd,
                        int step, float grad_scale, hipStream_t stream);
// clip_state [4] f32 = {norm, scale, finite, sumsq}, on the device.
hipError_t adamw_clipped_launch(void* p_bf16, const void* grad,
                                int grad_is_f32, void* m, void* v,
                                void* master, long n, float lr, float beta1,
                                float beta2, float eps, float wd, int step,
                                const void* clip_state, hipStream_t stream);
// Parameter groups: seg_end [n_seg] int64, strictly increasing exclusive end
// offsets with seg_end[n_seg - 1] == n; seg_lr_mult, seg_wd [n_seg] f32; all
// on the device, 1 <= n_seg <= 1024 (hipErrorInvalidValue otherwise).
// Element e of the first segment s with e < seg_end[s] is updated as
// adamw_launch would with lr * seg_lr_mult[s] and wd = seg_wd[s].
hipError_t adamw_grouped_launch(void* p_bf16, const void* grad,
                                int grad_is_f32, void* m, void* v,
                                void* master, long n, float lr, float beta1,
                                float beta2, float eps, int step,
                                const void* seg_end, const void* seg_lr_mult,
                                const void* seg_wd, int n_seg,
                                float grad_scale, hipStream_t stream);
hipError_t adamw_grouped_clipped_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, long n, float lr, float beta1, float beta2, float eps,
    int step, const void* seg_end, const void* seg_lr_mult,
    const void* seg_wd, int n_seg, const void* clip_state,
    hipStream_t stream);
// The EMA forms of the four: ema [n] f32 (not nullptr, hipErrorInvalidValue
// otherwise), the same flat layout as master, becomes
// ema_decay * ema + (1.f - ema_decay) * w with w the new master value: two f32
// products and one f32 sum, never fused.  p_bf16, m, v and master come out as
// from the launcher without _ema; a skipped step leaves ema untouched too.
hipError_t adamw_ema_launch(void* p_bf16, const void* grad, int grad_is_f32,
                            void* m, void* v, void* master, void* ema,
                            float ema_decay, long n, float lr, float beta1,
                            float beta2, float eps, float wd, int step,
                            float grad_scale, hipStream_t stream);
hipError_t adamw_clipped_ema_launch(void* p_bf16, const void* grad,
                                    int grad_is_f32, void* m, void* v,
                                    void* master, void* ema, float ema_decay,
                                    long n, float lr, float beta1,
                                    float beta2, float eps, float wd, int step,
                                    const void* clip_state,
                                    hipStream_t stream);
hipError_t adamw_grouped_ema_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, int step, const void* seg_end,
    const void* seg_lr_mult, const void* seg_wd, int n_seg, float grad_scale,
    hipStream_t stream);
hipError_t adamw_grouped_clipped_ema_launch(
    void* p_bf16, const void* grad, int grad_is_f32, void* m, void* v,
    void* master, void* ema, float ema_decay, long n, float lr, float beta1,
    float beta2, float eps, int step, const void* seg_end,
    const void* seg_lr_mult, const void* seg_wd, int n_seg,
    const void* clip_state, hipStream_t stream);
// partials is [grad_norm_grid(n)] f32; n % 8 == 0.
hipError_t grad_clip_state_launch(const void* grad, int grad_is_f32, long n,
                                  float grad_scale, float max_norm,
                                  void* partials, void* clip_state,
                                  hipStream_t stream);
int grad_norm_grid(long n);

// ---- cross_entropy.hip ------------------------------------------------------
// logits, dlogits [N, V] bf16, V % 8 == 0; target [N] int64; loss_rows, lse,
// grow [N] f32.  A row whose target is ignore_index or outside [0, V) is
// ignored: loss 0, gradient row zeros.  loss_rows = lse - logits[target];
// dlogits = (exp(logits - lse) - [col == target]) * grow[row], every element
// written.
hipError_t ce_fwd_launch(const void* logits, const void* target,
                         void* loss_rows, void* lse, int N, int V,
                         long ignore_index, hipStream_t stream);
hipError_t ce_bwd_launch(const void* logits, const void* target,
                         const void* lse, const void* grow, void* dlogits,
                         int N, int V, long ignore_index, hipStream_t stream);
// out [2] f32 = {sum(loss_rows) / n_valid, 1 / n_valid}, {0, 0} with no valid
// row; one block, fixed order.  N <= 2^24.
hipError_t ce_mean_launch(const void* loss_rows, const void* target, void* out,
                          int N, int V, long ignore_index, hipStream_t stream);

// ---- repack.hip -------------------------------------------------------------
// [B, L, 3, H, dh] <-> [3, B, H, L, dh] (backward = the inverse); dh % 8 == 0.
hipError_t qkv_repack_launch(const void* src, void* dst, int B, int L, int H,
                             int dh, int backward, hipStream_t stream);
// dq, dk, dv [B, H, L, dh] -> dsrc [B, L, 3, H, dh].
hipError_t qkv_repack_bwd3_launch(const void* dq, const void* dk,
                                  const void* dv, void* dsrc, int B, int L,
                                  int H, int dh, hipStream_t stream);
// [B, H, L, dh] <-> [B, L, H, dh] (backward = the inverse).
hipError_t out_repack_launch(const void* src, void* dst, int B, int L, int H,
                             int dh, int backward, hipStream_t stream);

// ---- flash_attn.hip ---------------------------------------------------------
// Head dim 64, L % 32 == 0.  q, k, v, o, dout, dq, dk, dv [B, H, L, 64] bf16;
// packed: qkv, dqkv [B, L, 3 * H * 64], o, dout [B, L, H * 64]; lse, ddot
// [B, H, L] f32.  mask (nullptr = none) [B, L] f32 additive; seg (nullptr =
// none) [B, L] int32, non-decreasing along a row; at most one of them is set.
// Dropout on the attention probabilities (philox.h): drop_thr in [1, 255]
// drops an element iff its random byte is below it, drop_thr = 0 is no
// dropout; drop_seed, drop_call, drop_site are the mask's key and counter
// words.  The forward and both backward kernels of one attention call take
// the same four.  Not together with ds or bias_ws.
hipError_t flash_fwd_launch(const void* q, const void* k, const void* v,
                            const void* mask, const void* seg, void* o,
                            void* lse, int B, int H, int L, float scale,
                            unsigned long long drop_seed, unsigned drop_call,
                            unsigned drop_site, unsigned drop_thr,
                            hipStream_t stream);
hipError_t flash_fwd_packed_launch(const void* qkv, const void* mask,
                                   const void* seg, void* o, void* lse, int B,
                                   int H, int L, float scale,
                                   unsigned long long drop_seed,
                                   unsigned drop_call, unsigned drop_site,
                                   unsigned drop_thr, hipStream_t stream);
// dead (nullptr = skip nothing) uint8 [B, H, L / 32], as fa_dot writes it:
// the backward kernels leave out the query tiles it marks, whose dO is all
// +-0 and whose contribution is exact zeros.
// ds (nullptr = none) [B, H, L, L] bf16; not together with seg, and with ds
// given dead is ignored (every dS tile is written).
hipError_t flash_bwd_fused_launch(const void* q, const void* k, const void* v,
                                  const void* dout, const void* mask,
                                  const void* seg, const void* lse,
                                  const void* ddot, const void* dead,
                                  void* ds, void* dk, void* dv, int B, int H,
                                  int L, float scale,
                                  unsigned long long drop_seed,
                                  unsigned drop_call, unsigned drop_site,
                                  unsigned drop_thr, hipStream_t stream);
// bias_ws (nullptr = none) is [flash_bias_ws_rows(B, L), 3 * H * 64] f32; the
// fused launcher fills its k and v thirds, the dq launcher its q third.
hipError_t flash_bwd_fused_packed_launch(const void* qkv, const void* dout,
                                         const void* mask, const void* seg,
                                         const void* lse, const void* ddot,
                                         const void* dead, void* dqkv,
                                         void* bias_ws, int B, int H, int L,
                                         float scale,
                                         unsigned long long drop_seed,
                                         unsigned drop_call,
                                         unsigned drop_site, unsigned drop_thr,
                                         hipStream_t stream);
hipError_t flash_dq_recompute_packed_launch(const void* qkv, const void* dout,
                                            const void* mask, const void* seg,
                                            const void* lse, const void* ddot,
                                            const void* dead, void* dqkv,
                                            void* bias_ws, int B, int H, int L,
                                            float scale,
                                            unsigned long long drop_seed,
                                            unsigned drop_call,
                                            unsigned drop_site,
                                            unsigned drop_thr,
                                            hipStream_t stream);
int flash_bias_ws_rows(int B, int L);
hipError_t flash_dq_recompute_launch(const void* q, const void* k,
                                     const void* v, const void* dout,
                                     const void* mask, const void* seg,
                                     const void* lse, const void* ddot,
                                     const void* dead, void* dq, int B, int H,
                                     int L, float scale,
                                     unsigned long long drop_seed,
                                     unsigned drop_call, unsigned drop_site,
                                     unsigned drop_thr, hipStream_t stream);
// ds [B, H, L, L] bf16.
hipError_t flash_dq_launch(const void* ds, const void* k, void* dq, int B,
                           int H, int L, hipStream_t stream);
// ddot [n_rows] f32 = rowsum(dout * o) over rows of 64; dead uint8
// [ceil(n_rows / 32)] (packed: [B, H, L / 32]) = 1 where all 32 x 64 dout
// elements of the tile are +-0, else 0.  Every element of both is written.
hipError_t fa_dot_launch(const void* dout, const void* o, void* ddot,
                         void* dead, long n_rows, hipStream_t stream);
hipError_t fa_dot_packed_launch(const void* dout, const void* o, void* ddot,
                                void* dead, int B, int H, int L,
                                hipStream_t stream);
// src [256] bf16 -> out [64, 4] bf16.
hipError_t tr_probe_launch(const void* src, void* out, int scheme,
                           hipStream_t stream);

// ---- pool.hip ---------------------------------------------------------------
// x, dx [B, L, D] bf16; mask (nullptr = none) [B, L] bool; pooled, dpooled
// [B, D] bf16; counts [B] f32; ws is [B, masked_pool_ws_splits(), D] f32.
hipError_t masked_pool_fwd_launch(const void* x, const void* mask,
                                  void* pooled, void* counts, void* ws, int B,
                                  int L, int D, hipStream_t stream);
int masked_pool_ws_splits(void);
hipError_t masked_pool_bwd_launch(const void* dpooled, const void* mask,
                                  const void* counts, void* dx, int B, int L,
                                  int D, hipStream_t stream);
// x, dx [T, D] bf16; seg_start, seg_len [N] int32; pos2seg [T] int32 (-1 =
// padding); pooled, dpooled [N, D] bf16.
hipError_t segment_pool_fwd_launch(const void* x, const void* seg_start,
                                   const void* seg_len, void* pooled, int N,
                                   long T, int D, hipStream_t stream);
hipError_t segment_pool_bwd_launch(const void* dpooled, const void* pos2seg,
                                   const void* seg_len, void* dx, int N,
                                   long T, int D, hipStream_t stream);

// ---- wgrad_gemm.hip ---------------------------------------------------------
// out [M, N] bf16 = a [K, M]^T @ b [K, N]; ws [S, M, N] f32 split-K partials;
// M, N multiples of 256, K / S a multiple of 32.
hipError_t wgrad_gemm_launch(const void* a, const void* b, void* ws, void* out,
                             int M, int N, long K, int S, hipStream_t stream);

}  // extern "C"
