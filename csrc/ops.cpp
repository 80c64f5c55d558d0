// Torch bindings for the tosem2021_amd gfx950 HIP kernels.
//
// Host-only translation unit: device code lives in the *.hip files, exposed
// through C-linkage launchers declared once in launchers.h.  A kernel file
// owns its launch geometry and workspace sizes; this file asks for them.
// Uses the HIP-native ATen stream API directly (c10::hip) — no CUDA names, no
// hipify translation of this file is needed.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "lt_gemm.h"

namespace {

#define CHECK_HIP(call)                                                   \
  do {                                                                    \
    hipError_t e_ = (call);                                               \
    TORCH_CHECK(e_ == hipSuccess, "HIP error: ", hipGetErrorString(e_));  \
  } while (0)

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.device().is_cuda(), name, " must be on GPU");
}

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be f32");
  TORCH_CHECK(t.device().is_cuda(), name, " must be on GPU");
}

// `t` is exactly `want`; `shape` is how the message spells it, e.g. "[B, L]".
void check_shape(const torch::Tensor& t, const char* name,
                 at::IntArrayRef want, const char* shape) {
  TORCH_CHECK(t.sizes() == want, name, " must be ", shape);
}

// `t` holds exactly `n` elements, whatever its rank.
void check_numel(const torch::Tensor& t, const char* name, long n,
                 const char* shape) {
  TORCH_CHECK(t.numel() == n, name, " must be ", shape);
}

void check_mult8(long v, const char* name) {
  TORCH_CHECK(v % 8 == 0, name, " must be a multiple of 8, got ", v);
}

// Optional additive softmax key mask: f32, contiguous, on the GPU, exactly
// [B, Lk] for 4-D scores [B, H, Lq, Lk].  Sets H_Lq, the score rows that
// share one mask row.
const void* softmax_mask_ptr(const c10::optional<torch::Tensor>& mask,
                             const torch::Tensor& scores, int* H_Lq) {
  *H_Lq = 1;
  if (!mask.has_value()) return nullptr;
  check_f32(*mask, "mask");
  TORCH_CHECK(scores.dim() == 4, "masked scores must be [B, H, Lq, Lk]");
  check_shape(*mask, "mask", {scores.size(0), scores.size(3)}, "[B, Lk]");
  *H_Lq = (int)(scores.size(1) * scores.size(2));
  return mask->data_ptr();
}

// Optional pooling mask: bool, contiguous, on x's device, exactly [B, L].
const void* pool_mask_ptr(const c10::optional<torch::Tensor>& mask,
                          const torch::Tensor& x, long B, long L) {
  if (!mask.has_value()) return nullptr;
  TORCH_CHECK(mask->scalar_type() == torch::kBool && mask->is_contiguous(),
              "mask must be contiguous bool");
  TORCH_CHECK(mask->device() == x.device(), "mask must be on the same device "
              "as the data");
  check_shape(*mask, "mask", {B, L}, "[B, L]");
  return mask->data_ptr();
}

// One column-sum chain (csrc/colsum.hip): ws [R, W] f32 -> [W], f32 or, with
// out_bf16, bf16 rounded by the final stage.  split_w is the width the split
// count derives from: W, or the narrower width of a layout that slabs were
// appended to, which keeps the earlier slabs' sums bit-identical.
torch::Tensor colsum(const torch::Tensor& ws, long split_w, bool out_bf16) {
  const long R = ws.size(0), W = ws.size(1);
  auto out = torch::empty(
      {W}, out_bf16 ? ws.options().dtype(torch::kBFloat16) : ws.options());
  auto scratch = torch::empty({colsum_scratch_rows(), W}, ws.options());
  CHECK_HIP(colsum_launch(ws.data_ptr(), scratch.data_ptr(), out.data_ptr(),
                          (int)R, (int)W, (int)split_w, out_bf16 ? 1 : 0,
                          cur_stream()));
  return out;
}

// ---- flash-attention argument checks ----------------------------------------
// The kernels index every operand from B, H, L alone, so each entry point
// pins all shapes here, before any launch.

struct FlashDims { long B, H, L; };
using NamedTensor = std::pair<const char*, torch::Tensor>;

// Optional additive key mask: f32, contiguous, on the GPU, exactly [B, L].
const void* flash_mask_ptr(const c10::optional<torch::Tensor>& mask,
                           const FlashDims& d) {
  if (!mask.has_value()) return nullptr;
  check_f32(*mask, "mask");
  TORCH_CHECK(mask->dim() == 2 && mask->size(0) == d.B &&
              mask->size(1) == d.L, "mask must be [B, L]");
  return mask->data_ptr();
}

// Optional segment ids (sequence packing): int32, contiguous, on x's device,
// exactly [B, L]; exclusive with mask.  Row-wise monotonicity is the
// caller's contract (checking it would need a device sync): a row that
// breaks it gives wrong numbers, never an out-of-bounds access.
const void* flash_seg_ptr(const c10::optional<torch::Tensor>& seg,
                          const c10::optional<torch::Tensor>& mask,
                          const torch::Tensor& x, const FlashDims& d) {
  if (!seg.has_value()) return nullptr;
  TORCH_CHECK(!mask.has_value(), "mask and seg are mutually exclusive");
  TORCH_CHECK(seg->scalar_type() == torch::kInt32, "seg must be int32");
  TORCH_CHECK(seg->device() == x.device(), "seg must be on the same device "
              "as the attention inputs");
  TORCH_CHECK(seg->is_contiguous(), "seg must be contiguous");
  TORCH_CHECK(seg->dim() == 2 && seg->size(0) == d.B && seg->size(1) == d.L,
              "seg must be [B, L]");
  return seg->data_ptr();
}

void check_i32(const torch::Tensor& t, const torch::Tensor& like,
               const char* name) {
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32");
  TORCH_CHECK(t.device() == like.device(), name, " must be on the same "
              "device as the data");
}

// Per-row f32 statistics (lse, ddot): [B, H, L].
void check_flash_rows(std::initializer_list<NamedTensor> rows,
                      const FlashDims& d) {
  for (const auto& [name, t] : rows) {
    check_f32(t, name);
    TORCH_CHECK(t.dim() == 3 && t.size(0) == d.B && t.size(1) == d.H &&
                t.size(2) == d.L, name, " must be [B, H, L]");
  }
}

// Attention-probability dropout words as the flash launchers take them
// (csrc/philox.h): thr = 0 is no dropout, else thr = round(p * 256) in
// [1, 255]; seed, call, site select the mask, site = 0x10000 + layer.
struct FlashDrop { unsigned long long seed; unsigned call, site, thr; };

FlashDrop flash_drop_args(uint64_t seed, int64_t call, int64_t site,
                          int64_t thr) {
  TORCH_CHECK(call >= 0 && call <= 0xffffffffLL, "drop_call must fit 32 bits");
  TORCH_CHECK(site >= 0 && site <= 0xffffffffLL, "drop_site must fit 32 bits");
  TORCH_CHECK(thr >= 0 && thr <= 255,
              "attention dropout threshold must be in [0, 255], got ", thr);
  return {seed, (unsigned)call, (unsigned)site, (unsigned)thr};
}

// [B, H, L, 64] family: `x` fixes the geometry, every tensor in `same` is
// bf16 of the same shape, every tensor in `rows` is f32 [B, H, L].
FlashDims check_flash_bhld(const char* xname, const torch::Tensor& x,
                           std::initializer_list<NamedTensor> same,
                           std::initializer_list<NamedTensor> rows) {
  check_bf16(x, xname);
  TORCH_CHECK(x.dim() == 4, xname, " must be [B, H, L, 64]");
  const FlashDims d{x.size(0), x.size(1), x.size(2)};
  TORCH_CHECK(x.size(3) == 64, "flash kernels are specialized for head_dim 64");
  TORCH_CHECK(d.L % 32 == 0, "flash kernels need L % 32 == 0");
  for (const auto& [name, t] : same) {
    check_bf16(t, name);
    TORCH_CHECK(t.sizes() == x.sizes(), name, " must match ", xname,
                "'s shape");
  }
  check_flash_rows(rows, d);
  return d;
}

// Packed family: qkv is [B, L, 3D] with D = H*64, every tensor in `outs` is
// bf16 [B, L, D], every tensor in `rows` is f32 [B, H, L].
FlashDims check_flash_packed(const torch::Tensor& qkv, long H,
                             std::initializer_list<NamedTensor> outs,
                             std::initializer_list<NamedTensor> rows) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, L, 3D]");
  const FlashDims d{qkv.size(0), H, qkv.size(1)};
  TORCH_CHECK(qkv.size(2) == 3 * H * 64, "qkv last dim must be 3*H*64");
  TORCH_CHECK(d.L % 32 == 0, "flash kernels need L % 32 == 0");
  for (const auto& [name, t] : outs) {
    check_bf16(t, name);
    TORCH_CHECK(t.dim() == 3 && t.size(0) == d.B && t.size(1) == d.L &&
                t.size(2) == H * 64, name, " must be [B, L, H*64]");
  }
  check_flash_rows(rows, d);
  return d;
}

}  // namespace

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x,
                                         c10::optional<torch::Tensor> residual,
                                         torch::Tensor gamma,
                                         torch::Tensor beta, double eps) {
  check_bf16(x, "x"); check_bf16(gamma, "gamma"); check_bf16(beta, "beta");
  const int D = (int)x.size(-1);
  const long N = x.numel() / D;
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8, got ", D);
  check_numel(gamma, "gamma", D, "[D]");
  check_numel(beta, "beta", D, "[D]");
  if (residual.has_value()) {
    check_bf16(*residual, "residual");
    TORCH_CHECK(residual->sizes() == x.sizes(), "residual shape mismatch");
  }
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({N}, opts);
  auto rstd = torch::empty({N}, opts);
  const void* res_ptr = nullptr;
  torch::Tensor s_out;
  void* s_ptr = nullptr;
  if (residual.has_value()) {
    res_ptr = residual->data_ptr();
    s_out = torch::empty_like(x);
    s_ptr = s_out.data_ptr();
  } else {
    s_out = x;  // residual stream unchanged
  }
  CHECK_HIP(ln_fwd_launch(x.data_ptr(), res_ptr, gamma.data_ptr(),
                          beta.data_ptr(), y.data_ptr(), s_ptr,
                          mean.data_ptr(), rstd.data_ptr(), (int)N, D,
                          (float)eps, cur_stream()));
  return {y, s_out, mean, rstd};
}

// Returns {dx, dgamma, dbeta} and, with want_dres, a fourth tensor dres_sum:
// the column sum of the bf16 dx this call returns (the bias gradient of the
// projection whose output was the LayerNorm's residual input).  The column
// outputs are f32, or bf16 with out_bf16; they are slices of one [n * D]
// tensor that a single colsum chain fills.
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor gamma, torch::Tensor mean,
                                         torch::Tensor rstd,
                                         c10::optional<torch::Tensor> ds_extra,
                                         bool want_dres, bool out_bf16) {
  check_bf16(dy, "dy"); check_bf16(x, "x"); check_bf16(gamma, "gamma");
  const int D = (int)x.size(-1);
  const long N = x.numel() / D;
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8, got ", D);
  TORCH_CHECK(dy.numel() == x.numel(), "dy shape mismatch");
  check_numel(gamma, "gamma", D, "[D]");
  check_f32(mean, "mean"); check_f32(rstd, "rstd");
  TORCH_CHECK(mean.numel() == N && rstd.numel() == N,
              "mean and rstd must be [N]");
  const void* de = nullptr;
  if (ds_extra.has_value()) {
    check_bf16(*ds_extra, "ds_extra");
    TORCH_CHECK(ds_extra->numel() == x.numel(), "ds_extra shape mismatch");
    de = ds_extra->data_ptr();
  }
  auto dx = torch::empty_like(x);
  const int n_out = want_dres ? 3 : 2;
  auto ws = torch::empty({ln_bwd_ws_rows((int)N, D), n_out * D},
                         x.options().dtype(torch::kFloat32));
  CHECK_HIP(ln_bwd_launch(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(),
                          mean.data_ptr(), rstd.data_ptr(), de, dx.data_ptr(),
                          ws.data_ptr(), n_out, (int)N, D, cur_stream()));
  // splits from the two-slab width, with or without the third slab
  auto cols = colsum(ws, 2 * D, out_bf16);
  std::vector<torch::Tensor> out = {dx, cols.narrow(0, 0, D),
                                    cols.narrow(0, D, D)};
  if (want_dres) out.push_back(cols.narrow(0, 2 * D, D));
  return out;
}

// The mask's words as the launchers take them (csrc/philox.h).
void check_drop_args(int64_t call, int64_t site, int64_t thr) {
  TORCH_CHECK(call >= 0 && call <= 0xffffffffLL, "call must fit 32 bits");
  TORCH_CHECK(site >= 0 && site <= 0xffffffffLL, "site must fit 32 bits");
  TORCH_CHECK(thr >= 1 && thr <= 65535,
              "dropout threshold must be in [1, 65535], got ", thr);
}

// layernorm_fwd with the residual dropped first:
// s = bf16(x + (keep ? residual * scale : 0)), y = LN(s).  thr is
// round(p * 65536); seed, call, site select the mask.
std::vector<torch::Tensor> layernorm_drop_fwd(torch::Tensor x,
                                              torch::Tensor residual,
                                              torch::Tensor gamma,
                                              torch::Tensor beta, double eps,
                                              uint64_t seed, int64_t call,
                                              int64_t site, int64_t thr) {
  check_bf16(x, "x"); check_bf16(gamma, "gamma"); check_bf16(beta, "beta");
  check_bf16(residual, "residual");
  const int D = (int)x.size(-1);
  const long N = x.numel() / D;
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8, got ", D);
  check_numel(gamma, "gamma", D, "[D]");
  check_numel(beta, "beta", D, "[D]");
  TORCH_CHECK(residual.sizes() == x.sizes(), "residual shape mismatch");
  // the forward kernels take any width; refuse here what the backward
  // cannot follow, before a training step is half done
  TORCH_CHECK(D <= ln_drop_bwd_max_d(), "fused dropout LayerNorm supports "
              "D <= ", ln_drop_bwd_max_d(), ", got ", D);
  check_drop_args(call, site, thr);
  auto y = torch::empty_like(x);
  auto s_out = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({N}, opts);
  auto rstd = torch::empty({N}, opts);
  CHECK_HIP(ln_drop_fwd_launch(x.data_ptr(), residual.data_ptr(),
                               gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                               s_out.data_ptr(), mean.data_ptr(),
                               rstd.data_ptr(), (int)N, D, (float)eps, seed,
                               (unsigned)call, (unsigned)site, (unsigned)thr,
                               cur_stream()));
  return {y, s_out, mean, rstd};
}

// Returns {dx, dres, dgamma, dbeta}: dx, dgamma and dbeta exactly as
// layernorm_bwd's, dres the gradient of the dropped residual, its mask
// regenerated from (seed, call, site, thr).
std::vector<torch::Tensor> layernorm_drop_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor gamma, torch::Tensor mean,
    torch::Tensor rstd, c10::optional<torch::Tensor> ds_extra, bool out_bf16,
    uint64_t seed, int64_t call, int64_t site, int64_t thr) {
  check_bf16(dy, "dy"); check_bf16(x, "x"); check_bf16(gamma, "gamma");
  const int D = (int)x.size(-1);
  const long N = x.numel() / D;
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8, got ", D);
  TORCH_CHECK(D <= ln_drop_bwd_max_d(), "fused dropout LayerNorm backward "
              "supports D <= ", ln_drop_bwd_max_d(), ", got ", D);
  TORCH_CHECK(dy.numel() == x.numel(), "dy shape mismatch");
  check_numel(gamma, "gamma", D, "[D]");
  check_f32(mean, "mean"); check_f32(rstd, "rstd");
  TORCH_CHECK(mean.numel() == N && rstd.numel() == N,
              "mean and rstd must be [N]");
  check_drop_args(call, site, thr);
  const void* de = nullptr;
  if (ds_extra.has_value()) {
    check_bf16(*ds_extra, "ds_extra");
    TORCH_CHECK(ds_extra->numel() == x.numel(), "ds_extra shape mismatch");
    de = ds_extra->data_ptr();
  }
  auto dx = torch::empty_like(x);
  auto dres = torch::empty_like(x);
  auto ws = torch::empty({ln_bwd_ws_rows((int)N, D), 2 * D},
                         x.options().dtype(torch::kFloat32));
  CHECK_HIP(ln_drop_bwd_launch(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(),
                               mean.data_ptr(), rstd.data_ptr(), de,
                               dx.data_ptr(), dres.data_ptr(), ws.data_ptr(),
                               (int)N, D, seed, (unsigned)call, (unsigned)site,
                               (unsigned)thr, cur_stream()));
  auto cols = colsum(ws, 2 * D, out_bf16);
  return {dx, dres, cols.narrow(0, 0, D), cols.narrow(0, D, D)};
}

torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor b) {
  check_bf16(x, "x"); check_bf16(b, "b");
  const int D = (int)x.size(-1);
  const long n = x.numel();
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8");
  check_numel(b, "b", D, "[D]");
  auto y = torch::empty_like(x);
  CHECK_HIP(bias_gelu_fwd_launch(x.data_ptr(), b.data_ptr(), y.data_ptr(), n,
                                 D, cur_stream()));
  return y;
}

// ---- MXFP8 operands (csrc/mx_quant.hip, MX output of csrc/layernorm.hip) ----
// Every producer returns {q, s}: uint8 e4m3fn bytes shaped like the bf16
// tensor they stand for, and uint8 e8m0 bytes [..., K / 32].

namespace {

long mx_check_k(const torch::Tensor& x, const char* name) {
  const long K = x.size(-1);
  TORCH_CHECK(K > 0 && K % 32 == 0, name, " needs a last dim that is a "
              "multiple of 32 for MXFP8, got ", K);
  return K;
}

std::pair<torch::Tensor, torch::Tensor> mx_outputs(const torch::Tensor& x,
                                                   long K) {
  auto u8 = x.options().dtype(torch::kUInt8);
  auto ssz = x.sizes().vec();
  ssz.back() = K / 32;
  return {torch::empty(x.sizes(), u8), torch::empty(ssz, u8)};
}

}  // namespace

std::vector<torch::Tensor> mx_quant_rows(torch::Tensor x) {
  check_bf16(x, "x");
  const long K = mx_check_k(x, "x");
  auto [q, s] = mx_outputs(x, K);
  if (x.numel() == 0) return {q, s};
  CHECK_HIP(mx_quant_rows_launch(x.data_ptr(), q.data_ptr(), s.data_ptr(),
                                 x.numel() / K, (int)K, cur_stream()));
  return {q, s};
}

std::vector<torch::Tensor> mx_bias_gelu(torch::Tensor h, torch::Tensor b) {
  check_bf16(h, "h"); check_bf16(b, "b");
  const long K = mx_check_k(h, "h");
  check_numel(b, "b", K, "[K]");
  auto [q, s] = mx_outputs(h, K);
  if (h.numel() == 0) return {q, s};
  CHECK_HIP(mx_bias_gelu_launch(h.data_ptr(), b.data_ptr(), q.data_ptr(),
                                s.data_ptr(), h.numel() / K, (int)K,
                                cur_stream()));
  return {q, s};
}

// {q, s, sum}: the MXFP8 form of layernorm_fwd's y, and its s_out (x itself
// without a residual).  No mean or rstd: inference only.
std::vector<torch::Tensor> mx_layernorm_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> residual,
    torch::Tensor gamma, torch::Tensor beta, double eps) {
  check_bf16(x, "x"); check_bf16(gamma, "gamma"); check_bf16(beta, "beta");
  const long D = mx_check_k(x, "x");
  TORCH_CHECK(D <= ln_mx_fwd_max_d(), "LayerNorm with MX output covers D <= ",
              ln_mx_fwd_max_d(), ", got ", D);
  const long N = x.numel() / D;
  check_numel(gamma, "gamma", D, "[D]");
  check_numel(beta, "beta", D, "[D]");
  auto [q, s] = mx_outputs(x, D);
  const void* res_ptr = nullptr;
  torch::Tensor sum = x;
  void* sum_ptr = nullptr;
  if (residual.has_value()) {
    check_bf16(*residual, "residual");
    TORCH_CHECK(residual->sizes() == x.sizes(), "residual shape mismatch");
    res_ptr = residual->data_ptr();
    sum = torch::empty_like(x);
    sum_ptr = sum.data_ptr();
  }
  if (N == 0) return {q, s, sum};
  CHECK_HIP(ln_mx_fwd_launch(x.data_ptr(), res_ptr, gamma.data_ptr(),
                             beta.data_ptr(), q.data_ptr(), s.data_ptr(),
                             sum_ptr, (int)N, (int)D, (float)eps,
                             cur_stream()));
  return {q, s, sum};
}

// dbias is f32, or bf16 with out_bf16 (rounded by the final colsum stage).
std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor b, bool out_bf16) {
  check_bf16(dy, "dy"); check_bf16(x, "x"); check_bf16(b, "b");
  const int D = (int)x.size(-1);
  const long n = x.numel();
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8");
  check_numel(b, "b", D, "[D]");
  TORCH_CHECK(dy.numel() == x.numel(), "dy shape mismatch");
  auto dx = torch::empty_like(x);
  auto ws = torch::empty({bias_gelu_bwd_ws_rows(n, D), D},
                         x.options().dtype(torch::kFloat32));
  CHECK_HIP(bias_gelu_bwd_launch(dy.data_ptr(), x.data_ptr(), b.data_ptr(),
                                 dx.data_ptr(), ws.data_ptr(), n, D,
                                 cur_stream()));
  return {dx, colsum(ws, D, out_bf16)};
}

torch::Tensor softmax_fwd(torch::Tensor scores, c10::optional<torch::Tensor> mask,
                          double scale) {
  check_bf16(scores, "scores");
  const int Lk = (int)scores.size(-1);
  const long n_rows = scores.numel() / Lk;
  check_mult8(Lk, "Lk");
  int H_Lq;
  const void* mptr = softmax_mask_ptr(mask, scores, &H_Lq);
  auto p = torch::empty_like(scores);
  CHECK_HIP(softmax_fwd_launch(scores.data_ptr(), mptr, p.data_ptr(), n_rows,
                               Lk, H_Lq, (float)scale, cur_stream()));
  return p;
}

torch::Tensor softmax_bwd(torch::Tensor dp, torch::Tensor p, double scale) {
  check_bf16(dp, "dp"); check_bf16(p, "p");
  const int Lk = (int)p.size(-1);
  const long n_rows = p.numel() / Lk;
  check_mult8(Lk, "Lk");
  TORCH_CHECK(dp.sizes() == p.sizes(), "dp must match p's shape");
  auto ds = torch::empty_like(p);
  CHECK_HIP(softmax_bwd_launch(dp.data_ptr(), p.data_ptr(), ds.data_ptr(),
                               n_rows, Lk, (float)scale, cur_stream()));
  return ds;
}

// The weight average of the EMA forms of the AdamW step: f32 [n], contiguous,
// 16-byte aligned (16 B per lane loads), on p's device; 0 <= decay < 1.
void check_ema(const torch::Tensor& ema, const torch::Tensor& p,
               double ema_decay) {
  check_f32(ema, "ema");
  TORCH_CHECK(ema.numel() == p.numel(), "ema must have p's length");
  TORCH_CHECK(ema.device() == p.device(), "ema must be on p's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ema.data_ptr()) % 16 == 0,
              "ema must be 16-byte aligned");
  TORCH_CHECK(ema_decay >= 0.0 && ema_decay < 1.0,
              "ema_decay must be in [0, 1), got ", ema_decay);
}

void adamw_step(torch::Tensor p, torch::Tensor grad, torch::Tensor m,
                torch::Tensor v, torch::Tensor master, double lr, double beta1,
                double beta2, double eps, double wd, long step,
                double grad_scale, c10::optional<torch::Tensor> ema,
                double ema_decay) {
  check_bf16(p, "p"); check_f32(m, "m"); check_f32(v, "v");
  check_f32(master, "master");
  TORCH_CHECK(grad.is_contiguous() && grad.device().is_cuda(), "bad grad");
  int gf32 = grad.scalar_type() == torch::kFloat32;
  TORCH_CHECK(gf32 || grad.scalar_type() == torch::kBFloat16,
              "grad must be f32 or bf16");
  const long n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat parameter buffer must be padded to 4 elems");
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n &&
              master.numel() == n, "size mismatch");
  if (ema.has_value()) {
    check_ema(*ema, p, ema_decay);
    CHECK_HIP(adamw_ema_launch(
        p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(), v.data_ptr(),
        master.data_ptr(), ema->data_ptr(), (float)ema_decay, n, (float)lr,
        (float)beta1, (float)beta2, (float)eps, (float)wd, (int)step,
        (float)grad_scale, cur_stream()));
    return;
  }
  CHECK_HIP(adamw_launch(p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(),
                         v.data_ptr(), master.data_ptr(), n, (float)lr,
                         (float)beta1, (float)beta2, (float)eps, (float)wd,
                         (int)step, (float)grad_scale, cur_stream()));
}

// The flat gradient buffer of the clipped step: bf16 or f32, contiguous, a
// multiple of 8 elements and 16-byte aligned (16 B per lane loads).
int check_flat_grad(const torch::Tensor& grad) {
  TORCH_CHECK(grad.is_contiguous() && grad.device().is_cuda(), "bad grad");
  int gf32 = grad.scalar_type() == torch::kFloat32;
  TORCH_CHECK(gf32 || grad.scalar_type() == torch::kBFloat16,
              "grad must be f32 or bf16");
  TORCH_CHECK(grad.numel() > 0 && grad.numel() % 8 == 0,
              "flat gradient buffer must be padded to 8 elems");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(grad.data_ptr()) % 16 == 0,
              "flat gradient buffer must be 16-byte aligned");
  return gf32;
}

// clip_state = {norm, scale, finite, sumsq} on the device (csrc/grad_norm.hip);
// nothing is read back here.
torch::Tensor grad_clip_state(torch::Tensor grad, double grad_scale,
                              double max_norm) {
  int gf32 = check_flat_grad(grad);
  TORCH_CHECK(max_norm > 0, "max_norm must be greater than 0");
  const long n = grad.numel();
  auto opts = torch::TensorOptions().dtype(torch::kFloat32)
                  .device(grad.device());
  auto partials = torch::empty({grad_norm_grid(n)}, opts);
  auto state = torch::empty({4}, opts);
  CHECK_HIP(grad_clip_state_launch(grad.data_ptr(), gf32, n,
                                   (float)grad_scale, (float)max_norm,
                                   partials.data_ptr(), state.data_ptr(),
                                   cur_stream()));
  return state;
}

void adamw_step_clipped(torch::Tensor p, torch::Tensor grad, torch::Tensor m,
                        torch::Tensor v, torch::Tensor master, double lr,
                        double beta1, double beta2, double eps, double wd,
                        long step, torch::Tensor clip_state,
                        c10::optional<torch::Tensor> ema, double ema_decay) {
  check_bf16(p, "p"); check_f32(m, "m"); check_f32(v, "v");
  check_f32(master, "master"); check_f32(clip_state, "clip_state");
  int gf32 = check_flat_grad(grad);
  TORCH_CHECK(clip_state.numel() == 4, "clip_state must hold 4 floats");
  const long n = p.numel();
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n &&
              master.numel() == n, "size mismatch");
  if (ema.has_value()) {
    check_ema(*ema, p, ema_decay);
    CHECK_HIP(adamw_clipped_ema_launch(
        p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(), v.data_ptr(),
        master.data_ptr(), ema->data_ptr(), (float)ema_decay, n, (float)lr,
        (float)beta1, (float)beta2, (float)eps, (float)wd, (int)step,
        clip_state.data_ptr(), cur_stream()));
    return;
  }
  CHECK_HIP(adamw_clipped_launch(p.data_ptr(), grad.data_ptr(), gf32,
                                 m.data_ptr(), v.data_ptr(),
                                 master.data_ptr(), n, (float)lr,
                                 (float)beta1, (float)beta2, (float)eps,
                                 (float)wd, (int)step, clip_state.data_ptr(),
                                 cur_stream()));
}

// The segment table of the grouped AdamW step: seg_end int64, seg_lr_mult
// and seg_wd f32, one length 1 <= S <= 1024, contiguous, on the device.
// That seg_end increases strictly up to n is checked on the host table
// before upload (tosem2021_amd.ops.check_segment_table), not read back here.
int check_segment_table(const torch::Tensor& seg_end,
                        const torch::Tensor& seg_lr_mult,
                        const torch::Tensor& seg_wd) {
  TORCH_CHECK(seg_end.is_contiguous() && seg_end.device().is_cuda() &&
              seg_end.scalar_type() == torch::kInt64 && seg_end.dim() == 1,
              "seg_end must be a contiguous 1-D int64 tensor on the GPU");
  check_f32(seg_lr_mult, "seg_lr_mult"); check_f32(seg_wd, "seg_wd");
  const long S = seg_end.numel();
  TORCH_CHECK(seg_lr_mult.dim() == 1 && seg_wd.dim() == 1 &&
              seg_lr_mult.numel() == S && seg_wd.numel() == S,
              "seg_end, seg_lr_mult and seg_wd must have one length");
  TORCH_CHECK(S >= 1 && S <= 1024,
              "the segment table holds 1 to 1024 segments, got ", S);
  return (int)S;
}

void adamw_step_grouped(torch::Tensor p, torch::Tensor grad, torch::Tensor m,
                        torch::Tensor v, torch::Tensor master,
                        torch::Tensor seg_end, torch::Tensor seg_lr_mult,
                        torch::Tensor seg_wd, double lr, double beta1,
                        double beta2, double eps, long step,
                        double grad_scale, c10::optional<torch::Tensor> ema,
                        double ema_decay) {
  check_bf16(p, "p"); check_f32(m, "m"); check_f32(v, "v");
  check_f32(master, "master");
  TORCH_CHECK(grad.is_contiguous() && grad.device().is_cuda(), "bad grad");
  int gf32 = grad.scalar_type() == torch::kFloat32;
  TORCH_CHECK(gf32 || grad.scalar_type() == torch::kBFloat16,
              "grad must be f32 or bf16");
  const long n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat parameter buffer must be padded to 4 elems");
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n &&
              master.numel() == n, "size mismatch");
  int S = check_segment_table(seg_end, seg_lr_mult, seg_wd);
  if (ema.has_value()) {
    check_ema(*ema, p, ema_decay);
    CHECK_HIP(adamw_grouped_ema_launch(
        p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(), v.data_ptr(),
        master.data_ptr(), ema->data_ptr(), (float)ema_decay, n, (float)lr,
        (float)beta1, (float)beta2, (float)eps, (int)step, seg_end.data_ptr(),
        seg_lr_mult.data_ptr(), seg_wd.data_ptr(), S, (float)grad_scale,
        cur_stream()));
    return;
  }
  CHECK_HIP(adamw_grouped_launch(
      p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(), v.data_ptr(),
      master.data_ptr(), n, (float)lr, (float)beta1, (float)beta2, (float)eps,
      (int)step, seg_end.data_ptr(), seg_lr_mult.data_ptr(),
      seg_wd.data_ptr(), S, (float)grad_scale, cur_stream()));
}

void adamw_step_grouped_clipped(torch::Tensor p, torch::Tensor grad,
                                torch::Tensor m, torch::Tensor v,
                                torch::Tensor master, torch::Tensor seg_end,
                                torch::Tensor seg_lr_mult,
                                torch::Tensor seg_wd, double lr, double beta1,
                                double beta2, double eps, long step,
                                torch::Tensor clip_state,
                                c10::optional<torch::Tensor> ema,
                                double ema_decay) {
  check_bf16(p, "p"); check_f32(m, "m"); check_f32(v, "v");
  check_f32(master, "master"); check_f32(clip_state, "clip_state");
  int gf32 = check_flat_grad(grad);
  TORCH_CHECK(clip_state.numel() == 4, "clip_state must hold 4 floats");
  const long n = p.numel();
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n &&
              master.numel() == n, "size mismatch");
  int S = check_segment_table(seg_end, seg_lr_mult, seg_wd);
  if (ema.has_value()) {
    check_ema(*ema, p, ema_decay);
    CHECK_HIP(adamw_grouped_clipped_ema_launch(
        p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(), v.data_ptr(),
        master.data_ptr(), ema->data_ptr(), (float)ema_decay, n, (float)lr,
        (float)beta1, (float)beta2, (float)eps, (int)step, seg_end.data_ptr(),
        seg_lr_mult.data_ptr(), seg_wd.data_ptr(), S, clip_state.data_ptr(),
        cur_stream()));
    return;
  }
  CHECK_HIP(adamw_grouped_clipped_launch(
      p.data_ptr(), grad.data_ptr(), gf32, m.data_ptr(), v.data_ptr(),
      master.data_ptr(), n, (float)lr, (float)beta1, (float)beta2, (float)eps,
      (int)step, seg_end.data_ptr(), seg_lr_mult.data_ptr(),
      seg_wd.data_ptr(), S, clip_state.data_ptr(), cur_stream()));
}

// Cross-entropy operands (csrc/cross_entropy.hip): logits [N, V] bf16 with
// V % 8 == 0 and a 16-byte aligned base (16 B per lane loads), target [N]
// int64 on the same device.  Sets N and V.
void check_ce(const torch::Tensor& logits, const torch::Tensor& target,
              long& N, long& V) {
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2, "logits must be [N, V]");
  N = logits.size(0);
  V = logits.size(1);
  TORCH_CHECK(V > 0, "V must be positive");
  check_mult8(V, "V");
  TORCH_CHECK(V <= (1L << 30) && N <= (1L << 24),
              "cross-entropy supports V <= 2^30 and N <= 2^24");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
              "logits must be 16-byte aligned");
  TORCH_CHECK(target.is_contiguous() &&
              target.scalar_type() == torch::kInt64,
              "target must be contiguous int64");
  TORCH_CHECK(target.device() == logits.device(),
              "target must be on the same device as logits");
  check_shape(target, "target", {N}, "[N]");
}

// Returns (mean f32[2] = {mean loss over the valid rows, 1 / n_valid},
// loss_rows [N] f32, lse [N] f32); nothing is read back here.
std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits,
                                             torch::Tensor target,
                                             long ignore_index) {
  long N, V;
  check_ce(logits, target, N, V);
  auto opts = torch::TensorOptions().dtype(torch::kFloat32)
                  .device(logits.device());
  auto loss_rows = torch::empty({N}, opts);
  auto lse = torch::empty({N}, opts);
  auto mean = torch::empty({2}, opts);
  CHECK_HIP(ce_fwd_launch(logits.data_ptr(), target.data_ptr(),
                          loss_rows.data_ptr(), lse.data_ptr(), (int)N,
                          (int)V, ignore_index, cur_stream()));
  CHECK_HIP(ce_mean_launch(loss_rows.data_ptr(), target.data_ptr(),
                           mean.data_ptr(), (int)N, (int)V, ignore_index,
                           cur_stream()));
  return {mean, loss_rows, lse};
}

torch::Tensor cross_entropy_bwd(torch::Tensor logits, torch::Tensor target,
                                torch::Tensor lse, torch::Tensor grow,
                                long ignore_index) {
  long N, V;
  check_ce(logits, target, N, V);
  check_f32(lse, "lse"); check_f32(grow, "grow");
  TORCH_CHECK(lse.device() == logits.device() &&
              grow.device() == logits.device(),
              "lse and grow must be on the same device as logits");
  check_shape(lse, "lse", {N}, "[N]");
  check_shape(grow, "grow", {N}, "[N]");
  // its own buffer; the kernel writes every element
  auto dlogits = torch::empty_like(logits);
  CHECK_HIP(ce_bwd_launch(logits.data_ptr(), target.data_ptr(),
                          lse.data_ptr(), grow.data_ptr(),
                          dlogits.data_ptr(), (int)N, (int)V, ignore_index,
                          cur_stream()));
  return dlogits;
}

torch::Tensor qkv_repack(torch::Tensor qkv, long H, bool backward) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(H > 0, "H must be positive");
  long B, L, dh;
  if (!backward) {
    // [B, L, 3*H*dh] or [B, L, 3, H, dh] -> [3, B, H, L, dh]
    TORCH_CHECK(qkv.dim() == 3 || qkv.dim() == 5,
                "qkv must be [B, L, 3*H*dh] or [B, L, 3, H, dh]");
    B = qkv.size(0); L = qkv.size(1);
    if (qkv.dim() == 3) {
      TORCH_CHECK(qkv.size(2) % (3 * H) == 0,
                  "qkv last dim must divide evenly by 3*H");
      dh = qkv.size(2) / (3 * H);
    } else {
      check_shape(qkv, "qkv", {B, L, 3, H, qkv.size(4)}, "[B, L, 3, H, dh]");
      dh = qkv.size(4);
    }
  } else {
    // grad [3, B, H, L, dh] -> [B, L, 3*H*dh]
    TORCH_CHECK(qkv.dim() == 5, "qkv grad must be [3, B, H, L, dh]");
    B = qkv.size(1); L = qkv.size(3);
    dh = qkv.size(4);
    check_shape(qkv, "qkv grad", {3, B, H, L, dh}, "[3, B, H, L, dh]");
  }
  check_mult8(dh, "head_dim");
  auto out = backward ? torch::empty({B, L, 3 * H * dh}, qkv.options())
                      : torch::empty({3, B, H, L, dh}, qkv.options());
  CHECK_HIP(qkv_repack_launch(qkv.data_ptr(), out.data_ptr(), (int)B, (int)L,
                              (int)H, (int)dh, backward ? 1 : 0,
                              cur_stream()));
  return out;
}

torch::Tensor qkv_repack_bwd3(torch::Tensor dq, torch::Tensor dk,
                              torch::Tensor dv) {
  check_bf16(dq, "dq"); check_bf16(dk, "dk"); check_bf16(dv, "dv");
  TORCH_CHECK(dq.dim() == 4, "dq must be [B, H, L, dh]");
  TORCH_CHECK(dk.sizes() == dq.sizes(), "dk must match dq's shape");
  TORCH_CHECK(dv.sizes() == dq.sizes(), "dv must match dq's shape");
  long B = dq.size(0), H = dq.size(1), L = dq.size(2), dh = dq.size(3);
  check_mult8(dh, "head_dim");
  auto out = torch::empty({B, L, 3 * H * dh}, dq.options());
  CHECK_HIP(qkv_repack_bwd3_launch(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                   out.data_ptr(), (int)B, (int)L, (int)H,
                                   (int)dh, cur_stream()));
  return out;
}

// [B, H, L, dh] -> [B, L, H*dh]
torch::Tensor out_repack(torch::Tensor x, bool backward) {
  check_bf16(x, "x");
  TORCH_CHECK(!backward,
              "pass the 4-D grad with explicit dims via out_repack_bwd");
  TORCH_CHECK(x.dim() == 4, "x must be [B, H, L, dh]");
  long B = x.size(0), H = x.size(1), L = x.size(2), dh = x.size(3);
  check_mult8(dh, "head_dim");
  auto out = torch::empty({B, L, H * dh}, x.options());
  CHECK_HIP(out_repack_launch(x.data_ptr(), out.data_ptr(), (int)B, (int)L,
                              (int)H, (int)dh, 0, cur_stream()));
  return out;
}

// [B, L, H*dh] -> [B, H, L, dh]
torch::Tensor out_repack_bwd(torch::Tensor dgrad, long H) {
  check_bf16(dgrad, "dgrad");
  TORCH_CHECK(dgrad.dim() == 3, "dgrad must be [B, L, H*dh]");
  TORCH_CHECK(H > 0 && dgrad.size(2) % H == 0,
              "dgrad last dim must divide evenly by H");
  long B = dgrad.size(0), L = dgrad.size(1), dh = dgrad.size(2) / H;
  check_mult8(dh, "head_dim");
  auto out = torch::empty({B, H, L, dh}, dgrad.options());
  CHECK_HIP(out_repack_launch(dgrad.data_ptr(), out.data_ptr(), (int)B,
                              (int)L, (int)H, (int)dh, 1, cur_stream()));
  return out;
}

std::vector<torch::Tensor> flash_fwd(torch::Tensor q, torch::Tensor k,
                                     torch::Tensor v,
                                     c10::optional<torch::Tensor> mask,
                                     double scale,
                                     c10::optional<torch::Tensor> seg,
                                     uint64_t drop_seed, int64_t drop_call,
                                     int64_t drop_site, int64_t drop_thr) {
  const auto [B, H, L] = check_flash_bhld("q", q, {{"k", k}, {"v", v}}, {});
  const auto dr = flash_drop_args(drop_seed, drop_call, drop_site, drop_thr);
  const void* mptr = flash_mask_ptr(mask, {B, H, L});
  const void* sptr = flash_seg_ptr(seg, mask, q, {B, H, L});
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, L}, q.options().dtype(torch::kFloat32));
  CHECK_HIP(flash_fwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), mptr,
                             sptr, o.data_ptr(), lse.data_ptr(), (int)B,
                             (int)H, (int)L, (float)scale, dr.seed, dr.call,
                             dr.site, dr.thr, cur_stream()));
  return {o, lse};
}

torch::Tensor p_from_lse(torch::Tensor scores, c10::optional<torch::Tensor> mask,
                         torch::Tensor lse, double scale) {
  check_bf16(scores, "scores"); check_f32(lse, "lse");
  const int Lk = (int)scores.size(-1);
  const long n_rows = scores.numel() / Lk;
  TORCH_CHECK(lse.numel() == n_rows, "lse size mismatch");
  check_mult8(Lk, "Lk");
  int H_Lq;
  const void* mptr = softmax_mask_ptr(mask, scores, &H_Lq);
  auto p = torch::empty_like(scores);
  CHECK_HIP(p_from_lse_launch(scores.data_ptr(), mptr, lse.data_ptr(),
                              p.data_ptr(), n_rows, Lk, H_Lq, (float)scale,
                              cur_stream()));
  return p;
}

// {ddot [B, H, L] f32, dead [ceil(B * H * L / 32)] bool}: one kernel, one read
// of dout.  dead marks the 32-row tiles of the flat [B * H * L, 64] view whose
// dout is all +-0.
std::vector<torch::Tensor> fa_dot_impl(torch::Tensor dout, torch::Tensor o) {
  check_bf16(dout, "dout"); check_bf16(o, "o");
  TORCH_CHECK(dout.dim() == 4 && o.sizes() == dout.sizes(),
              "dout and o must both be [B, H, L, 64]");
  const long n_rows = dout.numel() / dout.size(-1);
  TORCH_CHECK(dout.size(-1) == 64, "fa_dot expects head_dim 64");
  auto d = torch::empty({n_rows}, dout.options().dtype(torch::kFloat32));
  auto dead = torch::empty({(n_rows + 31) / 32},
                           dout.options().dtype(torch::kBool));
  CHECK_HIP(fa_dot_launch(dout.data_ptr(), o.data_ptr(), d.data_ptr(),
                          dead.data_ptr(), n_rows, cur_stream()));
  return {d.view({dout.size(0), dout.size(1), dout.size(2)}), dead};
}

torch::Tensor fa_dot(torch::Tensor dout, torch::Tensor o) {
  return fa_dot_impl(dout, o)[0];
}

// {ddot, dead [B, H, L / 32] bool}: the flags the backward kernels take.
std::vector<torch::Tensor> fa_dot_flags(torch::Tensor dout, torch::Tensor o) {
  TORCH_CHECK(dout.dim() == 4 && dout.size(2) % 32 == 0,
              "fa_dot_flags needs [B, H, L, 64] with L % 32 == 0");
  auto r = fa_dot_impl(dout, o);
  return {r[0], r[1].view({dout.size(0), dout.size(1), dout.size(2) / 32})};
}

// {ddot, dead} of the packed layout: dout, o [B, L, H * 64].
std::vector<torch::Tensor> fa_dot_packed_impl(const torch::Tensor& dout,
                                              const torch::Tensor& o, long B,
                                              long H, long L) {
  auto ddot = torch::empty({B, H, L}, dout.options().dtype(torch::kFloat32));
  auto dead = torch::empty({B, H, L / 32}, dout.options().dtype(torch::kBool));
  CHECK_HIP(fa_dot_packed_launch(dout.data_ptr(), o.data_ptr(),
                                 ddot.data_ptr(), dead.data_ptr(), (int)B,
                                 (int)H, (int)L, cur_stream()));
  return {ddot, dead};
}

std::vector<torch::Tensor> fa_dot_packed_flags(torch::Tensor dout,
                                               torch::Tensor o, long H) {
  check_bf16(dout, "dout"); check_bf16(o, "o");
  TORCH_CHECK(dout.dim() == 3 && o.sizes() == dout.sizes() &&
              dout.size(2) == H * 64 && dout.size(1) % 32 == 0,
              "dout and o must both be [B, L, H*64] with L % 32 == 0");
  return fa_dot_packed_impl(dout, o, dout.size(0), H, dout.size(1));
}

namespace {
// Optional dead-tile flags for the [B, H, L, 64] backward bindings: bool
// [B, H, L / 32], as fa_dot_flags returns them.
const void* flash_dead_ptr(const c10::optional<torch::Tensor>& dead,
                           const torch::Tensor& x, const FlashDims& d) {
  if (!dead.has_value()) return nullptr;
  TORCH_CHECK(dead->scalar_type() == torch::kBool, "dead must be bool");
  TORCH_CHECK(dead->device() == x.device() && dead->is_contiguous(),
              "dead must be contiguous and on the attention inputs' device");
  TORCH_CHECK(dead->dim() == 3 && dead->size(0) == d.B &&
              dead->size(1) == d.H && dead->size(2) == d.L / 32,
              "dead must be [B, H, L / 32]");
  return dead->data_ptr();
}
}  // namespace

std::vector<torch::Tensor> flash_bwd_fused(torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, torch::Tensor dout,
                                           c10::optional<torch::Tensor> mask,
                                           torch::Tensor lse,
                                           torch::Tensor ddot, double scale,
                                           bool emit_ds,
                                           c10::optional<torch::Tensor> seg,
                                           c10::optional<torch::Tensor> dead,
                                           uint64_t drop_seed,
                                           int64_t drop_call,
                                           int64_t drop_site,
                                           int64_t drop_thr) {
  const auto [B, H, L] = check_flash_bhld(
      "q", q, {{"k", k}, {"v", v}, {"dout", dout}},
      {{"lse", lse}, {"ddot", ddot}});
  const void* mptr = flash_mask_ptr(mask, {B, H, L});
  const void* sptr = flash_seg_ptr(seg, mask, q, {B, H, L});
  TORCH_CHECK(!(sptr && emit_ds), "seg with emit_ds=True is not supported: "
              "the flash_dq A/B path is unsegmented");
  const auto dr = flash_drop_args(drop_seed, drop_call, drop_site, drop_thr);
  TORCH_CHECK(!(dr.thr && emit_ds), "dropout with emit_ds=True is not "
              "supported: the flash_dq A/B path has no dropout");
  // with emit_ds the kernel ignores the flags: every dS tile is written
  const void* dptr = flash_dead_ptr(dead, q, {B, H, L});
  // emit_ds=false (the default): no [B, H, L, L] dS materialization — dQ
  // comes from flash_dq_recompute instead.
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  torch::Tensor ds;
  void* ds_ptr = nullptr;
  if (emit_ds) {
    ds = torch::empty({B, H, L, L}, q.options());
    ds_ptr = ds.data_ptr();
  }
  CHECK_HIP(flash_bwd_fused_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                   dout.data_ptr(), mptr, sptr,
                                   lse.data_ptr(), ddot.data_ptr(), dptr,
                                   ds_ptr, dk.data_ptr(), dv.data_ptr(), (int)B,
                                   (int)H, (int)L, (float)scale, dr.seed,
                                   dr.call, dr.site, dr.thr, cur_stream()));
  if (emit_ds) return {ds, dk, dv};
  return {dk, dv};
}

torch::Tensor wgrad_gemm(torch::Tensor dy, torch::Tensor x,
                         long splits) {
  // dW[M, N] = dy[K, M]^T @ x[K, N]; custom split-K MFMA kernel
  check_bf16(dy, "dy"); check_bf16(x, "x");
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2, "2-D operands required");
  const long K = dy.size(0), M = dy.size(1), N = x.size(1);
  TORCH_CHECK(x.size(0) == K, "K mismatch");
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0, "M, N must be 256-multiples");
  TORCH_CHECK(K % 32 == 0, "K must be a 32-multiple");
  int S = (int)splits;
  if (S <= 0) {   // auto: enough workgroups to fill 256 CUs
    long tiles = (M / 256) * (N / 256);
    S = 1;
    while (S < 32 && tiles * S < 512 && (K / (2L * S)) % 32 == 0) S *= 2;
  }
  TORCH_CHECK((K / S) % 32 == 0, "K/S must be a 32-multiple");
  auto ws = torch::empty({S, M, N}, dy.options().dtype(torch::kFloat32));
  auto out = torch::empty({M, N}, dy.options());
  CHECK_HIP(wgrad_gemm_launch(dy.data_ptr(), x.data_ptr(), ws.data_ptr(),
                              out.data_ptr(), (int)M, (int)N, K, S,
                              cur_stream()));
  return out;
}

torch::Tensor bias_grad(torch::Tensor dy) {
  check_bf16(dy, "dy");
  const int D = (int)dy.size(-1);
  const long N = dy.numel() / D;
  TORCH_CHECK(dy.dim() == 2, "dy must be [N, D]");
  TORCH_CHECK(D % 8 == 0, "D % 8 == 0 required");
  auto scratch = torch::empty({colsum_bf16_scratch_rows(), D},
                              dy.options().dtype(torch::kFloat32));
  auto out = torch::empty({D}, dy.options());
  CHECK_HIP(colsum_bf16_launch(dy.data_ptr(), scratch.data_ptr(),
                               out.data_ptr(), N, D, cur_stream()));
  return out;
}

std::vector<torch::Tensor> flash_fwd_packed(torch::Tensor qkv, long H,
                                            c10::optional<torch::Tensor> mask,
                                            double scale,
                                            c10::optional<torch::Tensor> seg,
                                            uint64_t drop_seed,
                                            int64_t drop_call,
                                            int64_t drop_site,
                                            int64_t drop_thr) {
  // qkv: [B, L, 3D] packed projection output, D = H*64
  const auto dims = check_flash_packed(qkv, H, {}, {});
  const auto dr = flash_drop_args(drop_seed, drop_call, drop_site, drop_thr);
  const long B = dims.B, L = dims.L;
  const void* mptr = flash_mask_ptr(mask, dims);
  const void* sptr = flash_seg_ptr(seg, mask, qkv, dims);
  auto o = torch::empty({B, L, H * 64}, qkv.options());
  auto lse = torch::empty({B, H, L}, qkv.options().dtype(torch::kFloat32));
  CHECK_HIP(flash_fwd_packed_launch(qkv.data_ptr(), mptr, sptr, o.data_ptr(),
                                    lse.data_ptr(), (int)B, (int)H, (int)L,
                                    (float)scale, dr.seed, dr.call, dr.site,
                                    dr.thr, cur_stream()));
  return {o, lse};
}

namespace {

// full packed backward: ddot + dK/dV + dQ, all into one [B, L, 3D] grad.
// With want_bias also dqkv_bias [3D] bf16, the column sum of dqkv over all
// B * L rows (the qkv projection's bias gradient): both kernels emit
// per-workgroup column partials of what they store into one
// [flash_bias_ws_rows(B, L), 3D] f32 workspace and one colsum chain reduces it.
std::vector<torch::Tensor> flash_bwd_packed_impl(
    torch::Tensor qkv, torch::Tensor o, torch::Tensor dout,
    c10::optional<torch::Tensor> mask, torch::Tensor lse, long H,
    double scale, c10::optional<torch::Tensor> seg, bool want_bias,
    bool skip_zero_do, const FlashDrop& dr) {
  const auto dims = check_flash_packed(qkv, H, {{"o", o}, {"dout", dout}},
                                       {{"lse", lse}});
  TORCH_CHECK(!(dr.thr && want_bias), "attention dropout with the folded qkv "
              "bias gradient is not supported");
  const long B = dims.B, L = dims.L;
  const void* mptr = flash_mask_ptr(mask, dims);
  const void* sptr = flash_seg_ptr(seg, mask, qkv, dims);
  const auto dd = fa_dot_packed_impl(dout, o, B, H, L);
  const auto& ddot = dd[0];
  // the flags are always computed (same kernel, same read of dout);
  // skip_zero_do only decides whether the two kernels act on them
  const void* dptr = skip_zero_do ? dd[1].data_ptr() : nullptr;
  auto dqkv = torch::empty_like(qkv);
  torch::Tensor ws;
  void* ws_ptr = nullptr;
  if (want_bias) {
    ws = torch::empty({flash_bias_ws_rows((int)B, (int)L), 3 * H * 64},
                      qkv.options().dtype(torch::kFloat32));
    ws_ptr = ws.data_ptr();
  }
  CHECK_HIP(flash_bwd_fused_packed_launch(
      qkv.data_ptr(), dout.data_ptr(), mptr, sptr, lse.data_ptr(),
      ddot.data_ptr(), dptr, dqkv.data_ptr(), ws_ptr, (int)B, (int)H, (int)L,
      (float)scale, dr.seed, dr.call, dr.site, dr.thr, cur_stream()));
  CHECK_HIP(flash_dq_recompute_packed_launch(
      qkv.data_ptr(), dout.data_ptr(), mptr, sptr, lse.data_ptr(),
      ddot.data_ptr(), dptr, dqkv.data_ptr(), ws_ptr, (int)B, (int)H, (int)L,
      (float)scale, dr.seed, dr.call, dr.site, dr.thr, cur_stream()));
  if (!want_bias) return {dqkv};
  return {dqkv, colsum(ws, ws.size(1), true)};
}

}  // namespace

torch::Tensor flash_bwd_packed(torch::Tensor qkv, torch::Tensor o,
                               torch::Tensor dout,
                               c10::optional<torch::Tensor> mask,
                               torch::Tensor lse, long H, double scale,
                               c10::optional<torch::Tensor> seg,
                               bool skip_zero_do, uint64_t drop_seed,
                               int64_t drop_call, int64_t drop_site,
                               int64_t drop_thr) {
  return flash_bwd_packed_impl(
      qkv, o, dout, mask, lse, H, scale, seg, false, skip_zero_do,
      flash_drop_args(drop_seed, drop_call, drop_site, drop_thr))[0];
}

// {dqkv, dqkv_bias}: see flash_bwd_packed_impl
std::vector<torch::Tensor> flash_bwd_packed_bias(
    torch::Tensor qkv, torch::Tensor o, torch::Tensor dout,
    c10::optional<torch::Tensor> mask, torch::Tensor lse, long H,
    double scale, c10::optional<torch::Tensor> seg, bool skip_zero_do) {
  return flash_bwd_packed_impl(qkv, o, dout, mask, lse, H, scale, seg, true,
                               skip_zero_do, FlashDrop{0, 0, 0, 0});
}

torch::Tensor flash_dq_recompute(torch::Tensor q, torch::Tensor k,
                                 torch::Tensor v, torch::Tensor dout,
                                 c10::optional<torch::Tensor> mask,
                                 torch::Tensor lse, torch::Tensor ddot,
                                 double scale,
                                 c10::optional<torch::Tensor> seg,
                                 c10::optional<torch::Tensor> dead,
                                 uint64_t drop_seed, int64_t drop_call,
                                 int64_t drop_site, int64_t drop_thr) {
  const auto [B, H, L] = check_flash_bhld(
      "q", q, {{"k", k}, {"v", v}, {"dout", dout}},
      {{"lse", lse}, {"ddot", ddot}});
  const auto dr = flash_drop_args(drop_seed, drop_call, drop_site, drop_thr);
  const void* mptr = flash_mask_ptr(mask, {B, H, L});
  const void* sptr = flash_seg_ptr(seg, mask, q, {B, H, L});
  const void* dptr = flash_dead_ptr(dead, q, {B, H, L});
  auto dq = torch::empty_like(q);
  CHECK_HIP(flash_dq_recompute_launch(q.data_ptr(), k.data_ptr(),
                                      v.data_ptr(), dout.data_ptr(), mptr,
                                      sptr, lse.data_ptr(), ddot.data_ptr(),
                                      dptr, dq.data_ptr(), (int)B, (int)H, (int)L,
                                      (float)scale, dr.seed, dr.call, dr.site,
                                      dr.thr, cur_stream()));
  return dq;
}

torch::Tensor flash_dq(torch::Tensor ds, torch::Tensor k) {
  const auto [B, H, L] = check_flash_bhld("k", k, {}, {});
  check_bf16(ds, "ds");
  TORCH_CHECK(ds.dim() == 4 && ds.size(0) == B && ds.size(1) == H &&
              ds.size(2) == L && ds.size(3) == L, "ds must be [B, H, L, L]");
  auto dq = torch::empty_like(k);
  CHECK_HIP(flash_dq_launch(ds.data_ptr(), k.data_ptr(), dq.data_ptr(),
                            (int)B, (int)H, (int)L, cur_stream()));
  return dq;
}

std::vector<torch::Tensor> masked_pool_fwd(torch::Tensor x,
                                           c10::optional<torch::Tensor> mask) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 3, "x must be [B, L, D]");
  long B = x.size(0), L = x.size(1), D = x.size(2);
  check_mult8(D, "D");
  const void* mptr = pool_mask_ptr(mask, x, B, L);
  auto pooled = torch::empty({B, D}, x.options());
  auto counts = torch::empty({B}, x.options().dtype(torch::kFloat32));
  auto ws = torch::empty({B, masked_pool_ws_splits(), D},
                         x.options().dtype(torch::kFloat32));
  CHECK_HIP(masked_pool_fwd_launch(x.data_ptr(), mptr, pooled.data_ptr(),
                                   counts.data_ptr(), ws.data_ptr(), (int)B,
                                   (int)L, (int)D, cur_stream()));
  return {pooled, counts};
}

torch::Tensor masked_pool_bwd(torch::Tensor dpooled,
                              c10::optional<torch::Tensor> mask,
                              torch::Tensor counts, long L) {
  check_bf16(dpooled, "dpooled");
  TORCH_CHECK(dpooled.dim() == 2, "dpooled must be [B, D]");
  long B = dpooled.size(0), D = dpooled.size(1);
  check_mult8(D, "D");
  TORCH_CHECK(L > 0, "L must be positive");
  check_f32(counts, "counts");
  check_shape(counts, "counts", {B}, "[B]");
  const void* mptr = pool_mask_ptr(mask, dpooled, B, L);
  auto dx = torch::empty({B, L, D}, dpooled.options());
  CHECK_HIP(masked_pool_bwd_launch(dpooled.data_ptr(), mptr,
                                   counts.data_ptr(), dx.data_ptr(), (int)B,
                                   (int)L, (int)D, cur_stream()));
  return dx;
}

// x [T, D] bf16 (T = the packed batch's flattened positions); seg_start /
// seg_len [N] int32 -> pooled [N, D]
torch::Tensor segment_pool_fwd(torch::Tensor x, torch::Tensor seg_start,
                               torch::Tensor seg_len) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 2, "x must be [T, D]");
  const long T = x.size(0), D = x.size(1);
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8");
  check_i32(seg_start, x, "seg_start");
  check_i32(seg_len, x, "seg_len");
  TORCH_CHECK(seg_start.dim() == 1 && seg_len.dim() == 1 &&
              seg_start.size(0) == seg_len.size(0),
              "seg_start and seg_len must both be [N]");
  const long N = seg_start.size(0);
  auto pooled = torch::empty({N, D}, x.options());
  CHECK_HIP(segment_pool_fwd_launch(x.data_ptr(), seg_start.data_ptr(),
                                    seg_len.data_ptr(), pooled.data_ptr(),
                                    (int)N, T, (int)D, cur_stream()));
  return pooled;
}

// dpooled [N, D] bf16, pos2seg [T] int32 (-1 = padding), seg_len [N] int32
// -> dx [T, D]
torch::Tensor segment_pool_bwd(torch::Tensor dpooled, torch::Tensor pos2seg,
                               torch::Tensor seg_len, long T) {
  check_bf16(dpooled, "dpooled");
  TORCH_CHECK(dpooled.dim() == 2, "dpooled must be [N, D]");
  const long N = dpooled.size(0), D = dpooled.size(1);
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8");
  check_i32(pos2seg, dpooled, "pos2seg");
  check_i32(seg_len, dpooled, "seg_len");
  TORCH_CHECK(pos2seg.dim() == 1 && pos2seg.size(0) == T,
              "pos2seg must be [T]");
  TORCH_CHECK(seg_len.dim() == 1 && seg_len.size(0) == N,
              "seg_len must be [N]");
  auto dx = torch::empty({T, D}, dpooled.options());
  CHECK_HIP(segment_pool_bwd_launch(dpooled.data_ptr(), pos2seg.data_ptr(),
                                    seg_len.data_ptr(), dx.data_ptr(), (int)N,
                                    T, (int)D, cur_stream()));
  return dx;
}

torch::Tensor tr_probe(torch::Tensor src, long scheme) {
  check_bf16(src, "src");
  TORCH_CHECK(src.numel() == 256);
  auto out = torch::zeros({64, 4}, src.options());
  CHECK_HIP(tr_probe_launch(src.data_ptr(), out.data_ptr(), (int)scheme,
                            cur_stream()));
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("tr_probe", &tr_probe, "ds_read_b64_tr_b16 semantics probe");
  m.def("masked_pool_fwd", &masked_pool_fwd, "masked mean-pool fwd");
  m.def("masked_pool_bwd", &masked_pool_bwd, "masked mean-pool bwd");
  m.def("segment_pool_fwd", &segment_pool_fwd,
        "per-segment mean-pool fwd (sequence packing)");
  m.def("segment_pool_bwd", &segment_pool_bwd,
        "per-segment mean-pool bwd (sequence packing)");
  m.def("flash_fwd", &flash_fwd,
        "flash attention fwd (gfx950 MFMA, dh=64); seg: optional int32 "
        "[B, L] non-decreasing segment ids, exclusive with mask",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("mask"),
        py::arg("scale"), py::arg("seg") = py::none(),
        py::arg("drop_seed") = 0, py::arg("drop_call") = 0,
        py::arg("drop_site") = 0, py::arg("drop_thr") = 0);
  m.def("flash_bwd_fused", &flash_bwd_fused,
        "fused flash bwd: register-accumulated dK/dV (+ optional dS)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dout"),
        py::arg("mask"), py::arg("lse"), py::arg("ddot"), py::arg("scale"),
        py::arg("emit_ds") = false, py::arg("seg") = py::none(),
        py::arg("dead") = py::none(),
        py::arg("drop_seed") = 0, py::arg("drop_call") = 0,
        py::arg("drop_site") = 0, py::arg("drop_thr") = 0);
  m.def("flash_dq_recompute", &flash_dq_recompute,
        "dQ by recompute: S/dP/dS in-register, no dS materialization",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dout"),
        py::arg("mask"), py::arg("lse"), py::arg("ddot"), py::arg("scale"),
        py::arg("seg") = py::none(), py::arg("dead") = py::none(),
        py::arg("drop_seed") = 0, py::arg("drop_call") = 0,
        py::arg("drop_site") = 0, py::arg("drop_thr") = 0);
  m.def("wgrad_gemm", &wgrad_gemm,
        "split-K wgrad GEMM: dW = dy^T @ x (custom MFMA)",
        py::arg("dy"), py::arg("x"), py::arg("splits") = 0);
  m.def("flash_fwd_packed", &flash_fwd_packed,
        "flash fwd on the packed [B,L,3D] QKV projection output",
        py::arg("qkv"), py::arg("H"), py::arg("mask"), py::arg("scale"),
        py::arg("seg") = py::none(),
        py::arg("drop_seed") = 0, py::arg("drop_call") = 0,
        py::arg("drop_site") = 0, py::arg("drop_thr") = 0);
  m.def("flash_bwd_packed", &flash_bwd_packed,
        "full packed flash bwd: ddot + dK/dV + dQ into one [B,L,3D] grad",
        py::arg("qkv"), py::arg("o"), py::arg("dout"), py::arg("mask"),
        py::arg("lse"), py::arg("H"), py::arg("scale"),
        py::arg("seg") = py::none(), py::arg("skip_zero_do") = true,
        py::arg("drop_seed") = 0, py::arg("drop_call") = 0,
        py::arg("drop_site") = 0, py::arg("drop_thr") = 0);
  m.def("flash_bwd_packed_bias", &flash_bwd_packed_bias,
        "flash_bwd_packed plus the column sum of dqkv (qkv bias grad, bf16)",
        py::arg("qkv"), py::arg("o"), py::arg("dout"), py::arg("mask"),
        py::arg("lse"), py::arg("H"), py::arg("scale"),
        py::arg("seg") = py::none(), py::arg("skip_zero_do") = true);
  m.def("fa_dot", &fa_dot, "rowsum(dO*O) per attention row");
  m.def("fa_dot_flags", &fa_dot_flags,
        "fa_dot plus dead [B, H, L/32] bool: query tiles whose dO is all +-0");
  m.def("fa_dot_packed_flags", &fa_dot_packed_flags,
        "fa_dot_flags on the packed [B, L, H*64] layout",
        py::arg("dout"), py::arg("o"), py::arg("H"));
  m.def("flash_dq", &flash_dq, "dQ = dS @ K (MFMA, tr_b16 K^T fragments)");
  m.def("bias_grad", &bias_grad, "bf16 column-sum for linear bias grads");
  m.def("p_from_lse", &p_from_lse, "probabilities from saved logsumexp");
  m.def("qkv_repack", &qkv_repack, "qkv layout repack (fwd/bwd)");
  m.def("qkv_repack_bwd3", &qkv_repack_bwd3, "qkv repack bwd from dq,dk,dv");
  m.def("out_repack", &out_repack, "attention output merge");
  m.def("out_repack_bwd", &out_repack_bwd, "attention output merge bwd");
  m.def("layernorm_fwd", &layernorm_fwd, "fused LayerNorm fwd (bf16, gfx950)");
  m.def("layernorm_bwd", &layernorm_bwd, "fused LayerNorm bwd",
        py::arg("dy"), py::arg("x"), py::arg("gamma"), py::arg("mean"),
        py::arg("rstd"), py::arg("ds_extra"), py::arg("want_dres") = false,
        py::arg("out_bf16") = false);
  m.def("layernorm_drop_fwd", &layernorm_drop_fwd,
        "fused residual dropout + add + LayerNorm fwd",
        py::arg("x"), py::arg("residual"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps"), py::arg("seed"), py::arg("call"), py::arg("site"),
        py::arg("thr"));
  m.def("layernorm_drop_bwd", &layernorm_drop_bwd,
        "fused residual dropout + add + LayerNorm bwd",
        py::arg("dy"), py::arg("x"), py::arg("gamma"), py::arg("mean"),
        py::arg("rstd"), py::arg("ds_extra"), py::arg("out_bf16"),
        py::arg("seed"), py::arg("call"), py::arg("site"), py::arg("thr"));
  m.def("bias_gelu_fwd", &bias_gelu_fwd, "fused bias+GeLU fwd");
  m.def("mx_quant_rows", &mx_quant_rows, "bf16 -> MXFP8 (q, s) along K");
  m.def("mx_bias_gelu", &mx_bias_gelu,
        "MXFP8 (q, s) of gelu_tanh(h + b), inference");
  m.def("mx_layernorm_fwd", &mx_layernorm_fwd,
        "(Add+)LayerNorm with MXFP8 output (q, s, sum), inference");
  m.def("lt_linear_gelu_bias", &lt_linear_gelu_bias,
        "hipBLASLt GEMM with fused GELU_BIAS epilogue (inference)");
  m.def("lt_bench_algos", &lt_bench_algos,
        "time the heuristic's top algos for a bf16 GEMM config");
  m.def("lt_probe_epilogue", &lt_probe_epilogue,
        "does this hipBLASLt have kernels for (m, n, k, epilogue)?");
  m.def("bias_gelu_bwd", &bias_gelu_bwd, "fused bias+GeLU bwd",
        py::arg("dy"), py::arg("x"), py::arg("b"),
        py::arg("out_bf16") = false);
  m.def("softmax_fwd", &softmax_fwd, "fused scaled masked softmax fwd");
  m.def("softmax_bwd", &softmax_bwd, "fused softmax bwd");
  // ema (None = off): the f32 weight average the EMA kernels keep
  m.def("adamw_step", &adamw_step, "fused AdamW over flat params",
        py::arg("p"), py::arg("grad"), py::arg("m"), py::arg("v"),
        py::arg("master"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("wd"), py::arg("step"), py::arg("grad_scale"),
        py::arg("ema") = py::none(), py::arg("ema_decay") = 0.0);
  m.def("grad_clip_state", &grad_clip_state,
        "deterministic global grad norm -> device {norm, scale, finite, "
        "sumsq}");
  m.def("cross_entropy_fwd", &cross_entropy_fwd,
        "row-wise softmax cross-entropy fwd over bf16 logits [N, V] -> "
        "({mean, 1 / n_valid}, loss_rows, lse)",
        py::arg("logits"), py::arg("target"), py::arg("ignore_index") = -100);
  m.def("cross_entropy_bwd", &cross_entropy_bwd,
        "cross-entropy bwd: (softmax - onehot) * grow[row], bf16, every "
        "element written",
        py::arg("logits"), py::arg("target"), py::arg("lse"),
        py::arg("grow"), py::arg("ignore_index") = -100);
  m.def("adamw_step_clipped", &adamw_step_clipped,
        "fused AdamW reading its grad scale / skip flag from clip_state",
        py::arg("p"), py::arg("grad"), py::arg("m"), py::arg("v"),
        py::arg("master"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("wd"), py::arg("step"), py::arg("clip_state"),
        py::arg("ema") = py::none(), py::arg("ema_decay") = 0.0);
  m.def("adamw_step_grouped", &adamw_step_grouped,
        "fused AdamW with per-segment lr multiplier and weight decay",
        py::arg("p"), py::arg("grad"), py::arg("m"), py::arg("v"),
        py::arg("master"), py::arg("seg_end"), py::arg("seg_lr_mult"),
        py::arg("seg_wd"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("step"), py::arg("grad_scale"),
        py::arg("ema") = py::none(), py::arg("ema_decay") = 0.0);
  m.def("adamw_step_grouped_clipped", &adamw_step_grouped_clipped,
        "adamw_step_grouped reading its grad scale / skip flag from "
        "clip_state",
        py::arg("p"), py::arg("grad"), py::arg("m"), py::arg("v"),
        py::arg("master"), py::arg("seg_end"), py::arg("seg_lr_mult"),
        py::arg("seg_wd"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("step"), py::arg("clip_state"),
        py::arg("ema") = py::none(), py::arg("ema_decay") = 0.0);
}
