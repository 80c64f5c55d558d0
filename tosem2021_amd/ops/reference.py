"""Plain-PyTorch fp32 reference implementations of the fused gfx950 ops.

These are the numerical ground truth for the HIP kernels (tests compare the
kernel output on GPU against these run in fp32) and the CPU execution path of
the model, so the full framework runs — slowly — on a GPU-less box.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch


def layernorm_fwd(
    x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (y in x.dtype, mean f32, rstd f32); stats over the last dim."""
    xf = x.float()
    mean = xf.mean(dim=-1)
    var = xf.var(dim=-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    xhat = (xf - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    y = xhat * gamma.float() + beta.float()
    return y.to(x.dtype), mean.reshape(-1), rstd.reshape(-1)


def add_layernorm_fwd(x, residual, gamma, beta, eps):
    """s = x + residual (rounded to x.dtype); y = LN(s). Returns (y, s, mean, rstd)."""
    s = (x.float() + residual.float()).to(x.dtype)
    y, mean, rstd = layernorm_fwd(s, gamma, beta, eps)
    return y, s, mean, rstd


def layernorm_bwd(
    dy: torch.Tensor,
    x: torch.Tensor,
    gamma: torch.Tensor,
    mean: torch.Tensor,
    rstd: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    D = x.shape[-1]
    xf = x.float().reshape(-1, D)
    dyf = dy.float().reshape(-1, D)
    mean = mean.reshape(-1, 1)
    rstd = rstd.reshape(-1, 1)
    xhat = (xf - mean) * rstd
    dyg = dyf * gamma.float()
    c1 = dyg.mean(dim=-1, keepdim=True)
    c2 = (dyg * xhat).mean(dim=-1, keepdim=True)
    dx = rstd * (dyg - c1 - xhat * c2)
    dgamma = (dyf * xhat).sum(dim=0)
    dbeta = dyf.sum(dim=0)
    return dx.reshape(x.shape).to(x.dtype), dgamma, dbeta


def folded_bias_grad(g: torch.Tensor) -> torch.Tensor:
    """Bias gradient of a projection whose output gradient is g: the f32 sum
    of g over every dim but the last — what addmm's backward computes with
    sum(0), and what the HIP kernels that produce g emit alongside it."""
    return g.float().reshape(-1, g.shape[-1]).sum(dim=0)


_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 with the Random123 constants (csrc/philox.h holds the
    same rounds for the kernels).  counter: four uint32 words, each a scalar
    or an array (broadcast together); key: two uint32 scalars.  Returns
    uint32 [..., 4].  uint64 NumPy arithmetic: a 32 x 32 product needs 64
    bits, which torch's int64 would overflow."""
    c0, c1, c2, c3 = np.broadcast_arrays(
        *(np.asarray(w, dtype=np.uint64) for w in counter))
    k0, k1 = (int(k) & _M32 for k in key)
    m32 = np.uint64(_M32)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c0
        p1 = np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0),
                          p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1),
                          p0 & m32)
        k0 = (k0 + _PHILOX_W0) & _M32
        k1 = (k1 + _PHILOX_W1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def dropout_threshold(p: float) -> Tuple[int, float]:
    """(thr, scale) of dropout probability p, 0 < p < 1: an element is
    dropped iff its 16 random bits are below thr = round(p * 65536), clamped
    to [1, 65535]; scale = 65536 / (65536 - thr) is the inverse of the
    effective keep rate, so the expectation is exact."""
    if not 0.0 < p < 1.0:
        raise ValueError(f"dropout probability must be in (0, 1), got {p}")
    thr = min(max(int(math.floor(p * 65536 + 0.5)), 1), 65535)
    return thr, 65536 / (65536 - thr)


def dropout_keep(N: int, D: int, p: float, seed: int, call: int,
                 site: int) -> torch.Tensor:
    """Keep mask (bool [N, D], D % 8 == 0) of the fused residual dropout: a
    pure function of (seed, call, site, element index).  One Philox call
    covers the 8-element packet pkt = (row * D + col) / 8: counter =
    (pkt lo, pkt hi, site, call), key = (seed lo, seed hi); output word w
    gives element 2w from its low and element 2w+1 from its high 16 bits."""
    if D % 8:
        raise ValueError(f"D must be a multiple of 8, got {D}")
    thr, _ = dropout_threshold(p)
    pkt = np.arange(N * D // 8, dtype=np.uint64)
    words = philox4x32_10(
        (pkt & np.uint64(_M32), pkt >> np.uint64(32), site & _M32,
         call & _M32),
        (seed & _M32, (seed >> 32) & _M32))                     # [P, 4]
    bits = np.stack([words & np.uint32(0xFFFF), words >> np.uint32(16)],
                    axis=-1)                                    # [P, 4, 2]
    return torch.from_numpy((bits >= thr).reshape(N, D))


ATTN_DROPOUT_SITE0 = 0x10000   # site of layer 0: above every residual site


def attn_dropout_threshold(p: float) -> Tuple[int, float]:
    """(thr, scale) of attention dropout probability p, 0 < p < 1: a
    probability is dropped iff its random BYTE is below thr = round(p * 256),
    clamped to [1, 255]; scale = 256 / (256 - thr) is the inverse of the
    effective keep rate.  The rate moves in steps of 1/256: p = 0.1 drops
    26/256 = 0.1016."""
    if not 0.0 < p < 1.0:
        raise ValueError(f"dropout probability must be in (0, 1), got {p}")
    thr = min(max(int(math.floor(p * 256 + 0.5)), 1), 255)
    return thr, 256 / (256 - thr)


def attn_dropout_keep(B: int, H: int, L: int, p: float, seed: int, call: int,
                      layer: int) -> torch.Tensor:
    """Keep mask (bool [B, H, L, L], query by key) of the dropout on the
    attention probabilities: a pure function of (seed, call, layer, b, h, q,
    k).  One Philox call covers one 4 x 4 block, nb = ceil(L / 4) blocks a
    side: counter = (blk lo, blk hi, 0x10000 + layer, call) with blk =
    ((b * H + h) * nb + q // 4) * nb + k // 4, key = (seed lo, seed hi);
    output word q & 3 holds row q of the block, its byte k & 3 (byte 0 the
    lowest) element (q, k).  csrc/philox.h holds the same definition for the
    flash kernels."""
    thr, _ = attn_dropout_threshold(p)
    nb = (L + 3) // 4
    blk = np.arange(B * H * nb * nb, dtype=np.uint64)
    words = philox4x32_10(
        (blk & np.uint64(_M32), blk >> np.uint64(32),
         (ATTN_DROPOUT_SITE0 + layer) & _M32, call & _M32),
        (seed & _M32, (seed >> 32) & _M32))                     # [P, 4]
    shifts = np.arange(4, dtype=np.uint32) * np.uint32(8)
    byte = (words[:, :, None] >> shifts) & np.uint32(0xFF)      # [P, q&3, k&3]
    keep = (byte >= thr).reshape(B, H, nb, nb, 4, 4)
    keep = keep.transpose(0, 1, 2, 4, 3, 5).reshape(B, H, 4 * nb, 4 * nb)
    return torch.from_numpy(np.ascontiguousarray(keep[:, :, :L, :L]))


def bias_gelu_fwd(x: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    pre = x.float() + b.float()
    return torch.nn.functional.gelu(pre, approximate="tanh").to(x.dtype)


def bias_gelu_bwd(
    dy: torch.Tensor, x: torch.Tensor, b: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    pre = (x.float() + b.float()).requires_grad_(True)
    with torch.enable_grad():
        y = torch.nn.functional.gelu(pre, approximate="tanh")
    (dpre,) = torch.autograd.grad(y, pre, dy.float())
    dbias = dpre.reshape(-1, x.shape[-1]).sum(dim=0)
    return dpre.to(x.dtype), dbias


def softmax_fwd(
    scores: torch.Tensor, mask: Optional[torch.Tensor], scale: float
) -> torch.Tensor:
    s = scores.float() * scale
    if mask is not None:
        # mask: [B, Lk] additive bias broadcast over heads and query positions
        s = s + mask.float().view(mask.shape[0], 1, 1, mask.shape[-1])
    return torch.softmax(s, dim=-1).to(scores.dtype)


def softmax_bwd(dp: torch.Tensor, p: torch.Tensor, scale: float) -> torch.Tensor:
    dpf = dp.float()
    pf = p.float()
    dot = (dpf * pf).sum(dim=-1, keepdim=True)
    return (scale * pf * (dpf - dot)).to(p.dtype)


def segment_bias(seg: torch.Tensor) -> torch.Tensor:
    """Additive attention bias of a packed batch: seg [B, L] integer segment
    ids -> [B, 1, L, L] f32, 0 where query and key share a segment and -1e9
    (the padding mask's convention) where they do not."""
    same = seg.unsqueeze(-1) == seg.unsqueeze(-2)
    zero = torch.zeros((), dtype=torch.float32, device=seg.device)
    return torch.where(same, zero, zero - 1e9).unsqueeze(1)


def flash_attention_fwd(q, k, v, mask, scale, bias=None, keep_scale=None):
    """fp32 reference of the flash forward: returns (o in q.dtype, lse f32).

    mask: optional [B, L] additive key bias; bias: optional additive bias
    broadcastable to [B, H, L, L] (segment_bias of a packed batch);
    keep_scale: optional f32 [B, H, L, L], attn_dropout_keep times the
    dropout scale — it multiplies the probabilities, lse stays that of the
    undropped softmax."""
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if mask is not None:
        s = s + mask.float().view(mask.shape[0], 1, 1, -1)
    if bias is not None:
        s = s + bias
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    if keep_scale is not None:
        p = p * keep_scale
    o = torch.matmul(p, v.float())
    return o.to(q.dtype), lse


def p_from_lse(scores, mask, lse, scale, bias=None):
    s = scores.float() * scale
    if mask is not None:
        s = s + mask.float().view(mask.shape[0], 1, 1, -1)
    if bias is not None:
        s = s + bias
    return torch.exp(s - lse.unsqueeze(-1)).to(scores.dtype)


def segment_pool_fwd(x, seg_start, seg_len, pos2seg):
    """Per-segment mean over the flattened positions of a packed batch.

    x [T, D]; seg_start/seg_len [N]; pos2seg [T] (segment of each position,
    -1 for padding).  Returns pooled [N, D] in x.dtype (f32 accumulation)."""
    n = seg_len.shape[0]
    valid = pos2seg >= 0
    acc = torch.zeros(n, x.shape[-1], dtype=torch.float32, device=x.device)
    acc.index_add_(0, pos2seg[valid].long(), x[valid].float())
    return (acc / seg_len.clamp(min=1).float().unsqueeze(-1)).to(x.dtype)


def segment_pool_bwd(dpooled, seg_len, pos2seg):
    """dx[t] = dpooled[pos2seg[t]] / seg_len; exact zeros at padding."""
    valid = pos2seg >= 0
    idx = pos2seg.clamp(min=0).long()
    g = dpooled.float() / seg_len.clamp(min=1).float().unsqueeze(-1)
    dx = g[idx] * valid.unsqueeze(-1).float()
    return dx.to(dpooled.dtype)


def adamw_step(
    p: torch.Tensor,
    grad: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    master: torch.Tensor,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    wd: float,
    step: int,
    grad_scale: float = 1.0,
    *,
    ema: Optional[torch.Tensor] = None,
    ema_decay: Optional[float] = None,
) -> None:
    _adamw_update(p, grad, m, v, master, lr, beta1, beta2, eps, wd, step,
                  grad_scale)
    _ema_update(ema, ema_decay, master)


def ema_decay_at(decay: float, t: int) -> float:
    """The weight average's decay at applied update t >= 1:
    min(decay, (1 + t) / (10 + t)).  The warm-up keeps the random initial
    heads out of a short run's average; decay 0 stays 0."""
    return min(decay, (1 + t) / (10 + t))


def _ema_update(ema, ema_decay, master) -> None:
    """ema = d * ema + (1 - d) * master as the kernel rounds it
    (csrc/adamw.hip): d and 1 - d are f32, and the two products and the sum
    are three separate f32 operations, never a fused multiply-add."""
    if ema is None:
        return
    d = torch.tensor(ema_decay, dtype=torch.float32, device=ema.device)
    omd = torch.ones((), dtype=torch.float32, device=ema.device) - d
    a = ema * d
    b = master * omd
    ema.copy_(a + b)


def _adamw_update(p, grad, m, v, master, lr, beta1, beta2, eps, wd, step,
                  grad_scale):
    """The AdamW arithmetic; lr and wd are floats or per-element f32 tensors."""
    g = grad.float() * grad_scale
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1.0 / (1.0 - beta1**step)
    bc2 = 1.0 / (1.0 - beta2**step)
    mhat = m * bc1
    vhat = v * bc2
    master.add_(-(lr * (mhat / (vhat.sqrt() + eps) + wd * master)))
    p.copy_(master.to(p.dtype))


def adamw_step_grouped(p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd,
                       lr, beta1, beta2, eps, step, grad_scale=1.0, *,
                       ema=None, ema_decay=None) -> None:
    """adamw_step with parameter groups over the flat buffer
    (csrc/adamw.hip): seg_end int64 [S] holds strictly increasing exclusive
    end offsets with seg_end[-1] == n, and the elements of segment s step at
    lr * seg_lr_mult[s], an f32 product as in the kernel, with weight decay
    seg_wd[s]."""
    f32 = torch.float32
    lens = torch.diff(seg_end, prepend=seg_end.new_zeros(1))
    lr_s = torch.tensor(lr, dtype=f32, device=master.device) \
        * seg_lr_mult.to(f32)
    lr_e = torch.repeat_interleave(lr_s, lens)
    wd_e = torch.repeat_interleave(seg_wd.to(f32), lens)
    _adamw_update(p, grad, m, v, master, lr_e, beta1, beta2, eps, wd_e, step,
                  grad_scale)
    _ema_update(ema, ema_decay, master)


def grad_clip_state(grad: torch.Tensor, grad_scale: float,
                    max_norm: float) -> torch.Tensor:
    """f32[4] = {norm, scale, finite, sumsq} of csrc/grad_norm.hip: the sum
    of squares accumulates in float64, the state is formed and stored in
    f32.  norm = grad_scale * sqrt(sumsq) is the norm of the gradient the
    optimizer sees; scale = grad_scale * min(1, max_norm / (norm + 1e-6))
    is clip_grad_norm_'s factor folded into the grad scale; finite is 0 when
    sumsq is inf or NaN in f32."""
    f32 = torch.float32
    sumsq64 = grad.detach().double().pow(2).sum().cpu()
    sumsq = sumsq64.to(f32)
    gs = torch.tensor(grad_scale, dtype=f32)
    norm = (gs.double() * sumsq64.sqrt()).to(f32)
    ratio = torch.tensor(max_norm, dtype=f32) / (norm + 1e-6)
    one = torch.ones((), dtype=f32)
    coef = torch.where(ratio < 1, ratio, one)   # a NaN ratio leaves coef at 1
    finite = torch.isfinite(sumsq).to(f32)
    return torch.stack([norm, gs * coef, finite, sumsq]).to(grad.device)


def adamw_step_clipped(p, grad, m, v, master, lr, beta1, beta2, eps, wd,
                       step, clip_state, *, ema=None, ema_decay=None) -> None:
    """adamw_step at the clipped grad scale; a non-finite gradient
    (clip_state[2] == 0) leaves every buffer untouched, ema included."""
    if float(clip_state[2]) == 0.0:
        return
    adamw_step(p, grad, m, v, master, lr, beta1, beta2, eps, wd, step,
               grad_scale=float(clip_state[1]), ema=ema, ema_decay=ema_decay)


def adamw_step_grouped_clipped(p, grad, m, v, master, seg_end, seg_lr_mult,
                               seg_wd, lr, beta1, beta2, eps, step,
                               clip_state, *, ema=None,
                               ema_decay=None) -> None:
    """adamw_step_grouped at the clipped grad scale; a non-finite gradient
    (clip_state[2] == 0) leaves every buffer untouched, ema included."""
    if float(clip_state[2]) == 0.0:
        return
    adamw_step_grouped(p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd,
                       lr, beta1, beta2, eps, step,
                       grad_scale=float(clip_state[1]), ema=ema,
                       ema_decay=ema_decay)


def dead_q_tiles(dout: torch.Tensor, n_heads: Optional[int] = None
                 ) -> torch.Tensor:
    """bool [B, H, L // 32]: True where a 32-row query tile of one head has an
    output gradient that is all +-0, the flags fa_dot writes next to ddot
    (csrc/flash_attn.hip).  A tile is live iff any of its 32 x 64 bf16
    elements has (bits & 0x7fff) != 0: -0.0 counts as zero, the smallest
    subnormal as live, NaN and inf as live.

    dout: bf16, [B, L, n_heads * 64] (packed) or [B, H, L, 64] (n_heads may
    then be omitted); L % 32 == 0."""
    if dout.dtype != torch.bfloat16:
        raise ValueError("dead_q_tiles expects bf16")
    if dout.dim() == 3:
        B, L, D = dout.shape
        if n_heads is None or D != n_heads * 64:
            raise ValueError("packed dout must be [B, L, n_heads * 64]")
        d4 = dout.view(B, L, n_heads, 64).permute(0, 2, 1, 3)
    elif dout.dim() == 4 and dout.shape[-1] == 64:
        d4 = dout
        B, _, L, _ = dout.shape
    else:
        raise ValueError("dout must be [B, L, H * 64] or [B, H, L, 64]")
    if L % 32:
        raise ValueError("L % 32 == 0 required")
    bits = d4.contiguous().view(torch.int16).to(torch.int32) & 0x7FFF
    live = (bits != 0).view(B, d4.shape[1], L // 32, 32 * 64).any(-1)
    return ~live


def _ce_valid(target: torch.Tensor, V: int, ignore_index: int) -> torch.Tensor:
    """bool [N]: rows that count.  A target that is neither ignore_index nor
    a column of the logits raises (the HIP kernels treat it as ignored so
    that it can never index memory; here it is reported)."""
    valid = target != ignore_index
    bad = valid & ((target < 0) | (target >= V))
    if bool(bad.any()):
        t = int(target[bad][0])
        raise IndexError(f"cross-entropy target {t} is out of range for "
                         f"{V} classes (ignore_index {ignore_index})")
    return valid


def cross_entropy_fwd(logits: torch.Tensor, target: torch.Tensor,
                      ignore_index: int = -100
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-wise softmax cross-entropy of csrc/cross_entropy.hip in f32, any
    dtype and any V: logits [N, V], target [N] int64 -> (loss_rows [N] f32 =
    lse - logits[target], 0 at ignored rows; lse [N] f32)."""
    x = logits.float()
    valid = _ce_valid(target, x.shape[1], ignore_index)
    lse = torch.logsumexp(x, dim=-1)
    xt = x.gather(1, target.clamp(min=0).unsqueeze(1)).squeeze(1)
    loss_rows = torch.where(valid, lse - xt, torch.zeros_like(lse))
    return loss_rows, lse


def cross_entropy_bwd(logits: torch.Tensor, target: torch.Tensor,
                      lse: torch.Tensor, grow: torch.Tensor,
                      ignore_index: int = -100) -> torch.Tensor:
    """dlogits [N, V] in logits.dtype = (exp(logits - lse) - onehot(target))
    * grow[row]; zeros at ignored rows.  grow [N] f32 is the per-row
    upstream gradient."""
    x = logits.float()
    valid = _ce_valid(target, x.shape[1], ignore_index)
    p = torch.exp(x - lse.unsqueeze(1))
    p.scatter_add_(1, target.clamp(min=0).unsqueeze(1),
                   -torch.ones_like(lse).unsqueeze(1))
    d = p * grow.unsqueeze(1)
    return torch.where(valid.unsqueeze(1), d, torch.zeros_like(d)).to(
        logits.dtype)


MX_BLOCK = 32       # elements of K that share one e8m0 scale


def mx_quantize(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """OCP MXFP8 along the last dim: x [..., K] (finite, K % 32 == 0) ->
    (q uint8 [..., K] holding e4m3fn bytes, s uint8 [..., K / 32] holding
    e8m0 bytes).  Per block of 32 consecutive elements, with E the biased f32
    exponent field of the largest magnitude: s = clamp(E - 8, 0, 254), meaning
    the scale 2^(s - 127), and q = e4m3fn(clamp(x * 2^(127 - s), -448, 448)),
    round to nearest even, subnormals kept.  The clamp comes before the
    conversion: a scaled magnitude reaches (448, 512) whenever the block
    maximum's mantissa is above 1.75, and the conversion alone would make it
    NaN.  This is the definition the HIP kernels (csrc/mx.h) match bit for
    bit."""
    K = x.shape[-1]
    if K == 0 or K % MX_BLOCK:
        raise ValueError(f"MXFP8 needs K % {MX_BLOCK} == 0, got K = {K}")
    xb = x.float().reshape(*x.shape[:-1], K // MX_BLOCK, MX_BLOCK)
    amax = xb.abs().amax(dim=-1)
    E = (amax.view(torch.int32) >> 23) & 0xFF
    s = (E - 8).clamp(0, 254)
    # 2^(127 - s) has the exponent field 254 - s >= 1: a normal f32
    mul = ((254 - s) << 23).view(torch.float32)
    q = (xb * mul.unsqueeze(-1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(x.shape), s.to(torch.uint8)


def mx_dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """f32 [..., K] = e4m3fn(q) * 2^(s - 127) per block of 32; exact."""
    K = q.shape[-1]
    qf = q.view(torch.float8_e4m3fn).float()
    sf = s.view(torch.float8_e8m0fnu).float()
    return (qf.reshape(*q.shape[:-1], K // MX_BLOCK, MX_BLOCK)
            * sf.unsqueeze(-1)).reshape(q.shape)
