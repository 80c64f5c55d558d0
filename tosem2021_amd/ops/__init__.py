"""Fused gfx950 ops: autograd wrappers dispatching to the in-tree HIP
extension on GPU and to the fp32 torch references on CPU.

Policy: on a GPU box the HIP extension is REQUIRED — a missing extension
raises instead of silently falling back to eager PyTorch, so a GPU test can
never pass on a non-native path.
"""
from __future__ import annotations

import os
import warnings
from typing import Optional

import torch

from . import reference

# A/B knob (TOSEM_FLASH_QSKIP=0 disables; default on): the flash backward
# leaves out 32-row query tiles whose output gradient is all +-0 — the
# padded rows of a batch.  Bitwise exact for finite inputs, see
# docs/KERNELS.md "Dead query tiles".  Read per call, so a test can flip it.
_FLASH_QSKIP = os.environ.get("TOSEM_FLASH_QSKIP", "1") != "0"

_EXT = None
_EXT_ERR: Optional[str] = None


def hip_ops():
    """Return the compiled HIP extension module; raise loudly if missing."""
    global _EXT, _EXT_ERR
    if _EXT is None:
        try:
            from tosem2021_amd import _hip_ops  # type: ignore

            _EXT = _hip_ops
        except ImportError as e:  # pragma: no cover
            _EXT_ERR = str(e)
            raise RuntimeError(
                "tosem2021_amd._hip_ops is not built. On a GPU box this is a "
                "hard error (no eager fallback). Build it in-tree with: "
                "PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace "
                f"(import error: {e})"
            ) from e
    return _EXT


def hip_available() -> bool:
    try:
        hip_ops()
        return True
    except RuntimeError:
        return False


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        if x.is_cuda:
            y, _, mean, rstd = hip_ops().layernorm_fwd(x, None, gamma, beta, eps)
        else:
            y, mean, rstd = reference.layernorm_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        if x.is_cuda:
            # the final colsum stage writes bf16: no convert launches
            dx, dgamma, dbeta = hip_ops().layernorm_bwd(
                dy, x, gamma, mean, rstd, None, False, True)
            return dx, dgamma, dbeta, None
        dx, dgamma, dbeta = reference.layernorm_bwd(dy, x, gamma, mean, rstd)
        return dx, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None


def fused_layernorm(x, gamma, beta, eps: float = 1e-5):
    return _LayerNormFn.apply(x.contiguous(), gamma, beta, eps)


class _AddLayerNormFn(torch.autograd.Function):
    """(y, s) = (LN(x + residual), x + residual) — the residual-stream add is
    fused into the LN kernel's first read (one kernel, no separate add).

    residual_bias (optional) is the bias of the projection that produced
    `residual`, called with that bias detached.  It takes no part in the
    forward; its gradient is the column sum of the dx this backward returns
    for `residual`, which the LN backward kernel emits next to dgamma/dbeta,
    so the projection's backward need not re-read dx to reduce it."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, residual_bias=None):
        ctx.rb_dtype = None if residual_bias is None else residual_bias.dtype
        if x.is_cuda:
            y, s, mean, rstd = hip_ops().layernorm_fwd(x, residual, gamma,
                                                       beta, eps)
        else:
            y, s, mean, rstd = reference.add_layernorm_fwd(x, residual, gamma,
                                                           beta, eps)
        ctx.save_for_backward(s, gamma, mean, rstd)
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, gamma, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        want_dres = ctx.rb_dtype is not None and ctx.needs_input_grad[5]
        dres = None
        if s.is_cuda:
            # the downstream residual grad ds is added INSIDE the kernel
            de = ds.contiguous() if ds is not None else None
            out = hip_ops().layernorm_bwd(dy, s, gamma, mean, rstd, de,
                                          want_dres, True)
            dx, dgamma, dbeta = out[:3]
            if want_dres:
                dres = out[3].to(ctx.rb_dtype)  # no-op for a bf16 bias
            return dx, dx, dgamma, dbeta, None, dres
        dx, dgamma, dbeta = reference.layernorm_bwd(dy, s, gamma, mean, rstd)
        if ds is not None:
            dx = dx + ds
        if want_dres:
            dres = reference.folded_bias_grad(dx).to(ctx.rb_dtype)
        return (dx, dx, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None,
                dres)


def fused_add_layernorm(x, residual, gamma, beta, eps: float = 1e-5,
                        residual_bias=None):
    """Returns (y, s): y = LN(x+residual), s = the new residual stream.

    residual_bias: see _AddLayerNormFn — the detached-in-forward bias of the
    projection behind `residual`, which receives its gradient from here."""
    return _AddLayerNormFn.apply(x.contiguous(), residual.contiguous(),
                                 gamma, beta, eps, residual_bias)


class _DropoutAddLayerNormFn(torch.autograd.Function):
    """(y, s) = (LN(s), x + dropout(residual)) with the dropout fused into
    the LN kernel's read of `residual` and, in backward, into its write of
    the residual's gradient.  The keep mask is a pure function of (seed,
    call, site, element index) — reference.dropout_keep, csrc/philox.h — so
    no mask tensor exists at any point: backward regenerates it from the
    Python ints kept on ctx."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, p, seed, call, site):
        thr, scale = reference.dropout_threshold(p)
        # the words the Philox key and counter hold
        seed, call, site = (seed & 0xFFFFFFFFFFFFFFFF, call & 0xFFFFFFFF,
                            site & 0xFFFFFFFF)
        ctx.drop = (p, seed, call, site, thr, scale)
        if x.is_cuda:
            y, s, mean, rstd = hip_ops().layernorm_drop_fwd(
                x, residual, gamma, beta, eps, seed, call, site, thr)
        else:
            keep = reference.dropout_keep(x.numel() // x.shape[-1],
                                          x.shape[-1], p, seed, call, site)
            y, s, mean, rstd = reference.add_layernorm_fwd(
                x, residual * keep.view(x.shape) * scale, gamma, beta, eps)
        ctx.save_for_backward(s, gamma, mean, rstd)
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, gamma, mean, rstd = ctx.saved_tensors
        p, seed, call, site, thr, scale = ctx.drop
        dy = dy.contiguous()
        if s.is_cuda:
            de = ds.contiguous() if ds is not None else None
            dx, dres, dgamma, dbeta = hip_ops().layernorm_drop_bwd(
                dy, s, gamma, mean, rstd, de, True, seed, call, site, thr)
            return dx, dres, dgamma, dbeta, None, None, None, None, None
        dx, dgamma, dbeta = reference.layernorm_bwd(dy, s, gamma, mean, rstd)
        if ds is not None:
            dx = dx + ds
        keep = reference.dropout_keep(s.numel() // s.shape[-1], s.shape[-1],
                                      p, seed, call, site)
        dres = dx * keep.view(s.shape) * scale
        return (dx, dres, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype),
                None, None, None, None, None)


def fused_dropout_add_layernorm(x, residual, gamma, beta, eps: float,
                                p: float, seed: int, call: int, site: int):
    """Returns (y, s): s = x + (keep ? residual * scale : 0) rounded to
    x.dtype, y = LN(s).  keep and scale: reference.dropout_keep and
    reference.dropout_threshold for probability p in (0, 1); p == 0 callers
    use fused_add_layernorm.  (seed, call, site) select the mask: the same
    ints give the same mask on the CPU and on the GPU, in forward and in
    backward."""
    reference.dropout_threshold(p)      # rejects p outside (0, 1)
    return _DropoutAddLayerNormFn.apply(x.contiguous(), residual.contiguous(),
                                        gamma, beta, eps, p, seed, call, site)


class _BiasGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b):
        ctx.save_for_backward(x, b)
        if x.is_cuda:
            return hip_ops().bias_gelu_fwd(x, b)
        return reference.bias_gelu_fwd(x, b)

    @staticmethod
    def backward(ctx, dy):
        x, b = ctx.saved_tensors
        dy = dy.contiguous()
        if x.is_cuda:
            # the final colsum stage writes bf16: no convert launch
            return tuple(hip_ops().bias_gelu_bwd(dy, x, b, True))
        dx, dbias = reference.bias_gelu_bwd(dy, x, b)
        return dx, dbias.to(b.dtype)


def fused_bias_gelu(x, b):
    """y = gelu_tanh(x + b), bf16, bias grad fused."""
    return _BiasGeluFn.apply(x.contiguous(), b)


class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, mask, scale):
        if scores.is_cuda:
            p = hip_ops().softmax_fwd(scores, mask, scale)
        else:
            p = reference.softmax_fwd(scores, mask, scale)
        ctx.save_for_backward(p)
        ctx.scale = scale
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        dp = dp.contiguous()
        if p.is_cuda:
            ds = hip_ops().softmax_bwd(dp, p, ctx.scale)
        else:
            ds = reference.softmax_bwd(dp, p, ctx.scale)
        return ds, None, None


def fused_softmax(scores, mask=None, scale: float = 1.0):
    """P = softmax(scale * scores + mask_bias) over the last dim.

    scores: [B, H, Lq, Lk] bf16; mask: optional [B, Lk] f32 additive bias.
    """
    return _SoftmaxFn.apply(scores.contiguous(), mask, scale)


class _QkvRepackFn(torch.autograd.Function):
    """[B, L, 3*H*dh] -> three contiguous [B, H, L, dh] (bmm-ready q/k/v).

    Backward gathers (dq, dk, dv) straight back to the Linear's layout in one
    kernel — no stack/cat materialization."""

    @staticmethod
    def forward(ctx, qkv, n_heads):
        ctx.n_heads = n_heads
        if qkv.is_cuda:
            stacked = hip_ops().qkv_repack(qkv, n_heads, False)
        else:
            B, L, _ = qkv.shape
            dh = qkv.shape[-1] // (3 * n_heads)
            stacked = (qkv.view(B, L, 3, n_heads, dh).permute(2, 0, 3, 1, 4)
                       .contiguous())
        q, k, v = stacked.unbind(0)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        dq = dq.contiguous(); dk = dk.contiguous(); dv = dv.contiguous()
        if dq.is_cuda:
            return hip_ops().qkv_repack_bwd3(dq, dk, dv), None
        B, H, L, dh = dq.shape
        g = torch.stack([dq, dk, dv], dim=0)
        return g.permute(1, 3, 0, 2, 4).reshape(B, L, 3 * H * dh), None


def qkv_repack(qkv, n_heads: int):
    return _QkvRepackFn.apply(qkv.contiguous(), n_heads)


class _OutRepackFn(torch.autograd.Function):
    """[B, H, L, dh] -> [B, L, H*dh] (attention output merge)."""

    @staticmethod
    def forward(ctx, x):
        ctx.n_heads = x.shape[1]
        if x.is_cuda:
            return hip_ops().out_repack(x, False)
        B, H, L, dh = x.shape
        return x.permute(0, 2, 1, 3).reshape(B, L, H * dh)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if g.is_cuda:
            return hip_ops().out_repack_bwd(g, ctx.n_heads)
        B, L, D = g.shape
        H = ctx.n_heads
        return g.view(B, L, H, D // H).permute(0, 2, 1, 3).contiguous()


def out_repack(x):
    return _OutRepackFn.apply(x.contiguous())


class _LinearFn(torch.autograd.Function):
    """F.linear with the bias gradient computed by the two-stage bf16
    column-sum kernel (csrc/colsum.hip colsum_bf16).  MEASURED NOTE: not
    used by the model — routing the projections through this Function cost
    13.7 ms/step because the explicit dgrad/wgrad matmuls here dispatch to
    slower hipBLASLt algos than torch's addmm backward (which reaches the
    tuned split-K Custom_*SK3 kernels); the ~38 us/call bias-grad saving
    cannot pay for that.  Kept as a standalone op (serving/other shapes)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.matmul(dy, w)
        dw = torch.matmul(dy.transpose(0, 1), x)
        db = hip_ops().bias_grad(dy) if dy.is_cuda else dy.sum(0)
        return dx, dw, db


def fused_linear(x, w, b):
    """x @ w^T + b with the custom bias-grad path (CUDA bf16 only)."""
    lead = x.shape[:-1]
    y = _LinearFn.apply(x.reshape(-1, x.shape[-1]).contiguous(), w, b)
    return y.view(*lead, -1)


class _LinearWgradFn(torch.autograd.Function):
    """Linear whose WEIGHT gradient runs through the custom split-K MFMA
    wgrad kernel (csrc/wgrad_gemm.hip) and the bias gradient through the
    colsum bias_grad kernel; forward is the same fused addmm GEMM, dgrad
    the same torch matmul dispatch."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        if b is None:
            return torch.matmul(x, w.t())
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.matmul(dy, w)
        dw = hip_ops().wgrad_gemm(dy, x, 0)
        db = hip_ops().bias_grad(dy) if ctx.has_bias else None
        return dx, dw, db


def wgrad_linear_supported(out_features: int, in_features: int,
                           tokens: int) -> bool:
    return out_features % 256 == 0 and in_features % 256 == 0 and \
        tokens % 32 == 0


def wgrad_linear(x, w, b=None):
    """Linear with the custom wgrad kernel (bf16 CUDA; 256-multiple
    features, token count % 32)."""
    lead = x.shape[:-1]
    y = _LinearWgradFn.apply(x.reshape(-1, x.shape[-1]).contiguous(), w, b)
    return y.view(*lead, -1)


def lt_linear_gelu_bias(x, w1, b1):
    """GELU(x @ w1^T + b1) in one hipBLASLt GEMM (GELU_BIAS epilogue) —
    inference only: this hipBLASLt has no aux epilogues (no pre-activation
    out), so training uses csrc/bias_gelu.hip instead."""
    return hip_ops().lt_linear_gelu_bias(x, w1, b1)


def _attn_dropout_words(dropout):
    """dropout = (p, seed, call, layer) of flash_attention -> None where
    today's call runs (None or p == 0), else (p, seed, call, layer, site,
    thr, scale) with the words the Philox key and counter hold."""
    if dropout is None:
        return None
    p, seed, call, layer = dropout
    if not 0.0 <= p < 1.0:
        raise ValueError(f"attention dropout probability must be in [0, 1), "
                         f"got {p}")
    if p == 0:
        return None
    thr, scale = reference.attn_dropout_threshold(p)
    site = (reference.ATTN_DROPOUT_SITE0 + layer) & 0xFFFFFFFF
    return (p, seed & 0xFFFFFFFFFFFFFFFF, call & 0xFFFFFFFF, layer, site,
            thr, scale)


def _hip_drop(drop):
    """The bindings' (drop_seed, drop_call, drop_site, drop_thr)."""
    if drop is None:
        return ()
    _, seed, call, _, site, thr, _ = drop
    return seed, call, site, thr


def _cpu_keep_scale(drop, B, H, L, like):
    """reference.attn_dropout_keep times the scale, in like's dtype: the
    CPU paths draw the GPU's mask."""
    if drop is None:
        return None
    p, seed, call, layer, _, _, scale = drop
    keep = reference.attn_dropout_keep(B, H, L, p, seed, call, layer)
    return keep.to(like.dtype) * scale


class _FlashAttentionFn(torch.autograd.Function):
    """Flash attention: MFMA forward (csrc/flash_attn.hip, O(L) memory, saves
    logsumexp); backward = two recompute kernels, O(L) memory end to end:
    flash_bwd_fused (register-accumulated dK/dV) + flash_dq_recompute
    (in-register S/dP/dS, accumulates dQ) — no [L, L] dS materialization."""

    @staticmethod
    def forward(ctx, q, k, v, mask, scale, seg=None, drop=None):
        if q.is_cuda:
            o, lse = hip_ops().flash_fwd(q, k, v, mask, scale, seg,
                                         *_hip_drop(drop))
        else:
            bias = reference.segment_bias(seg) if seg is not None else None
            ks = _cpu_keep_scale(drop, *q.shape[:3], q)
            o, lse = reference.flash_attention_fwd(q, k, v, mask, scale, bias,
                                                   ks)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.mask = mask
        ctx.seg = seg
        ctx.scale = scale
        ctx.drop = drop
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        mask, seg, scale = ctx.mask, ctx.seg, ctx.scale
        do = do.contiguous()
        if q.is_cuda:
            # two recompute MFMA kernels; dS never touches HBM (round 2 —
            # the round-1 pipeline wrote + re-read a [B, H, L, L] bf16 dS)
            ddot, dead = hip_ops().fa_dot_flags(do, o)
            if not _FLASH_QSKIP:
                dead = None
            drop = _hip_drop(ctx.drop)
            dk, dv = hip_ops().flash_bwd_fused(q, k, v, do, mask, lse,
                                               ddot, scale, False, seg, dead,
                                               *drop)
            dq = hip_ops().flash_dq_recompute(q, k, v, do, mask, lse,
                                              ddot, scale, seg, dead, *drop)
            return dq, dk, dv, None, None, None, None
        bias = reference.segment_bias(seg) if seg is not None else None
        s = torch.matmul(q, k.transpose(-1, -2))
        p = reference.p_from_lse(s, mask, lse, scale, bias)
        dp = torch.matmul(do, v.transpose(-1, -2))
        pd = p
        ks = _cpu_keep_scale(ctx.drop, *q.shape[:3], q)
        if ks is not None:
            # O = (keep * scale * P) V: dP carries the mask, and
            # softmax_bwd's rowsum(dP * P) is then rowsum(dO * O)
            dp, pd = dp * ks, p * ks
        dsc = reference.softmax_bwd(dp, p, scale)
        dq = torch.matmul(dsc, k)
        dk = torch.matmul(dsc.transpose(-1, -2), q)
        dv = torch.matmul(pd.transpose(-1, -2), do)
        return dq, dk, dv, None, None, None, None


def _check_mask_seg(mask, seg):
    if mask is not None and seg is not None:
        raise ValueError("mask and seg are mutually exclusive: a packed "
                         "batch marks its padding as a trailing segment")


def check_segments(seg: torch.Tensor) -> None:
    """Host-side check of the segment contract: seg is an integer [B, L]
    tensor whose rows never decrease.  Raises ValueError otherwise.  Syncs
    when seg is on the GPU — meant for the packer and for tests."""
    if seg.dim() != 2 or seg.dtype not in (torch.int32, torch.int64):
        raise ValueError("seg must be an integer [B, L] tensor")
    if seg.shape[1] > 1:
        bad = (seg[:, 1:] < seg[:, :-1]).any(dim=1)
        if bool(bad.any()):
            rows = torch.nonzero(bad).flatten().tolist()
            raise ValueError(f"seg rows {rows} are not non-decreasing")


def flash_attention(q, k, v, mask=None, scale: float = 1.0, seg=None,
                    dropout=None):
    """q/k/v: [B, H, L, 64] bf16 contiguous, L % 32 == 0.

    mask: optional [B, L] f32 additive key bias; a bias <= -1e8 is treated
    as fully masked (its probability is exactly 0 and wholly masked tiles
    are skipped).  seg: optional [B, L] int32 segment ids of a packed batch,
    exclusive with mask: position i attends to j iff seg[b, i] == seg[b, j].
    Each seg row must be non-decreasing, with the padding tail carrying one
    id above every real id; that is the caller's contract (check_segments
    verifies it on the host), not checked on the device.

    dropout: see flash_attention_packed."""
    _check_mask_seg(mask, seg)
    drop = _attn_dropout_words(dropout)
    if drop is None:
        return _FlashAttentionFn.apply(q.contiguous(), k.contiguous(),
                                       v.contiguous(), mask, scale, seg)
    return _FlashAttentionFn.apply(q.contiguous(), k.contiguous(),
                                   v.contiguous(), mask, scale, seg, drop)


class _FlashAttentionPackedFn(torch.autograd.Function):
    """Flash attention straight on the packed QKV projection output
    [B, L, 3D] -> attention output [B, L, D] (round 2).  The strided-
    geometry kernels read q/k/v from and write every gradient back into
    the packed layouts, eliminating the qkv_repack / out_repack kernel
    quartet (fwd gather, bwd3 merge, out fwd/bwd) from the step.

    qkv_bias (optional) is the bias of the projection that produced qkv,
    called with that bias detached.  It takes no part in the forward; its
    gradient is the column sum of dqkv, which the backward kernels emit as
    per-workgroup partials while the tiles are in registers, so the
    projection's backward need not re-read dqkv to reduce it."""

    @staticmethod
    def forward(ctx, qkv, n_heads, mask, scale, seg=None, qkv_bias=None,
                drop=None):
        ctx.qb_dtype = None if qkv_bias is None else qkv_bias.dtype
        ctx.drop = drop
        if qkv.is_cuda:
            o, lse = hip_ops().flash_fwd_packed(qkv, n_heads, mask, scale,
                                                seg, *_hip_drop(drop))
        else:
            B, L, D3 = qkv.shape
            d = D3 // 3
            q, k, v = (t.view(B, L, n_heads, 64).transpose(1, 2).contiguous()
                       for t in qkv.split(d, dim=-1))
            bias = reference.segment_bias(seg) if seg is not None else None
            ks = _cpu_keep_scale(drop, B, n_heads, L, q)
            o4, lse = reference.flash_attention_fwd(q, k, v, mask, scale,
                                                    bias, ks)
            o = o4.transpose(1, 2).reshape(B, L, d)
        ctx.save_for_backward(qkv, o, lse)
        ctx.n_heads = n_heads
        ctx.mask = mask
        ctx.seg = seg
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        n_heads, mask, scale = ctx.n_heads, ctx.mask, ctx.scale
        seg = ctx.seg
        do = do.contiguous()
        want_bias = ctx.qb_dtype is not None and ctx.needs_input_grad[5]
        if qkv.is_cuda:
            if want_bias:
                dqkv, dbias = hip_ops().flash_bwd_packed_bias(
                    qkv, o, do, mask, lse, n_heads, scale, seg,
                    _FLASH_QSKIP)
                # no-op for a bf16 bias
                return (dqkv, None, None, None, None,
                        dbias.to(ctx.qb_dtype), None)
            dqkv = hip_ops().flash_bwd_packed(qkv, o, do, mask, lse,
                                              n_heads, scale, seg,
                                              _FLASH_QSKIP,
                                              *_hip_drop(ctx.drop))
            return dqkv, None, None, None, None, None, None
        bias = reference.segment_bias(seg) if seg is not None else None
        B, L, D3 = qkv.shape
        d = D3 // 3
        q, k, v = (t.view(B, L, n_heads, 64).transpose(1, 2).contiguous()
                   for t in qkv.split(d, dim=-1))
        do4 = do.view(B, L, n_heads, 64).transpose(1, 2).contiguous()
        s = torch.matmul(q, k.transpose(-1, -2))
        p = reference.p_from_lse(s, mask, lse, scale, bias)
        dp = torch.matmul(do4, v.transpose(-1, -2))
        pd = p
        ks = _cpu_keep_scale(ctx.drop, B, n_heads, L, q)
        if ks is not None:      # as in _FlashAttentionFn.backward
            dp, pd = dp * ks, p * ks
        dsc = reference.softmax_bwd(dp, p, scale)
        dq = torch.matmul(dsc, k)
        dk = torch.matmul(dsc.transpose(-1, -2), q)
        dv = torch.matmul(pd.transpose(-1, -2), do4)
        dqkv = torch.cat(
            [t.transpose(1, 2).reshape(B, L, d) for t in (dq, dk, dv)],
            dim=-1)
        dbias = None
        if want_bias:
            dbias = reference.folded_bias_grad(dqkv).to(ctx.qb_dtype)
        return dqkv, None, None, None, None, dbias, None


def flash_attention_packed(qkv, n_heads: int, mask=None, scale: float = 1.0,
                           seg=None, qkv_bias=None, dropout=None):
    """qkv: [B, L, 3*n_heads*64] bf16 (the fused projection output);
    returns [B, L, n_heads*64] ready for the output projection.
    qkv_bias: see _FlashAttentionPackedFn — the detached-in-forward bias of
    the qkv projection, which receives its gradient from here.

    mask: optional [B, L] f32 additive key bias; a bias <= -1e8 is treated
    as fully masked (its probability is exactly 0 and wholly masked tiles
    are skipped).  seg: optional [B, L] int32 segment ids of a packed batch,
    exclusive with mask: position i attends to j iff seg[b, i] == seg[b, j].
    Each seg row must be non-decreasing, with the padding tail carrying one
    id above every real id; that is the caller's contract (check_segments
    verifies it on the host), not checked on the device.

    dropout: optional (p, seed, call, layer), dropout on the attention
    probabilities inside the flash kernels: O = (keep * dscale * P) V with
    keep = reference.attn_dropout_keep(B, H, L, p, seed, call, layer) and
    (thr, dscale) = reference.attn_dropout_threshold(p) — the effective rate
    is thr / 256.  The same ints give the same mask in forward and backward,
    on the GPU and on the CPU; lse stays the undropped softmax's.  None or
    p == 0 is the call without it; p outside [0, 1) raises ValueError, and
    so does dropout together with qkv_bias."""
    _check_mask_seg(mask, seg)
    drop = _attn_dropout_words(dropout)
    if dropout is not None and qkv_bias is not None:
        raise ValueError("dropout and qkv_bias are mutually exclusive: the "
                         "dropout kernels do not emit the folded bias "
                         "gradient")
    if drop is None:
        return _FlashAttentionPackedFn.apply(qkv.contiguous(), n_heads, mask,
                                             scale, seg, qkv_bias)
    return _FlashAttentionPackedFn.apply(qkv.contiguous(), n_heads, mask,
                                         scale, seg, None, drop)


def flash_supported(head_dim: int, L: int) -> bool:
    return head_dim == 64 and L % 32 == 0


class _MaskedPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        if x.is_cuda:
            pooled, counts = hip_ops().masked_pool_fwd(x, mask)
        else:
            if mask is not None:
                w = mask.to(x.dtype).unsqueeze(-1)
                counts = mask.sum(-1).clamp(min=1).float()
                pooled = ((x.float() * w.float()).sum(1) /
                          counts.unsqueeze(-1)).to(x.dtype)
            else:
                counts = torch.full((x.shape[0],), x.shape[1],
                                    dtype=torch.float32)
                pooled = x.float().mean(1).to(x.dtype)
        ctx.save_for_backward(counts)
        ctx.mask = mask
        ctx.L = x.shape[1]
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        (counts,) = ctx.saved_tensors
        mask = ctx.mask
        dpooled = dpooled.contiguous()
        if dpooled.is_cuda:
            dx = hip_ops().masked_pool_bwd(dpooled, mask, counts, ctx.L)
        else:
            g = (dpooled.float() / counts.unsqueeze(-1)).unsqueeze(1)
            dx = g.expand(-1, ctx.L, -1)
            if mask is not None:
                dx = dx * mask.unsqueeze(-1).float()
            dx = dx.to(dpooled.dtype)
        return dx, None


def masked_mean_pool(x, mask=None):
    """pooled[b] = mean over valid rows of x[b]; x [B,L,D] bf16, mask [B,L]."""
    return _MaskedPoolFn.apply(x.contiguous(),
                               mask.contiguous() if mask is not None else None)


class _SegmentPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg_start, seg_len, pos2seg):
        if x.is_cuda:
            pooled = hip_ops().segment_pool_fwd(x, seg_start, seg_len)
        else:
            pooled = reference.segment_pool_fwd(x, seg_start, seg_len,
                                                pos2seg)
        ctx.save_for_backward(seg_len, pos2seg)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        seg_len, pos2seg = ctx.saved_tensors
        dpooled = dpooled.contiguous()
        if dpooled.is_cuda:
            dx = hip_ops().segment_pool_bwd(dpooled, pos2seg, seg_len,
                                            pos2seg.shape[0])
        else:
            dx = reference.segment_pool_bwd(dpooled, seg_len, pos2seg)
        return dx, None, None, None


def segment_mean_pool(x, seg_start, seg_len, pos2seg):
    """Per-example mean-pool of a packed batch.

    x: [T, D] — the [R, row_len, D] activations flattened over positions
    (bf16 on the GPU, D % 8 == 0); seg_start/seg_len: [N] int32 first
    position and length of every segment; pos2seg: [T] int32 segment of
    every position, -1 at padding.  Returns pooled [N, D]; the gradient is
    exactly zero at padding positions."""
    return _SegmentPoolFn.apply(x.contiguous(), seg_start, seg_len, pos2seg)


class _CrossEntropyFn(torch.autograd.Function):
    """Mean softmax cross-entropy over the non-ignored rows of [N, V]
    logits (csrc/cross_entropy.hip).  Saves logits, target and the per-row
    logsumexp; backward recomputes the probabilities from them and writes
    the gradient into a buffer of its own.  The per-row upstream gradient
    (upstream scalar / valid rows) is formed on the device: no host sync in
    either direction."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        ctx.ignore_index = ignore_index
        if logits.is_cuda:
            mean, _, lse = hip_ops().cross_entropy_fwd(logits, target,
                                                       ignore_index)
            loss, inv_count = mean[0], mean[1]
        else:
            loss_rows, lse = reference.cross_entropy_fwd(logits, target,
                                                         ignore_index)
            count = (target != ignore_index).sum()
            inv_count = torch.where(count > 0, 1.0 / count.clamp(min=1),
                                    torch.zeros(())).float()
            loss = loss_rows.sum() * inv_count
        ctx.save_for_backward(logits, target, lse, inv_count)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse, inv_count = ctx.saved_tensors
        grow = (dloss.float() * inv_count).expand(logits.shape[0]).contiguous()
        if logits.is_cuda:
            d = hip_ops().cross_entropy_bwd(logits, target, lse, grow,
                                            ctx.ignore_index)
        else:
            d = reference.cross_entropy_bwd(logits, target, lse, grow,
                                            ctx.ignore_index)
        return d, None, None


def fused_cross_entropy(logits, target, ignore_index: int = -100):
    """0-d f32 mean of lse(logits[n]) - logits[n, target[n]] over the rows
    whose target is not ignore_index: F.cross_entropy(logits.float(), target,
    ignore_index=ignore_index), except that with no valid row the result is
    0 with zero gradients, not NaN.

    logits [N, V], target [N] int64.  On the GPU the logits must be bf16,
    contiguous and 16-byte aligned with V % 8 == 0 (ValueError otherwise: no
    eager fallback), the loss is bitwise reproducible, and a target outside
    [0, V) is ignored like ignore_index, never used as an index; checking
    the range would cost a host sync.  On the CPU (any dtype, any V) such a
    target raises IndexError."""
    if logits.dim() != 2 or target.shape != logits.shape[:1]:
        raise ValueError("fused_cross_entropy expects logits [N, V] and "
                         f"target [N], got {tuple(logits.shape)} and "
                         f"{tuple(target.shape)}")
    if target.dtype != torch.int64:
        raise ValueError("target must be int64")
    if logits.is_cuda:
        if logits.dtype != torch.bfloat16:
            raise ValueError("fused_cross_entropy on the GPU needs bf16 "
                             f"logits, got {logits.dtype}")
        if not logits.is_contiguous() or logits.data_ptr() % 16:
            raise ValueError("fused_cross_entropy on the GPU needs "
                             "contiguous, 16-byte aligned logits")
        if logits.shape[1] == 0 or logits.shape[1] % 8:
            raise ValueError("fused_cross_entropy on the GPU needs V % 8 == "
                             f"0, got V = {logits.shape[1]}")
        target = target.contiguous()
    return _CrossEntropyFn.apply(logits, target, ignore_index)


def _check_ema(p, ema, ema_decay):
    """The weight-average operands of the four AdamW steps: both None (off),
    or ema f32, contiguous, of p's length and on p's device with
    0 <= ema_decay < 1.  Returns whether the average is on."""
    if ema is None and ema_decay is None:
        return False
    if ema is None or ema_decay is None:
        raise ValueError("ema and ema_decay go together: got "
                         f"ema={'None' if ema is None else 'a tensor'}, "
                         f"ema_decay={ema_decay}")
    if ema.dtype != torch.float32:
        raise ValueError(f"ema must be f32, got {ema.dtype}")
    if ema.dim() != 1 or not ema.is_contiguous():
        raise ValueError("ema must be 1-D and contiguous")
    if ema.numel() != p.numel():
        raise ValueError(f"ema must have p's length {p.numel()}, got "
                         f"{ema.numel()}")
    if ema.device != p.device:
        raise ValueError(f"ema must be on {p.device}, got {ema.device}")
    if ema.is_cuda and ema.data_ptr() % 16:
        raise ValueError("ema on the GPU must be 16-byte aligned")
    if not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
    return True


def adamw_step(p, grad, m, v, master, *, lr, beta1=0.9, beta2=0.999, eps=1e-8,
               wd=0.01, step, grad_scale=1.0, ema=None, ema_decay=None):
    """Fused AdamW over the flat parameter buffer (see train.py).

    With ema (f32, p's length) and ema_decay = d the same kernel pass also
    keeps a weight average, ema = d * ema + (1 - d) * w with w the new f32
    master value: two f32 products and one f32 sum, never fused, so separate
    f32 torch ops reproduce it bit for bit.  p, m, v and master come out as
    without it.  The other three steps take the same two operands."""
    if _check_ema(p, ema, ema_decay):
        if p.is_cuda:
            hip_ops().adamw_step(p, grad, m, v, master, lr, beta1, beta2, eps,
                                 wd, step, grad_scale, ema, ema_decay)
        else:
            reference.adamw_step(p, grad, m, v, master, lr, beta1, beta2, eps,
                                 wd, step, grad_scale, ema=ema,
                                 ema_decay=ema_decay)
    elif p.is_cuda:
        hip_ops().adamw_step(p, grad, m, v, master, lr, beta1, beta2, eps, wd,
                             step, grad_scale)
    else:
        reference.adamw_step(p, grad, m, v, master, lr, beta1, beta2, eps, wd,
                             step, grad_scale)


def grad_clip_state(grad, *, grad_scale=1.0, max_norm):
    """Global-norm clip state of the flat gradient buffer, on grad's device:
    f32[4] = {norm, scale, finite, sumsq} with norm = grad_scale * |grad|,
    scale = grad_scale * min(1, max_norm / (norm + 1e-6)) and finite = 0 for
    an inf/NaN gradient (csrc/grad_norm.hip).  Deterministic; no host sync.
    max_norm=inf measures and guards without clipping."""
    if not max_norm > 0:
        raise ValueError(f"max_norm must be greater than 0, got {max_norm}")
    if grad.is_cuda:
        return hip_ops().grad_clip_state(grad, grad_scale, max_norm)
    return reference.grad_clip_state(grad, grad_scale, max_norm)


def adamw_step_clipped(p, grad, m, v, master, *, lr, beta1=0.9, beta2=0.999,
                       eps=1e-8, wd=0.01, step, clip_state, ema=None,
                       ema_decay=None):
    """adamw_step with the grad scale and the skip flag read on the device
    from grad_clip_state's result: a non-finite gradient leaves p, m, v and
    master untouched, and ema where it is given."""
    if _check_ema(p, ema, ema_decay):
        if p.is_cuda:
            hip_ops().adamw_step_clipped(p, grad, m, v, master, lr, beta1,
                                         beta2, eps, wd, step, clip_state,
                                         ema, ema_decay)
        else:
            reference.adamw_step_clipped(p, grad, m, v, master, lr, beta1,
                                         beta2, eps, wd, step, clip_state,
                                         ema=ema, ema_decay=ema_decay)
    elif p.is_cuda:
        hip_ops().adamw_step_clipped(p, grad, m, v, master, lr, beta1, beta2,
                                     eps, wd, step, clip_state)
    else:
        reference.adamw_step_clipped(p, grad, m, v, master, lr, beta1, beta2,
                                     eps, wd, step, clip_state)


MAX_SEGMENTS = 1024     # AD_MAX_SEGS of csrc/adamw.hip: the table's LDS image


def check_segment_table(seg_end, seg_lr_mult, seg_wd, n):
    """Validate a HOST segment table (sequences or CPU tensors) for a flat
    buffer of n elements: one length 1 <= S <= MAX_SEGMENTS, seg_end
    strictly increasing from above 0 and ending at n."""
    ends = [int(e) for e in seg_end]
    S = len(ends)
    if not (len(seg_lr_mult) == len(seg_wd) == S):
        raise ValueError("seg_end, seg_lr_mult and seg_wd must have one "
                         f"length, got {S}, {len(seg_lr_mult)}, "
                         f"{len(seg_wd)}")
    if not 1 <= S <= MAX_SEGMENTS:
        raise ValueError(f"the segment table holds 1 to {MAX_SEGMENTS} "
                         f"segments, got {S}")
    if ends[0] <= 0 or any(b <= a for a, b in zip(ends, ends[1:])):
        raise ValueError("seg_end must be strictly increasing from above 0")
    if ends[-1] != n:
        raise ValueError(f"the last segment must end at n = {n}, got "
                         f"{ends[-1]}")


def segment_table(seg_end, seg_lr_mult, seg_wd, n, device=None):
    """Check a host segment table (check_segment_table) and upload it:
    (seg_end int64, seg_lr_mult f32, seg_wd f32) on `device`, the operands of
    adamw_step_grouped.  Build it once; the step itself reads nothing back."""
    check_segment_table(seg_end, seg_lr_mult, seg_wd, n)
    return (torch.tensor([int(e) for e in seg_end], dtype=torch.int64,
                         device=device),
            torch.tensor([float(x) for x in seg_lr_mult],
                         dtype=torch.float32, device=device),
            torch.tensor([float(x) for x in seg_wd], dtype=torch.float32,
                         device=device))


def _check_grouped_operands(p, seg_end, seg_lr_mult, seg_wd):
    """What can be checked without reading a device table back: dtypes,
    shapes, placement.  A CPU table is checked in full."""
    if seg_end.dtype != torch.int64:
        raise ValueError(f"seg_end must be int64, got {seg_end.dtype}")
    for name, t in (("seg_lr_mult", seg_lr_mult), ("seg_wd", seg_wd)):
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be f32, got {t.dtype}")
    for name, t in (("seg_end", seg_end), ("seg_lr_mult", seg_lr_mult),
                    ("seg_wd", seg_wd)):
        if t.dim() != 1 or not t.is_contiguous() or t.device != p.device:
            raise ValueError(f"{name} must be 1-D, contiguous and on "
                             f"{p.device}")
    S = seg_end.numel()
    if not (seg_lr_mult.numel() == seg_wd.numel() == S):
        raise ValueError("seg_end, seg_lr_mult and seg_wd must have one "
                         "length")
    if not 1 <= S <= MAX_SEGMENTS:
        raise ValueError(f"the segment table holds 1 to {MAX_SEGMENTS} "
                         f"segments, got {S}")
    if not p.is_cuda:
        check_segment_table(seg_end.tolist(), seg_lr_mult, seg_wd, p.numel())


def adamw_step_grouped(p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd,
                       *, lr, beta1=0.9, beta2=0.999, eps=1e-8, step,
                       grad_scale=1.0, ema=None, ema_decay=None):
    """adamw_step with parameter groups over the flat buffer: element e
    belongs to the first segment s with e < seg_end[s] and steps at
    lr * seg_lr_mult[s] (an f32 product) with weight decay seg_wd[s], bit for
    bit what adamw_step computes with those two scalars.  The table comes
    from segment_table(), which checks its values on the host; on the GPU
    nothing is read back here."""
    _check_grouped_operands(p, seg_end, seg_lr_mult, seg_wd)
    if _check_ema(p, ema, ema_decay):
        if p.is_cuda:
            hip_ops().adamw_step_grouped(p, grad, m, v, master, seg_end,
                                         seg_lr_mult, seg_wd, lr, beta1,
                                         beta2, eps, step, grad_scale, ema,
                                         ema_decay)
        else:
            reference.adamw_step_grouped(p, grad, m, v, master, seg_end,
                                         seg_lr_mult, seg_wd, lr, beta1,
                                         beta2, eps, step, grad_scale,
                                         ema=ema, ema_decay=ema_decay)
    elif p.is_cuda:
        hip_ops().adamw_step_grouped(p, grad, m, v, master, seg_end,
                                     seg_lr_mult, seg_wd, lr, beta1, beta2,
                                     eps, step, grad_scale)
    else:
        reference.adamw_step_grouped(p, grad, m, v, master, seg_end,
                                     seg_lr_mult, seg_wd, lr, beta1, beta2,
                                     eps, step, grad_scale)


def adamw_step_grouped_clipped(p, grad, m, v, master, seg_end, seg_lr_mult,
                               seg_wd, *, lr, beta1=0.9, beta2=0.999,
                               eps=1e-8, step, clip_state, ema=None,
                               ema_decay=None):
    """adamw_step_grouped with the grad scale and the skip flag read on the
    device from grad_clip_state's result, as adamw_step_clipped."""
    _check_grouped_operands(p, seg_end, seg_lr_mult, seg_wd)
    if _check_ema(p, ema, ema_decay):
        if p.is_cuda:
            hip_ops().adamw_step_grouped_clipped(
                p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd, lr,
                beta1, beta2, eps, step, clip_state, ema, ema_decay)
        else:
            reference.adamw_step_grouped_clipped(
                p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd, lr,
                beta1, beta2, eps, step, clip_state, ema=ema,
                ema_decay=ema_decay)
    elif p.is_cuda:
        hip_ops().adamw_step_grouped_clipped(
            p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd, lr, beta1,
            beta2, eps, step, clip_state)
    else:
        reference.adamw_step_grouped_clipped(
            p, grad, m, v, master, seg_end, seg_lr_mult, seg_wd, lr, beta1,
            beta2, eps, step, clip_state)


# ---- MXFP8 serving (off by default; docs/KERNELS.md "MXFP8 operands") --------
# OCP MXFP8 operands for the four projections of an encoder block at
# inference: e4m3fn elements with one e8m0 power-of-two scale per 32
# consecutive elements of K, as reference.mx_quantize defines them.  A
# quantised tensor travels as (q, s): uint8 e4m3 bytes shaped like the tensor
# it stands for and uint8 e8m0 bytes [..., K / 32].  On the GPU the producers
# are HIP kernels that match the reference bit for bit and the GEMM is a
# library call (mx_gemm_backend); on the CPU every op is built from the
# reference, so a quantised model runs there as a fake-quant simulation.  No
# autograd.

def mx_quant_rows(x):
    """(q, s) = MXFP8 of x [..., K] along K, K % 32 == 0: activations on
    their way into a projection, and weights [N, K]."""
    if x.is_cuda:
        return tuple(hip_ops().mx_quant_rows(x.contiguous()))
    return reference.mx_quantize(x)


def mx_layernorm(x, gamma, beta, eps: float = 1e-5):
    """(q, s) = mx_quant_rows(fused_layernorm(x, gamma, beta, eps)), bit for
    bit, in one kernel that never writes the bf16 activations.  D % 32 == 0
    and D <= 4096 on the GPU."""
    if x.is_cuda:
        q, s, _ = hip_ops().mx_layernorm_fwd(x.contiguous(), None, gamma,
                                             beta, eps)
        return q, s
    return reference.mx_quantize(
        reference.layernorm_fwd(x, gamma, beta, eps)[0])


def mx_add_layernorm(x, residual, gamma, beta, eps: float = 1e-5):
    """(q, s, sum) with (y, sum) = fused_add_layernorm(x, residual, gamma,
    beta, eps) and (q, s) = mx_quant_rows(y), bit for bit."""
    if x.is_cuda:
        return tuple(hip_ops().mx_layernorm_fwd(
            x.contiguous(), residual.contiguous(), gamma, beta, eps))
    y, sm, _, _ = reference.add_layernorm_fwd(x, residual, gamma, beta, eps)
    return (*reference.mx_quantize(y), sm)


def mx_bias_gelu(h, b):
    """(q, s) = mx_quant_rows(fused_bias_gelu(h, b)), bit for bit, in one
    kernel: the down projection's operand from the up GEMM's bias-free bf16
    output."""
    if h.is_cuda:
        return tuple(hip_ops().mx_bias_gelu(h.contiguous(), b))
    return reference.mx_quantize(reference.bias_gelu_fwd(h, b))


def mx_supported(M: int, N: int, K: int) -> bool:
    """The (rows, out features, in features) lattice of mx_linear on the
    GPU: what the block-scaled GEMM of the installed library takes."""
    return (M > 0 and N > 0 and K > 0 and M % 32 == 0 and N % 32 == 0
            and K % 128 == 0)


def _mx_pad_scale_rows(s2):
    """torch._scaled_mm takes the scales of an [R, K] operand as
    round_up(R, 128) * K / 32 bytes: plain row-major [R, K / 32] with the
    rows filled up (2^0 scales for rows that do not exist)."""
    pad = -s2.shape[0] % 128
    if not pad:
        return s2
    return torch.cat([s2, s2.new_full((pad, s2.shape[1]), 127)])


def _mx_scaled_mm(q2, s2, wq, ws, bias=None):
    return torch._scaled_mm(
        q2.view(torch.float8_e4m3fn), wq.view(torch.float8_e4m3fn).t(),
        _mx_pad_scale_rows(s2).view(torch.float8_e8m0fnu),
        _mx_pad_scale_rows(ws).view(torch.float8_e8m0fnu),
        bias=bias, out_dtype=torch.bfloat16)


def _mx_dequant_linear(q2, s2, wq, ws, bias=None):
    return torch.nn.functional.linear(
        reference.mx_dequantize(q2, s2).to(torch.bfloat16),
        reference.mx_dequantize(wq, ws).to(torch.bfloat16), bias)


# (GEMM backend, whether its own bias argument is used), probed once.
#
# MEASUREMENT-ONLY on the library this was written against (torch 2.10 /
# ROCm 7 on MI355X): there the probe turns the block-scaled GEMM down (it
# truncates its bf16 output and takes no bias, docs/PERF.md "MXFP8
# serving"), so _mx_scaled_mm, the scale-row padding and the separate bias
# add run only under TOSEM_MX_GEMM=scaled_mm, for scripts/bench_mx_serving.py,
# and in tests/test_mx_gpu.py's test of that branch under the wider budget a
# truncating output needs.  They become the default path by themselves on a
# library whose block-scaled GEMM meets the contract.
_MX_BACKEND: Optional[tuple] = None
# shapes the block-scaled GEMM refused at run time (each reported once by a
# warning): they take the dequantised GEMM from then on
_MX_REFUSED: set = set()


def _mx_probe() -> tuple:
    """(plain GEMM within the contract, GEMM with bias within the contract).
    Run the block-scaled GEMM once, without and with its bias argument,
    on operands whose block scales differ within every row, and hold it to
    mx_linear's accuracy contract against float64 of the dequantised
    operands: per output 2^-8 |y| (the bf16 rounding or its neighbour) plus
    K 2^-24 sum_k |a_k w_k| (an f32 accumulation in any order).  A build
    without the MX path raises; one that read the scales in another layout
    than row-major [rows, K / 32] misses by orders of magnitude."""
    g = torch.Generator().manual_seed(0)
    M, N, K = 96, 160, 256

    def operand(R):
        e = torch.randint(-8, 9, (R, K // 32), generator=g).float()
        x = torch.randn(R, K, generator=g) * torch.exp2(e).repeat_interleave(
            32, 1)
        return reference.mx_quantize(x.bfloat16())

    (aq, asc), (wq, wsc) = operand(M), operand(N)
    a64 = reference.mx_dequantize(aq, asc).double()
    w64 = reference.mx_dequantize(wq, wsc).double()
    ref = a64 @ w64.t()
    acc = K * 2.0 ** -24 * (a64.abs() @ w64.abs().t())
    bias = (torch.randn(N, generator=g) * ref.std()).bfloat16()
    dev_ops = [t.cuda() for t in (aq, asc, wq, wsc)]

    def within(b):
        want = ref if b is None else ref + b.double()
        try:
            y = _mx_scaled_mm(*dev_ops, None if b is None else b.cuda())
        except (RuntimeError, AttributeError, TypeError):
            return False
        err = (y.double().cpu() - want).abs()
        return bool((err <= 2.0 ** -8 * want.abs() + acc).all())

    return within(None), within(bias)


def _mx_backend() -> tuple:
    global _MX_BACKEND
    if _MX_BACKEND is None:
        force = os.environ.get("TOSEM_MX_GEMM", "")
        if force == "dequant":
            _MX_BACKEND = ("dequant", True)
        else:
            ok, ok_bias = _mx_probe()
            # the dequantised GEMM takes its bias in F.linear
            _MX_BACKEND = (("scaled_mm", ok_bias)
                           if ok or force == "scaled_mm" else
                           ("dequant", True))
    return _MX_BACKEND


def mx_gemm_backend() -> str:
    """Which GEMM mx_linear runs on the GPU: "scaled_mm" (torch._scaled_mm's
    block-scaled hipBLASLt GEMM on the MXFP8 operands themselves) or
    "dequant" (operands dequantised to bf16, exact except for values below
    bf16's range, then F.linear: no speed to claim).  Probed once per
    process against mx_linear's accuracy contract (_mx_probe): a block-scaled
    GEMM that misses it is not used.  A/B knob: TOSEM_MX_GEMM=dequant or
    =scaled_mm forces one of them, the latter whatever the probe found."""
    return _mx_backend()[0]


def mx_bias_in_gemm() -> bool:
    """Whether mx_linear's bias goes through the GEMM's own bias argument
    (one rounding to bf16) or, where the library does not take one in this
    mode, through one torch add on the GEMM's bf16 output."""
    return _mx_backend()[1]


def mx_linear(q, s, wq, ws, bias=None, out_dtype=None):
    """y [..., N] = dequant(q, s) [..., K] @ dequant(wq, ws) [N, K]^T + bias,
    f32 accumulation.  GPU: bf16 out, through mx_gemm_backend(); (rows, N, K)
    off mx_supported's lattice raises ValueError.  CPU: F.linear of the
    dequantised operands in f32, cast to out_dtype (default f32)."""
    K = q.shape[-1]
    N = wq.shape[0]
    lead = q.shape[:-1]
    if wq.shape[-1] != K or s.shape != (*lead, K // 32) or \
            ws.shape != (N, K // 32):
        raise ValueError("mx_linear operands disagree: q "
                         f"{tuple(q.shape)}, s {tuple(s.shape)}, wq "
                         f"{tuple(wq.shape)}, ws {tuple(ws.shape)}")
    if not q.is_cuda:
        y = torch.nn.functional.linear(
            reference.mx_dequantize(q, s), reference.mx_dequantize(wq, ws),
            None if bias is None else bias.float())
        return y if out_dtype is None else y.to(out_dtype)
    if out_dtype not in (None, torch.bfloat16):
        raise ValueError(f"mx_linear on the GPU writes bf16, not {out_dtype}")
    M = q.numel() // K
    if not mx_supported(M, N, K):
        raise ValueError(
            "mx_linear on the GPU needs rows and out features that are "
            "multiples of 32 and in features a multiple of 128, got "
            f"(M, N, K) = ({M}, {N}, {K})")
    q2 = q.reshape(M, K)
    s2 = s.reshape(M, K // 32)
    backend, bias_in_gemm = _mx_backend()
    if backend == "scaled_mm" and (M, N, K) not in _MX_REFUSED:
        try:
            y = _mx_scaled_mm(q2, s2, wq, ws, bias if bias_in_gemm else None)
            if bias is not None and not bias_in_gemm:
                y = y + bias
            return y.view(*lead, N)
        except RuntimeError as e:
            # the library has no block-scaled kernel for this shape: say so,
            # once, and serve it through the dequantised GEMM
            warnings.warn(
                f"mx_linear: the block-scaled GEMM refused (M, N, K) = "
                f"({M}, {N}, {K}) and the dequantised GEMM takes this shape "
                f"from now on: {str(e).splitlines()[0]}")
            _MX_REFUSED.add((M, N, K))
    return _mx_dequant_linear(q2, s2, wq, ws, bias).view(*lead, N)
