"""MLTC — the learned test-case classifier (the framework's flagship model).

A bidirectional transformer encoder over tokenized test code / assertion text
that predicts the reference study's taxonomy labels (RQs/taxonomy_test2.csv:1):

  * 19 test strategies   (RQ1_tests.csv rows)      — multi-label
  * 21 quality properties (tests_prop_rq3.csv:1)   — multi-label
  * 9 ML workflow stages  (RQ1_tests.csv columns)  — single-label
  * 4 test methods        (tests_methods.csv:2-5)  — single-label

MI355X-first design: all parameters bf16 (flat-packed by the trainer), GEMMs
through hipBLASLt (torch.matmul / F.linear on ROCm), and the non-GEMM hot ops
(LayerNorm, bias+GeLU, masked softmax) are hand-written gfx950 HIP kernels
(csrc/*.hip) behind tosem2021_amd.ops.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from tosem2021_amd import ops

# Label spaces (mirrors tosem2021_amd.extract.schema; duplicated sizes only)
N_STRATEGIES = 19
N_PROPERTIES = 21
N_STAGES = 9
N_METHODS = 4

HEAD_SIZES = {
    "strategy": N_STRATEGIES,   # multi-label (BCE)
    "property": N_PROPERTIES,   # multi-label (BCE)
    "stage": N_STAGES,          # single-label (CE)
    "method": N_METHODS,        # single-label (CE)
}
MULTILABEL_HEADS = ("strategy", "property")


@dataclass
class MLTCConfig:
    vocab_size: int = 32768
    d_model: int = 1024
    n_heads: int = 16
    n_layers: int = 12
    d_ff: int = 4096
    max_seq: int = 512
    dropout: float = 0.0
    # fused_dropout: in training mode with dropout > 0 the residual dropout
    # runs inside the add+LayerNorm kernels (ops.fused_dropout_add_layernorm)
    # with a counter-based mask seeded by dropout_seed, instead of F.dropout
    # and torch's global generator.  Another random stream, so a switch.
    fused_dropout: bool = False
    dropout_seed: int = 0
    # attn_dropout: in training mode, dropout on the attention probabilities
    # with this rate, inside the flash kernels on the GPU
    # (ops.flash_attention_packed(dropout=)) and through the same
    # counter-based mask on the CPU.  Seeded by dropout_seed; independent of
    # `dropout` and `fused_dropout`.  The effective rate is
    # round(p * 256) / 256.
    attn_dropout: float = 0.0
    layer_norm_eps: float = 1e-5
    heads: Dict[str, int] = field(default_factory=lambda: dict(HEAD_SIZES))

    def __post_init__(self):
        # every way in (YAML model_cfg, train_classifier, the CLI) builds
        # this dataclass, so the rate is checked here, once
        if not 0.0 <= self.attn_dropout < 1.0:
            raise ValueError("attn_dropout must be in [0, 1), got "
                             f"{self.attn_dropout}")

    @property
    def head_dim(self) -> int:
        assert self.d_model % self.n_heads == 0
        return self.d_model // self.n_heads


CONFIGS: Dict[str, MLTCConfig] = {
    # flagship: the bench.py / BASELINE config
    "mltc-base": MLTCConfig(),
    # small config for fast CPU tests / smoke
    "mltc-tiny": MLTCConfig(vocab_size=512, d_model=128, n_heads=4, n_layers=2,
                            d_ff=256, max_seq=64),
    # scale-up config (1.28B params): exercises the same kernels at d=2048
    # (LN template PKTS=4, 32 flash heads) — sized for 288 GB HBM3E
    "mltc-large": MLTCConfig(d_model=2048, n_heads=32, n_layers=24,
                             d_ff=8192),
}


class FusedLayerNorm(nn.Module):
    def __init__(self, d: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))
        self.eps = eps

    def forward(self, x):
        return ops.fused_layernorm(x, self.weight, self.bias, self.eps)


# A/B knob (TOSEM_FUSED_LINEAR=1): route the bias-carrying projections
# through ops.fused_linear — torch addmm forward (same epilogue GEMM) but
# backward computes db with the colsum bias_grad kernel (~20 us) instead of
# at::native::reduce (~58 us).  RE-MEASURED round 2 with the committed
# TunableOp table active: still a 13.5 ms/step REGRESSION (97.6 vs 84.1 ms
# back-to-back on one box) — the explicit dgrad/wgrad matmul layouts are
# not in the tuned table and dispatch worse than addmm's backward, exactly
# as in round 1.  Default stays OFF; the at::native::reduce bias grads
# that addmm's backward ran were since removed without touching the GEMM
# calls (_FOLD_BIAS_GRAD below).
_USE_FUSED_LINEAR = os.environ.get("TOSEM_FUSED_LINEAR", "0") == "1"
# TOSEM_WGRAD=1: weight grads of the big projections through the custom
# split-K MFMA wgrad kernel (csrc/wgrad_gemm.hip) + colsum bias grad;
# forward addmm and dgrad dispatch unchanged.
_USE_WGRAD = os.environ.get("TOSEM_WGRAD", "0") == "1"


# Folded bias gradients (opt-in: TOSEM_FOLD_BIAS_GRAD=1, or the model's
# fold_bias_grad keyword): attn.qkv (on the flash path), attn.proj and ffn.down
# are called with their bias DETACHED — same addmm forward, same dgrad/wgrad
# mm calls in backward, but autograd no longer runs sum(0) over the
# [tokens, features] output gradient.  That gradient is exactly the dx the
# next fused add+LayerNorm backward stores (proj, down) or the dqkv the
# flash backward stores (qkv), and those kernels sum its columns while they
# are in registers (residual_bias of ops.fused_add_layernorm, qkv_bias of
# ops.flash_attention_packed).  This does not change how any GEMM is
# called, unlike TOSEM_FUSED_LINEAR above.
#
# MEASURED, and why the default is OFF: 2.8 ms/step faster (81.4 -> 78.6 ms),
# and after one step every gradient outside the three bias families is
# bit-equal to the unrouted model's.  But the bias sums are taken in another
# order, and AdamW normalises a gradient whatever its size: the k third of
# qkv.bias has an analytic gradient of zero, so what it sees there is pure
# rounding noise (~1e-7), and a reordered sum is DIFFERENT noise that moves
# the parameter by about lr per step in another direction.  After 3 steps
# those parameters are off by 80 % of their size, after 30 steps the loss
# differs in the third digit (3.063 vs 3.077) — a different, equally valid
# trajectory, not the same one.  With the routing off a 30-step run is
# bit-identical to the one before these kernels existed (docs/PERF.md).
_FOLD_BIAS_GRAD = os.environ.get("TOSEM_FOLD_BIAS_GRAD", "0") == "1"


def _linear(mod: nn.Linear, x: torch.Tensor,
            fold_bias: bool = False) -> torch.Tensor:
    if fold_bias:
        # the caller hands mod.bias to the LayerNorm that consumes the output
        return F.linear(x, mod.weight, mod.bias.detach())
    if x.is_cuda and torch.is_grad_enabled():
        if _USE_WGRAD and ops.wgrad_linear_supported(
                mod.out_features, mod.in_features,
                x.numel() // x.shape[-1]):
            return ops.wgrad_linear(x, mod.weight, mod.bias)
        if _USE_FUSED_LINEAR and mod.bias is not None:
            return ops.fused_linear(x, mod.weight, mod.bias)
    return mod(x)


class Attention(nn.Module):
    """Multi-head bidirectional self-attention.

    QK^T and PV run as batched hipBLASLt GEMMs (MFMA); the scaled masked
    softmax between them is the fused gfx950 kernel (csrc/softmax.hip).
    """

    def __init__(self, cfg: MLTCConfig, layer: int = 0):
        super().__init__()
        self.n_heads = cfg.n_heads
        self.head_dim = cfg.head_dim
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        self.layer = layer      # the attention dropout mask's layer word
        self.qkv = nn.Linear(cfg.d_model, 3 * cfg.d_model, bias=True)
        self.proj = nn.Linear(cfg.d_model, cfg.d_model, bias=True)

    def forward(self, x, mask_bias: Optional[torch.Tensor],
                seg: Optional[torch.Tensor] = None, fold_bias: bool = False,
                attn_drop=None):
        """seg: [B, L] int32 segment ids of a packed batch (exclusive with
        mask_bias): attention stays inside each segment.  fold_bias: proj
        runs with its bias detached; the caller routes proj.bias to the
        LayerNorm that consumes the output (see _FOLD_BIAS_GRAD).
        attn_drop: (p, seed, call) of this forward's dropout on the
        attention probabilities (never together with fold_bias); the mask
        is reference.attn_dropout_keep's for this block's layer."""
        dropout = None if attn_drop is None else (*attn_drop, self.layer)
        if ops.flash_supported(self.head_dim, x.shape[1]):
            # (with fold_bias the flash backward also returns qkv.bias's
            # gradient, the column sum of the dqkv it writes)
            qkv = _linear(self.qkv, x, fold_bias)
        else:
            qkv = self.qkv(x)
        out = self._attend(qkv, mask_bias, seg, fold_bias, dropout)
        return _linear(self.proj, out, fold_bias)

    def _attend(self, qkv, mask_bias, seg, fold_bias: bool = False,
                dropout=None):
        """[B, L, 3D] packed projection output -> [B, L, D] attention output,
        ready for proj.  dropout: (p, seed, call, layer) or None."""
        B, L, _ = qkv.shape
        if ops.flash_supported(self.head_dim, L):
            # MFMA flash kernels run straight on the packed [B, L, 3D]
            # projection output and write attention out (and, in backward,
            # every gradient) in the packed layouts — no repack kernels,
            # no [L, L] score tensor, O(L) attention memory
            return ops.flash_attention_packed(
                qkv, self.n_heads, mask_bias, self.scale, seg,
                self.qkv.bias if fold_bias else None, dropout)
        if dropout is not None and qkv.is_cuda:
            # no O(L^2) fallback: P exists only inside the flash kernels
            raise RuntimeError(
                "attention dropout on the GPU needs the flash kernels: "
                f"head_dim 64 and L % 32 == 0, got head_dim {self.head_dim}, "
                f"L {L}")
        if seg is not None or dropout is not None:
            if qkv.is_cuda:
                # no O(L^2) fallback: packing exists to cut attention work
                raise RuntimeError(
                    "sequence packing on the GPU needs the segment-aware "
                    f"flash kernels: head_dim 64 and L % 32 == 0, got "
                    f"head_dim {self.head_dim}, L {L}")
            # CPU reference for any shape: plain softmax over the
            # segment (or padding) bias, times the reference dropout mask
            q, k, v = ops.qkv_repack(qkv, self.n_heads)
            s = torch.matmul(q, k.transpose(-1, -2)).float() * self.scale
            if seg is not None:
                s = s + ops.reference.segment_bias(seg)
            elif mask_bias is not None:
                s = s + mask_bias.view(B, 1, 1, L)
            p = torch.softmax(s, dim=-1)
            if dropout is not None:
                keep = ops.reference.attn_dropout_keep(B, self.n_heads, L,
                                                       *dropout)
                p = p * keep * ops.reference.attn_dropout_threshold(
                    dropout[0])[1]
            out = torch.matmul(p.to(v.dtype), v)
            return ops.out_repack(out)
        # general-shape fallback: gather kernel to bmm-ready
        # [3, B, H, L, dh] (csrc/repack.hip), bmm + fused softmax
        q, k, v = ops.qkv_repack(qkv, self.n_heads)         # [B, H, L, dh]
        scores = torch.matmul(q, k.transpose(-1, -2))  # [B, H, L, L]
        p = ops.fused_softmax(scores, mask_bias, self.scale)
        return ops.out_repack(torch.matmul(p, v))      # [B, L, D]

    def forward_mx(self, q, s, mask_bias, seg=None):
        """forward on the MXFP8 form (q, s) of the normalised input, with
        the weights MLTC.quantize_mx() left on qkv and proj.  Attention
        itself is unchanged: the qkv GEMM writes bf16, and the attention
        output is quantised on its way into proj."""
        dt = self.qkv.weight.dtype
        qkv = ops.mx_linear(q, s, self.qkv.mx_q, self.qkv.mx_s, self.qkv.bias,
                            dt)
        out = self._attend(qkv, mask_bias, seg)
        return ops.mx_linear(*ops.mx_quant_rows(out), self.proj.mx_q,
                             self.proj.mx_s, self.proj.bias, dt)


class FFN(nn.Module):
    """d_model -> d_ff (bias+GeLU fused into the gfx950 kernel) -> d_model."""

    def __init__(self, cfg: MLTCConfig):
        super().__init__()
        self.up = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.up_bias = nn.Parameter(torch.zeros(cfg.d_ff))
        self.down = nn.Linear(cfg.d_ff, cfg.d_model, bias=True)

    def forward(self, x, fold_bias: bool = False):
        if x.is_cuda and not torch.is_grad_enabled():
            # inference: bias+GeLU fused into the up GEMM's epilogue
            B, L, D = x.shape
            a = ops.lt_linear_gelu_bias(x.reshape(-1, D).contiguous(),
                                        self.up.weight, self.up_bias)
            return self.down(a.view(B, L, -1))
        h = _linear(self.up, x)
        h = ops.fused_bias_gelu(h, self.up_bias)
        return _linear(self.down, h, fold_bias)

    def forward_mx(self, q, s):
        """forward on the MXFP8 form (q, s) of the normalised input: the up
        GEMM writes bf16 without bias, and one kernel adds the bias, applies
        GeLU and quantises the down GEMM's operand."""
        dt = self.up.weight.dtype
        h = ops.mx_linear(q, s, self.up.mx_q, self.up.mx_s, None, dt)
        return ops.mx_linear(*ops.mx_bias_gelu(h, self.up_bias),
                             self.down.mx_q, self.down.mx_s, self.down.bias,
                             dt)


class EncoderBlock(nn.Module):
    """Pre-LN block carrying an un-added (stream, delta) residual pair.

    The residual add is fused into the next LayerNorm's first read
    (ops.fused_add_layernorm), so the block never launches a separate
    elementwise add: it receives the previous sublayer's (x, delta), and
    returns its own.

    With fold_bias the bias gradient of the projection behind each delta is
    computed by the LayerNorm backward that consumes the delta: proj.bias
    goes to this block's ln2; the caller passes the previous block's
    ffn.down.bias in as delta_bias and hands this block's on to the next
    consumer of the returned delta (the next block's ln1, or ln_f).

    With drop = (p, seed, call), the fused residual dropout of this forward,
    the deltas travel un-dropped and each consuming add+LayerNorm drops its
    delta itself: block i's ln2 at site 2i (its attention delta), and the
    consumer of its ffn delta, the next block's ln1 or ln_f, at site 2i + 1.
    """

    def __init__(self, cfg: MLTCConfig, layer: int = 0):
        super().__init__()
        self.ln1 = FusedLayerNorm(cfg.d_model, cfg.layer_norm_eps)
        self.attn = Attention(cfg, layer)
        self.ln2 = FusedLayerNorm(cfg.d_model, cfg.layer_norm_eps)
        self.ffn = FFN(cfg)
        self.dropout = cfg.dropout

    def _drop(self, h):
        return F.dropout(h, self.dropout, self.training) if self.dropout else h

    def fold_ok(self) -> bool:
        """The delta's gradient is the LayerNorm's dx only when no dropout
        sits between the projection and the add."""
        return not (self.dropout and self.training)

    def forward(self, x, delta, mask_bias, seg=None, delta_bias=None,
                fold_bias: bool = False, drop=None, index: int = 0,
                attn_drop=None):
        if drop is not None:
            return self._forward_fused_dropout(x, delta, mask_bias, seg, drop,
                                               index, attn_drop)
        if delta is None:
            y1 = ops.fused_layernorm(x, self.ln1.weight, self.ln1.bias,
                                     self.ln1.eps)
            s1 = x
        else:
            y1, s1 = ops.fused_add_layernorm(x, delta, self.ln1.weight,
                                             self.ln1.bias, self.ln1.eps,
                                             delta_bias)
        fold_bias = fold_bias and self.fold_ok()
        h = self._drop(self.attn(y1, mask_bias, seg, fold_bias, attn_drop))
        y2, s2 = ops.fused_add_layernorm(
            s1, h, self.ln2.weight, self.ln2.bias, self.ln2.eps,
            self.attn.proj.bias if fold_bias else None)
        h2 = self._drop(self.ffn(y2, fold_bias))
        return s2, h2

    def forward_mx(self, x, delta, mask_bias, seg=None):
        """forward with MXFP8 projections (MLTC.quantize_mx; eval mode, no
        grad): LN-MX -> qkv -> attention (unchanged) -> quantise -> proj ->
        add+LN-MX -> up -> bias+GeLU+quantise -> down.  The LayerNorm
        kernels hand the GEMMs their quantised operand directly; the
        (stream, delta) pair travels as in forward."""
        if delta is None:
            q, s = ops.mx_layernorm(x, self.ln1.weight, self.ln1.bias,
                                    self.ln1.eps)
            s1 = x
        else:
            q, s, s1 = ops.mx_add_layernorm(x, delta, self.ln1.weight,
                                            self.ln1.bias, self.ln1.eps)
        h = self.attn.forward_mx(q, s, mask_bias, seg)
        q, s, s2 = ops.mx_add_layernorm(s1, h, self.ln2.weight, self.ln2.bias,
                                        self.ln2.eps)
        return s2, self.ffn.forward_mx(q, s)

    def _forward_fused_dropout(self, x, delta, mask_bias, seg, drop, index,
                               attn_drop=None):
        if delta is None:
            y1 = ops.fused_layernorm(x, self.ln1.weight, self.ln1.bias,
                                     self.ln1.eps)
            s1 = x
        else:
            y1, s1 = ops.fused_dropout_add_layernorm(
                x, delta, self.ln1.weight, self.ln1.bias, self.ln1.eps,
                *drop, 2 * index - 1)
        h = self.attn(y1, mask_bias, seg, attn_drop=attn_drop)
        y2, s2 = ops.fused_dropout_add_layernorm(
            s1, h, self.ln2.weight, self.ln2.bias, self.ln2.eps, *drop,
            2 * index)
        return s2, self.ffn(y2)


class MLTC(nn.Module):
    def __init__(self, cfg: MLTCConfig,
                 fold_bias_grad: Optional[bool] = None):
        """fold_bias_grad: None = on for GPU inputs if
        TOSEM_FOLD_BIAS_GRAD=1 (default off); True = on, also on the CPU
        reference path (for tests); False = off.  Whatever the setting, the fold is taken only
        where it is exact: see _fold_active."""
        super().__init__()
        self.cfg = cfg
        self.fold_bias_grad = fold_bias_grad
        # counter-based dropout (cfg.fused_dropout, cfg.attn_dropout):
        # training-mode forwards so far, the `call` word of every mask,
        # checkpointed by the Trainer so that a resumed run draws the masks
        # an uninterrupted one would; and the data-parallel rank, so that
        # ranks draw different masks
        self.dropout_call = 0
        self.dropout_rank = 0
        # quantize_mx(): the weights' version stamps at quantisation time
        self._mx_versions = None
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.pos_emb = nn.Embedding(cfg.max_seq, cfg.d_model)
        self.blocks = nn.ModuleList(EncoderBlock(cfg, i)
                                    for i in range(cfg.n_layers))
        self.ln_f = FusedLayerNorm(cfg.d_model, cfg.layer_norm_eps)
        self.heads = nn.ModuleDict(
            {name: nn.Linear(cfg.d_model, n) for name, n in cfg.heads.items()}
        )
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=0.02)
            if isinstance(m, nn.Linear) and m.bias is not None:
                nn.init.zeros_(m.bias)

    def _fold_active(self, x: torch.Tensor) -> bool:
        """Whether proj/down bias gradients are folded into the LayerNorm
        backward for this call: grad enabled, no active dropout, neither of
        the Linear-replacing A/B knobs set, and switched on."""
        if self.fold_bias_grad is None:
            on = _FOLD_BIAS_GRAD and x.is_cuda
        else:
            on = self.fold_bias_grad
        return (on and torch.is_grad_enabled()
                and not (self.cfg.dropout and self.training)
                and not (self.cfg.attn_dropout and self.training)
                and not _USE_FUSED_LINEAR and not _USE_WGRAD)

    def _dropout_args(self):
        """((p, seed, call) of this forward's fused residual dropout,
        (p, seed, call) of its attention dropout), each None where it is
        inactive: switch off, rate 0, or eval mode.  Both share the seed and
        the call counter, which advances once per training forward that has
        either active; their masks differ by site (csrc/philox.h)."""
        cfg = self.cfg
        fused = bool(cfg.fused_dropout and cfg.dropout and self.training)
        attn = bool(cfg.attn_dropout and self.training)
        if not (fused or attn):
            return None, None
        call = self.dropout_call
        self.dropout_call += 1
        seed = cfg.dropout_seed * 65536 + self.dropout_rank
        return ((cfg.dropout, seed, call) if fused else None,
                (cfg.attn_dropout, seed, call) if attn else None)

    def _mx_linears(self):
        """The projections quantize_mx covers, block by block."""
        for blk in self.blocks:
            yield from (blk.attn.qkv, blk.attn.proj, blk.ffn.up, blk.ffn.down)

    @torch.no_grad()
    def quantize_mx(self) -> "MLTC":
        """Serve with MXFP8 projections: quantise attn.qkv, attn.proj, ffn.up
        and ffn.down of every block (ops.mx_quant_rows along K) into
        non-persistent buffers mx_q, mx_s on those modules.  Parameters, the
        state dict and checkpoints do not change; embeddings, attention, the
        pool and the heads stay as they are.  From here until clear_mx() an
        eval-mode forward under no_grad runs EncoderBlock.forward_mx; one in
        training mode or with grad enabled raises, and so does one after a
        weight has been written (an EMA swap, a checkpoint load, an
        optimizer step; _mx_weight_versions says how that is seen under a
        Trainer): call quantize_mx() again.  Load the weights first, then
        quantise."""
        self.clear_mx()
        for lin in self._mx_linears():
            q, s = ops.mx_quant_rows(lin.weight.detach())
            lin.register_buffer("mx_q", q, persistent=False)
            lin.register_buffer("mx_s", s, persistent=False)
        self._mx_versions = self._mx_weight_versions()
        return self

    def _mx_weight_versions(self):
        """What a write to a quantised projection's weight moves: the
        parameter's own version counter and, for a model whose parameters
        are views into a trainer's flat buffer (train.FlatParams marks them
        with `_flat_owner`), that buffer's.  Rebinding `p.data` to a view
        leaves the parameter its own counter, so `flat.copy_(...)`, which is
        how an EMA swap and a checkpoint load write, shows only on the
        owner; the fused AdamW step writes through raw pointers and the
        Trainer bumps the owner's counter itself."""
        out = []
        for lin in self._mx_linears():
            owner = getattr(lin.weight, "_flat_owner", None)
            out.append((lin.weight._version, lin.weight.data_ptr(),
                        None if owner is None else owner._version))
        return out

    def clear_mx(self) -> "MLTC":
        """Drop quantize_mx()'s buffers: forwards run the bf16 path again."""
        for lin in self._mx_linears():
            for name in ("mx_q", "mx_s"):
                if hasattr(lin, name):
                    delattr(lin, name)
        self._mx_versions = None
        return self

    @property
    def mx_active(self) -> bool:
        return self._mx_versions is not None

    def _run_blocks_mx(self, x, mask_bias, seg):
        if self.training or torch.is_grad_enabled():
            raise RuntimeError(
                "the model is quantised for MXFP8 serving (quantize_mx): "
                "run it in eval mode under torch.no_grad(), or call "
                "clear_mx() first")
        if self._mx_versions != self._mx_weight_versions():
            raise RuntimeError(
                "weights changed since quantize_mx(): the quantised copies "
                "are stale; call quantize_mx() again")
        delta = None
        for blk in self.blocks:
            x, delta = blk.forward_mx(x, delta, mask_bias, seg)
        if delta is None:
            return self.ln_f(x)
        x, _ = ops.fused_add_layernorm(x, delta, self.ln_f.weight,
                                       self.ln_f.bias, self.ln_f.eps)
        return x

    def _run_blocks(self, x, mask_bias, seg):
        if self.mx_active:
            return self._run_blocks_mx(x, mask_bias, seg)
        drop, attn_drop = self._dropout_args()
        if drop is not None:
            delta = None
            for i, blk in enumerate(self.blocks):
                x, delta = blk(x, delta, mask_bias, seg, drop=drop, index=i,
                               attn_drop=attn_drop)
            if delta is None:
                return self.ln_f(x)
            x, _ = ops.fused_dropout_add_layernorm(
                x, delta, self.ln_f.weight, self.ln_f.bias, self.ln_f.eps,
                *drop, 2 * len(self.blocks) - 1)
            return x
        fold = self._fold_active(x)
        delta = delta_bias = None
        for blk in self.blocks:
            x, delta = blk(x, delta, mask_bias, seg, delta_bias, fold,
                           attn_drop=attn_drop)
            # the bias that belongs to this delta travels on with it
            delta_bias = blk.ffn.down.bias if fold and blk.fold_ok() else None
        if delta is None:
            return self.ln_f(x)
        x, _ = ops.fused_add_layernorm(x, delta, self.ln_f.weight,
                                       self.ln_f.bias, self.ln_f.eps,
                                       delta_bias)
        return x

    def forward(self, tokens: Optional[torch.Tensor],
                attn_mask: Optional[torch.Tensor] = None,
                packing=None) -> Dict[str, torch.Tensor]:
        """tokens: [B, L] int64; attn_mask: [B, L] bool (True = valid).

        packing: a data.packing.PackedBatch (exclusive with attn_mask;
        tokens may be None and defaults to packing.tokens).  Positions come
        from packing.pos, attention stays inside packing.seg's segments and
        the pool is per segment: logits are [N, .] in SEGMENT order —
        packing.unpermute() restores the examples' input order."""
        x = self.encode(tokens, attn_mask, packing)
        if packing is not None:
            # per-example mean-pool over the flattened positions
            R, L, _ = x.shape
            pooled = ops.segment_mean_pool(x.reshape(R * L, -1),
                                           packing.seg_start, packing.seg_len,
                                           packing.pos2seg)
        else:
            # masked mean-pool over valid tokens (fused kernel: csrc/pool.hip)
            pooled = ops.masked_mean_pool(x, attn_mask)
        return {name: head(pooled) for name, head in self.heads.items()}

    def encode(self, tokens: Optional[torch.Tensor],
               attn_mask: Optional[torch.Tensor] = None,
               packing=None) -> torch.Tensor:
        """The encoder up to and including ln_f: [B, L, D] hidden states
        ([R, row_len, D] for a packed batch).  Arguments as in forward."""
        if packing is not None:
            if attn_mask is not None:
                raise ValueError("attn_mask and packing are mutually "
                                 "exclusive: a packed batch carries its own "
                                 "padding segment")
            if tokens is None:
                tokens = packing.tokens
            x = self.tok_emb(tokens) + self.pos_emb(packing.pos)
            return self._run_blocks(x, None, packing.seg)
        B, L = tokens.shape
        pos = torch.arange(L, device=tokens.device)
        x = self.tok_emb(tokens) + self.pos_emb(pos)[None, :, :]
        mask_bias = None
        if attn_mask is not None:
            mask_bias = torch.where(
                attn_mask, 0.0, -1e9
            ).to(torch.float32).contiguous()
        return self._run_blocks(x, mask_bias, None)

    # rows of the LM-head GEMM come in multiples of this, filled up with
    # ignored rows: a bounded set of M values for the GEMM library, and the
    # loss kernel's ignore path runs in every step
    MLM_ROW_PAD = 256

    def mlm_loss(self, tokens: Optional[torch.Tensor],
                 attn_mask: Optional[torch.Tensor],
                 targets: torch.Tensor, packing=None) -> torch.Tensor:
        """Masked-LM loss (data.mlm.mlm_corrupt makes tokens and targets):
        mean cross-entropy of predicting targets at the positions where
        targets != -100, 0-d f32.  The decoder is the token embedding
        itself (tied weights, no bias, no transform), so the model has no
        parameter that only this loss uses; tok_emb.weight receives the sum
        of its embedding and decoder gradients.  Only the selected hidden
        rows reach the [rows, vocab] logits GEMM and
        ops.fused_cross_entropy.  Finding them reads the selection's size
        back from the device, one host sync per call."""
        h = self.encode(tokens, attn_mask, packing)
        flat_t = targets.reshape(-1)
        idx = torch.nonzero(flat_t != -100).flatten()
        t_sel = flat_t[idx]
        n_pad = -idx.numel() % self.MLM_ROW_PAD
        if n_pad:
            # position 0 is always there; its rows are ignored by the loss
            idx = torch.cat([idx, idx.new_zeros(n_pad)])
            t_sel = torch.cat([t_sel, t_sel.new_full((n_pad,), -100)])
        h_sel = h.reshape(-1, h.shape[-1]).index_select(0, idx)
        logits = F.linear(h_sel, self.tok_emb.weight)
        return ops.fused_cross_entropy(logits, t_sel)

    def set_pos_weights(self, weights: Dict[str, torch.Tensor]) -> None:
        """Per-class positive weights for the multi-label heads (label
        frequencies in the taxonomy are heavily imbalanced)."""
        for name, w in weights.items():
            self.register_buffer(f"_pw_{name}", w.float(), persistent=False)

    def set_loss_options(self, focal_gamma: Dict[str, float] = None,
                         label_smoothing: float = 0.0) -> None:
        """Per-head focal-BCE gamma (multilabel heads) + label smoothing —
        round-2 levers for the rare-class property head.
        """
        self._focal_gamma = dict(focal_gamma or {})
        self._label_smoothing = float(label_smoothing)

    def loss(self, logits: Dict[str, torch.Tensor],
             labels: Dict[str, torch.Tensor]) -> torch.Tensor:
        total = None
        gammas = getattr(self, "_focal_gamma", {})
        smooth = getattr(self, "_label_smoothing", 0.0)
        for name, lg in logits.items():
            if name not in labels:
                continue
            lg = lg.float()
            if name in MULTILABEL_HEADS:
                pw = getattr(self, f"_pw_{name}", None)
                y = labels[name].float()
                if smooth > 0:
                    y = y * (1.0 - smooth) + 0.5 * smooth
                gamma = gammas.get(name, 0.0)
                if gamma > 0:
                    # focal BCE: down-weight easy negatives/positives
                    bce = F.binary_cross_entropy_with_logits(
                        lg, y, pos_weight=pw, reduction="none")
                    p = torch.sigmoid(lg)
                    p_t = p * y + (1 - p) * (1 - y)
                    li = ((1 - p_t).clamp(min=1e-4) ** gamma * bce).mean()
                else:
                    li = F.binary_cross_entropy_with_logits(
                        lg, y, pos_weight=pw)
            else:
                li = F.cross_entropy(lg, labels[name],
                                     label_smoothing=smooth)
            total = li if total is None else total + li
        assert total is not None, "no labels matched any head"
        return total


def build_model(name_or_cfg, dtype=torch.bfloat16,
                fold_bias_grad: Optional[bool] = None) -> MLTC:
    cfg = CONFIGS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg
    model = MLTC(cfg, fold_bias_grad)
    return model.to(dtype)
