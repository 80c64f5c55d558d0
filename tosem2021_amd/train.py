"""Trainer for the MLTC classifier: flat bf16 parameters, fused AdamW,
bucketed-allreduce DP, checkpoint/resume, metrics and tracing.

Memory layout (MI355X-first): every parameter is a view into ONE contiguous
bf16 buffer; gradients accumulate into a matching flat bf16 buffer; the
optimizer keeps flat f32 master/m/v.  One fused kernel performs the whole
AdamW step (csrc/adamw.hip); DP reduces the flat grad buffer in large
buckets over RCCL/xGMI (parallel/ddp.py).

Capability parity: checkpoint/resume mirrors the corpus patterns the study
measured (DeepSpeech util/checkpoints.py:126,140; nni recoverable.py) —
atomic save, load-or-init, resume from step.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from tosem2021_amd import ops
from tosem2021_amd.data.packing import PackedBatch
from tosem2021_amd.models import MLTCConfig, build_model
from tosem2021_amd.ops.reference import ema_decay_at
from tosem2021_amd.parallel.ddp import BucketedAllReduce
from tosem2021_amd.utils.metrics import get_metrics
from tosem2021_amd.utils.trace import trace

PAD_ELEMS = 512  # flat buffers padded so the fused AdamW's 4-wide loop is exact


class FlatParams:
    """Flatten a model's parameters into contiguous training state."""

    def __init__(self, model: torch.nn.Module):
        params = [p for p in model.parameters() if p.requires_grad]
        total = sum(p.numel() for p in params)
        padded = (total + PAD_ELEMS - 1) // PAD_ELEMS * PAD_ELEMS
        device = params[0].device
        dtype = params[0].dtype
        self.flat = torch.zeros(padded, dtype=dtype, device=device)
        self.grad_flat = torch.zeros(padded, dtype=dtype, device=device)
        self.offsets: List[int] = []
        off = 0
        for p in params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view(p.shape)
            p.grad = self.grad_flat[off:off + n].view(p.shape)
            # the parameter keeps its own version counter: code that must
            # notice writes through the flat buffer (MLTC.quantize_mx)
            # reads the owner's
            p._flat_owner = self.flat
            self.offsets.append(off)
            off += n
        self.params = params
        self.numel = total
        self.padded = padded
        # f32 optimizer state
        self.master = self.flat.detach().clone().float()
        self.m = torch.zeros(padded, dtype=torch.float32, device=device)
        self.v = torch.zeros(padded, dtype=torch.float32, device=device)
        # f32 weight average, allocated by Trainer when cfg.ema_decay > 0
        self.ema: Optional[torch.Tensor] = None

    def zero_grad(self):
        self.grad_flat.zero_()


def param_depth(name: str, n_layers: int) -> int:
    """Layer-wise LR decay depth of a parameter by its name: the embeddings
    0, blocks.i.* i + 1, everything above the blocks (ln_f, heads.*)
    n_layers + 1."""
    if name.startswith(("tok_emb.", "pos_emb.")):
        return 0
    if name.startswith("blocks."):
        return int(name.split(".")[1]) + 1
    return n_layers + 1


def param_group_table(model: torch.nn.Module, n_layers: int, padded: int, *,
                      weight_decay: float, no_decay_1d: bool = False,
                      layer_decay: float = 1.0):
    """The segment table of ops.adamw_step_grouped for `model`'s parameters
    in FlatParams' order, as host lists (seg_end, seg_lr_mult, seg_wd).

    A parameter gets lr_mult = layer_decay ** (n_layers + 1 - depth)
    (param_depth) and wd = 0 if no_decay_1d and it is 1-D, else weight_decay.
    Neighbours with equal (lr_mult, wd) share a segment, and the padding
    tail up to `padded` joins the last one."""
    ends: List[int] = []
    mults: List[float] = []
    wds: List[float] = []
    off = 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        off += p.numel()
        mult = float(layer_decay) ** (n_layers + 1 - param_depth(name, n_layers))
        wd = 0.0 if no_decay_1d and p.dim() == 1 else float(weight_decay)
        if ends and (mults[-1], wds[-1]) == (mult, wd):
            ends[-1] = off
        else:
            ends.append(off)
            mults.append(mult)
            wds.append(wd)
    ends[-1] = padded
    return ends, mults, wds


@dataclass
class TrainConfig:
    model: str = "mltc-base"
    lr: float = 3e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    weight_decay: float = 0.01
    warmup_steps: int = 100
    total_steps: int = 10000
    bucket_mb: int = 64
    dtype: str = "bf16"  # "bf16" | "f32" (f32: CPU/gloo tests)
    ckpt_dir: Optional[str] = None
    ckpt_every: int = 0          # 0 = only on explicit save()
    ckpt_keep: int = 3           # retain the newest k checkpoints (0 = all)
    # global-norm gradient clipping + non-finite step skipping; 0 = off
    max_grad_norm: float = 0.0
    # parameter groups inside the fused AdamW step (param_group_table); with
    # both at their defaults the step is the ungrouped kernel
    no_decay_1d: bool = False    # no weight decay on 1-D parameters
    layer_decay: float = 1.0     # layer-wise LR decay factor, in (0, 1]
    # exponential moving average of the f32 master weights, kept by the fused
    # AdamW kernel (+4 B per parameter); in [0, 1), 0 = off.  The decay of
    # applied update t is ops.reference.ema_decay_at(ema_decay, t).
    ema_decay: float = 0.0

    def __post_init__(self):
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(
                f"ema_decay must be in [0, 1), got {self.ema_decay}")
        if not 0.0 < self.layer_decay <= 1.0:
            raise ValueError(
                f"layer_decay must be in (0, 1], got {self.layer_decay}")


class Trainer:
    def __init__(self, cfg: TrainConfig, device: Optional[torch.device] = None,
                 model_cfg: Optional[MLTCConfig] = None):
        self.cfg = cfg
        self.device = device or (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        dtype = torch.bfloat16 if cfg.dtype == "bf16" else torch.float32
        model = build_model(model_cfg if model_cfg is not None else cfg.model,
                            dtype=dtype)
        self.model = model.to(self.device)
        self.flat = FlatParams(self.model)
        self.ddp = BucketedAllReduce(self.flat.params, self.flat.grad_flat,
                                     self.flat.offsets,
                                     bucket_bytes=cfg.bucket_mb << 20)
        if self.ddp.enabled:
            # rank-0 init everywhere: broadcast the flat params once
            dist.broadcast(self.flat.flat, src=0)
            self.flat.master.copy_(self.flat.flat.float())
            # fused dropout: every rank draws its own masks
            self.model.dropout_rank = dist.get_rank()
        self.step_num = 0     # attempted steps: LR schedule, checkpoint names
        self.opt_step = 0     # applied updates: AdamW's bias correction
        self.skipped_steps = 0
        self.metrics: Dict[str, float] = {}
        self._clip_state: Optional[torch.Tensor] = None
        # parameter groups: a function of the config alone, so every rank
        # and a resumed run derive the same table; uploaded once
        self._seg_table = None
        if cfg.no_decay_1d or cfg.layer_decay != 1.0:
            self._seg_table = ops.segment_table(
                *param_group_table(self.model, self.model.cfg.n_layers,
                                   self.flat.padded,
                                   weight_decay=cfg.weight_decay,
                                   no_decay_1d=cfg.no_decay_1d,
                                   layer_decay=cfg.layer_decay),
                self.flat.padded, device=self.device)
        if cfg.ema_decay > 0:
            self.reset_ema()

    # ---- weight average -----------------------------------------------------
    def reset_ema(self):
        """(Re-)seed the weight average from the current master weights, e.g.
        after a warm start copied other weights into the model."""
        if not self.cfg.ema_decay > 0:
            raise RuntimeError("reset_ema() needs TrainConfig.ema_decay > 0")
        f = self.flat
        if f.ema is None:
            f.ema = f.master.detach().clone()
        else:
            f.ema.copy_(f.master)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model's flat parameters hold the weight
        average cast to the parameter dtype; on exit the previous flat buffer
        comes back bit for bit.  Touches neither master nor model.training."""
        f = self.flat
        if f.ema is None:
            raise RuntimeError("ema_weights() needs TrainConfig.ema_decay > 0")
        saved = f.flat.detach().clone()
        f.flat.copy_(f.ema)
        try:
            yield self.model
        finally:
            f.flat.copy_(saved)

    # ---- schedule -----------------------------------------------------------
    def _lr(self) -> float:
        s, c = self.step_num, self.cfg
        if s < c.warmup_steps:
            return c.lr * (s + 1) / max(c.warmup_steps, 1)
        t = (s - c.warmup_steps) / max(c.total_steps - c.warmup_steps, 1)
        return c.lr * 0.5 * (1.0 + math.cos(math.pi * min(t, 1.0)))

    def _forward(self, tokens, attn_mask):
        """tokens is a [B, L] tensor (with its optional attn_mask) or a
        data.packing.PackedBatch (attn_mask None; logits in segment order)."""
        if isinstance(tokens, PackedBatch):
            return self.model(tokens.tokens, attn_mask, packing=tokens)
        return self.model(tokens, attn_mask)

    # ---- optimizer ------------------------------------------------------------
    def _adamw(self, lr: float, grad_scale: float):
        """Launch the fused AdamW step; nothing here syncs with the host.

        With cfg.max_grad_norm > 0 the global norm of the averaged gradient
        is reduced on the device (ops.grad_clip_state) and the clip factor
        folds into the kernel's grad scale; a non-finite gradient makes the
        kernel leave every buffer untouched.  _finish_step() reads the
        outcome back where the step syncs anyway.

        With cfg.no_decay_1d or cfg.layer_decay != 1 the same step runs
        through the grouped entry points: lr is still the scheduled base
        rate, and the per-segment multiplier and weight decay come from the
        table built at construction.  The norm and the clip are global
        either way.

        With cfg.ema_decay > 0 whichever entry point is picked also updates
        the weight average.  opt_step is exact here, since _finish_step() has
        synced the previous step, so a skipped step advances neither the
        average (the kernel leaves it alone) nor its warm-up count."""
        f, c = self.flat, self.cfg
        hp = dict(lr=lr, beta1=c.beta1, beta2=c.beta2, eps=c.eps,
                  step=self.opt_step + 1)
        if f.ema is not None:
            hp.update(ema=f.ema,
                      ema_decay=ema_decay_at(c.ema_decay, self.opt_step + 1))
        bufs = (f.flat, f.grad_flat, f.m, f.v, f.master)
        if c.max_grad_norm > 0:
            self._clip_state = ops.grad_clip_state(
                f.grad_flat, grad_scale=grad_scale, max_norm=c.max_grad_norm)
            if self._seg_table is not None:
                ops.adamw_step_grouped_clipped(
                    *bufs, *self._seg_table, clip_state=self._clip_state,
                    **hp)
            else:
                ops.adamw_step_clipped(*bufs, clip_state=self._clip_state,
                                       wd=c.weight_decay, **hp)
        elif self._seg_table is not None:
            ops.adamw_step_grouped(*bufs, *self._seg_table,
                                   grad_scale=grad_scale, **hp)
        else:
            ops.adamw_step(*bufs, grad_scale=grad_scale,
                           wd=c.weight_decay, **hp)
        # the fused steps write through raw pointers: no version counter sees
        # them, so count the write here (no kernel, no sync)
        torch.autograd.graph.increment_version(f.flat)

    def _finish_step(self) -> dict:
        """Count the step as applied or skipped; returns the extra
        observe_step fields (none with clipping off).  Every rank reduces
        the same all-reduced gradient, so all ranks agree on the outcome."""
        if self._clip_state is None:
            self.opt_step += 1
            return {}
        norm, _, finite, _ = self._clip_state.tolist()   # the step's one sync
        self._clip_state = None
        skipped = finite == 0.0
        if skipped:
            self.skipped_steps += 1
        else:
            self.opt_step += 1
        self.metrics["grad_norm"] = norm
        return {"grad_norm": norm, "skipped": skipped}

    # ---- one optimization step ----------------------------------------------
    def step_accum(self, micro_batches) -> float:
        """One optimizer step over several micro-batches (gradient
        accumulation): collectives fire only on the last micro-backward,
        and the 1/n_micro mean folds into the AdamW grad scale.  A
        micro-batch is (tokens, attn_mask, labels) or, packed,
        (PackedBatch, None, labels in segment order)."""
        micro_batches = list(micro_batches)
        n = len(micro_batches)
        with trace("train_step_accum", step=self.step_num + 1, micro=n):
            self.flat.zero_grad()
            total_loss = 0.0
            for i, (tokens, attn_mask, labels) in enumerate(micro_batches):
                self.ddp.sync = (i == n - 1)
                logits = self._forward(tokens, attn_mask)
                loss = self.model.loss(logits, labels)
                loss.backward()
                total_loss += float(loss.detach())
            self.ddp.sync = True
            self.ddp.finalize()
            self.step_num += 1
            lr = self._lr()
            self._adamw(lr, self.ddp.grad_scale / n)
        get_metrics().observe_step(self.step_num, loss=total_loss / n, lr=lr,
                                   **self._finish_step())
        return total_loss / n

    def step(self, tokens, attn_mask: Optional[torch.Tensor],
             labels: Dict[str, torch.Tensor]) -> float:
        """tokens: [B, L] tensor, or a PackedBatch with attn_mask None and
        the labels in segment order (TaxonomyDataset.packed_batches)."""
        return self._step(
            lambda: self.model.loss(self._forward(tokens, attn_mask), labels))

    def step_mlm(self, tokens, attn_mask: Optional[torch.Tensor],
                 targets: torch.Tensor) -> float:
        """One masked-LM pretraining step (MLTC.mlm_loss): tokens is the
        corrupted [B, L] batch, or a PackedBatch whose .tokens are corrupted
        (attn_mask None); targets has the tokens' shape, -100 where nothing
        is predicted (data.mlm.mlm_corrupt).  The classification heads get
        no gradient in such a step; ddp.finalize reduces their buckets all
        the same, so the ranks stay in step."""
        if isinstance(tokens, PackedBatch):
            return self._step(lambda: self.model.mlm_loss(
                tokens.tokens, attn_mask, targets, packing=tokens))
        return self._step(
            lambda: self.model.mlm_loss(tokens, attn_mask, targets))

    def _step(self, loss_fn) -> float:
        """zero_grad, loss_fn() -> scalar loss, backward, all-reduce, AdamW,
        bookkeeping: the body step and step_mlm share."""
        with trace("train_step", step=self.step_num + 1):
            self.flat.zero_grad()
            loss = loss_fn()
            loss.backward()
            self.ddp.finalize()
            self.step_num += 1
            lr = self._lr()
            self._adamw(lr, self.ddp.grad_scale)
        get_metrics().observe_step(self.step_num, loss=float(loss.detach()),
                                   lr=lr, **self._finish_step())
        if self.cfg.ckpt_every and self.cfg.ckpt_dir and \
                self.step_num % self.cfg.ckpt_every == 0:
            self.save()
        return float(loss.detach())

    # ---- checkpoint / resume -------------------------------------------------
    def state_dict(self) -> dict:
        sd = self._state_dict()
        if self.flat.ema is not None:
            sd["ema"] = self.flat.ema
        return sd

    def _state_dict(self) -> dict:
        return {
            "step": self.step_num,
            "opt_step": self.opt_step,
            "skipped_steps": self.skipped_steps,
            # the fused dropout's call counter: with it a resumed run draws
            # the masks the uninterrupted run would have drawn
            "dropout_call": self.model.dropout_call,
            "flat": self.flat.flat,
            "master": self.flat.master,
            "m": self.flat.m,
            "v": self.flat.v,
            "model": self.cfg.model,
        }

    def save(self, path: Optional[str] = None) -> str:
        assert path or self.cfg.ckpt_dir, "no checkpoint path configured"
        if path is None:
            path = os.path.join(self.cfg.ckpt_dir, f"ckpt_{self.step_num:08d}.pt")
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        tmp = path + ".tmp"
        torch.save(self.state_dict(), tmp)
        os.replace(tmp, path)  # atomic publish (DeepSpeech-style durable ckpt)
        self._prune(os.path.dirname(path))
        return path

    def _prune(self, ckpt_dir: str):
        """Keep the newest cfg.ckpt_keep checkpoints (tune checkpoint_manager
        style retention)."""
        k = self.cfg.ckpt_keep
        if not k or not ckpt_dir:
            return
        cks = sorted(f for f in os.listdir(ckpt_dir)
                     if f.startswith("ckpt_") and f.endswith(".pt"))
        for f in cks[:-k]:
            try:
                os.remove(os.path.join(ckpt_dir, f))
            except OSError:
                pass

    def load(self, path: str):
        sd = torch.load(path, map_location=self.device, weights_only=True)
        self.flat.flat.copy_(sd["flat"])
        self.flat.master.copy_(sd["master"])
        self.flat.m.copy_(sd["m"])
        self.flat.v.copy_(sd["v"])
        if self.flat.ema is not None:
            # a checkpoint from a run without the average starts it here
            self.flat.ema.copy_(sd["ema"] if "ema" in sd else sd["master"])
        self.step_num = sd["step"]
        # checkpoints from before step skipping applied every step
        self.opt_step = sd.get("opt_step", sd["step"])
        self.skipped_steps = sd.get("skipped_steps", 0)
        self.model.dropout_call = sd.get("dropout_call", 0)

    @staticmethod
    def latest_checkpoint(ckpt_dir: str) -> Optional[str]:
        if not os.path.isdir(ckpt_dir):
            return None
        cks = sorted(f for f in os.listdir(ckpt_dir)
                     if f.startswith("ckpt_") and f.endswith(".pt"))
        return os.path.join(ckpt_dir, cks[-1]) if cks else None

    def load_or_init(self) -> bool:
        """nni-recoverable-style resume: load the newest checkpoint if any."""
        if not self.cfg.ckpt_dir:
            return False
        path = self.latest_checkpoint(self.cfg.ckpt_dir)
        if path:
            self.load(path)
            return True
        return False
