"""Masked-language-model corruption for self-supervised pretraining of the
MLTC encoder (MLTC.mlm_loss, Trainer.step_mlm).

BERT's recipe over the hashing tokenizer's ids: a fraction p of the real
tokens of a batch is selected; of the selected positions about 80 % become
MASK, about 10 % a random id, about 10 % stay; the model predicts the
original id at every selected position.

A position is maskable iff its id is >= N_RESERVED.  PAD and CLS are
reserved ids, so padded batches and packed batches (PackedBatch.tokens) are
handled alike and need no mask argument.
"""
from __future__ import annotations

from typing import Tuple

import torch

from tosem2021_amd.models.tokenizer import MASK, N_RESERVED

IGNORE = -100   # target of a position that is not predicted


def mlm_corrupt(tokens: torch.Tensor, p: float, seed: int, step: int,
                vocab_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """tokens: int64 of any shape -> (corrupted, targets), both of tokens'
    shape, dtype and device.

    Exactly k = max(1, round(p * n_maskable)) positions are selected (none
    when nothing is maskable), by a seeded permutation.  targets holds the
    original id at the selected positions and -100 elsewhere; corrupted
    differs from tokens at selected positions only.

    The result is a function of (tokens, p, seed, step) alone: every draw
    comes from a CPU generator seeded from (seed, step), whichever device
    tokens lives on, so a resumed run that passes its step counter draws
    the masks the uninterrupted run would have drawn."""
    if not 0.0 < p <= 1.0:
        raise ValueError(f"mlm_corrupt: p must be in (0, 1], got {p}")
    if vocab_size <= N_RESERVED:
        raise ValueError("vocab_size must exceed the reserved id range")
    flat = tokens.detach().reshape(-1).cpu()
    corrupted = flat.clone()
    targets = torch.full_like(flat, IGNORE)
    idx = torch.nonzero(flat >= N_RESERVED).flatten()
    n = int(idx.numel())
    if n > 0:
        g = torch.Generator()
        g.manual_seed((int(seed) * 0x9E3779B97F4A7C15 + int(step))
                      & 0x7FFFFFFFFFFFFFFF)
        k = max(1, round(p * n))
        sel = idx[torch.randperm(n, generator=g)[:k]]
        r = torch.rand(k, generator=g)
        rand_ids = torch.randint(N_RESERVED, vocab_size, (k,), generator=g)
        orig = flat[sel]
        targets[sel] = orig
        corrupted[sel] = torch.where(
            r < 0.8, torch.full_like(orig, MASK),
            torch.where(r < 0.9, rand_ids, orig))
    return (corrupted.view(tokens.shape).to(tokens.device),
            targets.view(tokens.shape).to(tokens.device))
