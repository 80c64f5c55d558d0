"""Sequence packing: several short examples share one fixed-length row.

The classifier's inputs are short (median ~31 tokens against a 256-token
row), so a padded batch is mostly PAD.  A packed batch lays examples end to
end in rows of `row_len` tokens; per-position segment ids keep them apart in
attention (ops.flash_attention*(seg=...)), positions restart per example,
and ops.segment_mean_pool pools per example.  Per-segment results come back
in segment order; PackedBatch.unpermute restores the input order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import torch

from tosem2021_amd import ops


def pack_lengths(lengths: Sequence[int], row_len: int) -> List[List[int]]:
    """First-fit-decreasing bin packing of `lengths` into rows of `row_len`.

    Returns the rows as lists of example indices, in placement order.
    Deterministic: examples are placed longest first, ties by original
    index, each into the first row it fits.  Lengths above row_len count as
    row_len (the packer truncates such examples)."""
    if row_len <= 0:
        raise ValueError("row_len must be positive")
    lens = [min(int(n), row_len) for n in lengths]
    if any(n < 1 for n in lens):
        raise ValueError("every example needs at least one token")
    order = sorted(range(len(lens)), key=lambda i: (-lens[i], i))
    rows: List[List[int]] = []
    free: List[int] = []
    for i in order:
        for r, room in enumerate(free):
            if lens[i] <= room:
                rows[r].append(i)
                free[r] -= lens[i]
                break
        else:
            rows.append([i])
            free.append(row_len - lens[i])
    return rows


@dataclass
class PackedBatch:
    """One packed batch of N examples in R rows.

    tokens    [R, row_len] int64   token ids, pad_id in the tail
    seg       [R, row_len] int32   segment id per position: 0, 1, ... in
                                   row order; the padding tail carries one
                                   id above the row's last real id
    pos       [R, row_len] int64   position within the example (restarts
                                   at 0 in every segment; 0 at padding)
    seg_start [N] int32            first flattened position of segment n
    seg_len   [N] int32            its length
    pos2seg   [R*row_len] int32    segment of every flattened position,
                                   -1 at padding
    order     [N] int64            original example index of segment n
    """
    tokens: torch.Tensor
    seg: torch.Tensor
    pos: torch.Tensor
    seg_start: torch.Tensor
    seg_len: torch.Tensor
    pos2seg: torch.Tensor
    order: torch.Tensor

    @property
    def n_segments(self) -> int:
        return int(self.order.shape[0])

    @property
    def n_positions(self) -> int:
        return int(self.tokens.numel())

    def to(self, device) -> "PackedBatch":
        return PackedBatch(*(getattr(self, f).to(device) for f in (
            "tokens", "seg", "pos", "seg_start", "seg_len", "pos2seg",
            "order")))

    def unpermute(self, x: torch.Tensor) -> torch.Tensor:
        """Per-segment results x [N, ...] -> the examples' input order."""
        out = torch.empty_like(x)
        out[self.order.to(x.device)] = x
        return out

    def gather(self, x: torch.Tensor) -> torch.Tensor:
        """Per-example values x [N, ...] in input order -> segment order."""
        return x[self.order.to(x.device)]


def pack_examples(examples: Sequence[Sequence[int]], row_len: int,
                  pad_id: int = 0) -> PackedBatch:
    """Pack token-id lists into a PackedBatch (on the CPU).

    row_len must be a multiple of 64 (the flash kernels' row granularity);
    an example longer than row_len is truncated to it."""
    if row_len % 64 != 0:
        raise ValueError("row_len must be a multiple of 64")
    examples = [list(e)[:row_len] for e in examples]
    rows = pack_lengths([len(e) for e in examples], row_len)
    R, N = len(rows), len(examples)
    tokens = torch.full((R, row_len), pad_id, dtype=torch.long)
    seg = torch.zeros(R, row_len, dtype=torch.int32)
    pos = torch.zeros(R, row_len, dtype=torch.long)
    pos2seg = torch.full((R * row_len,), -1, dtype=torch.int32)
    seg_start = torch.zeros(N, dtype=torch.int32)
    seg_len = torch.zeros(N, dtype=torch.int32)
    order = torch.zeros(N, dtype=torch.long)
    n = 0
    for r, members in enumerate(rows):
        at = 0
        for s, i in enumerate(members):
            ids = examples[i]
            k = len(ids)
            tokens[r, at:at + k] = torch.tensor(ids, dtype=torch.long)
            seg[r, at:at + k] = s
            pos[r, at:at + k] = torch.arange(k)
            pos2seg[r * row_len + at:r * row_len + at + k] = n
            seg_start[n] = r * row_len + at
            seg_len[n] = k
            order[n] = i
            at += k
            n += 1
        seg[r, at:] = len(members)      # padding: its own trailing segment
    ops.check_segments(seg)
    return PackedBatch(tokens, seg, pos, seg_start, seg_len, pos2seg, order)
