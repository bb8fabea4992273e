"""The definition `sf_kv_rope_shift` equals bit for bit, in torch on the host.

Attention scores depend on the temporal position only through pos_q - pos_k, so a session may subtract the same
`delta_frames` from every temporal position it still holds, provided the cached keys, which were stored rotated, are rotated
back by `delta_frames`.  Of a head's 64 complex pairs (columns 2j, 2j + 1) the temporal ones are j < 22, with angles from
table columns 0..21: the split of `sf_qkv_norm_rope_cache` (64 - 2 * (64 // 3), causal_model.py:32).  With
c = rope_cos[delta][j], s = rope_sin[delta][j] and (a, b) the stored pair read as float32:

    a' = bf16(fl(fl(a c) + fl(b s)))        b' = bf16(fl(fl(b c) - fl(a s)))

Every float32 operation is rounded on its own (no fused multiply-add), the bf16 rounding is round-to-nearest-even.  Nothing
else of a row changes.
"""
from __future__ import annotations

from typing import Optional

import torch

TEMPORAL_PAIRS = 22          # 64 - 2 * (64 // 3)
TEMPORAL_COLUMNS = 2 * TEMPORAL_PAIRS
MAX_DELTA = 1023             # the tables have 1024 rows


def shift_keys(k_cache: torch.Tensor, rope_cos: torch.Tensor, rope_sin: torch.Tensor, delta_frames: int, row0: int = 0,
               rows: Optional[int] = None) -> torch.Tensor:
    """k_cache bf16 [B, S, H, 128]; rope_cos / rope_sin float32 [1024, 64] (model.rope_tables) -> a new tensor in which
    rows [row0, row0 + rows) of every sample are rotated back by `delta_frames`.  Runs wherever the tensors are; the
    elementwise float32 products and sums of torch are rounded one by one on every backend."""
    if k_cache.dtype != torch.bfloat16 or k_cache.dim() != 4 or k_cache.shape[3] != 128:
        raise ValueError(f"k_cache must be bf16 [B, S, H, 128], got {tuple(k_cache.shape)} {k_cache.dtype}")
    if not 1 <= delta_frames <= MAX_DELTA:
        raise ValueError(f"delta_frames must be in 1..{MAX_DELTA}, got {delta_frames}")
    S = k_cache.shape[1]
    rows = S - row0 if rows is None else rows
    if row0 < 0 or rows < 0 or row0 + rows > S:
        raise ValueError(f"rows [{row0}, {row0} + {rows}) lie outside the cache of {S}")
    out = k_cache.clone()
    part = k_cache[:, row0:row0 + rows, :, :TEMPORAL_COLUMNS].to(torch.float32)
    a, b = part[..., 0::2], part[..., 1::2]
    c = rope_cos[delta_frames, :TEMPORAL_PAIRS].to(device=a.device, dtype=torch.float32)
    s = rope_sin[delta_frames, :TEMPORAL_PAIRS].to(device=a.device, dtype=torch.float32)
    ac, bs, bc, as_ = a * c, b * s, b * c, a * s
    new = torch.stack((ac + bs, bc - as_), dim=-1).flatten(-2)
    out[:, row0:row0 + rows, :, :TEMPORAL_COLUMNS] = new.to(torch.bfloat16)
    return out
