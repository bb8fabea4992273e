"""Plain-torch restatement of `CLIPModel.visual` (wan/modules/clip.py:527-542): preprocessing plus the vision tower with
`use_31_block=True`, written from the maths.  TEST INFRASTRUCTURE like `jpeg_reference.py`: the comparison target of the
GPU encoder at shapes that have no recorded fixture, itself pinned to the reference's recorded outputs by
tests/test_clip_host.py.  Runs on the CPU (or wherever its inputs live); the product never calls it.

Dtype policies:
  "fp32"           every operation in float32.
  "autocast_bf16"  the rounding points of the reference under `torch.autocast(dtype=torch.bfloat16)`: every matrix product
                   (patch convolution, to_qkv, proj, mlp.0, mlp.2) takes bf16 operands and a bf16 bias, accumulates in
                   fp32 and rounds its result to bf16; attention takes those bf16 q, k, v, keeps scores and softmax in fp32,
                   rounds the probabilities to bf16 in front of P.V and its output to bf16; GELU (erf form) is evaluated
                   in fp32 on a bf16 input and rounded to bf16; the layer norms and the RESIDUAL STREAM stay fp32
                   (`LayerNorm.forward` does `x.float()`, and bf16 sub-layer outputs are added into an fp32 `x`).
`residual="bf16"` additionally rounds the stream after every add -- what a bf16-to-bf16 residual kernel would compute; it
exists to measure what the fp32 stream buys.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn.functional as F

from .clip_weights import CLIP_MEAN, CLIP_STD, ClipVisionShape, visual_state_dict

Tensor = torch.Tensor
POLICIES = ("fp32", "autocast_bf16")


def clip_preprocess(videos: Sequence[Tensor], image_size: int) -> Tensor:
    """List of [3, T, H, W] in [-1, 1] -> [sum T, 3, image_size, image_size] float32: bicubic resize (align_corners=False,
    A = -0.75, no antialiasing, overshoot kept), then (v/2 + 1/2 - mean) / std."""
    frames = torch.cat([F.interpolate(u.transpose(0, 1).float(), size=(image_size, image_size), mode="bicubic", align_corners=False)
                        for u in videos])
    mean = torch.tensor(CLIP_MEAN, device=frames.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, device=frames.device).view(1, 3, 1, 1)
    return (frames * 0.5 + 0.5 - mean) / std


def patch_rows(frames: Tensor, patch: int, kp: int) -> Tensor:
    """[n, 3, S, S] -> [n * (S/patch)^2, kp]: row = (frame, patch row-major), column k = (c*patch + i)*patch + j, zero pad."""
    n, c, S, _ = frames.shape
    g = S // patch
    rows = frames.reshape(n, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, c * patch * patch)
    return F.pad(rows, (0, kp - rows.shape[1]))


def _r(t: Tensor) -> Tensor:
    return t.to(torch.bfloat16).float()


def clip_visual_reference(state_dict: Dict[str, Tensor], shape: ClipVisionShape, videos: Sequence[Tensor],
                          policy: str = "fp32", residual: str = "fp32") -> Tensor:
    """`CLIPModel.visual(videos)` -> float32 [sum T, seq_len, dim]."""
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {POLICIES}")
    s = shape
    sd = {k: v.float() for k, v in visual_state_dict(state_dict, s).items()}
    low = policy == "autocast_bf16"
    r = _r if low else (lambda t: t)
    rs = _r if (low and residual == "bf16") else (lambda t: t)

    def linear(x, name):
        return r(F.linear(r(x), r(sd[name + ".weight"]), r(sd[name + ".bias"])))

    def norm(x, name):
        return F.layer_norm(x, (s.dim,), sd[name + ".weight"], sd[name + ".bias"], s.eps)

    frames = clip_preprocess(videos, s.image_size)
    n = frames.shape[0]
    rows = patch_rows(frames, s.patch_size, s.patch_k)
    x = r(r(rows) @ r(sd["patch_embedding.weight"].reshape(s.dim, -1)).t()).reshape(n, s.num_patches, s.dim)
    x = torch.cat([sd["cls_embedding"].expand(n, -1, -1), x], 1) + sd["pos_embedding"]
    x = rs(norm(x, "pre_norm"))
    scale = s.head_dim ** -0.5
    for i in range(s.layers_built):
        p = f"transformer.{i}."
        qkv = linear(norm(x, p + "norm1"), p + "attn.to_qkv").view(n, s.seq_len, 3, s.num_heads, s.head_dim)
        q, k, v = (t.transpose(1, 2) for t in qkv.unbind(2))                       # [n, H, L, d]
        prob = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
        attn = r(r(prob) @ v).transpose(1, 2).reshape(n, s.seq_len, s.dim)
        x = rs(x + linear(attn, p + "attn.proj"))
        h = r(F.gelu(linear(norm(x, p + "norm2"), p + "mlp.0")))
        x = rs(x + linear(h, p + "mlp.2"))
    return x
