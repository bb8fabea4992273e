"""Shape description and weight handling of the CLIP image encoder (frames -> `clip_feature` [n, 257, 1280]).

Key names are those of the reference's `XLMRobertaCLIP.state_dict()` (wan/modules/clip.py:328-404), i.e. of
`models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth`: the vision tower lives under `visual.`.  `CLIPModel.visual`
runs it with `use_31_block=True` (clip.py:541, :295-297): the last transformer block, `post_norm` and `head` never run, so
they are checked for shape when present but never uploaded; `textual.*` and `log_scale` are ignored.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Dict, Tuple

import torch

Tensor = torch.Tensor

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # clip.py:457-458
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PREFIX = "visual."


@dataclass(frozen=True)
class ClipVisionShape:
    """Vision-tower arguments of `clip_xlm_roberta_vit_h_14` (clip.py:471-498): pool_type 'token', pre_norm, exact GELU."""
    image_size: int = 224
    patch_size: int = 14
    dim: int = 1280
    num_heads: int = 16
    num_layers: int = 32
    mlp_ratio: int = 4
    out_dim: int = 1024
    eps: float = 1e-5

    @property
    def head_dim(self) -> int:
        return self.dim // self.num_heads

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid * self.grid

    @property
    def seq_len(self) -> int:
        return self.num_patches + 1

    @property
    def mlp_dim(self) -> int:
        return self.dim * self.mlp_ratio

    @property
    def layers_built(self) -> int:
        """`use_31_block`: every block but the last."""
        return self.num_layers - 1

    @property
    def patch_k(self) -> int:
        return 3 * self.patch_size * self.patch_size

    @property
    def patch_kp(self) -> int:
        """Row length of the patch rows and of the repacked patch weight: `patch_k` rounded up to the GEMM's k-tile of 64."""
        return (self.patch_k + 63) // 64 * 64

    def as_dict(self) -> dict:
        return asdict(self)


CLIP_VIT_H_14 = ClipVisionShape()
# reduced tower for the parity fixtures: the head dimension stays 80, the patch 14
CLIP_REDUCED = ClipVisionShape(dim=320, num_heads=4, num_layers=3, out_dim=64)


def clip_param_shapes(s: ClipVisionShape) -> Dict[str, Tuple[int, ...]]:
    """`VisionTransformer.state_dict()` in its own order, under `visual.`."""
    out: Dict[str, Tuple[int, ...]] = {
        "cls_embedding": (1, 1, s.dim),
        "pos_embedding": (1, s.seq_len, s.dim),
        "head": (s.dim, s.out_dim),
        "patch_embedding.weight": (s.dim, 3, s.patch_size, s.patch_size),
        "pre_norm.weight": (s.dim,),
        "pre_norm.bias": (s.dim,),
    }
    for i in range(s.num_layers):
        p = f"transformer.{i}."
        out[p + "norm1.weight"] = (s.dim,)
        out[p + "norm1.bias"] = (s.dim,)
        out[p + "attn.to_qkv.weight"] = (3 * s.dim, s.dim)
        out[p + "attn.to_qkv.bias"] = (3 * s.dim,)
        out[p + "attn.proj.weight"] = (s.dim, s.dim)
        out[p + "attn.proj.bias"] = (s.dim,)
        out[p + "norm2.weight"] = (s.dim,)
        out[p + "norm2.bias"] = (s.dim,)
        out[p + "mlp.0.weight"] = (s.mlp_dim, s.dim)
        out[p + "mlp.0.bias"] = (s.mlp_dim,)
        out[p + "mlp.2.weight"] = (s.dim, s.mlp_dim)
        out[p + "mlp.2.bias"] = (s.dim,)
    out["post_norm.weight"] = (s.dim,)
    out["post_norm.bias"] = (s.dim,)
    return {PREFIX + k: v for k, v in out.items()}


def never_run(name: str, s: ClipVisionShape) -> bool:
    """Tensors of the vision tower that `use_31_block` leaves unused (bare or prefixed name)."""
    name = name[len(PREFIX):] if name.startswith(PREFIX) else name
    return name == "head" or name.startswith("post_norm.") or name.startswith(f"transformer.{s.num_layers - 1}.")


def needed_param_shapes(s: ClipVisionShape) -> Dict[str, Tuple[int, ...]]:
    """The tensors the encoder uploads, bare names."""
    return {k[len(PREFIX):]: v for k, v in clip_param_shapes(s).items() if not never_run(k, s)}


def visual_state_dict(sd: Dict[str, Tensor], s: ClipVisionShape) -> Dict[str, Tensor]:
    """The vision tower's tensors under bare names, from the full checkpoint (`visual.*`, `textual.*`, `log_scale`) or from a
    dict of bare names.  KeyError naming an absent tensor the encoder needs; ValueError for a wrong shape (also of a
    never-run tensor, when it is present)."""
    if any(k.startswith(PREFIX) for k in sd):
        sd = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
    out: Dict[str, Tensor] = {}
    for name, shp in clip_param_shapes(s).items():
        bare = name[len(PREFIX):]
        if bare not in sd:
            if never_run(bare, s):
                continue
            raise KeyError(f"CLIP state dict lacks {name!r} (the vision tower needs every tensor but the last block, post_norm and head)")
        if tuple(sd[bare].shape) != tuple(shp):
            raise ValueError(f"{name}: expected shape {shp}, got {tuple(sd[bare].shape)}")
        out[bare] = sd[bare]
    return out


def repack_patch_weight(w: Tensor, kp: int) -> Tensor:
    """`patch_embedding.weight` [dim, 3, p, p] -> [dim, kp]: column k = (c*p + i)*p + j as the patch rows of
    `sf_clip_preprocess` are laid out, the pad columns zero -- the stride-p convolution becomes one GEMM."""
    dim = w.shape[0]
    flat = w.reshape(dim, -1)
    if flat.shape[1] > kp:
        raise ValueError(f"patch weight has {flat.shape[1]} columns, more than kp={kp}")
    out = torch.zeros(dim, kp, dtype=w.dtype)
    out[:, :flat.shape[1]] = flat
    return out


def synth_clip_state_dict(s: ClipVisionShape, seed: int = 0, dtype=torch.float32) -> Dict[str, Tensor]:
    """Seeded random vision-tower weights on the CPU under `visual.` names, drawn tensor by tensor in `clip_param_shapes`
    order (one fp32 tensor at a time is alive before its cast to `dtype`).  Matrices ~ N(0, 1/fan_in), biases ~ N(0, .02),
    norm weights ~ 1 + N(0, .1) with biases ~ N(0, .1) (the reference's ones / zeros would leave the affine part untested),
    the embeddings ~ N(0, 1/dim) as clip.py:247-258.  Norms and embeddings stay fp32 whatever `dtype` is."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd: Dict[str, Tensor] = {}
    for name, shape in clip_param_shapes(s).items():
        t = torch.randn(shape, generator=g)
        if "norm" in name:
            t = (1.0 + 0.1 * t) if name.endswith("weight") else 0.1 * t
        elif name.endswith("embedding") or name.endswith("head"):
            t = t * s.dim ** -0.5
        elif name.endswith("bias"):
            t = (0.02 * t).to(dtype)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = (t * fan_in ** -0.5).to(dtype)
        sd[name] = t
    return sd


def synth_frames(seed: int, n: int, height: int, width: int) -> Tensor:
    """Seeded test frames [3, n, height, width] in [-1, 1] (the `[3, T, H, W]` form `CLIPModel.visual` takes)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(3, n, height, width, generator=g) * 2.0 - 1.0
