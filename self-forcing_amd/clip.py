"""CLIP image encoder on the GPU behind the reference's `CLIPModel` surface (wan/modules/clip.py:501-542).

    clip = CLIPModel(dtype=torch.bfloat16, device="cuda", checkpoint_path=".../models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth")
    feat = clip.visual([video])          # video [3, T, H, W] in [-1, 1]  ->  float32 [T, 257, 1280]

`visual` is ONE C call (`sf_clip_encode`, csrc/clip_encoder.hip): bicubic resize to 224 x 224 and CLIP normalisation straight
into bf16 patch rows, the patch embedding as a GEMM, and the ViT-H/14 tower with `use_31_block=True` -- bf16 MFMA GEMMs
around an fp32 residual stream, attention at head dimension 80 and the erf GELU.  There is no eager/CPU fallback.  Only the
vision tower exists here: the text tower (`textual.*`), `visual.head`, `visual.post_norm` and the last transformer block are
never uploaded (`use_31_block` skips them), and `pos_interpolate` (`interpolation=True`) is not built.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib, torch_ops
from .clip_weights import CLIP_VIT_H_14, ClipVisionShape, repack_patch_weight, visual_state_dict
from .device_model import DeviceModel

Tensor = torch.Tensor


class CLIPVisionEncoder(DeviceModel):
    """Device-resident vision-tower weights + the C model descriptor (counterpart of `VisionTransformer`, clip.py:209-300).
    Matrices and their biases are bf16 (what autocast feeds the reference's GEMMs); the norms, `cls_embedding` and
    `pos_embedding` stay fp32 like the stream they act on."""

    def __init__(self, shape: ClipVisionShape, state_dict: Dict[str, Tensor], device):
        super().__init__(device)
        self.shape = s = shape
        sd = visual_state_dict(state_dict, s)
        if s.head_dim != 80 or s.dim % 64 or s.image_size % s.patch_size or s.num_layers < 1:
            raise ValueError("supported vision shapes: head_dim 80, dim a multiple of 64, image_size a multiple of patch_size")
        f32 = torch.float32
        m = _lib.ClipModel()
        m.image_size, m.patch, m.dim, m.heads, m.mlp_dim = s.image_size, s.patch_size, s.dim, s.num_heads, s.mlp_dim
        m.layers_built, m.eps = s.layers_built, s.eps
        m.patch_w = self._dev(repack_patch_weight(sd["patch_embedding.weight"].float(), s.patch_kp)).data_ptr()
        m.cls = self._dev(sd["cls_embedding"].reshape(s.dim), f32).data_ptr()
        m.pos = self._dev(sd["pos_embedding"].reshape(s.seq_len, s.dim), f32).data_ptr()
        m.pre_norm_w = self._dev(sd["pre_norm.weight"], f32).data_ptr()
        m.pre_norm_b = self._dev(sd["pre_norm.bias"], f32).data_ptr()
        layers = (_lib.ClipLayer * max(1, s.layers_built))()
        for i in range(s.layers_built):
            p, ly = f"transformer.{i}.", layers[i]
            ly.norm1_w, ly.norm1_b = self._dev(sd[p + "norm1.weight"], f32).data_ptr(), self._dev(sd[p + "norm1.bias"], f32).data_ptr()
            ly.qkv_w, ly.qkv_b = self._dev(sd[p + "attn.to_qkv.weight"]).data_ptr(), self._dev(sd[p + "attn.to_qkv.bias"]).data_ptr()
            ly.proj_w, ly.proj_b = self._dev(sd[p + "attn.proj.weight"]).data_ptr(), self._dev(sd[p + "attn.proj.bias"]).data_ptr()
            ly.norm2_w, ly.norm2_b = self._dev(sd[p + "norm2.weight"], f32).data_ptr(), self._dev(sd[p + "norm2.bias"], f32).data_ptr()
            ly.fc1_w, ly.fc1_b = self._dev(sd[p + "mlp.0.weight"]).data_ptr(), self._dev(sd[p + "mlp.0.bias"]).data_ptr()
            ly.fc2_w, ly.fc2_b = self._dev(sd[p + "mlp.2.weight"]).data_ptr(), self._dev(sd[p + "mlp.2.bias"]).data_ptr()
        self._layers = layers
        m.layers_host = C.cast(layers, C.POINTER(_lib.ClipLayer))
        self.cmodel = m
        self._handle = torch_ops.register_model(self)

    def workspace_bytes(self, n: int) -> int:
        nbytes = int(_lib.lib().sf_clip_workspace_bytes(C.byref(self.cmodel), n))
        if nbytes == 0:
            _lib.check(-1, "sf_clip_workspace_bytes")
        return nbytes

    def __call__(self, frames: Tensor) -> Tensor:
        """frames [n, 3, H, W] float32 or bfloat16 in [-1, 1] -> float32 [n, seq_len, dim]."""
        if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 1:
            raise ValueError(f"expected frames [n, 3, H, W], got {tuple(frames.shape)}")
        if self.device.type != "cuda":
            raise ValueError(f"the encoder lives on {self.device}: the HIP path has no CPU fallback, construct it on a GPU device")
        if frames.dtype not in (torch.float32, torch.bfloat16):
            frames = frames.float()
        frames = frames.to(self.device).contiguous()
        n = frames.shape[0]
        ws = self._stream_bytes((n,), lambda: self.workspace_bytes(n))
        return torch.ops.sf_hip.clip_encode(self._handle, frames, ws)


def load_clip_checkpoint(path: str) -> Dict[str, Tensor]:
    """`models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth`, loaded with `weights_only=True` (the reference unpickles
    it with the default, clip.py:518-519)."""
    if not path or not os.path.exists(path):
        raise FileNotFoundError(f"CLIP checkpoint {path!r} not found: download it as the reference's README describes, or construct "
                                "CLIPModel(state_dict=...) / inject an image_encoder= into the pipeline")
    return torch.load(path, map_location="cpu", weights_only=True)


class CLIPModel:
    """Drop-in for the reference's `CLIPModel` (clip.py:501-542): `CLIPModel(dtype, device, checkpoint_path, tokenizer_path)`
    or, without a file, `CLIPModel(state_dict=..., shape=...)`.  `dtype` is the autocast dtype of the reference; this path
    computes in bfloat16 around an fp32 stream whatever it says.  `tokenizer_path` is accepted and unused: the text tower
    is not built."""

    def __init__(self, dtype=torch.bfloat16, device="cuda", checkpoint_path: Optional[str] = None, tokenizer_path: Optional[str] = None,
                 state_dict: Optional[Dict[str, Tensor]] = None, shape: ClipVisionShape = CLIP_VIT_H_14):
        self.dtype = dtype
        self.device = torch.device(device)
        self.checkpoint_path = checkpoint_path
        self.tokenizer_path = tokenizer_path
        if state_dict is None:
            state_dict = load_clip_checkpoint(checkpoint_path)
        self.shape = shape
        self.model = CLIPVisionEncoder(shape, state_dict, device)

    def visual(self, videos: Sequence[Tensor], interpolation: bool = False) -> Tensor:
        """`videos`: a list of [3, T, H, W] tensors in [-1, 1] (each may have its own T, H, W) -> float32 [sum T, L, dim],
        the un-normed output of the second-to-last block, frames in list order."""
        if interpolation:
            raise NotImplementedError("pos_interpolate (interpolation=True) is not built: frames are always resized to image_size")
        outs: List[Tensor] = []
        for u in videos:
            if u.dim() != 4 or u.shape[0] != 3:
                raise ValueError(f"visual() takes [3, T, H, W] tensors (clip.py:532 transposes them to frames), got {tuple(u.shape)}")
            outs.append(self.model(u.transpose(0, 1)))
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def textual(self, *args, **kwargs):
        raise NotImplementedError("the CLIP text tower (XLM-RoBERTa) is not built: the generator is conditioned on the image tower only")

    @property
    def tokenizer(self):
        raise NotImplementedError("the CLIP text tower and its tokenizer are not built")
