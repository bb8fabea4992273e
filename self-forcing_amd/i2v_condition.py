"""The conditioning of an i2v generator for one clip, produced as the rollout needs it.

    cond = I2VConditioner(vae, image_encoder, pose_embedder=None, device="cuda")
    clip_feature = cond.begin(image, height, width, random_ref_dwpose=None)    # CLIP once, the reference-pose map once
    y = cond.frames(n)                                                         # the next n latent frames: bf16 [1, 20, n, h, w]

`CausalDiffusionInferencePipeline.encode_image` builds `y` for a clip of known length: the pixel clip "image, then zeros"
whole, one VAE encode of all of it, then torch `zeros` / `cat` / casts.  A stream of open length has no whole clip.  Here
the VAE encoder keeps the clip's convolution histories between calls (`WanVAEEncoder.begin_clip` / `continue_clip`: the
calls `encode` makes, in the same order, so the same bits; the zero frames are one small persistent buffer) and one kernel
(`sf_i2v_assemble_y`, csrc/i2v.hip) writes a chunk of `y` from the encoder's fp32 rows: the 4 mask channels, the 16 latent
channels rounded to bf16, and, with a reference-pose map, that map added with a second rounding -- the bits
`encode_image(...)["y"] (+ embed_ref(...))` has.  `frames` enqueues nothing but VAE encode calls and that kernel.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import torch_ops  # noqa: F401  (registers torch.ops.sf_hip.*)
from .weights import I2V_Y_CHANNELS

Tensor = torch.Tensor


def prepare_image(image, height: int, width: int) -> Tensor:
    """The image checks of `encode_image` (causal_diffusion_inference.py:147-158): a tensor [1, 3, height, width] or
    [3, height, width] in [-1, 1], or a PIL image (resized to width x height, scaled by 2/255 - 1) -> float32 [3, height, width]."""
    if height % 8 or width % 8:
        raise ValueError(f"height and width must be multiples of 8, got {height}x{width}")
    if not torch.is_tensor(image):
        import numpy as np
        image = torch.from_numpy(np.array(image.resize((width, height)), dtype=np.float32) * (2 / 255) - 1).permute(2, 0, 1)
    if image.dim() == 4 and image.shape[0] == 1:
        image = image[0]
    if tuple(image.shape) != (3, height, width):
        raise ValueError(f"image must be [1, 3, {height}, {width}] or [3, {height}, {width}], got {tuple(image.shape)}")
    return image


class I2VConditioner:
    """Owns one clip's `clip_feature` and `y`.  `vae`: a `WanVAEWrapper` with encoder weights; `image_encoder`: a
    `clip.CLIPModel`; `pose_embedder` (a `pose.PoseEmbedder`) only for `begin(..., random_ref_dwpose=)`."""

    def __init__(self, vae, image_encoder, pose_embedder=None, device="cuda", dtype=torch.bfloat16):
        encoder = getattr(vae, "encoder", None)
        if encoder is None or not hasattr(encoder, "begin_clip"):
            raise NotImplementedError("the incremental y needs the Wan VAE encoder (a WanVAEWrapper whose state dict holds the "
                                      "encoder.* / conv1.* tensors); this VAE has none")
        self.encoder = encoder
        self.image_encoder = image_encoder
        self.pose_embedder = pose_embedder
        self.device = torch.device(device)
        self.dtype = dtype
        self.position = 0                   # latent frames of y handed out since begin()
        self._image: Optional[Tensor] = None
        self._ref_map: Optional[Tensor] = None

    def begin(self, image, height: int, width: int, random_ref_dwpose: Optional[Tensor] = None) -> Tensor:
        """Start a clip of height x width pixels: `clip_feature` (bf16 [1, L, dim], `image_encoder.visual` of the image as a
        one-frame video) is returned; the reference-pose map, when asked for, is computed here, once.  Nothing of the VAE
        runs yet: the image's own frame is encoded with the first `frames` call, on that call's stream."""
        image = prepare_image(image, height, width).to(self.device, torch.float32)
        clip_feature = self.image_encoder.visual([image.unsqueeze(1)]).to(self.dtype)
        self._ref_map = None
        if random_ref_dwpose is not None:
            if self.pose_embedder is None:
                raise ValueError("random_ref_dwpose needs a pose embedder")
            ref = self.pose_embedder.embed_ref(random_ref_dwpose)                      # [1, 20, 1, h, w], a view of [h, w, 20]
            self._ref_map = ref[0, :, 0].permute(1, 2, 0)
            assert self._ref_map.is_contiguous() and tuple(self._ref_map.shape) == (height // 8, width // 8, I2V_Y_CHANNELS), \
                f"the reference-pose map must be channels-last [{height // 8}, {width // 8}, {I2V_Y_CHANNELS}], got {tuple(ref.shape)}"
        self._image = image.to(self.dtype)      # the clip's first frame as the whole-clip path rounds it
        self.position = 0
        return clip_feature

    def frames(self, n: int) -> Tensor:
        """The next `n` latent frames of y, bf16 [1, 20, n, h, w]: VAE encode calls for the 4 n pixel frames (the first
        call: the image, then 4 (n - 1) zero frames) and one `sf_i2v_assemble_y` launch."""
        if self._image is None:
            raise RuntimeError("frames() before begin()")
        if n < 1:
            raise ValueError(f"frames: n must be positive, got {n}")
        enc = self.encoder
        _, H, W = self._image.shape
        sf = enc.shape.spatial_factor
        latent = torch.empty(n, enc.shape.z_dim, H // sf, W // sf, dtype=torch.float32, device=self.device)
        first = self.position == 0
        if first:
            enc.begin_clip(self._image, out=latent[:1])
            if n > 1:
                enc.continue_clip(n - 1, out=latent[1:])
        else:
            enc.continue_clip(n, out=latent)
        y = torch.empty(1, I2V_Y_CHANNELS, n, H // sf, W // sf, dtype=self.dtype, device=self.device)
        torch.ops.sf_hip.i2v_assemble_y(latent, y[0], first, self._ref_map)
        self.position += n
        return y
