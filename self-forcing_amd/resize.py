"""Frame resizer on the GPU path: uint8 frames on the device change their size without a host round trip (csrc/resize.hip
behind sf_resize_frames), with the bits of the thing the reference calls: Pillow's antialiased bilinear
(`transforms.Resize` on a PIL image, inference.py:84-88) and bicubic (`image.resize`, causal_diffusion_inference.py:158).
The definition of every number is `resize_reference.py`; its coefficient tables are what the kernel reads."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from . import resize_reference as rr

Tensor = torch.Tensor
_DTYPES = (torch.uint8, torch.float32, torch.bfloat16)
_FITS = ("stretch", "cover")


def check_arguments(size, filter: str, dtype, crop, fit: str, who: str = "FrameResizer") -> Tuple[int, int]:
    """The checks of `FrameResizer.resize` that need neither frames nor a device: (height, width) of the output."""
    oh, ow = rr.check_size(size)
    rr.check_filter(filter)
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
    if fit not in _FITS:
        raise ValueError(f"fit must be 'stretch' or 'cover', got {fit!r}")
    if fit == "cover" and crop is not None:
        raise ValueError(f"{who}: fit='cover' chooses the crop itself; pass either crop or fit='cover', not both")
    return oh, ow


def crop_box(h: int, w: int, oh: int, ow: int, crop, fit: str) -> Tuple[int, int, int, int]:
    """(top, left, height, width) of the input that is resampled, checked against the frame and the kernel's ratio limit."""
    box = rr.cover_box(h, w, oh, ow) if fit == "cover" else rr.check_crop(crop, h, w)
    rr.check_ratio(box[2], oh, "height")
    rr.check_ratio(box[3], ow, "width")
    return box


class FrameResizer:
    """`resize(frames, size)` -> the frames at another size, every number as `resize_reference.resize` (= Pillow) defines it.

    frames: uint8 on the device, layout "hwc" [N, H, W, 3], "pose" [3, N, H, W] or "chw" [N, 3, H, W] (the decoder's three).
    The output may have any of these layouts and be uint8, or float32 / bfloat16 as u8 / 127.5 - 1 (the decoder's
    conversion).  `crop=(top, left, height, width)` is `im.crop(...).resize(...)`: no tap reaches outside it;
    `fit="cover"` takes the largest centred crop with the output's aspect ratio (`resize_reference.cover_box`).  Along
    each axis the input may be at most `resize_reference.MAX_RATIO` times the output (any enlargement is fine).  The
    coefficient tables are computed once per (in, out, filter) on the host and kept on the device.  Work runs on the
    current stream."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._tables: Dict[Tuple[int, int, str], Tuple[Tensor, Tensor]] = {}

    def tables(self, in_size: int, out_size: int, filter: str, device=None) -> Tuple[Tensor, Tensor]:
        """(bounds int32 [out, 2], coefs int32 [out, ksize]) of one axis on the device (the frames' own), cached."""
        device = self.device if device is None else device
        key = (in_size, out_size, filter, device)
        if key not in self._tables:
            bounds, coefs = rr.coefficients(in_size, out_size, filter)
            self._tables[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coefs).to(device))
        return self._tables[key]

    def resize(self, frames: Tensor, size: Sequence[int], filter: str = "bilinear", layout: str = "hwc", out_layout: Optional[str] = None,
               dtype=torch.uint8, crop: Optional[Sequence[int]] = None, fit: str = "stretch", out: Optional[Tensor] = None) -> Tensor:
        oh, ow = check_arguments(size, filter, dtype, crop, fit)
        out_layout = layout if out_layout is None else out_layout
        for name in (layout, out_layout):
            if name not in _lib.JPEG_LAYOUTS:
                raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {name!r}")
        if not isinstance(frames, Tensor) or frames.dtype != torch.uint8:
            raise ValueError(f"FrameResizer: frames must be a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
        want = {"hwc": "[N, H, W, 3]", "pose": "[3, N, H, W]", "chw": "[N, 3, H, W]"}[layout]
        if frames.dim() != 4 or frames.shape[{"hwc": 3, "pose": 0, "chw": 1}[layout]] != 3 or frames.numel() == 0:
            raise ValueError(f"FrameResizer: expected {want} for layout {layout!r}, got {tuple(frames.shape)}")
        n, h, w = (int(frames.shape[d]) for d in {"hwc": (0, 1, 2), "pose": (1, 2, 3), "chw": (0, 2, 3)}[layout])
        box = crop_box(h, w, oh, ow, crop, fit)
        if not frames.is_cuda:
            raise ValueError("FrameResizer: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
        shape = {"hwc": (n, oh, ow, 3), "pose": (3, n, oh, ow), "chw": (n, 3, oh, ow)}[out_layout]
        if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or out.device != frames.device or not out.is_contiguous()
                                or out.data_ptr() % 16):
            raise ValueError(f"FrameResizer: out must be a contiguous, 16-byte-aligned {dtype} tensor {shape} on {frames.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
        frames = frames.contiguous()
        if frames.data_ptr() % 4:                                  # a view that starts inside a dword: the kernel fetches whole dwords
            frames = frames.clone()
        with torch.cuda.device(frames.device):
            return ops.resize_frames(frames, self.tables(box[3], ow, filter, frames.device), self.tables(box[2], oh, filter, frames.device), filter,
                                     layout, out_layout, dtype, None if box == (0, 0, h, w) else box, out)
