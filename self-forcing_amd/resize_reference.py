"""The definition of the frame resizer's numbers (numpy, no GPU): Pillow's 8-bit resampler restated.

`PIL.Image.resize` on an 8-bit image is exact integer arithmetic: per axis a table of 22-bit fixed-point coefficients
(computed in IEEE double), one pass `clamp((2**21 + sum px * coef) >> 22, 0, 255)` with an arithmetic shift, horizontal
first, then vertical over the uint8 result of the first.  `coefficients` builds the table, `resize` applies it; both equal
Pillow (12.2) bit for bit for "bilinear" (`Image.BILINEAR`, what `transforms.Resize` on a PIL image does, reference
inference.py:84-88) and "bicubic" (`Image.BICUBIC`, `image.resize((w, h))`'s default,
pipeline/causal_diffusion_inference.py:158).  csrc/resize.hip takes these tables as they stand and equals `resize` bit for
bit.  Pillow skips an axis whose size does not change; the table of such an axis has the single weight 1 << 22 on the
pixel itself, which gives the same bits."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

FILTERS = {"bilinear": 0, "bicubic": 1}          # enum sf_resize_filter
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}
PRECISION_BITS = 22
MAX_RATIO = 8                                    # SF_RESIZE_MAX_RATIO: in / out per axis the kernel takes


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_KERNELS = {"bilinear": _bilinear, "bicubic": _bicubic}


def check_filter(filter: str) -> str:
    if filter not in FILTERS:
        raise ValueError(f"filter must be 'bilinear' or 'bicubic', got {filter!r}")
    return filter


def kernel_size(in_size: int, out_size: int, filter: str) -> int:
    """Columns of the coefficient table: ceil(support) * 2 + 1."""
    support = SUPPORT[check_filter(filter)] * max(in_size / out_size, 1.0)
    return int(math.ceil(support)) * 2 + 1


def coefficients(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = (xmin, xmax), coefs int32 [out, ksize]): output xx = sum over x < xmax of
    px[xmin + x] * coefs[xx, x]; coefficients past xmax are 0.  All arithmetic in Python floats (IEEE double)."""
    f = _KERNELS[check_filter(filter)]
    if in_size < 1 or out_size < 1:
        raise ValueError(f"sizes must be >= 1, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coefs = np.zeros((out_size, ksize), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            coefs[xx, x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)
        bounds[xx] = (xmin, xmax)
    return bounds, coefs


def resample_axis(px: np.ndarray, axis: int, bounds: np.ndarray, coefs: np.ndarray) -> np.ndarray:
    """One pass along `axis` of a uint8 array: clamp((2**21 + sum px[xmin + x] * coef[x]) >> 22, 0, 255), int32 accumulation."""
    px = np.moveaxis(px, axis, -1)
    acc = np.full(px.shape[:-1] + (bounds.shape[0],), 1 << (PRECISION_BITS - 1), np.int32)
    last = px.shape[-1] - 1
    for k in range(coefs.shape[1]):
        if not coefs[:, k].any():
            continue
        idx = np.minimum(bounds[:, 0] + k, last)                  # past xmax the coefficient is 0
        acc += px[..., idx].astype(np.int32) * coefs[:, k]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def check_crop(crop: Optional[Sequence[int]], h: int, w: int) -> Tuple[int, int, int, int]:
    """(top, left, height, width) of `crop` inside an h x w frame (None: the whole frame); integers only."""
    if crop is None:
        return 0, 0, h, w
    if len(crop) != 4 or any(int(v) != v for v in crop):
        raise ValueError(f"crop must be four integers (top, left, height, width), got {crop!r}")
    top, left, ch, cw = (int(v) for v in crop)
    if top < 0 or left < 0 or ch < 1 or cw < 1 or top + ch > h or left + cw > w:
        raise ValueError(f"crop {(top, left, ch, cw)} does not lie inside a {h}x{w} frame")
    return top, left, ch, cw


def check_size(size) -> Tuple[int, int]:
    if len(size) != 2 or any(int(v) != v for v in size) or min(size) < 1:
        raise ValueError(f"size must be (height, width), both >= 1, got {size!r}")
    return int(size[0]), int(size[1])


def resize(frames: np.ndarray, size: Tuple[int, int], filter: str = "bilinear", crop: Optional[Sequence[int]] = None) -> np.ndarray:
    """uint8 [N, H, W, 3] -> uint8 [N, size[0], size[1], 3]: `Image.fromarray(f).crop(...).resize((size[1], size[0]), filter)`
    per frame.  crop = (top, left, height, width): taps never reach outside it."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be uint8 [N, H, W, 3], got {frames.dtype} {frames.shape}")
    oh, ow = check_size(size)
    top, left, ch, cw = check_crop(crop, frames.shape[1], frames.shape[2])
    x = frames[:, top:top + ch, left:left + cw]
    x = resample_axis(x, 2, *coefficients(cw, ow, filter))
    return np.ascontiguousarray(resample_axis(x, 1, *coefficients(ch, oh, filter)))


def cover_box(in_h: int, in_w: int, out_h: int, out_w: int) -> Tuple[int, int, int, int]:
    """(top, left, height, width) of the largest centred crop of an in_h x in_w frame with the aspect ratio of out_h x out_w:
    sizes and offsets floored, sizes at least 1."""
    if min(in_h, in_w, out_h, out_w) < 1:
        raise ValueError(f"sizes must be >= 1, got {in_h}x{in_w} -> {out_h}x{out_w}")
    if in_w * out_h >= in_h * out_w:                               # the input is wider than the output: cut the sides
        ch, cw = in_h, max(in_h * out_w // out_h, 1)
    else:
        ch, cw = max(in_w * out_h // out_w, 1), in_w
    return (in_h - ch) // 2, (in_w - cw) // 2, ch, cw


def check_ratio(in_size: int, out_size: int, axis: str) -> None:
    """The kernel's limit: at most MAX_RATIO input pixels per output pixel along each axis (any enlargement)."""
    if in_size > MAX_RATIO * out_size:
        raise ValueError(f"resize: {axis} {in_size} -> {out_size} reduces by more than {MAX_RATIO}x, the kernel's limit per axis "
                         "(resize in two steps)")
