"""Raw YUV video on the GPU path: NV12, I420, I422, I444, YUYV, UYVY and gray frames become RGB frames on the device, and
decoded frames leave it as I420 / NV12 / I422 / I444 (csrc/yuv.hip behind sf_yuv_*).

Replaces what the reference does on the host for every frame it is given (PIL / cv2 loads, inference.py:84-88 and the pose
loaders): a webcam's YUYV, a hardware decoder's NV12 and the planes a software tool pipes cross the bus at 1.5 or 2 bytes
per pixel and are converted where they are used.  The definition of every number is `yuv_reference.py`; `y4m.py` reads and
writes the YUV4MPEG2 streams that carry such frames through a pipe."""
from __future__ import annotations

from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import resize as resize_mod
from . import yuv_reference as yr
from .torch_ops import _dtype_name

Tensor = torch.Tensor
_DTYPES = (torch.uint8, torch.float32, torch.bfloat16)


def _check_hw(hw) -> Tuple[int, int]:
    try:
        h, w = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError(f"hw must be (height, width), got {hw!r}") from None
    return h, w


class YuvDecoder:
    """`decode(raw, fmt, hw)` -> the frames of raw YUV bytes on the device, every number as `yuv_reference.decode` defines it.

    raw: a device uint8 tensor [n, frame_bytes], one frame's `bytes`, or a sequence of them.  Host bytes go up in one pinned,
    non-blocking copy (the pinned block comes from torch's host allocator, which takes it back only after the copy has run); the
    call reads nothing back and never synchronises.  Work runs on the current stream."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._resizer = None

    def _upload(self, frames: List[bytes], need: int) -> Tensor:
        n = len(frames)
        for k, f in enumerate(frames):
            if not isinstance(f, (bytes, bytearray, memoryview)):
                raise ValueError(f"YuvDecoder: frame {k} is {type(f).__name__}, expected bytes")
            if len(f) != need:
                raise ValueError(f"YuvDecoder: frame {k} has {len(f)} bytes, expected {need}")
        total = n * need
        if total >= 1 << 31:
            raise ValueError(f"YuvDecoder: {total} bytes in one call; split it (2 GiB at most)")
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)           # from torch's pinned cache: a block returns to it
        view = host.numpy()                                                      # only after the copy that read it has run
        for k, f in enumerate(frames):
            view[k * need:(k + 1) * need] = np.frombuffer(f, np.uint8)
        return host.to(self.device, non_blocking=True).view(n, need)             # the call's one upload

    def decode(self, raw, fmt: str, hw: Sequence[int], layout: str = "hwc", dtype=torch.uint8, matrix: str = "bt601", range: str = "limited",
               chroma: str = "triangle", size: Optional[Sequence[int]] = None, filter: str = "bilinear", fit: str = "stretch") -> Tensor:
        """layout "hwc": [N, H, W, 3]; "pose": [3, N, H, W]; "chw": [N, 3, H, W].  dtype uint8: the samples; float32 /
        bfloat16: u8 / 127.5 - 1, the JPEG decoder's conversion.  size=(H, W): the frames are converted as uint8 "hwc"
        (a buffer of torch's caching allocator, reused from call to call), then resized on the device as `FrameResizer.resize` does it."""
        h, w = _check_hw(hw)
        yr.check_format(fmt, h, w)
        yr.check_chroma(chroma)
        k = yr.constants(matrix, range)
        if layout not in _lib.JPEG_LAYOUTS:
            raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
        if self.device.type != "cuda":
            raise ValueError(f"YuvDecoder: needs a CUDA/ROCm device (the HIP path has no CPU fallback), got {self.device}")
        if size is not None:
            oh, ow = resize_mod.check_arguments(size, filter, dtype, None, fit, "YuvDecoder")
            resize_mod.crop_box(h, w, oh, ow, None, fit)           # the ratio limit, before anything is uploaded
        need = yr.frame_bytes(fmt, h, w)
        if isinstance(raw, Tensor):
            if raw.dtype != torch.uint8 or raw.dim() != 2 or raw.shape[0] < 1 or raw.shape[1] != need:
                raise ValueError(f"YuvDecoder: raw must be uint8 [n, {need}] for {h}x{w} {fmt}, got {raw.dtype} {tuple(raw.shape)}")
            if not raw.is_cuda:
                raise ValueError(f"YuvDecoder: raw must be on a CUDA/ROCm device (pass host frames as bytes), got {raw.device}")
        with torch.cuda.device(raw.device if isinstance(raw, Tensor) else self.device):
            if not isinstance(raw, Tensor):
                frames = [raw] if isinstance(raw, (bytes, bytearray, memoryview)) else list(raw)
                if not frames:
                    raise ValueError("YuvDecoder: no frames")
                raw = self._upload(frames, need)
            raw = raw.contiguous()
            if size is None:
                return ops.yuv_decode_frames(raw, fmt, h, w, k, chroma, layout, dtype)
            full = ops.yuv_decode_frames(raw, fmt, h, w, k, chroma, "hwc", torch.uint8)
            if self._resizer is None:
                self._resizer = resize_mod.FrameResizer(self.device)
            return self._resizer.resize(full, (oh, ow), filter, "hwc", layout, dtype, fit=fit)


class YuvEncoder:
    """`encode(frames)` -> one raw frame (bytes) per frame, every number as `yuv_reference.encode` defines it.

    frames: float32 / bfloat16 [T, 3, H, W] or [B, T, 3, H, W] in `value_range` ((-1, 1): the decoders' output, truncated as
    `JpegEncoder` does; (0, 1)), or uint8 [T, H, W, 3] / [B, T, H, W, 3].  Any H and W.  It also is a `frame_encoder` of
    `CausalInferencePipeline.stream` / `open_session`: the chunks' frames then come as raw `fmt` bytes."""

    def __init__(self, fmt: str = "i420", matrix: str = "bt601", range: str = "limited", value_range: Tuple[float, float] = (-1, 1), device="cuda"):
        if fmt not in yr.ENCODE_FORMATS:
            raise ValueError(f"YuvEncoder writes {', '.join(yr.ENCODE_FORMATS)}, got {fmt!r}")
        self.constants = yr.constants(matrix, range)               # ValueError for an unknown matrix or range
        if tuple(value_range) not in _lib.JPEG_RANGES:
            raise ValueError(f"value_range must be (-1, 1) or (0, 1), got {value_range}")
        self.fmt, self.matrix, self.range = fmt, matrix, range
        self.value_range = tuple(value_range)
        self.device = torch.device(device)
        self._host: Optional[Tensor] = None

    def _prepare(self, frames: Tensor) -> Tensor:
        if not isinstance(frames, Tensor) or not frames.is_cuda:
            raise ValueError("YuvEncoder: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
        name = _dtype_name(frames)
        if name not in _lib.JPEG_DTYPES:
            raise ValueError(f"YuvEncoder: frames must be float32, bfloat16 or uint8, got {frames.dtype}")
        if frames.dim() not in (4, 5):
            raise ValueError(f"YuvEncoder: expected [T, 3, H, W] or [B, T, 3, H, W] (uint8: channels last), got {tuple(frames.shape)}")
        if frames.dim() == 5:
            frames = frames.reshape(-1, *frames.shape[2:])
        c = frames.shape[3] if name == "uint8" else frames.shape[1]
        if c != 3 or frames.shape[0] < 1:
            raise ValueError(f"YuvEncoder: frames of shape {tuple(frames.shape)} do not hold three channels")
        return frames.contiguous()

    def _encode(self, frames: Tensor) -> Tuple[Tensor]:
        """(uint8 [n, frame_bytes] on the device,): what `_to_host` takes."""
        x = self._prepare(frames)
        with torch.cuda.device(x.device):
            return (ops.yuv_encode_frames(x, self.fmt, self.constants, self.value_range),)

    def encode_to_device(self, frames: Tensor) -> Tensor:
        """uint8 [n, frame_bytes] on the device, nothing synchronised ([B, T, ...] flattened to B * T)."""
        return self._encode(frames)[0]

    def _to_host(self, out: Tensor) -> List[bytes]:
        n, need = out.shape
        if self._host is None or self._host.numel() < n * need:
            self._host = torch.empty(max(n * need, 1 << 20), dtype=torch.uint8, pin_memory=True)
        host = self._host[:n * need]
        host.copy_(out.reshape(-1))                                # one copy for all frames; it synchronises
        view = memoryview(host.numpy())
        return [bytes(view[k * need:(k + 1) * need]) for k in range(n)]

    def encode(self, frames: Tensor) -> List[bytes]:
        """One raw frame per frame, in order.  One device-to-host copy per call."""
        return self._to_host(*self._encode(frames))


def frame_feed(raw_frames: Iterable[bytes], decoder: YuvDecoder, fmt: str, hw: Sequence[int], frames_per_piece: int = 12, layout: str = "pose",
               size: Optional[Sequence[int]] = None, matrix: str = "bt601", range: str = "limited", chroma: str = "triangle", filter: str = "bilinear",
               fit: str = "stretch") -> Iterator[Tensor]:
    """Raw YUV frames as the pieces `CausalInferencePipeline.stream(pose_feed=...)` / `open_session(pose_feed=...)` pull:
    uint8 [3, n, H, W], n = `frames_per_piece` (the last piece may be shorter), each decoded when it is asked for; with
    layout="hwc" the pieces `keypoint_feed(frame_pieces, estimator, max_people)` takes.  `raw_frames` may be any iterable, a
    live source (a `y4m.Y4mReader` over a pipe) included: it is pulled from only when a piece is asked for.  size=(H, W)
    resizes every piece on the device."""
    if frames_per_piece < 1:
        raise ValueError(f"frames_per_piece must be >= 1, got {frames_per_piece}")
    h, w = _check_hw(hw)
    yr.check_format(fmt, h, w)
    yr.check_chroma(chroma)
    yr.check_colour(matrix, range)
    if layout not in _lib.JPEG_LAYOUTS:
        raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
    if size is not None:
        resize_mod.check_arguments(size, filter, torch.uint8, None, fit, "frame_feed")

    def pieces():
        piece: List[bytes] = []
        for f in raw_frames:
            piece.append(f)
            if len(piece) == frames_per_piece:
                yield decoder.decode(piece, fmt, (h, w), layout, torch.uint8, matrix, range, chroma, size, filter, fit)
                piece = []
        if piece:
            yield decoder.decode(piece, fmt, (h, w), layout, torch.uint8, matrix, range, chroma, size, filter, fit)
    return pieces()
