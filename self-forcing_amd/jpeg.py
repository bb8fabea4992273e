"""JPEG encoder on the GPU path: decoded frames leave the device as JFIF files (csrc/jpeg.hip behind sf_jpeg_*).

Replaces what the reference's demo does on the host for every frame (demo.py:162-187, `tensor_to_base64_frame`: clamp,
* 127.5 + 127.5, uint8, PIL save at quality 100) up to the base64 step, which stays a host one-liner of the caller.  The
format and the definition of every number are in `jpeg_reference.py`."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib, ops
from . import jpeg_reference as jr

Tensor = torch.Tensor


def default_restart_interval(subsampling: str) -> int:
    """MCUs per restart interval when none is given: the most whole MCUs whose blocks fit one wave (64 lanes, one block
    each) -- 10 MCUs of "420", 21 of "444".  Measured against 5 / 26 / 52 MCUs in DESIGN.md section 14."""
    return 64 // jr.blocks_per_mcu(subsampling)


class JpegEncoder:
    """`encode(frames)` -> one JPEG file (bytes) per frame.

    frames: float32 / bfloat16 [T, 3, H, W] or [B, T, 3, H, W] in `value_range` ((-1, 1): the decoders' output, truncated as
    the demo does; (0, 1): `generate.py`'s `255 * x`), or uint8 [T, H, W, 3] / [B, T, H, W, 3].  H and W must be multiples
    of the MCU (16 for "420", 8 for "444").  Work runs on the current stream; an encoder owns one workspace, so use one
    encoder per stream."""

    def __init__(self, quality: int = 90, subsampling: str = "420", restart_interval: Optional[int] = None,
                 value_range: Tuple[float, float] = (-1, 1), device="cuda"):
        jr.quant_tables(quality)                                   # ValueError outside 1..100
        jr.mcu_size(subsampling)
        if tuple(value_range) not in _lib.JPEG_RANGES:
            raise ValueError(f"value_range must be (-1, 1) or (0, 1), got {value_range}")
        if restart_interval is None:
            restart_interval = default_restart_interval(subsampling)
        if not 1 <= int(restart_interval) <= 65535:
            raise ValueError(f"restart_interval must be 1..65535, got {restart_interval}")
        self.quality, self.subsampling, self.restart_interval = int(quality), subsampling, int(restart_interval)
        self.value_range = tuple(value_range)
        self.device = torch.device(device)
        self._ws: Optional[Tensor] = None
        self._host: Optional[Tensor] = None

    # ------------------------------------------------------------------------------------------
    def _prepare(self, frames: Tensor):
        if not isinstance(frames, Tensor) or not frames.is_cuda:
            raise ValueError("JpegEncoder: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
        name = str(frames.dtype).replace("torch.", "")
        if name not in _lib.JPEG_DTYPES:
            raise ValueError(f"JpegEncoder: frames must be float32, bfloat16 or uint8, got {frames.dtype}")
        if frames.dim() not in (4, 5):
            raise ValueError(f"JpegEncoder: expected [T, 3, H, W] or [B, T, 3, H, W] (uint8: channels last), got {tuple(frames.shape)}")
        if frames.dim() == 5:
            frames = frames.reshape(-1, *frames.shape[2:])
        if name == "uint8":
            n, h, w, c = frames.shape
        else:
            n, c, h, w = frames.shape
        if c != 3 or n < 1:
            raise ValueError(f"JpegEncoder: frames of shape {tuple(frames.shape)} do not hold three channels")
        jr.check_geometry(h, w, self.subsampling)                  # ValueError off the MCU grid
        return frames.contiguous(), n, h, w

    def _workspace(self, n: int, h: int, w: int, device) -> Tuple[Tensor, int]:
        need = ops.jpeg_workspace_bytes(n, h, w, self.subsampling, self.restart_interval)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws, need

    # ------------------------------------------------------------------------------------------
    def coefficients(self, frames: Tensor) -> Tensor:
        """The transform kernel's output: int16 [N, blocks, 64], quantised, zigzagged, blocks in MCU scan order."""
        x, n, h, w = self._prepare(frames)
        mx, my = jr.check_geometry(h, w, self.subsampling)
        coef = torch.empty(n, mx * my * jr.blocks_per_mcu(self.subsampling), 64, dtype=torch.int16, device=x.device)
        return ops.jpeg_transform(x, coef, n, h, w, self.subsampling, self.quality, self.value_range)

    def entropy(self, coef: Tensor, h: int, w: int) -> Tuple[Tensor, Tensor]:
        """Entropy-code and pack a coefficient buffer [N, blocks, 64] (int16): (bytes_tensor, meta) as `_encode`."""
        if not coef.is_cuda or coef.dtype != torch.int16 or coef.dim() != 3 or coef.shape[2] != 64:
            raise ValueError("JpegEncoder.entropy: expected a device int16 tensor [N, blocks, 64]")
        mx, my = jr.check_geometry(h, w, self.subsampling)
        if coef.shape[1] != mx * my * jr.blocks_per_mcu(self.subsampling):
            raise ValueError(f"JpegEncoder.entropy: {coef.shape[1]} blocks do not match a {h}x{w} frame")
        coef, n = coef.contiguous(), coef.shape[0]
        ws, need = self._workspace(n, h, w, coef.device)
        out = torch.empty(need, dtype=torch.uint8, device=coef.device)
        meta = torch.empty(n + 2, dtype=torch.int64, device=coef.device)
        ops.jpeg_entropy(coef, n, h, w, self.subsampling, self.quality, self.restart_interval, ws, out, meta)
        return out, meta

    def _encode(self, frames: Tensor) -> Tuple[Tensor, Tensor]:
        """(bytes_tensor uint8 sized for the worst case, meta int64 [N + 2]: offsets[N + 1], then the status word)."""
        x, n, h, w = self._prepare(frames)
        ws, need = self._workspace(n, h, w, x.device)
        out = torch.empty(need, dtype=torch.uint8, device=x.device)
        meta = torch.empty(n + 2, dtype=torch.int64, device=x.device)
        ops.jpeg_encode_frames(x, n, h, w, self.subsampling, self.quality, self.restart_interval, self.value_range, ws, out, meta)
        return out, meta

    def encode_to_device(self, frames: Tensor) -> Tuple[Tensor, Tensor]:
        """(bytes_tensor, offsets) on the device, nothing synchronised: file f is bytes_tensor[offsets[f]:offsets[f + 1]].
        For callers that overlap the copy themselves; `bytes_tensor` is sized for the worst case, only offsets[-1] bytes
        are meaningful.  `self.status` (a device int32 view) is 0 when every file is complete."""
        out, meta = self._encode(frames)
        self.status = meta[-1:].view(torch.int32)[:1]
        return out, meta[:-1]

    @staticmethod
    def _raise_on(status: int) -> None:
        if status:
            what = "; ".join(text for bit, text in _lib.JPEG_STATUS.items() if status & bit)
            raise _lib.SfHipError(f"JPEG encode failed (status {status}): {what}")

    def _to_host(self, out: Tensor, meta: Tensor) -> List[bytes]:
        meta_h = meta.cpu()                                        # offsets + status: 8 (N + 2) bytes, the call's first synchronisation
        self._raise_on(int(meta_h[-1]) & 0xFFFFFFFF)
        offsets = meta_h[:-1].tolist()
        total = offsets[-1]
        if self._host is None or self._host.numel() < total:
            self._host = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
        host = self._host[:total]
        host.copy_(out[:total])                                    # the used bytes only, one copy for all frames
        view = memoryview(host.numpy())
        return [bytes(view[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]

    def encode(self, frames: Tensor) -> List[bytes]:
        """One JPEG file per frame, in order ([B, T, ...] flattened to B * T).  One device-to-host copy of the used bytes
        per call (after one 8 (N + 2)-byte read of the offsets that sizes it), not one per frame."""
        return self._to_host(*self._encode(frames))

    def encode_coefficients(self, coef: Tensor, h: int, w: int) -> List[bytes]:
        """`encode` from a coefficient buffer (the entropy and pack kernels alone)."""
        return self._to_host(*self.entropy(coef, h, w))
