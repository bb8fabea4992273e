"""JPEG encoder on the GPU path: decoded frames leave the device as JFIF files (csrc/jpeg.hip behind sf_jpeg_*).

Replaces what the reference's demo does on the host for every frame (demo.py:162-187, `tensor_to_base64_frame`: clamp,
* 127.5 + 127.5, uint8, PIL save at quality 100) up to the base64 step, which stays a host one-liner of the caller.  The
format and the definition of every number are in `jpeg_reference.py`.

`JpegDecoder` is the way back in (csrc/jpeg_decode.hip behind sf_jpeg_decode_*): JPEG files -- pose frames from a renderer
behind a socket, a webcam, an MJPEG file this project wrote -- become uint8 / float frames on the device without a host
decode; `pose_feed` turns a list of them into the pieces `CausalInferencePipeline.stream(pose_feed=...)` pulls."""
from __future__ import annotations

from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import jpeg_reference as jr
from . import resize as resize_mod
from .torch_ops import _dtype_name

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
        name = _dtype_name(frames)
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


# one file's entry of the upload's table block (include/sf_hip.h, SF_JPEG_DECODE_FILE_BYTES)
_HUFF_DTYPE = np.dtype([("look", "<u2", 512), ("maxcode", "<i4", 18), ("valoff", "<i4", 18), ("vals", "u1", 256)])
_FILE_DTYPE = np.dtype([("scan_off", "<u4"), ("scan_len", "<u4"), ("ri", "<u4"), ("intervals", "<u4"), ("quant", "<u2", (3, 64)),
                        ("huff", _HUFF_DTYPE, (3, 2)), ("pad", "u1", 16)])
assert _FILE_DTYPE.itemsize == _lib.JPEG_DECODE_FILE_BYTES
_DECODE_DTYPES = (torch.uint8, torch.float32, torch.bfloat16)


class JpegDecoder:
    """`decode(files)` -> the frames of JPEG files on the device, every number as `jpeg_reference.decode` defines it.

    Takes baseline JPEG (8 bit, Huffman, one interleaved scan; 4:4:4, 4:2:2, 4:2:0 or grayscale; any tables, with or without
    restart markers, any size); `jpeg_reference.parse` says what else is refused, with a ValueError.  The files of one
    call share height, width and sampling; tables, quality and restart interval may differ from file to file.  The host
    reads the header segments only; the scans go up in one pinned copy.  One lane decodes one restart interval, so files
    with a DRI segment (as `JpegEncoder` writes them) decode in parallel and a file without one on a single lane --
    correct, and slow.  Work runs on the current stream; a decoder owns one workspace, so use one decoder per stream."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._ws: Optional[Tensor] = None
        self._host: Optional[Tensor] = None
        self._dev: Optional[Tensor] = None
        self._full: Optional[Tensor] = None                        # decode(size=...): the frames at the files' own size
        self._resizer = None
        self.status: List[int] = []                                # per file of the last call: _lib.JPEG_DECODE_STATUS bits

    @staticmethod
    def info(file: bytes) -> Tuple[int, int, str, int]:
        """(height, width, sampling "420" / "444" / "422" / "gray", restart interval in MCUs or 0) of one file's header."""
        i = jr.parse(file)
        return i.height, i.width, i.sampling, i.restart_interval

    # ------------------------------------------------------------------------------------------
    def _parse(self, files: Sequence[bytes]):
        """The files' headers, checked (host only): (files, infos)."""
        if self.device.type != "cuda":
            raise ValueError("JpegDecoder: needs a CUDA/ROCm device (the HIP path has no CPU fallback)")
        files = list(files)
        if not files:
            raise ValueError("JpegDecoder: no files")
        infos = [jr.parse(f) for f in files]
        first = infos[0]
        for k, i in enumerate(infos):
            if (i.height, i.width, i.sampling) != (first.height, first.width, first.sampling):
                raise ValueError(f"JpegDecoder: file {k} is {i.height}x{i.width} {i.sampling}, file 0 {first.height}x{first.width} {first.sampling}: "
                                 "the files of one call share size and sampling")
        return files, infos

    def _upload(self, files: List[bytes], infos):
        """Build the table block, copy it and the scans to the device: (upload, bytes, info, max_intervals)."""
        n, first = len(files), infos[0]
        table = np.zeros(n, _FILE_DTYPE)
        pos = n * _FILE_DTYPE.itemsize
        for k, i in enumerate(infos):
            e = table[k]
            e["scan_off"], e["scan_len"] = pos, i.scan_end - i.scan_offset
            e["ri"], e["intervals"] = i.restart_interval or i.blocks // i.blocks_per_mcu, i.intervals
            for c in range(i.components):
                e["quant"][c] = i.quant[c]
                for cls, spec in enumerate((i.dc[c], i.ac[c])):
                    h = e["huff"][c][cls]
                    h["look"], h["maxcode"], h["valoff"], h["vals"] = jr.decode_tables(*spec)
            pos = (pos + i.scan_end - i.scan_offset + 15) & ~15
        total = pos
        if total >= 1 << 31:
            raise ValueError(f"JpegDecoder: {total} bytes in one call; split it (2 GiB at most)")
        if self._host is None or self._host.numel() < total:
            self._host = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self._dev = torch.empty(self._host.numel(), dtype=torch.uint8, device=self.device)
        host = self._host.numpy()
        host[:n * _FILE_DTYPE.itemsize] = table.view(np.uint8)
        for e, f, i in zip(table, files, infos):
            a, m = int(e["scan_off"]), int(e["scan_len"])
            host[a:a + m] = np.frombuffer(f, np.uint8, m, i.scan_offset)
        self._dev[:total].copy_(self._host[:total], non_blocking=True)          # tables and scans: the call's one upload
        return self._dev, total, first, max(i.intervals for i in infos)

    def _workspace(self, n: int, info, max_intervals: int) -> Tensor:
        need = ops.jpeg_decode_workspace_bytes(n, info.height, info.width, info.sampling, max_intervals)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _finish(self, status: Tensor, strict: bool) -> None:
        """Read the status words (the call's synchronisation: the pinned buffer is free again afterwards)."""
        self.status = [int(v) for v in status.cpu().tolist()]
        bad = [(k, v) for k, v in enumerate(self.status) if v]
        if bad and strict:
            what = "; ".join(f"file {k}: " + ", ".join(text for bit, text in _lib.JPEG_DECODE_STATUS.items() if v & bit) + f" (status {v})" for k, v in bad[:8])
            raise _lib.SfHipError(f"JPEG decode failed for {len(bad)} of {len(self.status)} files: {what}")

    # ------------------------------------------------------------------------------------------
    def coefficients(self, files: Sequence[bytes], strict: bool = True) -> Tensor:
        """The entropy decoder's output: int16 [N, blocks, 64], quantised, zigzagged, blocks in MCU scan order (the
        encoder's layout for "420" / "444"; Y0 Y1 Cb Cr for "422", raster 8x8 blocks for grayscale), padding MCUs included."""
        files, infos = self._parse(files)
        with torch.cuda.device(self.device):
            up, nbytes, info, max_iv = self._upload(files, infos)
            n = len(files)
            coef = torch.empty(n, info.blocks, 64, dtype=torch.int16, device=self.device)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            ops.jpeg_decode_entropy(up, nbytes, n, info.height, info.width, info.sampling, max_iv, self._workspace(n, info, max_iv), coef, status)
            self._finish(status, strict)
        return coef

    def _decode_resized(self, files: Sequence[bytes], layout: str, dtype, strict: bool, size, filter: str, fit: str) -> Tensor:
        """`decode` with `size`: the files' own size as uint8 "hwc" into a reused buffer, then the resizer into layout / dtype."""
        oh, ow = resize_mod.check_arguments(size, filter, dtype, None, fit, "JpegDecoder")
        files, infos = self._parse(files)
        n, h, w = len(files), infos[0].height, infos[0].width
        resize_mod.crop_box(h, w, oh, ow, None, fit)               # the ratio limit, before anything is uploaded
        with torch.cuda.device(self.device):
            up, nbytes, info, max_iv = self._upload(files, infos)
            if self._full is None or self._full.numel() < n * h * w * 3:
                self._full = torch.empty(n * h * w * 3, dtype=torch.uint8, device=self.device)
            full = self._full[:n * h * w * 3].view(n, h, w, 3)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            ops.jpeg_decode_frames(up, nbytes, n, h, w, info.sampling, max_iv, self._workspace(n, info, max_iv), full, "hwc", status)
            if self._resizer is None:
                self._resizer = resize_mod.FrameResizer(self.device)
            out = self._resizer.resize(full, (oh, ow), filter, "hwc", layout, dtype, fit=fit)
            self._finish(status, strict)
        return out

    def decode(self, files: Sequence[bytes], layout: str = "hwc", dtype=torch.uint8, strict: bool = True, size: Optional[Sequence[int]] = None,
               filter: str = "bilinear", fit: str = "stretch") -> Tensor:
        """The files' frames.  layout "hwc": [N, H, W, 3] (what `JpegEncoder` takes as uint8); "pose": [3, N, H, W] (what
        `PoseEmbedder.embed` / `PoseStream.push` take); "chw": [N, 3, H, W] (what the VAE encoders take as float).  dtype
        uint8: the samples; float32 / bfloat16: u8 / 127.5 - 1 (each operation rounded to fp32, bf16 to nearest even).
        A damaged file (a truncated scan, a bad code) raises SfHipError naming the file and what is wrong with it; with
        strict=False the frames are returned anyway (undecoded blocks are grey) and `self.status` holds each file's bits.
        size=(H, W): the frames resized on the device to H x W as `FrameResizer.resize` does it (`filter` "bilinear" /
        "bicubic", `fit` "stretch" / "cover"; Pillow's bits on the decoded samples): they are decoded as uint8 "hwc" into a
        buffer the decoder keeps, then resampled into `layout` / `dtype`."""
        if layout not in _lib.JPEG_LAYOUTS:
            raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
        if dtype not in _DECODE_DTYPES:
            raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
        if size is not None:
            return self._decode_resized(files, layout, dtype, strict, size, filter, fit)
        files, infos = self._parse(files)
        with torch.cuda.device(self.device):
            up, nbytes, info, max_iv = self._upload(files, infos)
            n, h, w = len(files), info.height, info.width
            shape = {"hwc": (n, h, w, 3), "pose": (3, n, h, w), "chw": (n, 3, h, w)}[layout]
            out = torch.empty(shape, dtype=dtype, device=self.device)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            ops.jpeg_decode_frames(up, nbytes, n, h, w, info.sampling, max_iv, self._workspace(n, info, max_iv), out, layout, status)
            self._finish(status, strict)
        return out


def pose_feed(files: Sequence[bytes], decoder: JpegDecoder, frames_per_piece: int = 12, size: Optional[Sequence[int]] = None, filter: str = "bilinear",
              fit: str = "stretch") -> Iterator[Tensor]:
    """JPEG pose frames as the pieces `CausalInferencePipeline.stream(pose_feed=...)` pulls: uint8 [3, n, H, W], n =
    `frames_per_piece` (the last piece may be shorter), each decoded when it is asked for.  `files` may be any iterable,
    a live source included.  size=(H, W) resizes every piece on the device (`JpegDecoder.decode(size=, filter=, fit=)`), so
    the source's frames may have any size."""
    if frames_per_piece < 1:
        raise ValueError(f"frames_per_piece must be >= 1, got {frames_per_piece}")
    if size is not None:
        resize_mod.check_arguments(size, filter, torch.uint8, None, fit, "pose_feed")
    piece: List[bytes] = []
    for f in files:
        piece.append(f)
        if len(piece) == frames_per_piece:
            yield decoder.decode(piece, layout="pose", size=size, filter=filter, fit=fit)
            piece = []
    if piece:
        yield decoder.decode(piece, layout="pose", size=size, filter=filter, fit=fit)
