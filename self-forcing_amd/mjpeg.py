"""Motion-JPEG in a RIFF AVI container: every frame is a whole JPEG file in a `00dc` chunk, the stream's codec is `MJPG`,
and an `idx1` index lists the chunks.  No container library: the layout below is the AVI 1.0 one (one video stream, no
audio, no OpenDML extension, so a file stays below 2 GiB)."""
from __future__ import annotations

import struct
from typing import List, Sequence

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_MAX_RIFF = (1 << 31) - 1


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _list(kind: bytes, payload: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload


def write_avi(path: str, frames: Sequence[bytes], fps: float, width: int, height: int) -> None:
    """Write `frames` (JPEG files of width x height) as an MJPEG AVI at `fps` frames per second."""
    frames = [bytes(f) for f in frames]
    if not frames:
        raise ValueError("write_avi: no frames")
    if any(f[:2] != b"\xff\xd8" for f in frames):
        raise ValueError("write_avi: every frame must be a JPEG file (SOI marker missing)")
    if not fps > 0 or width <= 0 or height <= 0:
        raise ValueError(f"write_avi: bad fps / size ({fps}, {width}x{height})")
    scale = 1000
    rate = int(round(fps * scale))
    biggest = max(len(f) for f in frames)
    movi, index, pos = bytearray(), bytearray(), 4                      # idx1 offsets count from the 'movi' fourcc
    for f in frames:
        index += b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, pos, len(f))
        c = _chunk(b"00dc", f)
        movi += c
        pos += len(c)
    avih = struct.pack("<14I", int(round(1e6 / fps)), int(biggest * fps), 0, AVIF_HASINDEX, len(frames), 0, 1, biggest,
                       width, height, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, len(frames), biggest, 0xFFFFFFFF, 0,
                                           0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    body = b"AVI " + hdrl + _list(b"movi", bytes(movi)) + _chunk(b"idx1", bytes(index))
    if len(body) > _MAX_RIFF:
        raise ValueError(f"write_avi: {len(body)} bytes do not fit one RIFF chunk; split the clip")
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def read_avi(path: str) -> List[bytes]:
    """The `00dc` chunks of an AVI file's `movi` list, in order."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    end = 8 + struct.unpack_from("<I", data, 4)[0]
    if end > len(data):
        raise ValueError(f"{path}: truncated (RIFF size {end}, file {len(data)})")
    pos, frames = 12, []
    while pos + 8 <= end:
        fourcc, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if fourcc == b"LIST" and data[pos + 8:pos + 12] == b"movi":
            p, stop = pos + 12, pos + 8 + size
            while p + 8 <= stop:
                cid, n = data[p:p + 4], struct.unpack_from("<I", data, p + 4)[0]
                if cid == b"00dc":
                    frames.append(data[p + 8:p + 8 + n])
                p += 8 + n + (n & 1)
        pos += 8 + size + (size & 1)
    return frames
