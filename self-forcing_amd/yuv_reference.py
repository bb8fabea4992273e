"""Raw YUV frames <-> RGB, the definition (numpy, exact integer arithmetic): what csrc/yuv.hip equals bit for bit.

Formats (8 bit, tightly packed; ch = ceil(h / 2), cw = ceil(w / 2) where a format subsamples):
    i420   Y [h][w], U [ch][cw], V [ch][cw]
    nv12   Y [h][w], UV [ch][cw][2]
    i422   Y [h][w], U [h][cw], V [h][cw]
    i444   Y, U, V [h][w] each
    gray   Y [h][w]                             (decode only; U = V = 128)
    yuyv   [h][w / 2][4] = Y0 U Y1 V            (w even; decode only)
    uyvy   [h][w / 2][4] = U Y0 V Y1            (w even; decode only)

Constants: F(x) = int(x * 65536 + 0.5); (Kr, Kb) = (0.299, 0.114) for bt601, (0.2126, 0.0722) for bt709, Kg = 1 - Kr - Kb;
range "limited" scales luma by 219 / 255 (offset 16) and chroma by 224 / 255, "full" scales neither.  `constants` gives
(yoff, CY, CRV, CGU, CGV, CBU, YR, YG, YB, UR, UG, UB, VR, VG, VB, 0); YG, UB and VR are derived so that the rows close:
grey maps to U = V = 128 exactly, white to 255 (full) or 235 (limited).

    y = (Y - yoff) CY     cb = U - 128     cr = V - 128                       (arithmetic shifts, clamp to 0..255)
    R = clamp((y + CRV cr + 32768) >> 16)
    G = clamp((y - CGU cb - CGV cr + 32768) >> 16)
    B = clamp((y + CBU cb + 32768) >> 16)
    Y = clamp(( YR R + YG G + YB B + (yoff << 16) + 32768) >> 16)
    U = clamp((-UR R - UG G + UB B + (128 << 16) + 32767) >> 16)
    V = clamp(( VR R - VG G - VB B + (128 << 16) + 32767) >> 16)

For bt601 full the decode is `jpeg_reference.decode`'s colour step.  Chroma up-sampling is "nearest" (replication) or
"triangle": `jpeg_reference.upsample`, libjpeg's "fancy" filter for centre-sited chroma, edges replicated over the
component's true size.  MPEG-2's left-sited chroma is not modelled.  The encoder converts every pixel at full resolution
and averages: 2 x 2 as (a + b + c + d + 2) >> 2, 2 x 1 as (a + b + 1) >> 1, the edge's value standing in for the missing
column or row of an odd size."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from . import jpeg_reference as jr

FORMATS = {"i420": 0, "nv12": 1, "i422": 2, "i444": 3, "gray": 4, "yuyv": 5, "uyvy": 6}       # enum sf_yuv_format
ENCODE_FORMATS = ("i420", "nv12", "i422", "i444")
CHROMAS = {"nearest": 0, "triangle": 1}                                                       # enum sf_yuv_chroma
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("full", "limited")
MAX_SIZE = 16384                                                                              # SF_YUV_MAX_SIZE
# (horizontal, vertical) chroma step of a format
_STEP = {"i420": (2, 2), "nv12": (2, 2), "i422": (2, 1), "i444": (1, 1), "gray": (1, 1), "yuyv": (2, 1), "uyvy": (2, 1)}


def F(x: float) -> int:
    return int(x * 65536 + 0.5)


def check_format(fmt: str, h: int, w: int) -> Tuple[int, int]:
    """(h, w) as ints; ValueError for an unknown format, a size outside 1..MAX_SIZE or an odd width of a packed format."""
    if fmt not in FORMATS:
        raise ValueError(f"format must be one of {', '.join(FORMATS)}, got {fmt!r}")
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f"frame size must be 1..{MAX_SIZE} per axis, got {h}x{w}")
    if fmt in ("yuyv", "uyvy") and w % 2:
        raise ValueError(f"{fmt} needs an even width, got {w}")
    return h, w


def chroma_size(fmt: str, h: int, w: int) -> Tuple[int, int]:
    sx, sy = _STEP[fmt]
    return -(-h // sy), -(-w // sx)


def frame_bytes(fmt: str, h: int, w: int) -> int:
    h, w = check_format(fmt, h, w)
    if fmt == "gray":
        return h * w
    if fmt in ("yuyv", "uyvy"):
        return 2 * h * w
    ch, cw = chroma_size(fmt, h, w)
    return h * w + 2 * ch * cw


def plane_offsets(fmt: str, h: int, w: int) -> Dict[str, int]:
    """Byte offset of each plane's first sample in a frame (packed formats: of the first Y, U and V)."""
    h, w = check_format(fmt, h, w)
    ch, cw = chroma_size(fmt, h, w)
    if fmt == "gray":
        return {"y": 0}
    if fmt == "nv12":
        return {"y": 0, "u": h * w, "v": h * w + 1}
    if fmt == "yuyv":
        return {"y": 0, "u": 1, "v": 3}
    if fmt == "uyvy":
        return {"y": 1, "u": 0, "v": 2}
    return {"y": 0, "u": h * w, "v": h * w + ch * cw}


def check_colour(matrix: str, range: str) -> None:
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be 'bt601' or 'bt709', got {matrix!r}")
    if range not in RANGES:
        raise ValueError(f"range must be 'full' or 'limited', got {range!r}")


def check_chroma(chroma: str) -> None:
    if chroma not in CHROMAS:
        raise ValueError(f"chroma must be 'nearest' or 'triangle', got {chroma!r}")


def constants(matrix: str = "bt601", range: str = "limited") -> Tuple[int, ...]:
    """The sixteen integers the kernels take (the last one is 0, reserved)."""
    check_colour(matrix, range)
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    ls, cs, yoff = (219 / 255, 224 / 255, 16) if range == "limited" else (1.0, 1.0, 0)
    cy, crv, cbu = F(1 / ls), F(2 * (1 - kr) / cs), F(2 * (1 - kb) / cs)
    cgu, cgv = F(2 * kb * (1 - kb) / kg / cs), F(2 * kr * (1 - kr) / kg / cs)
    yr, yb = F(kr * ls), F(kb * ls)
    yg = F(ls) - yr - yb
    ur, ug = F(0.5 * kr / (1 - kb) * cs), F(0.5 * kg / (1 - kb) * cs)
    vg, vb = F(0.5 * kg / (1 - kr) * cs), F(0.5 * kb / (1 - kr) * cs)
    return (yoff, cy, crv, cgu, cgv, cbu, yr, yg, yb, ur, ug, ur + ug, vg + vb, vg, vb, 0)


def planes(raw, fmt: str, h: int, w: int) -> List[np.ndarray]:
    """One frame's bytes -> [Y [h, w], U, V] (uint8; the chroma planes at the format's own size; gray: [Y])."""
    need = frame_bytes(fmt, h, w)
    a = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else raw.reshape(-1)
    if a.size != need:
        raise ValueError(f"a {h}x{w} {fmt} frame has {need} bytes, got {a.size}")
    ch, cw = chroma_size(fmt, h, w)
    if fmt == "gray":
        return [a.reshape(h, w)]
    if fmt in ("yuyv", "uyvy"):
        p = a.reshape(h, w // 2, 4)
        iy, iu = (0, 1) if fmt == "yuyv" else (1, 0)
        return [p[:, :, [iy, iy + 2]].reshape(h, w), p[:, :, iu], p[:, :, iu + 2]]
    y, c = a[:h * w].reshape(h, w), a[h * w:]
    if fmt == "nv12":
        c = c.reshape(ch, cw, 2)
        return [y, c[:, :, 0], c[:, :, 1]]
    return [y, c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)]


def upsample(c: np.ndarray, fmt: str, h: int, w: int, chroma: str = "triangle") -> np.ndarray:
    """One chroma plane at the format's size -> int64 [h, w]."""
    check_chroma(chroma)
    sx, sy = _STEP[fmt]
    if chroma == "nearest" or (sx, sy) == (1, 1):
        return np.repeat(np.repeat(np.asarray(c, np.int64), sy, 0), sx, 1)[:h, :w]
    return jr.upsample(np.asarray(c), "420" if sy == 2 else "422", h, w)


def yuv_to_rgb(y, u, v, k) -> np.ndarray:
    """Samples (any equal shapes) -> uint8 [..., 3] with the constants `k`."""
    y = (np.asarray(y, np.int64) - k[0]) * k[1]
    cb, cr = np.asarray(u, np.int64) - 128, np.asarray(v, np.int64) - 128
    r = (y + k[2] * cr + 32768) >> 16
    g = (y - k[3] * cb - k[4] * cr + 32768) >> 16
    b = (y + k[5] * cb + 32768) >> 16
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def rgb_to_yuv(rgb, k) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [..., 3] = (Y, U, V) of every pixel."""
    rgb = np.asarray(rgb, np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (k[6] * r + k[7] * g + k[8] * b + (k[0] << 16) + 32768) >> 16
    u = (-k[9] * r - k[10] * g + k[11] * b + (128 << 16) + 32767) >> 16
    v = (k[12] * r - k[13] * g - k[14] * b + (128 << 16) + 32767) >> 16
    return np.clip(np.stack([y, u, v], -1), 0, 255).astype(np.uint8)


def decode(raw, fmt: str, h: int, w: int, matrix: str = "bt601", range: str = "limited", chroma: str = "triangle") -> np.ndarray:
    """One frame's bytes -> uint8 [h, w, 3]."""
    check_chroma(chroma)
    k = constants(matrix, range)
    p = planes(raw, fmt, h, w)
    if fmt == "gray":
        return yuv_to_rgb(p[0], 128, 128, k)
    return yuv_to_rgb(p[0], upsample(p[1], fmt, h, w, chroma), upsample(p[2], fmt, h, w, chroma), k)


def _box(c: np.ndarray, sx: int, sy: int) -> np.ndarray:
    h, w = c.shape
    c = np.pad(c.astype(np.int64), ((0, -h % sy), (0, -w % sx)), mode="edge")
    if sx == 2:
        c = c[:, 0::2] + c[:, 1::2]
    if sy == 2:
        c = c[0::2] + c[1::2]
    n = sx * sy
    return ((c + n // 2) >> (n.bit_length() - 1)).astype(np.uint8)


def encode(rgb_u8, fmt: str = "i420", matrix: str = "bt601", range: str = "limited") -> bytes:
    """uint8 [h, w, 3] -> one frame's bytes."""
    if fmt not in ENCODE_FORMATS:
        raise ValueError(f"the encoder writes {', '.join(ENCODE_FORMATS)}, got {fmt!r}")
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected uint8 [h, w, 3], got {rgb.dtype} {rgb.shape}")
    check_format(fmt, rgb.shape[0], rgb.shape[1])
    yuv = rgb_to_yuv(rgb, constants(matrix, range))
    sx, sy = _STEP[fmt]
    u, v = _box(yuv[..., 1], sx, sy), _box(yuv[..., 2], sx, sy)
    if fmt == "nv12":
        return yuv[..., 0].tobytes() + np.stack([u, v], -1).tobytes()
    return yuv[..., 0].tobytes() + u.tobytes() + v.tobytes()
