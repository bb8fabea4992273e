"""Host reference of the JPEG format the GPU encoder writes (csrc/jpeg.hip), in numpy float64, written from ITU-T T.81
and the JFIF 1.02 note.  It is the oracle of the tests and the documentation of the format; nothing here is fast.  The
second half (`parse`, `decode_coefficients`, `decode`) is the definition of the GPU decoder (csrc/jpeg_decode.hip), in
exact integers; it takes more than the encoder writes (any tables, 4:2:2, grayscale, any size, files without DRI).

The format: baseline sequential JFIF, 8 bit, three components (Y, Cb, Cr; JFIF's full-range BT.601 matrix), 4:2:0 (chroma =
the 2x2 mean) or 4:4:4, libjpeg's quality scaling of the Annex K quantisation tables, the Annex K Huffman tables, a DRI
segment and RST0..7 markers every `restart_interval` MCUs.

The numbers, stage by stage (the GPU runs the same definition: the truncation in fp32 as torch does, the rest in fp64):
  u8      = trunc(clamp(p, -1, 1) * 127.5 + 127.5)  for value_range (-1, 1); trunc(255 * clamp(x, 0, 1)) for (0, 1); fp32
  Y,Cb,Cr = the JFIF matrix on u8; Y - 128 (level shift), Cb and Cr without their + 128
  chroma  = mean of each 2x2 for "420"
  c       = D X D^T, the orthonormal 8x8 DCT-II
  q       = rint(c / Q) (ties to even), zigzagged, int16
  blocks  = MCU-interleaved scan order: Y00 Y01 Y10 Y11 Cb Cr per 16x16 MCU for "420", Y Cb Cr per 8x8 MCU for "444"
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import numpy as np

SUBSAMPLINGS = {"420": 0, "444": 1}

# T.81 Annex K.1: luminance / chrominance quantisation tables (natural order)
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32)

# T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the four typical tables
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
# (class, id) -> (BITS, HUFFVAL), in the order the header writes them
HUFFMAN_SPECS = {(0, 0): (DC_LUMA_BITS, DC_VALS), (1, 0): (AC_LUMA_BITS, AC_LUMA_VALS),
                 (0, 1): (DC_CHROMA_BITS, DC_VALS), (1, 1): (AC_CHROMA_BITS, AC_CHROMA_VALS)}


def _zigzag() -> np.ndarray:
    """ZIGZAG[k] = natural index (row * 8 + column) of the k-th coefficient of the scan (T.81 figure 5)."""
    order = []
    for s in range(15):
        rows = range(max(0, s - 7), min(s, 7) + 1)
        order += [r * 8 + (s - r) for r in (rows if s % 2 else reversed(rows))]
    return np.array(order)


ZIGZAG = _zigzag()
# D[k][n] = c(k) / 2 cos((2n + 1) k pi / 16), c(0) = 1 / sqrt(2): the orthonormal DCT-II
DCT = np.array([[(np.sqrt(0.5) if k == 0 else 1.0) / 2 * np.cos((2 * n + 1) * k * np.pi / 16) for n in range(8)] for k in range(8)])


def mcu_size(subsampling: str) -> int:
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be '420' or '444', got {subsampling!r}")
    return 16 if subsampling == "420" else 8


def check_geometry(h: int, w: int, subsampling: str) -> Tuple[int, int]:
    """(MCUs per row, MCU rows); ValueError when the frame does not fit the MCU grid."""
    m = mcu_size(subsampling)
    if h <= 0 or w <= 0 or h % m or w % m:
        raise ValueError(f"frame {h}x{w} is not a multiple of the {m}x{m} MCU of subsampling {subsampling!r}")
    if h > 65535 or w > 65535:
        raise ValueError(f"frame {h}x{w} exceeds JPEG's 65535")
    return w // m, h // m


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """libjpeg's jpeg_set_quality on the Annex K tables (baseline: entries clamped to 1..255); natural order."""
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be 1..100, got {quality}")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(bits: Sequence[int], vals: Sequence[int]) -> dict:
    """symbol -> (code, length), T.81 Annex C."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def to_uint8(frames, value_range=(-1, 1)) -> np.ndarray:
    """Float frames [N, 3, H, W] -> uint8 [N, H, W, 3] by the demo's truncation, in fp32 as torch computes it."""
    x = np.asarray(frames, dtype=np.float32)
    if tuple(value_range) == (-1, 1):
        y = np.clip(x, np.float32(-1), np.float32(1)) * np.float32(127.5) + np.float32(127.5)
    elif tuple(value_range) == (0, 1):
        y = np.float32(255) * np.clip(x, np.float32(0), np.float32(1))
    else:
        raise ValueError(f"value_range must be (-1, 1) or (0, 1), got {value_range}")
    return np.ascontiguousarray(np.trunc(y).astype(np.uint8).transpose(0, 2, 3, 1))


def _blocks(plane: np.ndarray) -> np.ndarray:
    """[N, H, W] -> [N, H/8, W/8, 8, 8]"""
    n, h, w = plane.shape
    return plane.reshape(n, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4)


def coefficients(frames_u8: np.ndarray, quality: int, subsampling: str = "420", dtype=np.float64) -> np.ndarray:
    """uint8 frames [N, H, W, 3] -> quantised zigzagged coefficients, int16 [N, blocks, 64] in MCU scan order."""
    u8 = np.asarray(frames_u8)
    if u8.dtype != np.uint8 or u8.ndim != 4 or u8.shape[3] != 3:
        raise ValueError(f"expected uint8 [N, H, W, 3], got {u8.dtype} {u8.shape}")
    n, h, w, _ = u8.shape
    mx, my = check_geometry(h, w, subsampling)
    ql, qc = (q.astype(dtype) for q in quant_tables(quality))
    r, g, b = (u8[..., i].astype(dtype) for i in range(3))
    f = dtype
    y = f(0.299) * r + f(0.587) * g + f(0.114) * b - f(128)
    cb = f(-0.168736) * r - f(0.331264) * g + f(0.5) * b
    cr = f(0.5) * r - f(0.418688) * g - f(0.081312) * b
    if subsampling == "420":
        cb, cr = (c.reshape(n, h // 2, 2, w // 2, 2).sum(axis=(2, 4)) * f(0.25) for c in (cb, cr))
    d = DCT.astype(dtype)

    def quantised(plane, q):
        c = d @ _blocks(plane) @ d.T                                  # [N, by, bx, 8, 8]
        z = np.rint(c.reshape(*c.shape[:3], 64) / q)[..., ZIGZAG]
        return z.astype(np.int16)

    yq, cbq, crq = quantised(y, ql), quantised(cb, qc), quantised(cr, qc)
    if subsampling == "420":
        yq = yq.reshape(n, my, 2, mx, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(n, my * mx, 4, 64)
    else:
        yq = yq.reshape(n, my * mx, 1, 64)
    out = np.concatenate([yq, cbq.reshape(n, my * mx, 1, 64), crq.reshape(n, my * mx, 1, 64)], axis=2)
    return np.ascontiguousarray(out.reshape(n, -1, 64))


# ------------------------------------------------------------------------------------------------- entropy coding
class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, length: int):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)                                     # byte stuffing, T.81 F.1.2.3
        self.acc &= (1 << self.n) - 1

    def finish(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)              # pad with 1-bits
        return bytes(self.out)


def _magnitude(v: int) -> Tuple[int, int]:
    """(category, the category's low bits): T.81 F.1.2.1; negative values are coded as v - 1."""
    cat = abs(v).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


_CODES = {key: huffman_codes(*spec) for key, spec in HUFFMAN_SPECS.items()}


def blocks_per_mcu(subsampling: str) -> int:
    return 6 if mcu_size(subsampling) == 16 else 3


def _components(subsampling: str) -> List[int]:
    return [0, 0, 0, 0, 1, 2] if subsampling == "420" else [0, 1, 2]


def entropy_intervals(coef: np.ndarray, subsampling: str, restart_interval: int) -> List[bytes]:
    """One frame's coefficients [blocks, 64] -> the entropy-coded bytes of each restart interval (stuffed, padded)."""
    comps = _components(subsampling)
    bpm = len(comps)
    coef = np.asarray(coef).astype(np.int64).reshape(-1, 64)
    mcus = coef.shape[0] // bpm
    if coef.shape[0] != mcus * bpm or restart_interval < 1:
        raise ValueError("coefficient count / restart interval do not fit the MCU")
    out = []
    for start in range(0, mcus, restart_interval):
        bw, pred = _BitWriter(), [0, 0, 0]
        for m in range(start, min(start + restart_interval, mcus)):
            for k, comp in enumerate(comps):
                blk = coef[m * bpm + k]
                tid = 0 if comp == 0 else 1
                dc, ac = _CODES[(0, tid)], _CODES[(1, tid)]
                cat, low = _magnitude(int(blk[0]) - pred[comp])
                pred[comp] = int(blk[0])
                code, length = dc[cat]
                bw.put((code << cat) | low, length + cat)
                run_from = 1
                for pos in np.flatnonzero(blk[1:]) + 1:
                    run = int(pos) - run_from
                    while run >= 16:
                        bw.put(*ac[0xF0])                              # ZRL
                        run -= 16
                    cat, low = _magnitude(int(blk[pos]))
                    code, length = ac[(run << 4) | cat]
                    bw.put((code << cat) | low, length + cat)
                    run_from = int(pos) + 1
                if run_from <= 63:
                    bw.put(*ac[0x00])                                  # EOB
        out.append(bw.finish())
    return out


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(h: int, w: int, quality: int, subsampling: str = "420", restart_interval: int = 1) -> bytes:
    """SOI, APP0 (JFIF 1.01, no density), DQT x 2, SOF0, DHT x 4, DRI, SOS: depends on nothing but its arguments."""
    check_geometry(h, w, subsampling)
    if not 1 <= restart_interval <= 65535:
        raise ValueError(f"restart_interval must be 1..65535, got {restart_interval}")
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for tid, q in enumerate((ql, qc)):
        out += _segment(0xDB, bytes([tid]) + bytes(int(v) for v in q[ZIGZAG]))
    hv = 0x22 if subsampling == "420" else 0x11
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (cls, tid), (bits, vals) in HUFFMAN_SPECS.items():
        out += _segment(0xC4, bytes([(cls << 4) | tid]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode_coefficients(coef: np.ndarray, h: int, w: int, quality: int, subsampling: str = "420", restart_interval: int = 1) -> bytes:
    """One frame's coefficient buffer -> the whole file."""
    mx, my = check_geometry(h, w, subsampling)
    if np.asarray(coef).size != mx * my * blocks_per_mcu(subsampling) * 64:
        raise ValueError("coefficient buffer does not match the frame")
    body = bytearray()
    for i, chunk in enumerate(entropy_intervals(coef, subsampling, restart_interval)):
        if i:
            body += bytes([0xFF, 0xD0 + (i - 1) % 8])
        body += chunk
    return header(h, w, quality, subsampling, restart_interval) + bytes(body) + b"\xff\xd9"


def encode(frames_u8: np.ndarray, quality: int = 90, subsampling: str = "420", restart_interval: int = 1) -> List[bytes]:
    """uint8 frames [N, H, W, 3] -> one JPEG file per frame."""
    coef = coefficients(frames_u8, quality, subsampling)
    h, w = frames_u8.shape[1:3]
    return [encode_coefficients(c, h, w, quality, subsampling, restart_interval) for c in coef]


# ================================================================================================= decoding
# The definition of the GPU decoder (csrc/jpeg_decode.hip), in exact integers: `parse` reads a file's header segments,
# `decode_coefficients` the entropy-coded scan, `decode` the pixels.  Accepted: baseline sequential DCT (SOF0), 8 bit,
# Huffman, one interleaved scan; Y Cb Cr with luma sampling 1x1 / 2x1 / 2x2 and chroma 1x1, or one component; up to four
# 8-bit DQT and 4 + 4 DHT tables of any content; with or without DRI; any H, W >= 1 (the padding blocks are decoded and
# cropped).  Everything else is a ValueError that names the reason.
#
#   X       = coef * Q                                 integers, natural order
#   t       = IDCT_INT^T X IDCT_INT                    exact (64-bit), IDCT_INT[k][n] = rint(2^13 b(k, n))
#   sample  = clamp(((t + 2^25) >> 26) + 128, 0, 255)  arithmetic shift
#   chroma  = libjpeg's "fancy" triangle filter over the component's true size, edges replicated
#   r, g, b = the JFIF matrix in 16.16 fixed point (F(x) = int(x * 65536 + 0.5)), clamped
#
# An integer IDCT because a DC-only block is DC * Q / 8 + 128, an exact tie one time in eight: a float evaluation's order
# would decide those pixels, and a pose frame is mostly such blocks.
DECODE_SAMPLINGS = {"420": 0, "444": 1, "422": 2, "gray": 3}
# sampling -> (luma blocks across, down) of one MCU
_LUMA_BLOCKS = {"420": (2, 2), "444": (1, 1), "422": (2, 1), "gray": (1, 1)}
IDCT_BITS = 13
IDCT_INT = np.rint(DCT * (1 << IDCT_BITS)).astype(np.int64)           # [k][n]
LOOKUP_BITS = 9                                                        # first-level Huffman lookup of the decoder


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


FIX_CR_R, FIX_CB_G, FIX_CR_G, FIX_CB_B = _fix(1.402), _fix(0.344136286), _fix(0.714136286), _fix(1.772)

_SOF_NAMES = {0xC1: "extended sequential DCT", 0xC2: "progressive DCT", 0xC3: "lossless", 0xC5: "differential sequential DCT",
              0xC6: "differential progressive DCT", 0xC7: "differential lossless", 0xC9: "arithmetic coding", 0xCA: "arithmetic coding",
              0xCB: "arithmetic coding", 0xCD: "arithmetic coding", 0xCE: "arithmetic coding", 0xCF: "arithmetic coding"}


class JpegInfo:
    """What `parse` reads from a file's header segments.

    height, width; sampling ("420" / "444" / "422" / "gray"); restart_interval (MCUs, 0 = no DRI); quant: per component the
    quantiser in natural order (int64 [64]); dc / ac: per component (BITS, HUFFVAL); scan_offset / scan_end: the entropy-coded
    bytes are file[scan_offset:scan_end] (scan_end = where the EOI marker stands)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def components(self) -> int:
        return 1 if self.sampling == "gray" else 3

    @property
    def mcu_grid(self) -> Tuple[int, int]:
        """(MCUs per row, MCU rows), the padding MCUs included."""
        bx, by = _LUMA_BLOCKS[self.sampling]
        return -(-self.width // (8 * bx)), -(-self.height // (8 * by))

    @property
    def blocks_per_mcu(self) -> int:
        bx, by = _LUMA_BLOCKS[self.sampling]
        return bx * by + (0 if self.sampling == "gray" else 2)

    @property
    def blocks(self) -> int:
        mx, my = self.mcu_grid
        return mx * my * self.blocks_per_mcu

    @property
    def intervals(self) -> int:
        mx, my = self.mcu_grid
        return -(-(mx * my) // self.restart_interval) if self.restart_interval else 1


def parse(file: bytes) -> JpegInfo:
    """Read the header segments of one file (nothing of the scan); ValueError for whatever the decoder does not take."""
    data = bytes(file)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: SOI marker missing")
    quant, huff, frame, ri, pos = {}, {}, None, 0, 2
    while True:
        while pos < len(data) and data[pos] == 0xFF and pos + 1 < len(data) and data[pos + 1] == 0xFF:
            pos += 1                                                   # fill bytes in front of a marker, T.81 B.1.1.2
        if pos + 4 > len(data):
            raise ValueError("SOF / SOS marker missing: the file ends inside its header" if frame is None
                             else "SOS marker missing: the file ends inside its header")
        if data[pos] != 0xFF:
            raise ValueError(f"no marker at byte {pos} of the header")
        marker, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if marker == 0xD9:
            raise ValueError("SOS marker missing: EOI in the header" if frame is not None else "SOF marker missing: EOI in the header")
        if length < 2 or pos + 2 + length > len(data):
            raise ValueError(f"segment length {length} of marker 0x{marker:02X} runs past the file")
        p = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker in _SOF_NAMES:
            raise ValueError(f"{_SOF_NAMES[marker]} (SOF marker 0x{marker:02X}) is not baseline sequential DCT")
        if marker == 0xC0:
            if frame is not None:
                raise ValueError("a second SOF segment")
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise ValueError("malformed SOF segment")
            if p[0] != 8:
                raise ValueError(f"{p[0]} bit samples: only 8 bit is baseline")
            frame = (int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big"), [(p[6 + 3 * i], p[7 + 3 * i], p[8 + 3 * i]) for i in range(p[5])])
        elif marker == 0xDB:
            while p:
                if p[0] >> 4:
                    raise ValueError("16-bit DQT table: only 8-bit tables are baseline")
                if (p[0] & 15) > 3 or len(p) < 65:
                    raise ValueError("malformed DQT segment")
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(p[1:65], np.uint8)
                quant[p[0] & 15] = q
                p = p[65:]
        elif marker == 0xC4:
            while p:
                if len(p) < 17 or (p[0] >> 4) > 1 or (p[0] & 15) > 3:
                    raise ValueError("malformed DHT segment")
                bits = list(p[1:17])
                if len(p) < 17 + sum(bits) or sum(bits) > 256:
                    raise ValueError("malformed DHT segment")
                huff[(p[0] >> 4, p[0] & 15)] = (bits, list(p[17:17 + sum(bits)]))
                p = p[17 + sum(bits):]
        elif marker == 0xDD:
            if len(p) != 2:
                raise ValueError("malformed DRI segment")
            ri = int.from_bytes(p, "big")
        elif marker == 0xDA:
            break
        elif not (0xE0 <= marker <= 0xEF or marker == 0xFE):
            raise ValueError(f"marker 0x{marker:02X} in the header is not supported")
    if frame is None:
        raise ValueError("SOF marker missing in front of SOS")
    h, w, comps = frame
    if h < 1 or w < 1:
        raise ValueError(f"frame {h}x{w}: the size must be given in SOF")
    if len(comps) not in (1, 3):
        raise ValueError(f"{len(comps)} components: only Y Cb Cr or grayscale")
    if len(p) < 1 or len(p) != 4 + 2 * p[0]:
        raise ValueError("malformed SOS segment")
    if p[0] != len(comps):
        raise ValueError(f"a scan of {p[0]} of {len(comps)} components: multiple scans are not supported")
    if tuple(p[-3:]) != (0, 63, 0):
        raise ValueError("spectral selection / successive approximation in SOS: not baseline")
    if len(comps) == 1:
        sampling = "gray"
    else:
        hv = [c[1] for c in comps]
        sampling = {0x11: "444", 0x21: "422", 0x22: "420"}.get(hv[0])
        if sampling is None or hv[1] != 0x11 or hv[2] != 0x11:
            raise ValueError("sampling factors " + " ".join(f"{v >> 4}x{v & 15}" for v in hv) + ": only 1x1 / 2x1 / 2x2 luma over 1x1 chroma")
    q, dc, ac = [], [], []
    for i, (cid, _, tq) in enumerate(comps):
        if p[1 + 2 * i] != cid:
            raise ValueError("the scan's components are not in the frame's order")
        td, ta = p[2 + 2 * i] >> 4, p[2 + 2 * i] & 15
        if tq not in quant or (0, td) not in huff or (1, ta) not in huff:
            raise ValueError(f"component {cid} uses a table the file does not define")
        q.append(quant[tq])
        dc.append(huff[(0, td)])
        ac.append(huff[(1, ta)])
    for bits, vals in dc + ac:
        decode_tables(bits, vals)                                      # ValueError for an over-subscribed code
    end = data.rfind(b"\xff\xd9")
    if end < pos:
        raise ValueError("EOI marker missing")
    return JpegInfo(height=h, width=w, sampling=sampling, restart_interval=ri, quant=q, dc=dc, ac=ac, scan_offset=pos, scan_end=end)


def decode_tables(bits: Sequence[int], vals: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The decoder's form of one Huffman table (T.81 F.2.2.3): (look uint16 [512], maxcode int32 [18], valoff int32 [18],
    vals uint8 [256]).  look[next 9 bits] = (length << 8) | symbol for codes of up to 9 bits, 0 for longer ones; a code of
    length L > 9 is the first L for which the next L bits are <= maxcode[L] (-1: no code of that length), its symbol
    vals[code + valoff[L]].  The arrays are cached per table: read them, do not write them."""
    return _decode_tables(tuple(int(b) for b in bits), bytes(bytearray(vals)))


@functools.lru_cache(maxsize=256)
def _decode_tables(bits: tuple, vals: bytes):
    look = np.zeros(1 << LOOKUP_BITS, np.uint16)
    maxcode, valoff = np.full(18, -1, np.int32), np.zeros(18, np.int32)
    table = np.zeros(256, np.uint8)
    table[:len(vals)] = np.frombuffer(vals, np.uint8)
    code, k = 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if n:
            if code + n > (1 << length):
                raise ValueError("a DHT table assigns more codes than its lengths allow")
            valoff[length] = k - code
            maxcode[length] = code + n - 1
            if length <= LOOKUP_BITS:
                for i in range(n):
                    lo = (code + i) << (LOOKUP_BITS - length)
                    look[lo:lo + (1 << (LOOKUP_BITS - length))] = (length << 8) | int(table[k + i])
            code += n
            k += n
        code <<= 1
    return look, maxcode, valoff, table


class _BitReader:
    """The bits of one restart interval: 0xFF 0x00 unstuffed; zeros behind the end, and `overrun` says they were used."""

    def __init__(self, data: bytes):
        self.data, self.pos, self.acc, self.n, self.phantom = data.replace(b"\xff\x00", b"\xff"), 0, 0, 0, 0

    def _fill(self, want: int):
        while self.n < want:
            if self.pos < len(self.data):
                byte = self.data[self.pos]
            else:
                byte, self.phantom = 0, self.phantom + 8
            self.pos += 1
            self.acc = ((self.acc << 8) | byte) & 0xFFFFFFFFFFFF
            self.n += 8

    def peek(self, length: int) -> int:
        self._fill(length)
        return (self.acc >> (self.n - length)) & ((1 << length) - 1)

    def skip(self, length: int):
        self.n -= length

    def receive(self, size: int) -> int:
        """T.81 F.2.2.1 EXTEND of the next `size` bits."""
        if size == 0:
            return 0
        v = self.peek(size)
        self.skip(size)
        return v if v >> (size - 1) else v - (1 << size) + 1

    @property
    def overrun(self) -> bool:
        return self.n < self.phantom


def _symbol(br: _BitReader, tables) -> int:
    look, maxcode, valoff, vals = tables
    e = int(look[br.peek(LOOKUP_BITS)])
    if e:
        br.skip(e >> 8)
        return e & 255
    for length in range(LOOKUP_BITS + 1, 17):
        code = br.peek(length)
        if code <= maxcode[length]:
            br.skip(length)
            return int(vals[(code + int(valoff[length])) & 255])
    raise ValueError("bad Huffman code in the scan")


def block_components(sampling: str) -> List[int]:
    """The component of each block of one MCU."""
    bx, by = _LUMA_BLOCKS[sampling]
    return [0] * (bx * by) + ([] if sampling == "gray" else [1, 2])


def decode_coefficients(file: bytes, info: JpegInfo = None) -> np.ndarray:
    """The scan's quantised coefficients, int16 [blocks, 64], zigzagged, blocks in MCU scan order (Y.. Cb Cr per MCU: the
    encoder's layout for "420" / "444", Y0 Y1 Cb Cr for "422", raster 8x8 blocks for grayscale), the padding MCUs included."""
    import re
    info = info or parse(file)
    scan = bytes(file)[info.scan_offset:info.scan_end]
    marks = [m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", scan)]
    if len(marks) != info.intervals - 1:
        raise ValueError(f"{len(marks)} restart markers in the scan, {info.intervals - 1} expected")
    comps = block_components(info.sampling)
    bpm = len(comps)
    mcus = info.blocks // bpm
    ri = info.restart_interval or mcus
    dc = [decode_tables(*t) for t in info.dc]
    ac = [decode_tables(*t) for t in info.ac]
    out = np.zeros((info.blocks, 64), np.int64)
    for iv, (a, b) in enumerate(zip([0] + [m + 2 for m in marks], marks + [len(scan)])):
        br, pred = _BitReader(scan[a:b]), [0, 0, 0]
        for blk in range(iv * ri * bpm, min((iv + 1) * ri, mcus) * bpm):
            comp = comps[blk % bpm]
            size = _symbol(br, dc[comp])
            if size > 11:
                raise ValueError("bad Huffman code in the scan: a DC category beyond 11")
            pred[comp] += br.receive(size)
            out[blk, 0] = pred[comp]
            k = 1
            while k < 64:
                rs = _symbol(br, ac[comp])
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run != 15:
                        break                                          # EOB
                    k += 16                                            # ZRL
                    continue
                k += run
                if k > 63:
                    raise ValueError("a zero run past the 63rd coefficient")
                out[blk, k] = br.receive(size)
                k += 1
        if br.overrun:
            raise ValueError(f"restart interval {iv} is truncated")
    return out.astype(np.int16)


def idct_blocks(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Zigzagged coefficients [..., 64] and a quantiser (natural order) -> uint8 samples [..., 8, 8] by the integer IDCT."""
    x = np.zeros(coef.shape, np.int64)
    x[..., ZIGZAG] = coef.astype(np.int64)
    x = (x * q.astype(np.int64)).reshape(*coef.shape[:-1], 8, 8)
    t = np.einsum("kn,...kl,lm->...nm", IDCT_INT, x, IDCT_INT)
    return np.clip(((t + (1 << (2 * IDCT_BITS - 1))) >> (2 * IDCT_BITS)) + 128, 0, 255).astype(np.uint8)


def component_planes(coef: np.ndarray, info: JpegInfo) -> List[np.ndarray]:
    """The components' sample planes (uint8, padded to whole MCUs) of one file's coefficient buffer."""
    mx, my = info.mcu_grid
    bx, by = _LUMA_BLOCKS[info.sampling]
    c = np.asarray(coef).reshape(my, mx, info.blocks_per_mcu, 64)
    luma = idct_blocks(c[:, :, :bx * by], info.quant[0]).reshape(my, mx, by, bx, 8, 8)
    planes = [luma.transpose(0, 2, 4, 1, 3, 5).reshape(my * by * 8, mx * bx * 8)]
    for i in range(1, info.components):
        s = idct_blocks(c[:, :, bx * by + i - 1], info.quant[i])       # [my, mx, 8, 8]
        planes.append(s.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return planes


def upsample(c: np.ndarray, sampling: str, h: int, w: int) -> np.ndarray:
    """One chroma plane (padded) -> [h, w] by libjpeg's "fancy" triangle filter over the component's true size."""
    bx, by = _LUMA_BLOCKS[sampling]
    ch, cw = -(-h // by), -(-w // bx)
    c = c[:ch, :cw].astype(np.int64)
    prev = lambda a, axis: np.concatenate([a.take([0], axis), a.take(range(a.shape[axis] - 1), axis)], axis)          # noqa: E731
    nxt = lambda a, axis: np.concatenate([a.take(range(1, a.shape[axis]), axis), a.take([-1], axis)], axis)           # noqa: E731
    if by == 2:
        t = np.empty((2 * ch, cw), np.int64)
        t[0::2], t[1::2] = 3 * c + prev(c, 0), 3 * c + nxt(c, 0)
        out = np.empty((2 * ch, 2 * cw), np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * t + prev(t, 1) + 8) >> 4, (3 * t + nxt(t, 1) + 7) >> 4
    elif bx == 2:
        out = np.empty((ch, 2 * cw), np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * c + prev(c, 1) + 1) >> 2, (3 * c + nxt(c, 1) + 2) >> 2
    else:
        out = c
    return out[:h, :w]


def decode(file: bytes) -> np.ndarray:
    """One file -> uint8 [H, W, 3]."""
    info = parse(file)
    planes = component_planes(decode_coefficients(file, info), info)
    h, w = info.height, info.width
    y = planes[0][:h, :w].astype(np.int64)
    if info.components == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    cb, cr = (upsample(p, info.sampling, h, w) - 128 for p in planes[1:])
    r = y + ((FIX_CR_R * cr + 32768) >> 16)
    g = y + ((-FIX_CB_G * cb - FIX_CR_G * cr + 32768) >> 16)
    b = y + ((FIX_CB_B * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def to_float(u8: np.ndarray) -> np.ndarray:
    """u8 / 127.5 - 1, the divide and the subtract each rounded to fp32: the range the VAE encoders take."""
    return np.asarray(u8).astype(np.float32) / np.float32(127.5) - np.float32(1)
