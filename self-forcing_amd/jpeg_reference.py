"""Host reference of the JPEG format the GPU encoder writes (csrc/jpeg.hip), in numpy float64, written from ITU-T T.81
and the JFIF 1.02 note.  It is the oracle of the tests and the documentation of the format; nothing here is fast.

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
