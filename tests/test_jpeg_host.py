"""Host-side tests of the JPEG path (no GPU): the float64 reference encoder `jpeg_reference` against PIL (tables, decodable
files, quality and size against PIL's own encode), the MJPEG AVI writer, and the argument checks of the C entry points.

The bounds against PIL are conditions, not measurements: a file of the reference may decode at most 0.1 dB below PIL's
own encode at the same quality, subsampling and restart interval, and may be at most 1 % larger."""
import io
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import mjpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_SUB = {"420": 2, "444": 0}


def pil_encode(u8, quality, subsampling, restart_interval=0):
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, "JPEG", quality=quality, subsampling=PIL_SUB[subsampling], restart_marker_blocks=restart_interval)
    return buf.getvalue()


def decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def sample_frames(h=96, w=128, seed=0):
    """smooth, smooth plus noise, uniform random: uint8 [H, W, 3] each"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([127 + 100 * np.sin(xx / 17 + yy / 9), 127 + 100 * np.cos(xx / 11), 127 + 90 * np.sin(yy / 7)], -1)
    to8 = lambda a: np.clip(a, 0, 255).astype(np.uint8)     # noqa: E731
    return {"smooth": to8(smooth), "noise": to8(smooth + rng.normal(0, 12, smooth.shape)), "random": to8(rng.uniform(0, 256, smooth.shape))}


def segments(data):
    """[(marker, payload)] of a JPEG file up to and including SOS"""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        marker, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((marker, data[i + 4:i + 2 + n]))
        i += 2 + n
        if marker == 0xDA:
            return out, i


@pytest.mark.parametrize("quality", [1, 30, 50, 75, 90, 100])
def test_quantisation_tables_equal_pil(quality):
    q = Image.open(io.BytesIO(pil_encode(np.zeros((16, 16, 3), np.uint8), quality, "420"))).quantization
    luma, chroma = jr.quant_tables(quality)
    assert list(q[0]) == luma.tolist() and list(q[1]) == chroma.tolist()
    # and the header writes them in zigzag order, as T.81 B.2.4.1 asks
    segs, _ = segments(jr.header(16, 16, quality))
    dqt = [p for m, p in segs if m == 0xDB]
    assert [p[0] for p in dqt] == [0, 1] and list(dqt[0][1:]) == luma[jr.ZIGZAG].tolist() and list(dqt[1][1:]) == chroma[jr.ZIGZAG].tolist()


def test_huffman_tables_equal_pil():
    def dht(data):
        tables = {}
        for m, p in segments(data)[0]:
            while m == 0xC4 and p:
                n = sum(p[1:17])
                tables[(p[0] >> 4, p[0] & 15)] = (list(p[1:17]), list(p[17:17 + n]))
                p = p[17 + n:]
        return tables
    pil = dht(pil_encode(np.zeros((16, 16, 3), np.uint8), 90, "420"))
    assert len(pil) == 4
    assert pil == {k: (list(b), list(v)) for k, (b, v) in jr.HUFFMAN_SPECS.items()}
    assert dht(jr.header(16, 16, 90)) == pil
    # 162 AC symbols each, every (run, size) once, and a prefix-free code of at most 16 bits
    for key, (bits, vals) in jr.HUFFMAN_SPECS.items():
        codes = jr.huffman_codes(bits, vals)
        assert len(codes) == len(vals) == sum(bits) == (162 if key[0] else 12)
        words = sorted(format(c, f"0{n}b") for c, n in codes.values())
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))


def test_zigzag_and_dct_basics():
    assert jr.ZIGZAG[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and jr.ZIGZAG[-3:].tolist() == [55, 62, 63]
    assert sorted(jr.ZIGZAG.tolist()) == list(range(64))
    assert np.allclose(jr.DCT @ jr.DCT.T, np.eye(8), atol=1e-14)
    c = jr.coefficients(np.full((1, 16, 16, 3), 200, np.uint8), 100, "420")
    assert c.shape == (1, 6, 64) and c.dtype == np.int16
    assert c[0, :4, 0].tolist() == [8 * (200 - 128)] * 4 and not c[0, :, 1:].any() and not c[0, 4:, 0].any()


def test_truncation_is_the_fp32_expression():
    import torch
    x = torch.linspace(-1.2, 1.2, 4001).reshape(1, 1, 1, -1).repeat(1, 3, 1, 1)
    want = (x.clamp(-1, 1) * 127.5 + 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(jr.to_uint8(x.numpy(), (-1, 1)), want)
    y = torch.linspace(-0.1, 1.1, 4001).reshape(1, 1, 1, -1).repeat(1, 3, 1, 1)
    assert np.array_equal(jr.to_uint8(y.numpy(), (0, 1)), (255.0 * y.clamp(0, 1)).to(torch.uint8).permute(0, 2, 3, 1).numpy())
    with pytest.raises(ValueError):
        jr.to_uint8(x.numpy(), (0, 255))


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_reference_files_decode_in_pil(subsampling):
    u8 = sample_frames()["noise"]
    h, w = u8.shape[:2]
    mcus_x = w // jr.mcu_size(subsampling)
    n_mcus = mcus_x * (h // jr.mcu_size(subsampling))
    for ri in (1, 4, mcus_x, n_mcus + 5):
        data = jr.encode(u8[None], 90, subsampling, ri)[0]
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        segs, body = segments(data)
        assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
        assert int.from_bytes(dict(segs)[0xDD], "big") == ri
        # RSTn markers in the entropy-coded data: one between consecutive intervals, cycling 0..7
        rst = [data[i + 1] for i in range(body, len(data) - 2) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
        assert rst == [0xD0 + i % 8 for i in range(-(-n_mcus // ri) - 1)]
        img = decode(data)
        assert img.shape == u8.shape and psnr(img, u8) > 25


@pytest.mark.parametrize("subsampling", ["420", "444"])
@pytest.mark.parametrize("quality", [100, 90, 75, 30])
@pytest.mark.parametrize("kind", ["smooth", "noise", "random"])
def test_quality_and_size_against_pil(kind, quality, subsampling):
    u8 = sample_frames()[kind]
    mine = jr.encode(u8[None], quality, subsampling, 4)[0]
    pil = pil_encode(u8, quality, subsampling, 4)
    p_mine, p_pil = psnr(decode(mine), u8), psnr(decode(pil), u8)
    print(f"{kind} q{quality} {subsampling}: PSNR {p_mine:.3f} dB (PIL {p_pil:.3f}), {len(mine)} bytes (PIL {len(pil)})")
    assert p_mine >= p_pil - 0.1
    assert len(mine) <= 1.01 * len(pil)


def test_entropy_coder_special_symbols():
    """ZRL, a non-zero 63rd coefficient (no EOB), the largest categories and all-zero blocks in one MCU: PIL reads it."""
    coef = np.zeros((6, 64), np.int16)
    coef[0, 0], coef[0, 63] = 100, 3            # no EOB
    coef[1, 0], coef[1, 40] = -1024, -5         # DC difference of category 11, two ZRL
    coef[2, 0], coef[2, 1] = 1016, 1023         # DC difference of category 11 (2040), AC category 10
    data = jr.encode_coefficients(coef, 16, 16, 100, "420", 1)
    assert decode(data).shape == (16, 16, 3)
    bits = jr.entropy_intervals(coef, "420", 1)[0]
    assert len(bits) < 64
    with pytest.raises(ValueError):
        jr.encode_coefficients(coef[:5], 16, 16, 100, "420", 1)


def test_dimensions_off_the_mcu_grid_raise():
    for h, w, sub in ((480, 840, "420"), (24, 16, "420"), (20, 16, "444"), (0, 16, "444")):
        with pytest.raises(ValueError):
            jr.check_geometry(h, w, sub)
        with pytest.raises(ValueError):
            jr.header(h, w, 90, sub)
    assert jr.check_geometry(480, 832, "420") == (52, 30) and jr.check_geometry(24, 16, "444") == (2, 3)
    with pytest.raises(ValueError):
        jr.coefficients(np.zeros((1, 24, 16, 3), np.uint8), 90, "420")
    with pytest.raises(ValueError):
        jr.mcu_size("422")
    for bad in (0, 101):
        with pytest.raises(ValueError):
            jr.quant_tables(bad)
    with pytest.raises(ValueError):
        sfa.JpegEncoder(quality=0)
    with pytest.raises(ValueError):
        sfa.JpegEncoder(subsampling="411")
    with pytest.raises(ValueError):
        sfa.JpegEncoder(value_range=(0, 255))
    with pytest.raises(ValueError):
        sfa.JpegEncoder(restart_interval=0)
    import torch
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.JpegEncoder().encode(torch.zeros(1, 3, 16, 16))
    assert sfa.JpegEncoder().restart_interval == 10 and sfa.JpegEncoder(subsampling="444").restart_interval == 21


def test_avi_round_trip_and_riff_consistency(tmp_path):
    u8 = sample_frames(32, 48)
    frames = [jr.encode(u8[k][None], q, "420", 2)[0] for k, q in (("smooth", 90), ("noise", 50), ("random", 100), ("smooth", 10))]
    frames[1] += b"\0" * (1 - len(frames[1]) % 2)                   # an odd-length chunk (padded in the file) is among them
    path = str(tmp_path / "clip.avi")
    mjpeg.write_avi(path, frames, 16, 48, 32)
    assert mjpeg.read_avi(path) == frames
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    # walk the top-level chunks: hdrl, movi, idx1 fill the file exactly
    pos, top = 12, {}
    while pos < len(data):
        fourcc, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        top[data[pos + 8:pos + 12] if fourcc == b"LIST" else fourcc] = (pos, size)
        pos += 8 + size + (size & 1)
    assert pos == len(data) and list(top) == [b"hdrl", b"movi", b"idx1"]
    hdrl = data[top[b"hdrl"][0]:top[b"movi"][0]]
    avih = hdrl.index(b"avih")
    usec, _, _, flags, total, _, streams, _, width, height = struct.unpack_from("<10I", hdrl, avih + 8)
    assert (usec, flags & mjpeg.AVIF_HASINDEX, total, streams, width, height) == (62500, mjpeg.AVIF_HASINDEX, 4, 1, 48, 32)
    strh = hdrl.index(b"strh")
    assert hdrl[strh + 8:strh + 16] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack_from("<4I", hdrl, strh + 8 + 20)
    assert rate / scale == 16 and length == 4
    strf = hdrl.index(b"strf")
    assert struct.unpack_from("<Iii", hdrl, strf + 8) == (40, 48, 32) and hdrl[strf + 8 + 16:strf + 8 + 20] == b"MJPG"
    # every index entry points at its 00dc chunk, relative to the 'movi' fourcc
    movi = top[b"movi"][0] + 8
    ipos, isize = top[b"idx1"]
    assert isize == 16 * len(frames)
    for k, f in enumerate(frames):
        cid, fl, off, n = struct.unpack_from("<4sIII", data, ipos + 8 + 16 * k)
        assert cid == b"00dc" and fl == mjpeg.AVIIF_KEYFRAME and n == len(f)
        assert data[movi + off:movi + off + 4] == b"00dc" and data[movi + off + 8:movi + off + 8 + n] == f
    for f in mjpeg.read_avi(path):
        assert decode(f).shape == (32, 48, 3)
    with pytest.raises(ValueError):
        mjpeg.write_avi(path, [], 16, 48, 32)
    with pytest.raises(ValueError):
        mjpeg.write_avi(path, [b"not a jpeg"], 16, 48, 32)
    bad = tmp_path / "bad.avi"
    bad.write_bytes(b"RIFFxxxxWAVE")
    with pytest.raises(ValueError):
        mjpeg.read_avi(str(bad))


def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    assert lib.sf_jpeg_workspace_bytes(1, 480, 832, 0, 10) > 0
    assert lib.sf_jpeg_workspace_bytes(1, 480, 840, 0, 10) == 0 and b"not a multiple of the 16x16 MCU" in lib.sf_last_error()
    assert lib.sf_jpeg_workspace_bytes(1, 480, 840, 1, 10) > 0                                  # 840 = 105 x 8 fits "444"
    assert lib.sf_jpeg_workspace_bytes(1, 480, 832, 2, 10) == 0 and b"subsampling" in lib.sf_last_error()
    assert lib.sf_jpeg_workspace_bytes(0, 480, 832, 0, 10) == 0 and b"n=0" in lib.sf_last_error()
    assert lib.sf_jpeg_workspace_bytes(1, 480, 832, 0, 0) == 0 and b"restart_interval" in lib.sf_last_error()
    assert lib.sf_jpeg_workspace_bytes(1, 480, 832, 0, 70000) == 0
    # the workspace holds the coefficients, a worst-case slot per interval (208 bytes per block, doubled for stuffing) and
    # the files themselves
    blocks, intervals = 52 * 30 * 6, 156
    assert lib.sf_jpeg_workspace_bytes(1, 480, 832, 0, 10) >= blocks * 128 + intervals * 60 * 416 + 8 * intervals + 640
    assert lib.sf_jpeg_workspace_bytes(3, 480, 832, 0, 10) >= 3 * (blocks * 128 + intervals * 60 * 416)

    assert lib.sf_jpeg_transform(None, 1, 0, 1, 16, 16, 0, 90, None, None) != 0 and b"null buffer" in lib.sf_last_error()
    assert lib.sf_jpeg_transform(4096, 3, 0, 1, 16, 16, 0, 90, 4096, None) != 0 and b"dtype" in lib.sf_last_error()
    assert lib.sf_jpeg_transform(4096, 1, 2, 1, 16, 16, 0, 90, 4096, None) != 0 and b"value range" in lib.sf_last_error()
    assert lib.sf_jpeg_transform(4096, 1, 0, 1, 16, 16, 0, 0, 4096, None) != 0 and b"quality=0" in lib.sf_last_error()
    assert lib.sf_jpeg_transform(4096, 1, 0, 1, 16, 24, 0, 90, 4096, None) != 0 and b"MCU" in lib.sf_last_error()
    assert lib.sf_jpeg_transform(4100, 1, 0, 1, 16, 16, 0, 90, 4096, None) != 0 and b"aligned" in lib.sf_last_error()

    ws = lib.sf_jpeg_workspace_bytes(1, 16, 16, 0, 1)
    ok = (4096, 1, 16, 16, 0, 90, 1, 4096, ws, 4096, ws, 4096, 4096, None)
    def entropy(**kw):                                                                          # noqa: E306
        names = ("coef", "n", "h", "w", "sub", "quality", "ri", "ws", "ws_bytes", "out", "cap", "offsets", "status", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.sf_jpeg_entropy(*args.values())
    assert entropy(coef=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert entropy(status=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert entropy(ws_bytes=ws - 1) != 0 and b"needed" in lib.sf_last_error()
    assert entropy(cap=100) != 0 and b"out_capacity" in lib.sf_last_error()
    assert entropy(ws=4100) != 0 and b"aligned" in lib.sf_last_error()
    assert entropy(quality=101) != 0 and entropy(ri=0) != 0 and entropy(h=24) != 0 and entropy(sub=7) != 0

    enc = lambda *a: lib.sf_jpeg_encode_frames(*a)                                              # noqa: E731
    assert enc(None, 1, 0, 1, 16, 16, 0, 90, 1, 4096, ws, 4096, ws, 4096, 4096, None) != 0 and b"null buffer" in lib.sf_last_error()
    assert enc(4096, 1, 0, 1, 16, 16, 0, 90, 1, None, ws, 4096, ws, 4096, 4096, None) != 0 and b"workspace" in lib.sf_last_error()
    assert enc(4096, 1, 0, 1, 16, 16, 0, 90, 1, 4096, 10, 4096, ws, 4096, 4096, None) != 0 and b"needed" in lib.sf_last_error()
    assert enc(4096, 1, 0, 1, 16, 16, 0, 90, 1, 4096, ws, None, ws, 4096, 4096, None) != 0
    assert enc(4096, 1, 0, 1, 16, 20, 0, 90, 1, 4096, ws, 4096, ws, 4096, 4096, None) != 0 and b"MCU" in lib.sf_last_error()
    assert enc(4096, 1, 0, 1, 16, 16, 0, 900, 1, 4096, ws, 4096, ws, 4096, 4096, None) != 0 and b"quality" in lib.sf_last_error()


def test_python_mirror_matches_the_header():
    """The enum values `_lib.py` uses are those include/sf_hip.h declares (argument counts: test_host_logic)."""
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    enum = lambda name: int(re.search(name + r" = (\d+)", text).group(1))                        # noqa: E731
    assert sfa._lib.JPEG_SUBSAMPLINGS == {"420": enum("SF_JPEG_420"), "444": enum("SF_JPEG_444")}
    assert sfa._lib.JPEG_DTYPES == {"uint8": enum("SF_JPEG_U8"), "float32": enum("SF_JPEG_F32"), "bfloat16": enum("SF_JPEG_BF16")}
    assert sfa._lib.JPEG_RANGES == {(-1, 1): enum("SF_JPEG_RANGE_PM1"), (0, 1): enum("SF_JPEG_RANGE_01")}
    assert sorted(sfa._lib.JPEG_STATUS) == [enum("SF_JPEG_SLOT_OVERFLOW"), enum("SF_JPEG_COEF_RANGE"), enum("SF_JPEG_OUT_OVERFLOW")]
    for name in ("sf_jpeg_workspace_bytes", "sf_jpeg_transform", "sf_jpeg_entropy", "sf_jpeg_encode_frames"):
        getattr(sfa._lib.lib(), name)
    assert (sfa.jpeg_reference.SUBSAMPLINGS == sfa._lib.JPEG_SUBSAMPLINGS)


def test_generate_video_format_flag():
    gen = os.path.join(ROOT, "generate.py")
    base = [sys.executable, gen, "--config_path", "c", "--data_path", "d", "--output_folder", "o"]
    r = subprocess.run(base + ["--video_format", "mp4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--video_format" in r.stderr
    r = subprocess.run(base + ["--video_format", "mjpeg", "--jpeg_quality", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--jpeg_quality" in r.stderr
    r = subprocess.run(base + ["--jpeg_subsampling", "422"], capture_output=True, text=True)
    assert r.returncode == 2 and "--jpeg_subsampling" in r.stderr
