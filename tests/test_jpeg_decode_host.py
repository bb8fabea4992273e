"""Host-side tests of the JPEG decoder (no GPU): the integer reference decoder `jpeg_reference.parse / decode_coefficients /
decode` against the reference encoder (coefficient round trip) and against PIL's decode of PIL-written files, the refusals,
the `JpegDecoder` checks that need no device, and the argument checks of the sf_jpeg_decode_* entry points.

The bounds against PIL are conditions.  libjpeg's `islow` IDCT rounds between its two passes, the definition here once at
the end, so single samples differ by a few levels: for 4:4:4 / 4:2:0 on the MCU grid at most 4 levels and 0.1 in the mean
(measured with this file's inputs: 3 and 0.074; the margin is one level for another libjpeg build); for 4:2:2, grayscale and
sizes off the grid the largest difference measured with this file's inputs (4:2:2: 3, mean 0.056; 50x70: 3, mean 0.051;
grayscale: 1; libjpeg-turbo behind PIL 12.2) plus one level."""
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEVELS, MAX_MEAN = 4, 0.1          # on the MCU grid, 4:4:4 / 4:2:0
MAX_LEVELS_OTHER = 3 + 1               # 4:2:2, grayscale, 50x70: measured 3


def images(h, w, seed=0):
    """smooth, uniform noise, skeleton-like (thin coloured lines on black): uint8 [h, w, 3] each"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([127 + 100 * np.sin(xx / 17 + yy / 9), 127 + 100 * np.cos(xx / 11), 127 + 90 * np.sin(yy / 7)], -1)
    skeleton = np.zeros((h, w, 3), np.uint8)
    skeleton[h // 4:h // 4 + 3, :] = (255, 0, 0)
    skeleton[:, w // 3:w // 3 + 2] = (0, 255, 80)
    skeleton[np.abs(yy - xx * h // w) < 2] = (30, 90, 255)
    return {"smooth": np.clip(smooth, 0, 255).astype(np.uint8), "noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "skeleton": skeleton}


def pil_file(u8, quality=90, subsampling=2, optimize=True, restart=0, **kw):
    """subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0, "L" = grayscale (the first channel)"""
    buf = io.BytesIO()
    if subsampling == "L":
        Image.fromarray(u8[..., 0]).save(buf, "JPEG", quality=quality, optimize=optimize, restart_marker_blocks=restart, **kw)
    else:
        Image.fromarray(u8).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=optimize, restart_marker_blocks=restart, **kw)
    return buf.getvalue()


def pil_decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def segments(data):
    """[(marker, offset of the marker's 0xFF, total length)] of a file's header, SOS included"""
    out, i = [], 2
    while True:
        marker, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((marker, i, 2 + n))
        i += 2 + n
        if marker == 0xDA:
            return out


def patched(data, marker, at, value):
    """`data` with byte `at` of the first `marker` segment's payload replaced"""
    off = next(o for m, o, _ in segments(data) if m == marker)
    b = bytearray(data)
    b[off + 4 + at] = value
    return bytes(b)


def without(data, marker):
    m, off, n = next(s for s in segments(data) if s[0] == marker)
    return data[:off] + data[off + n:]


# ============================================================================================== coefficient round trip
def crafted_coefficients():
    """The crafted cases of test_jpeg_host.py's entropy-coder test, one MCU of 4:2:0 each"""
    special = np.zeros((6, 64), np.int16)
    special[0, 0], special[0, 63] = 100, 3            # a non-zero 63rd coefficient: no EOB
    special[1, 0], special[1, 40] = -1024, -5         # DC difference of category 11, two ZRL
    special[2, 0], special[2, 1] = 1016, 1023         # DC difference of category 11 (2040), AC category 10
    zrl_only = np.zeros((6, 64), np.int16)
    zrl_only[:, 49] = [1, -1, 2, -2, 255, -255]       # three ZRL, then a coefficient
    zrl_only[3, 63] = -1023
    return {"special": special, "zrl": zrl_only, "all_zero": np.zeros((6, 64), np.int16)}


@pytest.mark.parametrize("name", ["special", "zrl", "all_zero"])
def test_round_trip_of_crafted_coefficients(name):
    c = crafted_coefficients()[name]
    for ri in (1, 5):
        data = jr.encode_coefficients(c, 16, 16, 100, "420", ri)
        assert np.array_equal(jr.decode_coefficients(data), c)
    # several MCUs, so that the DC prediction and its reset at a restart marker matter
    many = np.concatenate([c, np.roll(c, 1, axis=0), c[::-1], c])
    for ri in (1, 3, 4, 100):
        data = jr.encode_coefficients(many, 32, 32, 100, "420", ri)
        got = jr.decode_coefficients(data)
        assert got.dtype == np.int16 and got.shape == (24, 64) and np.array_equal(got, many)


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_round_trip_of_a_noise_frame_with_stuffed_bytes(subsampling):
    u8 = images(64, 96)["noise"]
    c = jr.coefficients(u8[None], 100, subsampling)[0]
    for ri in (1, 7, 10 ** 4):
        data = jr.encode_coefficients(c, 64, 96, 100, subsampling, ri)
        assert data.count(b"\xff\x00") > 5
        assert np.array_equal(jr.decode_coefficients(data), c)
    info = jr.parse(data)
    assert (info.height, info.width, info.sampling, info.restart_interval, info.intervals) == (64, 96, subsampling, 10 ** 4, 1)
    assert [q.tolist() for q in info.quant[:2]] == [q.tolist() for q in jr.quant_tables(100)]
    assert data[info.scan_end:] == b"\xff\xd9" and data[info.scan_offset - 3:info.scan_offset] == bytes([0, 63, 0])


def test_idct_and_colour_definition():
    assert jr.IDCT_INT[0].tolist() == [2896] * 8 and jr.IDCT_INT.dtype == np.int64 and abs(jr.IDCT_INT).max() == 4017
    assert (jr.FIX_CR_R, jr.FIX_CB_G, jr.FIX_CR_G, jr.FIX_CB_B) == (91881, 22553, 46802, 116130)
    # a DC-only block is DC * Q / 8 + 128, a tie for DC * Q = 8 k + 4.  In integers it is none: 2896^2 is a shade below 2^23,
    # so t / 2^26 = (k + 1/2) (1 - 2.1e-4) and every such sample goes to the value nearer 128 (the shift is arithmetic)
    c = np.zeros((6, 64), np.int16)
    c[:, 0] = [4, 12, -4, -12, 8, -8]
    assert jr.idct_blocks(c, np.ones(64, np.int64))[:, 0, 0].tolist() == [128, 129, 128, 127, 129, 127]
    assert all((jr.idct_blocks(c, np.ones(64, np.int64)) == jr.idct_blocks(c, np.ones(64, np.int64))[:, :1, :1]).all(axis=(1, 2)))
    big = np.zeros((2, 64), np.int16)
    big[:, 0] = [2047, -2047]
    assert jr.idct_blocks(big, np.full(64, 255))[:, 3, 3].tolist() == [255, 0]           # |t| near 2^45: no overflow, clamped
    assert np.array_equal(jr.to_float(np.arange(256, dtype=np.uint8)), np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1))


# ============================================================================================== against PIL
@pytest.mark.parametrize("h,w", [(16, 16), (64, 96), (50, 70)])
@pytest.mark.parametrize("subsampling", [0, 1, 2, "L"])
def test_decode_against_pil(subsampling, h, w):
    on_grid = (h, w) != (50, 70) and subsampling in (0, 2)
    for kind, u8 in images(h, w).items():
        for quality in (50, 90, 100):
            for restart in (0, 3):
                data = pil_file(u8, quality, subsampling, True, restart)
                info = jr.parse(data)
                assert (info.height, info.width, info.sampling) == (h, w, {0: "444", 1: "422", 2: "420", "L": "gray"}[subsampling])
                assert bool(info.restart_interval) == bool(restart)
                mine, ref = jr.decode(data), pil_decode(data)
                assert mine.shape == ref.shape == (h, w, 3) and mine.dtype == np.uint8
                diff = np.abs(mine.astype(int) - ref.astype(int))
                print(f"{h}x{w} {kind} sub={subsampling} q{quality} rst={restart}: max {diff.max()}, mean {diff.mean():.4f}")
                if on_grid:
                    assert diff.max() <= MAX_LEVELS and diff.mean() <= MAX_MEAN
                else:
                    assert diff.max() <= MAX_LEVELS_OTHER


def test_standard_tables_comments_and_app_segments():
    u8 = images(32, 48)["smooth"]
    plain = pil_file(u8, 75, 2, optimize=False)
    data = pil_file(u8, 75, 2, optimize=False, comment=b"a comment", exif=b"Exif\0\0" + b"\0" * 40)
    assert len(data) > len(plain) and {m for m, _, _ in segments(data)} >= {0xFE, 0xE1}
    assert np.array_equal(jr.decode(data), jr.decode(plain))
    assert {k: (list(b), list(v)) for k, (b, v) in jr.HUFFMAN_SPECS.items()}[(0, 0)] == (jr.parse(plain).dc[0][0], jr.parse(plain).dc[0][1])
    # the reference encoder's own files: what PIL decodes, within the same bounds
    for sub in ("420", "444"):
        f = jr.encode(u8[None], 90, sub, 5)[0]
        diff = np.abs(jr.decode(f).astype(int) - pil_decode(f).astype(int))
        assert diff.max() <= MAX_LEVELS and diff.mean() <= MAX_MEAN


# ============================================================================================== refusals
def base_file():
    return jr.encode(images(16, 16)["smooth"][None], 90, "420", 1)[0]


def test_refused_formats_name_their_reason():
    u8 = images(32, 32)["smooth"]
    with pytest.raises(ValueError, match="progressive"):
        jr.parse(pil_file(u8, 90, 2, progressive=True))
    good = base_file()
    sof = next(o for m, o, _ in segments(good) if m == 0xC0)
    for marker, reason in ((0xC1, "extended"), (0xC3, "lossless"), (0xC9, "arithmetic"), (0xCA, "arithmetic")):
        bad = bytearray(good)
        bad[sof + 1] = marker
        with pytest.raises(ValueError, match=reason):
            jr.parse(bytes(bad))
    with pytest.raises(ValueError, match="12 bit"):
        jr.parse(patched(good, 0xC0, 0, 12))
    with pytest.raises(ValueError, match="16-bit DQT"):
        jr.parse(patched(good, 0xDB, 0, 0x10))
    for hv in (0x41, 0x12, 0x44):
        with pytest.raises(ValueError, match="sampling factors"):
            jr.parse(patched(good, 0xC0, 7, hv))
    with pytest.raises(ValueError, match="sampling factors"):
        jr.parse(patched(good, 0xC0, 10, 0x21))                                   # subsampled luma over chroma that is not 1x1
    buf = io.BytesIO()
    Image.new("CMYK", (16, 16), (10, 20, 30, 40)).save(buf, "JPEG")
    with pytest.raises(ValueError, match="4 components"):
        jr.parse(buf.getvalue())
    # a scan of one of the three components: a file of several scans
    m, off, n = next(s for s in segments(good) if s[0] == 0xDA)
    one_scan = good[:off] + b"\xff\xda" + (8).to_bytes(2, "big") + bytes([1, 1, 0x00, 0, 63, 0]) + good[off + n:]
    with pytest.raises(ValueError, match="multiple scans"):
        jr.parse(one_scan)
    with pytest.raises(ValueError, match="SOI"):
        jr.parse(good[2:])
    with pytest.raises(ValueError, match="SOF"):
        jr.parse(without(good, 0xC0))
    with pytest.raises(ValueError, match="SOS"):
        jr.parse(good[:off] + b"\xff\xd9")
    with pytest.raises(ValueError, match="SOS"):
        jr.parse(good[:off])
    with pytest.raises(ValueError, match="EOI"):
        jr.parse(good[:-2])
    dht = next(o for m, o, _ in segments(good) if m == 0xC4)
    bad = bytearray(good)
    bad[dht + 2:dht + 4] = (60000).to_bytes(2, "big")
    with pytest.raises(ValueError, match="runs past the file"):
        jr.parse(bytes(bad))
    with pytest.raises(ValueError, match="does not define"):
        jr.parse(without(good, 0xDB))
    with pytest.raises(ValueError, match="more codes"):
        jr.parse(patched(patched(good, 0xC4, 1, 3), 0xC4, 3, 2))                  # DC luma BITS 0 1 5 -> 3 1 2: three codes of one bit
    assert jr.parse(good).sampling == "420"                                      # and the file they were made from is taken


def test_damaged_scans_raise_in_the_reference():
    u8 = images(32, 48)["noise"]
    good = jr.encode(u8[None], 90, "420", 2)[0]
    info = jr.parse(good)
    half = (info.scan_offset + info.scan_end) // 2
    with pytest.raises(ValueError, match="restart markers"):
        jr.decode(good[:half] + b"\xff\xd9")
    single = jr.encode(u8[None], 90, "420", 1000)[0]
    info = jr.parse(single)
    with pytest.raises(ValueError, match="truncated|Huffman|zero run"):
        jr.decode(single[:(info.scan_offset + info.scan_end) // 2] + b"\xff\xd9")


def test_decoder_checks_that_need_no_device():
    dec = sfa.JpegDecoder()
    a = jr.encode(images(16, 16)["smooth"][None], 90, "420", 1)[0]
    assert dec.info(a) == (16, 16, "420", 1) and dec.info(pil_file(images(50, 70)["noise"], 90, 1)) == (50, 70, "422", 0)
    for other in (jr.encode(images(16, 32)["smooth"][None], 90, "420", 1)[0], jr.encode(images(16, 16)["smooth"][None], 90, "444", 1)[0]):
        with pytest.raises(ValueError, match="share size and sampling"):
            dec.decode([a, other])
        with pytest.raises(ValueError, match="share size and sampling"):
            dec.coefficients([a, other])
    with pytest.raises(ValueError, match="no files"):
        dec.decode([])
    with pytest.raises(ValueError, match="progressive"):
        dec.decode([a, pil_file(images(16, 16)["smooth"], 90, 2, progressive=True)])
    with pytest.raises(ValueError, match="layout"):
        dec.decode([a], layout="nchw")
    with pytest.raises(ValueError, match="dtype"):
        dec.decode([a], dtype=np.float32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.JpegDecoder(device="cpu").decode([a])
    with pytest.raises(ValueError, match="frames_per_piece"):
        next(sfa.jpeg.pose_feed([a], dec, 0))
    assert "JpegDecoder" in sfa.__all__


# ============================================================================================== the C entry points
def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    ws = lib.sf_jpeg_decode_workspace_bytes
    # 480x832 4:2:0: 9360 blocks of 128 bytes, the three planes, 156 marker slots
    assert ws(1, 480, 832, 0, 156) >= 9360 * 128 + 480 * 832 * 3 // 2 + 156 * 4
    assert ws(3, 480, 832, 0, 156) >= 3 * (9360 * 128 + 480 * 832 * 3 // 2)
    assert ws(1, 50, 70, 2, 1) >= (7 * 5 * 4) * 128 + 56 * 80 + 2 * 56 * 40       # off the grid: the padding MCUs are counted
    assert ws(1, 1, 1, 3, 1) > 0
    assert ws(1, 480, 832, 4, 1) == 0 and b"sampling" in lib.sf_last_error()
    assert ws(0, 480, 832, 0, 1) == 0 and b"n=0" in lib.sf_last_error()
    assert ws(1, 0, 832, 0, 1) == 0 and b"frame 0x832" in lib.sf_last_error()
    assert ws(1, 480, 70000, 0, 1) == 0
    assert ws(1, 480, 832, 0, 0) == 0 and b"max_intervals" in lib.sf_last_error()
    assert ws(1, 480, 832, 0, 1561) == 0 and b"max_intervals" in lib.sf_last_error()

    need = ws(1, 16, 16, 0, 1)
    up_bytes = sfa._lib.JPEG_DECODE_FILE_BYTES + 64
    ok = dict(upload=4096, upload_bytes=up_bytes, n=1, h=16, w=16, sampling=0, max_intervals=1, ws=4096, ws_bytes=need, coef=4096, status=4096, stream=None)

    def entropy(**kw):
        return lib.sf_jpeg_decode_entropy(*{**ok, **kw}.values())
    assert entropy(upload=None) != 0 and b"upload" in lib.sf_last_error()
    assert entropy(upload=4100) != 0 and b"16-byte-aligned" in lib.sf_last_error()
    assert entropy(upload_bytes=up_bytes - 8) != 0 and b"multiple of 16" in lib.sf_last_error()
    assert entropy(upload_bytes=4096) != 0 and b"table entries" in lib.sf_last_error()
    assert entropy(coef=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert entropy(status=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert entropy(ws=4100) != 0 and b"aligned" in lib.sf_last_error()
    assert entropy(ws_bytes=need - 1) != 0 and b"needed" in lib.sf_last_error()
    assert entropy(sampling=9) != 0 and entropy(h=0) != 0 and entropy(max_intervals=2) != 0 and entropy(n=70000) != 0

    import ctypes as C
    table = sfa.ops._idct_table()
    assert list(table) == jr.IDCT_INT.reshape(-1).tolist()
    okp = dict(coef=4096, upload=4096, upload_bytes=up_bytes, table=table, n=1, h=16, w=16, sampling=0, ws=4096, ws_bytes=need, out=4096, layout=0, dtype=0,
               stream=None)

    def pixels(**kw):
        return lib.sf_jpeg_decode_pixels(*{**okp, **kw}.values())
    assert pixels(coef=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert pixels(table=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert pixels(layout=3) != 0 and b"layout" in lib.sf_last_error()
    assert pixels(dtype=3) != 0 and b"dtype" in lib.sf_last_error()
    assert pixels(out=4100) != 0 and b"aligned" in lib.sf_last_error()
    assert pixels(ws_bytes=10) != 0 and b"needed" in lib.sf_last_error()
    wrong = (C.c_int32 * 64)(*([9000] * 64))
    assert pixels(table=wrong) != 0 and b"idct_table" in lib.sf_last_error()

    okf = dict(upload=4096, upload_bytes=up_bytes, table=table, n=1, h=16, w=16, sampling=0, max_intervals=1, ws=4096, ws_bytes=need, out=4096, layout=0,
               dtype=0, status=4096, stream=None)

    def frames(**kw):
        return lib.sf_jpeg_decode_frames(*{**okf, **kw}.values())
    assert frames(ws=None) != 0 and b"workspace" in lib.sf_last_error()
    assert frames(ws_bytes=need - 1) != 0 and b"needed" in lib.sf_last_error()
    assert frames(status=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert frames(upload=None) != 0 and frames(w=0) != 0 and frames(sampling=-1) != 0


def test_python_mirror_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    enum = lambda name: int(re.search(name + r" = (\d+)", text).group(1))                        # noqa: E731
    L = sfa._lib
    assert L.JPEG_DECODE_SAMPLINGS == {"420": enum("SF_JPEG_DEC_420"), "444": enum("SF_JPEG_DEC_444"), "422": enum("SF_JPEG_DEC_422"),
                                       "gray": enum("SF_JPEG_DEC_GRAY")} == jr.DECODE_SAMPLINGS
    assert {k: L.JPEG_DECODE_SAMPLINGS[k] for k in L.JPEG_SUBSAMPLINGS} == L.JPEG_SUBSAMPLINGS            # the encoder's two keep their values
    assert L.JPEG_LAYOUTS == {"hwc": enum("SF_JPEG_HWC"), "pose": enum("SF_JPEG_POSE"), "chw": enum("SF_JPEG_CHW")}
    assert sorted(L.JPEG_DECODE_STATUS) == [enum("SF_JPEG_DEC_BAD_CODE"), enum("SF_JPEG_DEC_RUN_PAST_63"), enum("SF_JPEG_DEC_TRUNCATED"),
                                            enum("SF_JPEG_DEC_MARKER_COUNT")]
    assert L.JPEG_DECODE_FILE_BYTES == int(re.search(r"#define SF_JPEG_DECODE_FILE_BYTES (\d+)", text).group(1)) == sfa.jpeg._FILE_DTYPE.itemsize
    for name in ("sf_jpeg_decode_workspace_bytes", "sf_jpeg_decode_entropy", "sf_jpeg_decode_pixels", "sf_jpeg_decode_frames"):
        getattr(L.lib(), name)
    assert int(re.search(r"#define SF_HIP_ABI_VERSION (\d+)", text).group(1)) == 11 == L.ABI_VERSION == L.lib().sf_abi_version()


def test_generate_pose_flags(tmp_path):
    import subprocess
    import sys
    gen = os.path.join(ROOT, "generate.py")
    clip = tmp_path / "clip.avi"
    sfa.mjpeg.write_avi(str(clip), [base_file()], 16, 16, 16)
    base = [sys.executable, gen, "--config_path", "c", "--data_path", "d", "--output_folder", "o", "--pose_random_init_seed", "0"]
    r = subprocess.run(base + ["--pose_path", str(clip)], capture_output=True, text=True)
    assert r.returncode == 2 and "--ref_pose_path" in r.stderr
    r = subprocess.run(base + ["--pose_path", str(clip), "--ref_pose_path", str(tmp_path / "missing.jpg")], capture_output=True, text=True)
    assert r.returncode == 2 and "no such file" in r.stderr
    pt = tmp_path / "pose.pt"
    pt.write_bytes(b"")
    r = subprocess.run(base + ["--pose_path", str(pt), "--ref_pose_path", str(clip)], capture_output=True, text=True)
    assert r.returncode == 2 and "--ref_pose_path" in r.stderr and ".avi" in r.stderr
