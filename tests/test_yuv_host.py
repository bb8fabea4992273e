"""Host-side tests of the raw YUV path (no GPU): the numpy definition `yuv_reference` (the constants table, closure of the
rows, the ranges and the round trip over all 2^24 colours, Pillow's YCbCr, the planes of real JPEG files against
`jpeg_reference.decode` bit for bit, the formats' sizes and offsets, box averaging and edge replication of the encoder),
`y4m`'s reader and writer (headers, FRAME parameters, a live pipe, truncation, refused tags), and the argument checks of the
sf_yuv_* entry points, which return before any launch.  The bounds of the exhaustive tests are the definition's own maxima,
stated as conditions: there are no tolerances."""
import ctypes as C
import io
import os
import threading
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import y4m
from self_forcing_amd import yuv_reference as yr

TABLE = {
    ("bt601", "full"): [0, 65536, 91881, 22553, 46802, 116130, 19595, 38470, 7471, 11058, 21710, 32768, 32768, 27439, 5329],
    ("bt601", "limited"): [16, 76309, 104597, 25675, 53279, 132201, 16829, 33039, 6416, 9714, 19071, 28785, 28784, 24103, 4681],
    ("bt709", "full"): [0, 65536, 103206, 12276, 30679, 121609, 13933, 46871, 4732, 7509, 25259, 32768, 32768, 29763, 3005],
    ("bt709", "limited"): [16, 76309, 117489, 13975, 34925, 138438, 11966, 40254, 4064, 6596, 22189, 28785, 28784, 26145, 2639],
}
ROWS = list(TABLE)
SIZES = [(1, 1), (3, 5), (16, 64), (17, 66)]


@pytest.fixture(scope="module")
def all_rgb():
    """Every (R, G, B) once: uint8 [4096, 4096, 3]."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


# ------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(r))
def test_constants_table(row):
    k = yr.constants(*row)
    assert len(k) == 16 and list(k[:15]) == TABLE[row] and k[15] == 0
    if row == ("bt601", "full"):
        assert (k[2], k[3], k[4], k[5]) == (jr.FIX_CR_R, jr.FIX_CB_G, jr.FIX_CR_G, jr.FIX_CB_B)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(r))
def test_grey_has_neutral_chroma_and_white_its_level(row):
    k = yr.constants(*row)
    g = np.arange(256, dtype=np.uint8)
    yuv = yr.rgb_to_yuv(np.stack([g, g, g], -1), k)
    assert (yuv[:, 1] == 128).all() and (yuv[:, 2] == 128).all()
    assert yuv[255, 0] == (255 if row[1] == "full" else 235) and yuv[0, 0] == k[0]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(r))
def test_ranges_and_round_trip_over_all_colours(row, all_rgb):
    k = yr.constants(*row)
    yuv = yr.rgb_to_yuv(all_rgb, k)
    lo, hi = yuv.reshape(-1, 3).min(0), yuv.reshape(-1, 3).max(0)
    if row[1] == "limited":
        assert (lo[0], hi[0]) == (16, 235) and (lo[1], hi[1]) == (16, 240) and (lo[2], hi[2]) == (16, 240)
    else:
        assert (lo[0], hi[0]) == (0, 255)
    back = yr.yuv_to_rgb(yuv[..., 0], yuv[..., 1], yuv[..., 2], k)
    err = np.abs(back.astype(np.int16) - all_rgb.astype(np.int16)).reshape(-1, 3).max(0)
    print(row, "round-trip maxima", err)
    bound = (1, 1, 1) if row[1] == "full" else (1, 1, 2)
    assert all(int(e) <= b for e, b in zip(err, bound))


def test_bt601_full_is_within_one_of_pillow(all_rgb):
    k = yr.constants("bt601", "full")
    ours = yr.rgb_to_yuv(all_rgb, k)
    im = Image.fromarray(all_rgb).convert("YCbCr")
    theirs = np.asarray(im)
    d = np.abs(ours.astype(np.int16) - theirs.astype(np.int16)).reshape(-1, 3).max(0)
    print("YCbCr vs Pillow", d)
    assert (d <= 1).all()
    back_ours = yr.yuv_to_rgb(theirs[..., 0], theirs[..., 1], theirs[..., 2], k)
    back_theirs = np.asarray(im.convert("RGB"))
    d = np.abs(back_ours.astype(np.int16) - back_theirs.astype(np.int16)).reshape(-1, 3).max(0)
    print("RGB of Pillow's YCbCr vs Pillow", d)
    assert (d <= 1).all()


def _jpeg(h, w, subsampling):
    rng = np.random.default_rng(h * 1000 + w)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, "JPEG", quality=90, subsampling=subsampling)
    return buf.getvalue()


@pytest.mark.parametrize("h,w,subsampling,fmt", [(19, 33, "4:2:0", "i420"), (17, 65, "4:2:2", "i422"), (16, 64, "4:2:0", "i420"), (1, 1, "4:2:0", "i420"),
                                                 (5, 3, "4:4:4", "i444")])
def test_decode_of_jpeg_planes_equals_the_jpeg_decoder(h, w, subsampling, fmt):
    file = _jpeg(h, w, subsampling)
    info = jr.parse(file)
    assert (info.height, info.width) == (h, w)
    planes = jr.component_planes(jr.decode_coefficients(file, info), info)
    ch, cw = yr.chroma_size(fmt, h, w)
    raw = planes[0][:h, :w].astype(np.uint8).tobytes() + b"".join(p[:ch, :cw].astype(np.uint8).tobytes() for p in planes[1:])
    assert len(raw) == yr.frame_bytes(fmt, h, w)
    assert np.array_equal(yr.decode(raw, fmt, h, w, "bt601", "full", "triangle"), jr.decode(file))


@pytest.mark.parametrize("fmt", ["i420", "i422"])
def test_triangle_filter_is_the_jpeg_decoders(fmt):
    rng = np.random.default_rng(3)
    for h, w in [(1, 1), (2, 2), (5, 7), (16, 64), (17, 33)]:
        ch, cw = yr.chroma_size(fmt, h, w)
        c = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        assert np.array_equal(yr.upsample(c, fmt, h, w, "triangle"), jr.upsample(c, "420" if fmt == "i420" else "422", h, w))
        near = yr.upsample(c, fmt, h, w, "nearest")
        sx, sy = (2, 2) if fmt == "i420" else (2, 1)
        assert all(near[y, x] == c[y // sy, x // sx] for y in range(h) for x in range(w))


@pytest.mark.parametrize("h,w", SIZES)
def test_frame_bytes_and_plane_offsets(h, w):
    ch, cw = -(-h // 2), -(-w // 2)
    assert yr.frame_bytes("i420", h, w) == h * w + 2 * ch * cw and yr.plane_offsets("i420", h, w) == {"y": 0, "u": h * w, "v": h * w + ch * cw}
    assert yr.frame_bytes("nv12", h, w) == h * w + 2 * ch * cw and yr.plane_offsets("nv12", h, w) == {"y": 0, "u": h * w, "v": h * w + 1}
    assert yr.frame_bytes("i422", h, w) == h * w + 2 * h * cw and yr.plane_offsets("i422", h, w) == {"y": 0, "u": h * w, "v": h * w + h * cw}
    assert yr.frame_bytes("i444", h, w) == 3 * h * w and yr.plane_offsets("i444", h, w) == {"y": 0, "u": h * w, "v": 2 * h * w}
    assert yr.frame_bytes("gray", h, w) == h * w and yr.plane_offsets("gray", h, w) == {"y": 0}
    for fmt, off in (("yuyv", {"y": 0, "u": 1, "v": 3}), ("uyvy", {"y": 1, "u": 0, "v": 2})):
        if w % 2:
            with pytest.raises(ValueError, match=str(w)):
                yr.frame_bytes(fmt, h, w)
        else:
            assert yr.frame_bytes(fmt, h, w) == 2 * h * w and yr.plane_offsets(fmt, h, w) == off
    # the planes stand where the offsets say
    for fmt in yr.FORMATS:
        if fmt in ("yuyv", "uyvy") and w % 2:
            continue
        raw = np.random.default_rng(h + w).integers(0, 256, yr.frame_bytes(fmt, h, w), dtype=np.uint8)
        p = yr.planes(raw.tobytes(), fmt, h, w)
        off = yr.plane_offsets(fmt, h, w)
        assert p[0][0, 0] == raw[off["y"]] and p[0].shape == (h, w)
        if fmt != "gray":
            assert p[1][0, 0] == raw[off["u"]] and p[2][0, 0] == raw[off["v"]] and p[1].shape == p[2].shape == yr.chroma_size(fmt, h, w)
    for bad in (0, yr.MAX_SIZE + 1):
        with pytest.raises(ValueError, match=str(bad)):
            yr.frame_bytes("i420", bad, 4)
    with pytest.raises(ValueError, match="p010"):
        yr.frame_bytes("p010", 4, 4)


@pytest.mark.parametrize("h,w", [(2, 2), (3, 6), (16, 64), (17, 66)])
@pytest.mark.parametrize("chroma", ["nearest", "triangle"])
def test_layouts_of_the_same_samples_decode_equal(h, w, chroma):
    rng = np.random.default_rng(7)
    ch, cw = yr.chroma_size("i420", h, w)
    y, u, v = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    i420 = y.tobytes() + u.tobytes() + v.tobytes()
    nv12 = y.tobytes() + np.stack([u, v], -1).tobytes()
    assert np.array_equal(yr.decode(i420, "i420", h, w, chroma=chroma), yr.decode(nv12, "nv12", h, w, chroma=chroma))
    u2, v2 = rng.integers(0, 256, (h, w // 2), dtype=np.uint8), rng.integers(0, 256, (h, w // 2), dtype=np.uint8)
    i422 = y.tobytes() + u2.tobytes() + v2.tobytes()
    yuyv = np.stack([y[:, 0::2], u2, y[:, 1::2], v2], -1).tobytes()
    uyvy = np.stack([u2, y[:, 0::2], v2, y[:, 1::2]], -1).tobytes()
    want = yr.decode(i422, "i422", h, w, chroma=chroma)
    assert np.array_equal(yr.decode(yuyv, "yuyv", h, w, chroma=chroma), want) and np.array_equal(yr.decode(uyvy, "uyvy", h, w, chroma=chroma), want)
    grey = yr.decode(y.tobytes(), "gray", h, w, "bt601", "full")
    assert np.array_equal(grey, np.repeat(y[..., None], 3, 2))


@pytest.mark.parametrize("fmt", yr.ENCODE_FORMATS)
def test_encode_box_average_and_edge_replication(fmt):
    k = yr.constants("bt601", "limited")
    for h, w in [(3, 5), (1, 1), (2, 2), (5, 3)]:
        flat = np.empty((h, w, 3), np.uint8)
        flat[:] = (200, 30, 90)
        p = yr.planes(yr.encode(flat, fmt), fmt, h, w)
        y0, u0, v0 = (int(c) for c in yr.rgb_to_yuv(flat[0, 0], k))
        assert (p[0] == y0).all() and (p[1] == u0).all() and (p[2] == v0).all()             # replication keeps a flat colour flat
        a, b = np.array((255, 0, 0), np.uint8), np.array((0, 0, 255), np.uint8)
        checker = np.where(((np.arange(h)[:, None] + np.arange(w)[None]) % 2 == 0)[..., None], a, b).astype(np.uint8)
        p = yr.planes(yr.encode(checker, fmt), fmt, h, w)
        full = yr.rgb_to_yuv(checker, k)
        assert np.array_equal(p[0], full[..., 0])
        sx, sy = {"i420": (2, 2), "nv12": (2, 2), "i422": (2, 1), "i444": (1, 1)}[fmt]
        for c in (1, 2):
            for cy in range(p[c].shape[0]):
                for cx in range(p[c].shape[1]):
                    vals = [int(full[min(cy * sy + dy, h - 1), min(cx * sx + dx, w - 1), c]) for dy in range(sy) for dx in range(sx)]
                    n = len(vals)
                    assert p[c][cy, cx] == (sum(vals) + n // 2) // n
    with pytest.raises(ValueError, match="yuyv"):
        yr.encode(np.zeros((2, 2, 3), np.uint8), "yuyv")


# ------------------------------------------------------------------------------------------ y4m
def _frames(fmt, h, w, n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, yr.frame_bytes(fmt, h, w), dtype=np.uint8).tobytes() for _ in range(n)]


@pytest.mark.parametrize("fmt", ["i420", "i422", "i444", "gray"])
@pytest.mark.parametrize("range_", ["limited", "full"])
def test_y4m_round_trip(fmt, range_):
    frames = _frames(fmt, 5, 7, 3)
    buf = io.BytesIO()
    w = y4m.Y4mWriter(buf, 7, 5, Fraction(30000, 1001), fmt, range_)
    assert buf.getvalue() == b""                                   # the header goes out with the first write
    assert w.write(frames[:1]) == 1 and w.write(frames[1:]) == 2
    w.close()
    r = y4m.Y4mReader(io.BytesIO(buf.getvalue()))
    assert (r.width, r.height, r.fps, r.fmt, r.range) == (7, 5, Fraction(30000, 1001), fmt, range_)
    assert list(r) == frames


@pytest.mark.parametrize("tag,fmt", [("C420jpeg", "i420"), ("C420mpeg2", "i420"), ("C420paldv", "i420"), ("C420", "i420"), ("C422", "i422"), ("C444", "i444"),
                                     ("Cmono", "gray"), ("", "i420")])
def test_y4m_header_tags_and_frame_parameters(tag, fmt):
    frames = _frames(fmt, 4, 6, 2)
    data = f"YUV4MPEG2 W6 H4 F16:1 I? A1:1 {tag} XYSCSS=420JPEG\n".encode() + b"FRAME Ip Xfoo=1\n" + frames[0] + b"FRAME\n" + frames[1]
    r = y4m.Y4mReader(io.BytesIO(data))
    assert (r.width, r.height, r.fps, r.fmt, r.range) == (6, 4, Fraction(16), fmt, "limited")
    assert list(r) == frames


def test_y4m_reader_is_live_over_a_pipe():
    frames = _frames("i420", 6, 8, 3)
    rfd, wfd = os.pipe()
    go = [threading.Event() for _ in frames]
    with os.fdopen(wfd, "wb", buffering=0) as wf, os.fdopen(rfd, "rb", buffering=0) as rf:
        def produce():
            w = y4m.Y4mWriter(wf, 8, 6, 16)
            for f, e in zip(frames, go):
                e.wait()
                w.write([f])
        t = threading.Thread(target=produce)
        t.start()
        go[0].set()
        r = y4m.Y4mReader(rf)                                       # returns with frame 0 written and nothing behind it
        for k, f in enumerate(frames):
            assert next(r) == f                                    # frame k arrives before frame k + 1 is written
            if k + 1 < len(frames):
                go[k + 1].set()
        t.join()
        wf.close()
        assert next(r, None) is None


def test_y4m_refusals():
    frame = _frames("i420", 4, 6, 1)[0]
    good = b"YUV4MPEG2 W6 H4 F16:1 Ip\nFRAME\n" + frame
    with pytest.raises(ValueError, match="truncated"):
        list(y4m.Y4mReader(io.BytesIO(good[:-1])))
    with pytest.raises(ValueError, match="FRAME"):
        list(y4m.Y4mReader(io.BytesIO(good + b"FRAM")))
    for tag in ("C420p10", "It", "C444alpha"):
        with pytest.raises(ValueError, match=tag):
            y4m.Y4mReader(io.BytesIO(f"YUV4MPEG2 W6 H4 F16:1 {tag}\n".encode()))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        y4m.Y4mReader(io.BytesIO(b"RIFF....AVI \n"))
    with pytest.raises(ValueError, match="nv12"):
        y4m.Y4mWriter(io.BytesIO(), 6, 4, 16, "nv12")
    w = y4m.Y4mWriter(io.BytesIO(), 6, 4, 16)
    with pytest.raises(ValueError, match="35"):
        w.write([frame[:-1]])


# ------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_check_their_arguments_before_any_launch():
    lib = sfa._lib.lib()
    assert lib.sf_abi_version() == 11 == sfa._lib.ABI_VERSION
    for name in ("sf_yuv_frame_bytes", "sf_yuv_decode_frames", "sf_yuv_encode_frames"):
        assert name in sfa._lib.SIGNATURES
    for fmt, code in yr.FORMATS.items():
        assert sfa._lib.YUV_FORMATS[fmt] == code
        for h, w in SIZES:
            if fmt in ("yuyv", "uyvy") and w % 2:
                assert lib.sf_yuv_frame_bytes(code, h, w) == 0 and b"even width" in lib.sf_last_error()
            else:
                assert lib.sf_yuv_frame_bytes(code, h, w) == yr.frame_bytes(fmt, h, w)
    assert sfa._lib.YUV_CHROMAS == yr.CHROMAS and sfa._lib.YUV_MAX_SIZE == yr.MAX_SIZE
    assert lib.sf_yuv_frame_bytes(7, 4, 4) == 0 and b"unknown format 7" in lib.sf_last_error()
    assert lib.sf_yuv_frame_bytes(0, 0, 4) == 0 and lib.sf_yuv_frame_bytes(0, 4, yr.MAX_SIZE + 1) == 0

    k = (C.c_int32 * 16)(*yr.constants())
    p = 4096                                                       # never dereferenced: every call below is refused first
    dec = lambda raw=p, fmt=0, n=1, h=4, w=4, kk=k, chroma=1, out=p * 2, layout=0, dtype=0: lib.sf_yuv_decode_frames(raw, fmt, n, h, w, kk, chroma, out, layout,
                                                                                                                       dtype, None)       # noqa: E731
    enc = lambda frames=p, dtype=0, vr=0, n=1, h=4, w=4, kk=k, out=p * 2, fmt=0: lib.sf_yuv_encode_frames(frames, dtype, vr, n, h, w, kk, out, fmt, None)  # noqa: E731
    for call, text in [(lambda: dec(raw=None), "null"), (lambda: dec(out=None), "null"), (lambda: dec(kk=None), "null"), (lambda: dec(fmt=7), "unknown format 7"),
                       (lambda: dec(fmt=-1), "unknown format -1"), (lambda: dec(fmt=5, w=5), "even width"), (lambda: dec(n=0), "n=0"),
                       (lambda: dec(h=0), "0x4"), (lambda: dec(chroma=2), "chroma filter 2"), (lambda: dec(layout=3), "layout 3"), (lambda: dec(dtype=3), "dtype 3"),
                       (lambda: dec(out=p + 8), "16-byte"), (lambda: dec(raw=p * 2), "overlap"),
                       (lambda: enc(frames=None), "null"), (lambda: enc(out=None), "null"), (lambda: enc(kk=None), "null"), (lambda: enc(fmt=4), "decode only"),
                       (lambda: enc(fmt=5), "decode only"), (lambda: enc(fmt=9), "unknown format 9"), (lambda: enc(dtype=-1), "dtype -1"),
                       (lambda: enc(vr=2), "value range 2"), (lambda: enc(n=-3), "n=-3"), (lambda: enc(w=0), "4x0"), (lambda: enc(out=p), "overlap")]:
        assert call() != 0
        assert text in lib.sf_last_error().decode(), (text, lib.sf_last_error())


def test_python_surface_refuses_without_a_device():
    import torch
    with pytest.raises(ValueError, match="nv21"):
        sfa.YuvEncoder("nv21")
    with pytest.raises(ValueError, match="yuyv"):
        sfa.YuvEncoder("yuyv")
    with pytest.raises(ValueError, match="bt2020"):
        sfa.YuvEncoder(matrix="bt2020")
    with pytest.raises(ValueError, match="value_range"):
        sfa.YuvEncoder(value_range=(0, 255))
    d = sfa.YuvDecoder()
    frame = bytes(yr.frame_bytes("i420", 4, 6))
    for kwargs, text in [(dict(fmt="p010"), "p010"), (dict(fmt="yuyv", hw=(4, 5)), "5"), (dict(layout="nhwc"), "nhwc"), (dict(dtype=torch.float16), "float16"),
                         (dict(matrix="bt2020"), "bt2020"), (dict(range="tv"), "tv"), (dict(chroma="cubic"), "cubic"), (dict(hw=(4, 6, 1)), "hw"),
                         (dict(size=(0, 4)), "0"), (dict(size=(1, 1), hw=(4, 60), raw=bytes(yr.frame_bytes("i420", 4, 60))), "width")]:
        args = dict(raw=frame, fmt="i420", hw=(4, 6))
        args.update(kwargs)
        with pytest.raises(ValueError, match=text):
            d.decode(**args)
    with pytest.raises(ValueError, match="cpu"):
        sfa.YuvDecoder("cpu").decode(frame, "i420", (4, 6))
    with pytest.raises(ValueError, match="uint8 \\[n, 36\\]"):
        d.decode(torch.zeros(1, 35, dtype=torch.uint8), "i420", (4, 6))
    with pytest.raises(ValueError, match="cpu"):
        d.decode(torch.zeros(1, 36, dtype=torch.uint8), "i420", (4, 6))
    with pytest.raises(ValueError, match="frames_per_piece"):
        sfa.yuv.frame_feed([], d, "i420", (4, 6), frames_per_piece=0)
    with pytest.raises(ValueError, match="p010"):
        sfa.yuv.frame_feed([], d, "p010", (4, 6))
    pulled = []

    def source():
        pulled.append(1)
        yield frame
    feed = sfa.yuv.frame_feed(source(), d, "i420", (4, 6))
    assert not pulled                                              # nothing is pulled before a piece is asked for


def test_fake_kernels_give_the_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    k = list(yr.constants())
    with FakeTensorMode():
        raw = torch.empty(3, yr.frame_bytes("nv12", 19, 33), dtype=torch.uint8, device="cuda")
        for layout, shape in (("hwc", (3, 19, 33, 3)), ("pose", (3, 3, 19, 33)), ("chw", (3, 3, 19, 33))):
            out = torch.ops.sf_hip.yuv_decode_frames(raw, "nv12", 19, 33, k, "triangle", layout, torch.bfloat16)
            assert tuple(out.shape) == shape and out.dtype == torch.bfloat16
        out = torch.ops.sf_hip.yuv_encode_frames(torch.empty(2, 3, 17, 66, device="cuda"), "i422", k, False)
        assert tuple(out.shape) == (2, yr.frame_bytes("i422", 17, 66)) and out.dtype == torch.uint8
        out = torch.ops.sf_hip.yuv_encode_frames(torch.empty(2, 17, 66, 3, dtype=torch.uint8, device="cuda"), "i420", k, False)
        assert tuple(out.shape) == (2, yr.frame_bytes("i420", 17, 66))


def test_generate_refuses_misplaced_yuv_flags(tmp_path):
    import subprocess
    import sys
    gen = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "generate.py")
    base = [sys.executable, gen, "--config_path", "c", "--data_path", "d", "--output_folder", "o"]
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(b"YUV4MPEG2 W4 H4 F16:1\n")
    for extra, text in [(["--video_format", "yuv"], "--video_format"),
                        (["--pose_yuv_matrix", "bt709"], "need --pose_path"),
                        (["--pose_path", str(clip), "--pose_random_init_seed", "0"], "clip.y4m needs --ref_pose_path"),
                        (["--pose_path", str(tmp_path / "clip.pt"), "--pose_random_init_seed", "0", "--pose_yuv_chroma", "nearest"], "no such file")]:
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 2 and text in r.stderr, r.stderr[-500:]
