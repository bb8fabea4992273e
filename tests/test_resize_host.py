"""Host-side tests of the frame resizer (no GPU): the numpy definition `resize_reference.coefficients / resize / cover_box`
against `PIL.Image.resize` bit for bit (bilinear and bicubic; reduction, enlargement, one axis only, a 1-row input, a mixed
7.1x reduction / 6x enlargement, one real 720x1280 -> 480x832 frame; noise and sparse saturated content, which drives the
bicubic overshoot into both clamps), the header against `_lib.SIGNATURES`, the torch operator's fake implementation, the
argument checks of the sf_resize_* entry points, and the ValueErrors of `FrameResizer`, `JpegDecoder.decode(size=)` and
`pose_feed(size=)` that need no device.  There are no tolerances: the arithmetic is integer."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import pose_weights as pw
from self_forcing_amd import resize_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
GEOMETRIES = [((37, 53), (16, 24)), ((16, 24), (37, 53)), ((45, 80), (24, 40)), ((24, 40), (24, 64)), ((90, 161), (40, 72)), ((1, 7), (5, 3)),
              ((33, 33), (33, 17)), ((50, 50), (7, 300))]


def content(kind, h, w, seed=0):
    """uint8 [h, w, 3]: uniform noise, or 10 % random pixels on black"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "sparse":
        x = x * (rng.random((h, w, 1)) < 0.1).astype(np.uint8)
    return x


def pil_resize(x, size, filter, box=None):
    im = Image.fromarray(x)
    if box is not None:
        top, left, ch, cw = box
        im = im.crop((left, top, left + cw, top + ch))
    return np.asarray(im.resize((size[1], size[0]), PIL_FILTERS[filter]))


# ============================================================================================== the definition against Pillow
@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
@pytest.mark.parametrize("kind", ["noise", "sparse"])
@pytest.mark.parametrize("src,dst", GEOMETRIES)
def test_mirror_equals_pillow(src, dst, kind, filter):
    x = content(kind, *src, seed=src[0] + dst[1])
    got = rr.resize(x[None], dst, filter)
    assert got.dtype == np.uint8 and got.shape == (1, *dst, 3)
    assert np.array_equal(got[0], pil_resize(x, dst, filter))


def test_sparse_content_reaches_both_clamps():
    """The bicubic pass on the sparse content overshoots below 0 and above 255 before the clamp: the test above covers both."""
    x = content("sparse", 90, 161, seed=1).astype(np.int64)
    bounds, coefs = rr.coefficients(161, 72, "bicubic")
    acc = np.full((90, 72, 3), 1 << 21, np.int64)
    for k in range(coefs.shape[1]):
        acc += x[:, np.minimum(bounds[:, 0] + k, 160)] * coefs[:, k].astype(np.int64)[None, :, None]
    assert (acc >> 22).min() < 0
    bright = np.full((8, 161, 3), 255, np.int64)
    bright[:, ::7] = 0
    acc = np.full((8, 72, 3), 1 << 21, np.int64)
    for k in range(coefs.shape[1]):
        acc += bright[:, np.minimum(bounds[:, 0] + k, 160)] * coefs[:, k].astype(np.int64)[None, :, None]
    assert (acc >> 22).max() > 255 and np.abs(acc).max() < 2 ** 31              # and int32 holds every sum
    assert np.array_equal(rr.resize(bright.astype(np.uint8)[None], (8, 72), "bicubic")[0], pil_resize(bright.astype(np.uint8), (8, 72), "bicubic"))


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_a_real_pose_frame_720p_to_480x832(filter):
    frame = pw.synth_pose_clip(92, 1, 720, 1280, "skeleton")[:, 0].permute(1, 2, 0).contiguous().numpy()
    assert frame.dtype == np.uint8 and frame.shape == (720, 1280, 3) and frame.any()
    assert np.array_equal(rr.resize(frame[None], (480, 832), filter)[0], pil_resize(frame, (480, 832), filter))


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_crop_is_crop_then_resize(filter):
    x = content("noise", 61, 83, seed=4)
    for box, size in (((3, 5, 37, 53), (16, 24)), ((7, 1, 33, 71), (50, 40)), ((0, 0, 61, 83), (20, 30)), ((60, 82, 1, 1), (3, 3))):
        assert np.array_equal(rr.resize(x[None], size, filter, crop=box)[0], pil_resize(x, size, filter, box)), (box, size)
    for bad in ((0, 0, 62, 83), (-1, 0, 5, 5), (0, 80, 5, 4), (0, 0, 0, 5), (0, 0, 5.5, 5), (0, 0, 5)):
        with pytest.raises(ValueError, match="crop"):
            rr.resize(x[None], (8, 8), filter, crop=bad)


def test_cover_box():
    # 16:9 into 832:480 (26:15): the sides go; 720 * 832 / 480 = 1248
    assert rr.cover_box(720, 1280, 480, 832) == (0, 16, 720, 1248)
    assert rr.cover_box(1080, 1920, 480, 832) == (0, 24, 1080, 1872)
    # a portrait input: top and bottom go; 720 * 480 / 832 = 415.38 -> 415, offset floor((1280 - 415) / 2)
    assert rr.cover_box(1280, 720, 480, 832) == (432, 0, 415, 720)
    assert rr.cover_box(480, 832, 480, 832) == (0, 0, 480, 832) and rr.cover_box(96, 160, 64, 96) == (0, 8, 96, 144)
    assert rr.cover_box(1, 500, 300, 2) == (0, 249, 1, 1) and rr.cover_box(500, 1, 2, 300) == (249, 0, 1, 1)           # sizes at least 1
    for h, w, oh, ow in ((720, 1280, 480, 832), (1280, 720, 480, 832), (97, 31, 5, 64)):
        top, left, ch, cw = rr.cover_box(h, w, oh, ow)
        assert 0 <= top and top + ch <= h and 0 <= left and left + cw <= w and (ch == h or cw == w)
        assert top in ((h - ch) // 2,) and left == (w - cw) // 2
    x = content("noise", 72, 128, seed=5)
    box = rr.cover_box(72, 128, 48, 83)
    assert np.array_equal(rr.resize(x[None], (48, 83), "bicubic", crop=box)[0], pil_resize(x, (48, 83), "bicubic", box))
    with pytest.raises(ValueError, match=">= 1"):
        rr.cover_box(0, 5, 5, 5)


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_identity_table_returns_the_input(filter):
    """An axis that keeps its size: the table is one weight of 1 << 22 on the pixel itself, so the pass changes nothing
    (Pillow skips it)."""
    bounds, coefs = rr.coefficients(29, 29, filter)
    for xx in range(29):
        row = np.zeros(29, np.int64)
        row[bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = coefs[xx, :bounds[xx, 1]]
        assert row[xx] == 1 << 22 and np.count_nonzero(row) == 1
    x = content("noise", 29, 31, seed=6)[None]
    assert np.array_equal(rr.resize(x, (29, 31), filter), x)
    assert np.array_equal(rr.resize(x, (29, 12), filter)[0], pil_resize(x[0], (29, 12), filter))


def test_table_format():
    for in_size, out_size, filter in ((1280, 832, "bicubic"), (720, 480, "bilinear"), (7, 3, "bicubic"), (24, 64, "bilinear"), (800, 100, "bicubic"),
                                      (1, 5, "bicubic")):
        bounds, coefs = rr.coefficients(in_size, out_size, filter)
        ks = rr.kernel_size(in_size, out_size, filter)
        assert bounds.dtype == coefs.dtype == np.int32 and bounds.shape == (out_size, 2) and coefs.shape == (out_size, ks)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ks).all() and (bounds.sum(1) <= in_size).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()            # the kernel's tile extent relies on it
        assert all(not coefs[xx, bounds[xx, 1]:].any() for xx in range(out_size))
        assert np.abs(coefs.sum(1) - (1 << 22)).max() <= ks                      # each row sums to one, up to its roundings
        assert 255 * np.abs(coefs.astype(np.int64)).sum(1).max() < 2 ** 31 - 2 ** 21
        # what one 64-column / 16-row output tile reaches stays inside the bound csrc/resize.hip sizes its LDS with
        scale, support = in_size / out_size, rr.SUPPORT[filter] * max(in_size / out_size, 1.0)
        for tile in (16, 64):
            ends = bounds.sum(1)
            extent = max(ends[min(t + tile, out_size) - 1] - bounds[t, 0] for t in range(0, out_size, tile))
            assert extent <= min(int((tile - 1) * scale + 2 * support) + 3, in_size)
    with pytest.raises(ValueError, match="filter"):
        rr.coefficients(8, 4, "lanczos")
    with pytest.raises(ValueError, match=">= 1"):
        rr.coefficients(8, 0, "bilinear")


# ============================================================================================== header, signatures, operator
def test_python_mirror_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    enum = lambda name: int(re.search(name + r" = (\d+)", text).group(1))                        # noqa: E731
    L = sfa._lib
    assert L.RESIZE_FILTERS == {"bilinear": enum("SF_RESIZE_BILINEAR"), "bicubic": enum("SF_RESIZE_BICUBIC")} == rr.FILTERS
    assert L.RESIZE_MAX_RATIO == int(re.search(r"#define SF_RESIZE_MAX_RATIO (\d+)", text).group(1)) == rr.MAX_RATIO == 8
    for name in ("sf_resize_kernel_size", "sf_resize_frames"):
        getattr(L.lib(), name)                                                   # exported
    assert int(re.search(r"#define SF_HIP_ABI_VERSION (\d+)", text).group(1)) == 11 == L.ABI_VERSION == L.lib().sf_abi_version()
    for in_size, out_size in ((720, 480), (1280, 832), (7, 3), (24, 64), (800, 100), (1, 5), (65535, 8192)):
        for filter in rr.FILTERS:
            assert sfa.ops.resize_kernel_size(in_size, out_size, filter) == rr.kernel_size(in_size, out_size, filter)
    assert "FrameResizer" in sfa.__all__ and "resize_reference" in sfa.__all__


def test_fake_operator_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "resize_frames" in sfa.torch_ops.OPS and "resize_frames_out" in sfa.torch_ops.OPS
    assert "Tensor(a0!) out" in str(torch.ops.sf_hip.resize_frames_out.default._schema)
    shapes = {"hwc": (2, 45, 80, 3), "pose": (3, 2, 45, 80), "chw": (2, 3, 45, 80)}
    outs = {"hwc": (2, 24, 40, 3), "pose": (3, 2, 24, 40), "chw": (2, 3, 24, 40)}
    with FakeTensorMode():
        tables = [torch.empty(s, dtype=torch.int32) for s in ((40, 2), (40, 5), (24, 2), (24, 5))]
        for layout, shape in shapes.items():
            for out_layout, want in outs.items():
                for dtype in (torch.uint8, torch.float32, torch.bfloat16):
                    got = torch.ops.sf_hip.resize_frames(torch.empty(shape, dtype=torch.uint8), *tables, "bilinear", layout, out_layout, dtype, None)
                    assert tuple(got.shape) == want and got.dtype == dtype
        assert torch.ops.sf_hip.resize_frames_out(torch.empty(outs["pose"], dtype=torch.uint8), torch.empty(shapes["hwc"], dtype=torch.uint8), *tables,
                                                  "bicubic", "hwc", "pose", [1, 2, 30, 60]) is None
        with pytest.raises(Exception, match="layout"):
            torch.ops.sf_hip.resize_frames(torch.empty(shapes["hwc"], dtype=torch.uint8), *tables, "bilinear", "nhwc", "hwc", torch.uint8, None)


# ============================================================================================== the C entry points
def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    import ctypes as C
    lib = sfa._lib.lib()
    ks = lib.sf_resize_kernel_size
    assert ks(720, 480, 1) == 7 and ks(720, 480, 0) == 5 and ks(480, 720, 1) == 5 and ks(480, 720, 0) == 3 and ks(800, 100, 1) == 33
    assert ks(720, 480, 2) == 0 and b"filter" in lib.sf_last_error()
    assert ks(0, 480, 0) == 0 and b"sizes" in lib.sf_last_error()
    assert ks(720, 0, 0) == 0 and b"sizes" in lib.sf_last_error()

    box = lambda *v: (C.c_int32 * 4)(*v)                                                           # noqa: E731
    ok = dict(frames=4096, layout=0, n=2, h=45, w=80, crop=None, bh=4096, kh=4096, bv=4096, kv=4096, filter=0, out=4096, out_layout=1, dtype=0, oh=24, ow=40,
              stream=None)

    def frames(**kw):
        return lib.sf_resize_frames(*{**ok, **kw}.values())
    for name in ("frames", "out", "bh", "kh", "bv", "kv"):
        assert frames(**{name: None}) != 0 and b"null buffer" in lib.sf_last_error(), name
    assert frames(layout=3) != 0 and b"layout" in lib.sf_last_error()
    assert frames(out_layout=-1) != 0 and b"layout" in lib.sf_last_error()
    assert frames(dtype=3) != 0 and b"dtype" in lib.sf_last_error()
    assert frames(filter=2) != 0 and b"filter" in lib.sf_last_error()
    assert frames(n=0) != 0 and b"n=0" in lib.sf_last_error()
    assert frames(n=70000) != 0 and b"n=70000" in lib.sf_last_error()
    assert frames(h=0) != 0 and b"frame 0x80" in lib.sf_last_error()
    assert frames(w=70000) != 0 and b"frame" in lib.sf_last_error()
    assert frames(oh=0) != 0 and b"output 0x40" in lib.sf_last_error()
    assert frames(ow=-3) != 0 and b"output" in lib.sf_last_error()
    for bad in (box(0, 0, 46, 80), box(-1, 0, 10, 10), box(0, 41, 10, 40), box(0, 0, 0, 10), box(40, 0, 6, 10), box(0, 0, 10, 0)):
        assert frames(crop=bad) != 0 and b"crop" in lib.sf_last_error() and b"45x80" in lib.sf_last_error(), list(bad)
    # 45 -> 5 is 9x down; 40 -> 5 is exactly the limit and passes this check (it fails the next one: the alignment)
    assert frames(oh=5) != 0 and b"more than 8x" in lib.sf_last_error()
    assert frames(ow=9) != 0 and b"more than 8x" in lib.sf_last_error()
    assert frames(crop=box(0, 0, 40, 72), oh=5, ow=9, out=4100) != 0 and b"aligned" in lib.sf_last_error()
    assert frames(crop=box(3, 5, 9, 17), oh=1) != 0 and b"more than 8x" in lib.sf_last_error()      # the crop's size counts, not the frame's
    assert frames(frames=4098) != 0 and b"aligned" in lib.sf_last_error()
    assert frames(out=4104) != 0 and b"aligned" in lib.sf_last_error()
    assert frames(kv=4097) != 0 and b"tables" in lib.sf_last_error()


# ============================================================================================== the Python surface
def test_frame_resizer_checks_that_need_no_device():
    rs = sfa.FrameResizer()
    x = torch.zeros(2, 45, 80, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        rs.resize(x, (24, 40))
    with pytest.raises(ValueError, match="uint8"):
        rs.resize(x.float(), (24, 40))
    with pytest.raises(ValueError, match="uint8"):
        rs.resize(x.numpy(), (24, 40))
    for bad in (x[0], x.permute(0, 3, 1, 2), x[:0]):
        with pytest.raises(ValueError, match=r"expected \[N, H, W, 3\]"):
            rs.resize(bad, (24, 40))
    with pytest.raises(ValueError, match=r"expected \[3, N, H, W\]"):
        rs.resize(x, (24, 40), layout="pose")
    with pytest.raises(ValueError, match=r"expected \[N, 3, H, W\]"):
        rs.resize(x, (24, 40), layout="chw")
    for size in ((0, 40), (24, -1), (24,), (24.5, 40)):
        with pytest.raises(ValueError, match="size"):
            rs.resize(x, size)
    with pytest.raises(ValueError, match="filter"):
        rs.resize(x, (24, 40), filter="nearest")
    with pytest.raises(ValueError, match="layout"):
        rs.resize(x, (24, 40), layout="nhwc")
    with pytest.raises(ValueError, match="layout"):
        rs.resize(x, (24, 40), out_layout="nchw")
    with pytest.raises(ValueError, match="dtype"):
        rs.resize(x, (24, 40), dtype=torch.float16)
    with pytest.raises(ValueError, match="fit"):
        rs.resize(x, (24, 40), fit="contain")
    with pytest.raises(ValueError, match="not both"):
        rs.resize(x, (24, 40), crop=(0, 0, 10, 10), fit="cover")
    with pytest.raises(ValueError, match="crop"):
        rs.resize(x, (24, 40), crop=(0, 0, 46, 80))
    with pytest.raises(ValueError, match="more than 8x"):
        rs.resize(x, (5, 40))                                                    # 45 -> 5
    with pytest.raises(ValueError, match="more than 8x"):
        rs.resize(x, (24, 2), crop=(0, 0, 45, 17))                               # the crop's width counts: 17 -> 2
    wide = torch.zeros(1, 10, 900, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="more than 8x"):
        rs.resize(wide, (10, 10))
    with pytest.raises(ValueError, match="no CPU fallback"):
        rs.resize(wide, (10, 10), fit="cover")                                   # the cover box is 10 x 10: the ratio check passes


def test_decoder_and_pose_feed_checks_that_need_no_device():
    dec = sfa.JpegDecoder()
    a = jr.encode(np.zeros((1, 64, 96, 3), np.uint8), 90, "420", 10)[0]
    with pytest.raises(ValueError, match="size"):
        dec.decode([a], size=(0, 10))
    with pytest.raises(ValueError, match="filter"):
        dec.decode([a], size=(32, 64), filter="box")
    with pytest.raises(ValueError, match="fit"):
        dec.decode([a], size=(32, 64), fit="pad")
    with pytest.raises(ValueError, match="layout"):
        dec.decode([a], layout="nchw", size=(32, 64))
    with pytest.raises(ValueError, match="dtype"):
        dec.decode([a], dtype=torch.float16, size=(32, 64))
    with pytest.raises(ValueError, match="more than 8x"):
        dec.decode([a], size=(7, 64))                                            # 64 -> 7
    with pytest.raises(ValueError, match="no files"):
        dec.decode([], size=(32, 64))
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.JpegDecoder(device="cpu").decode([a], size=(32, 64))
    with pytest.raises(ValueError, match="size"):
        next(sfa.jpeg.pose_feed([a], dec, 4, size=(32,)))
    with pytest.raises(ValueError, match="filter"):
        next(sfa.jpeg.pose_feed([a], dec, 4, size=(32, 64), filter="area"))
    with pytest.raises(ValueError, match="fit"):
        next(sfa.jpeg.pose_feed([a], dec, 4, size=(32, 64), fit="fill"))
    with pytest.raises(ValueError, match="frames_per_piece"):
        next(sfa.jpeg.pose_feed([a], dec, 0, size=(32, 64)))


def test_generate_pose_resize_flag(tmp_path):
    import subprocess
    import sys
    gen = os.path.join(ROOT, "generate.py")
    pt = tmp_path / "pose.pt"
    pt.write_bytes(b"")
    base = [sys.executable, gen, "--config_path", "c", "--data_path", "d", "--output_folder", "o", "--pose_random_init_seed", "0"]
    r = subprocess.run(base + ["--pose_path", str(pt), "--pose_resize", "cover"], capture_output=True, text=True)
    assert r.returncode == 2 and "--pose_resize" in r.stderr and ".avi" in r.stderr
    r = subprocess.run(base + ["--pose_path", str(pt), "--pose_resize", "fill"], capture_output=True, text=True)
    assert r.returncode == 2 and "invalid choice" in r.stderr
    r = subprocess.run([sys.executable, gen, "--config_path", "c", "--data_path", "d", "--output_folder", "o", "--pose_resize", "stretch"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--pose_resize" in r.stderr
