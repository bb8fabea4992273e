"""GPU tests of the frame resizer (csrc/resize.hip behind `FrameResizer`), all exact (`torch.equal`; the arithmetic is
integer): the kernel against the host definition `resize_reference.resize` and against Pillow over the host tests'
geometries, the kernel's own edges (an output of exactly one tile grid, one more than it, the 8x ratio limit), frame
stride, every layout and type, `crop` / `fit="cover"`, `out=`, and the places the frames go: `JpegDecoder.decode(size=)`,
`pose_feed(size=)`, a `PoseStream`, `generate.py --pose_resize`.  Run with `-m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import pose_weights as pw
from self_forcing_amd import resize_reference as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TILE_H, TILE_W = 16, 64                     # csrc/resize.hip: TH, TW
GEOMETRIES = [((37, 53), (16, 24)), ((16, 24), (37, 53)), ((45, 80), (24, 40)), ((24, 40), (24, 64)), ((90, 161), (40, 72)), ((1, 7), (5, 3)),
              ((33, 33), (33, 17)), ((50, 50), (7, 300)),
              ((50, 190), (2 * TILE_H, 2 * TILE_W)),              # whole tiles in both axes
              ((50, 190), (2 * TILE_H + 1, 2 * TILE_W + 1)),      # one row and one column more
              ((8 * 19, 40), (19, 40)),                           # exactly the 8x limit, vertically (two tiles)
              ((20, 8 * 70), (20, 70))]                           # and horizontally (two tiles)


@pytest.fixture(scope="module")
def rs():
    return sfa.FrameResizer(device=DEV)


def content(kind, n, h, w, seed=0):
    """uint8 [n, h, w, 3]: uniform noise, or 10 % random pixels on black; every frame differs"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "sparse":
        x = x * (rng.random((n, h, w, 1)) < 0.1).astype(np.uint8)
    return x


def to_layout(hwc, layout):
    """torch uint8 [n, h, w, 3] in `layout`"""
    return {"hwc": hwc, "pose": hwc.permute(3, 0, 1, 2), "chw": hwc.permute(0, 3, 1, 2)}[layout].contiguous()


# ============================================================================================== geometries
@pytest.mark.parametrize("src,dst", GEOMETRIES)
def test_geometries_equal_the_mirror(rs, src, dst):
    for kind in ("noise", "sparse"):
        x = content(kind, 1, *src, seed=src[1] + dst[0])
        xd = torch.from_numpy(x).to(DEV)
        for filter in ("bilinear", "bicubic"):
            got = rs.resize(xd, dst, filter)
            assert got.dtype == torch.uint8 and got.shape == (1, *dst, 3) and got.is_contiguous()
            want = rr.resize(x, dst, filter)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (kind, filter, int((got.cpu().numpy() != want).sum()))


def test_frames_differ_and_equal_pillow(rs):
    """n = 3 frames of different content in one call, against Pillow itself."""
    x = content("noise", 3, 45, 80, seed=11)
    x[1] = content("sparse", 1, 45, 80, seed=12)[0]
    for filter, pil in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
        got = rs.resize(torch.from_numpy(x).to(DEV), (24, 40), filter).cpu().numpy()
        for k in range(3):
            assert np.array_equal(got[k], np.asarray(Image.fromarray(x[k]).resize((40, 24), pil))), (filter, k)
    assert not np.array_equal(got[0], got[2])


# ============================================================================================== layouts and types
def test_layouts_and_dtypes(rs):
    x = content("noise", 3, 45, 80, seed=13)
    want = torch.from_numpy(rr.resize(x, (24, 40), "bicubic"))
    hwc = torch.from_numpy(x)
    for layout in ("hwc", "pose", "chw"):
        xd = to_layout(hwc, layout).to(DEV)
        for out_layout in ("hwc", "pose", "chw"):
            got = rs.resize(xd, (24, 40), "bicubic", layout=layout, out_layout=out_layout)
            assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu(), to_layout(want, out_layout)), (layout, out_layout)
            for dtype in (torch.float32, torch.bfloat16):
                got = rs.resize(xd, (24, 40), "bicubic", layout=layout, out_layout=out_layout, dtype=dtype)
                ref = torch.from_numpy(jr.to_float(to_layout(want, out_layout).numpy())).to(dtype)       # the decoder's conversion
                assert got.dtype == dtype and torch.equal(got.cpu(), ref), (layout, out_layout, dtype)
        assert torch.equal(rs.resize(xd, (24, 40), "bicubic", layout=layout).cpu(), to_layout(want, layout))       # out_layout defaults to layout
    # widths that are no multiple of four take the element-wise stores
    odd = torch.from_numpy(rr.resize(x, (23, 37), "bilinear"))
    for out_layout in ("hwc", "pose", "chw"):
        for dtype in (torch.uint8, torch.float32, torch.bfloat16):
            got = rs.resize(hwc.to(DEV), (23, 37), "bilinear", out_layout=out_layout, dtype=dtype)
            ref = to_layout(odd, out_layout)
            ref = ref if dtype == torch.uint8 else torch.from_numpy(jr.to_float(ref.numpy())).to(dtype)
            assert torch.equal(got.cpu(), ref), (out_layout, dtype)


def test_out_is_honoured(rs):
    x = content("noise", 2, 45, 80, seed=14)
    xd = torch.from_numpy(x).to(DEV)
    want = to_layout(torch.from_numpy(rr.resize(x, (24, 40), "bilinear")), "pose")
    out = torch.full((3, 2, 24, 40), 7, dtype=torch.uint8, device=DEV)
    got = rs.resize(xd, (24, 40), out_layout="pose", out=out)
    assert got is out and torch.equal(out.cpu(), want)
    outf = torch.zeros(3, 2, 24, 40, dtype=torch.float32, device=DEV)
    assert rs.resize(xd, (24, 40), out_layout="pose", dtype=torch.float32, out=outf) is outf
    assert torch.equal(outf.cpu(), torch.from_numpy(jr.to_float(want.numpy())))
    for bad in (torch.zeros(3, 2, 24, 41, dtype=torch.uint8, device=DEV), outf, out.cpu()):
        with pytest.raises(ValueError, match="out must be"):
            rs.resize(xd, (24, 40), out_layout="pose", out=bad)
    # a view that starts inside a dword is taken too
    assert torch.equal(rs.resize(xd.reshape(-1)[3:3 + 44 * 80 * 3].view(1, 44, 80, 3), (24, 40)).cpu(),
                       torch.from_numpy(rr.resize(x.reshape(-1)[3:3 + 44 * 80 * 3].reshape(1, 44, 80, 3), (24, 40))))


# ============================================================================================== crop and cover
def test_crop_and_cover(rs):
    x = content("noise", 2, 72, 128, seed=15)
    xd = torch.from_numpy(x).to(DEV)
    for box, size, filter in (((3, 5, 37, 53), (16, 24), "bicubic"), ((7, 1, 33, 71), (50, 40), "bilinear"), ((71, 127, 1, 1), (3, 5), "bicubic")):
        got = rs.resize(xd, size, filter, crop=box)
        assert torch.equal(got.cpu(), torch.from_numpy(rr.resize(x, size, filter, crop=box))), box
    # planar input with a crop: the three runs of a row start at the crop's left edge
    got = rs.resize(to_layout(torch.from_numpy(x), "pose").to(DEV), (16, 24), "bicubic", layout="pose", out_layout="hwc", crop=(3, 5, 37, 53))
    assert torch.equal(got.cpu(), torch.from_numpy(rr.resize(x, (16, 24), "bicubic", crop=(3, 5, 37, 53))))
    box = rr.cover_box(72, 128, 48, 83)
    assert box == (0, 2, 72, 124)
    got = rs.resize(xd, (48, 83), "bilinear", fit="cover")
    assert torch.equal(got.cpu(), torch.from_numpy(rr.resize(x, (48, 83), "bilinear", crop=box)))
    assert torch.equal(got, rs.resize(xd, (48, 83), "bilinear", crop=box))
    for k in range(2):                                       # and Pillow directly
        im = Image.fromarray(x[k]).crop((box[1], box[0], box[1] + box[3], box[0] + box[2])).resize((83, 48), Image.BILINEAR)
        assert np.array_equal(got[k].cpu().numpy(), np.asarray(im))


def test_ratio_beyond_the_limit_raises(rs):
    x = torch.zeros(1, 8 * 19 + 1, 40, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="more than 8x"):
        rs.resize(x, (19, 40))
    tv, th = rs.tables(8 * 19 + 1, 19, "bilinear"), rs.tables(40, 40, "bilinear")
    with pytest.raises(sfa._lib.SfHipError, match="more than 8x"):          # the C entry point refuses it too
        sfa.ops.resize_frames(x, th, tv, "bilinear")
    assert rs.resize(x[:, 1:], (19, 40)).shape == (1, 19, 40, 3)


# ============================================================================================== the decoder
def pose_files(n, h, w, seed=92):
    """n skeleton pose frames of h x w as JPEG files (the reference encoder's)"""
    clip = pw.synth_pose_clip(seed, n, h, w, "skeleton").permute(1, 2, 3, 0).contiguous().numpy()
    return jr.encode(clip, 90, "420", 10)


def test_decoder_resizes_what_it_decodes(rs):
    dec = sfa.JpegDecoder(device=DEV)
    files = pose_files(13, 64, 96)
    full = dec.decode(files, "hwc")
    assert full.shape == (13, 64, 96, 3)
    for filter, fit in (("bilinear", "stretch"), ("bicubic", "stretch"), ("bilinear", "cover")):
        want = rs.resize(full, (32, 64), filter, out_layout="pose", fit=fit)
        got = dec.decode(files, layout="pose", size=(32, 64), filter=filter, fit=fit)
        assert got.dtype == torch.uint8 and got.shape == (3, 13, 32, 64) and torch.equal(got, want), (filter, fit)
    # the host definition end to end: the integer decode, then the integer resize
    ref = rr.resize(np.stack([jr.decode(f) for f in files]), (32, 64), "bilinear")
    assert torch.equal(dec.decode(files, size=(32, 64)).cpu(), torch.from_numpy(ref))
    gotf = dec.decode(files, layout="chw", dtype=torch.bfloat16, size=(32, 64))
    assert torch.equal(gotf.cpu(), torch.from_numpy(jr.to_float(ref)).permute(0, 3, 1, 2).to(torch.bfloat16))
    assert torch.equal(dec.decode(files, "hwc"), full)              # without size: what it was
    for piece in (5, 12):
        pieces = list(sfa.jpeg.pose_feed(iter(files), dec, piece, size=(32, 64)))
        assert [p.shape[1] for p in pieces] == [piece] * (13 // piece) + [13 % piece]
        assert torch.equal(torch.cat(pieces, dim=1).cpu(), torch.from_numpy(ref).permute(3, 0, 1, 2))


def test_pose_stream_fed_from_larger_frames():
    """A PoseStream at 64x96, fed by pose_feed from 96x160 JPEG frames, gives the bits of PoseEmbedder.embed on the resized clip."""
    emb = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=DEV)
    dec = sfa.JpegDecoder(device=DEV)
    files = pose_files(9, 96, 160)
    clip = torch.from_numpy(rr.resize(np.stack([jr.decode(f) for f in files]), (64, 96), "bilinear")).permute(3, 0, 1, 2).contiguous()
    want, fhw = emb.embed(clip.to(DEV))
    stream = sfa.PoseStream(emb, 64, 96)
    rows = []
    for piece in sfa.jpeg.pose_feed(files, dec, 4, size=(64, 96)):
        assert piece.dtype == torch.uint8 and piece.shape[0] == 3 and piece.shape[2:] == (64, 96)
        rows.append(stream.push(piece)[0])
    rows.append(stream.close()[0])
    assert fhw == (3, 4, 6) and stream.latent_frames_done == 3 and torch.equal(torch.cat(rows, dim=1), want)


def test_generate_resizes_a_pose_clip_of_another_size(tmp_path):
    """generate.py --pose_path clip.avi --ref_pose_path ref.jpg --pose_resize cover with a 96x176 clip and a 80x112 reference image
    on the 64x96 tiny configuration writes the latents of the .pt dict that holds the same frames resized by the host definition."""
    files = pose_files(9, 96, 176)
    image = pw.synth_pose_image(93, 80, 112, "skeleton").numpy()
    ref_file = jr.encode(image[None], 95, "444", 21)[0]
    sfa.mjpeg.write_avi(str(tmp_path / "clip.avi"), files, 16, 176, 96)
    (tmp_path / "ref.jpg").write_bytes(ref_file)
    frames = np.stack([jr.decode(f) for f in files])
    clip = rr.resize(frames, (64, 96), "bilinear", crop=rr.cover_box(96, 176, 64, 96))
    ref = rr.resize(jr.decode(ref_file)[None], (64, 96), "bilinear", crop=rr.cover_box(80, 112, 64, 96))[0]
    torch.save({"dwpose_data": torch.from_numpy(clip).permute(3, 0, 1, 2).contiguous(), "random_ref_dwpose": torch.from_numpy(ref)}, tmp_path / "pose.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\n"
                   "independent_first_frame: false\nmodel_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n")
    (tmp_path / "p.txt").write_text("a red fox\n")
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", str(cfg), "--data_path", str(tmp_path / "p.txt"),
            "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height", "8", "--latent_width", "12", "--seed", "5",
            "--pose_random_init_seed", "0"]
    runs = {"avi": ["--pose_path", str(tmp_path / "clip.avi"), "--ref_pose_path", str(tmp_path / "ref.jpg"), "--pose_resize", "cover"],
            "pt": ["--pose_path", str(tmp_path / "pose.pt")]}
    for folder, extra in runs.items():
        res = subprocess.run(base + extra + ["--output_folder", str(tmp_path / folder)], capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, res.stderr[-2000:]
    avi, pt = (torch.load(tmp_path / k / "0-0.pt") for k in runs)
    assert avi.shape == (3, 16, 8, 12) and bool(torch.isfinite(avi.float()).all()) and bool(avi.float().abs().sum() > 0)
    assert torch.equal(avi, pt)
