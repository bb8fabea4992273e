"""GPU tests of the JPEG decoder (csrc/jpeg_decode.hip behind `JpegDecoder`), all exact: the entropy decoder against the
encoder's own coefficient buffer, the pixels against the integer host definition `jpeg_reference.decode` for files the
encoder, the reference encoder and PIL wrote (4:4:4, 4:2:2, 4:2:0, grayscale; optimised Huffman tables; with and without
restart markers; on and off the MCU grid) in every layout and type, damaged files, and the three places the frames go:
`PoseEmbedder.embed`, `pose_feed`, `generate.py --pose_path clip.avi`.  Run with `-m gpu`."""
import io
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SAMPLING = {0: "444", 1: "422", 2: "420", "L": "gray"}


@pytest.fixture(scope="module")
def dec():
    return sfa.JpegDecoder(device=DEV)


def frames_u8(n, h, w, seed=0):
    """uint8 [n, h, w, 3]: noise, a smooth picture, a skeleton-like one (thin lines on black), in turn"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        if k % 3 == 0:
            f = rng.integers(0, 256, (h, w, 3))
        elif k % 3 == 1:
            f = np.stack([127 + 100 * np.sin(xx / 17 + yy / 9 + k), 127 + 100 * np.cos(xx / 11 - k), 127 + 90 * np.sin(yy / 7 + 2 * k)], -1)
        else:
            f = np.zeros((h, w, 3))
            f[(h // 4 + k) % h] = (255, 0, 0)
            f[:, (w // 3 + k) % w] = (0, 255, 80)
            f[np.abs(yy - xx * h // w) < 2] = (30, 90, 255)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(out)


def pil_file(u8, quality, subsampling, optimize, restart):
    buf = io.BytesIO()
    if subsampling == "L":
        Image.fromarray(u8[..., 0]).save(buf, "JPEG", quality=quality, optimize=optimize, restart_marker_blocks=restart)
    else:
        Image.fromarray(u8).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=optimize, restart_marker_blocks=restart)
    return buf.getvalue()


_CLASSES = {}


def file_class(h, w, subsampling):
    """(files, reference frames uint8 [n, h, w, 3]) of one size and sampling, computed once: PIL-written files that differ in
    content, quality, Huffman tables (optimised or Annex K) and restart interval."""
    key = (h, w, subsampling)
    if key not in _CLASSES:
        u8 = frames_u8(3, h, w, seed=h + w)
        files = [pil_file(u8[0], 90, subsampling, True, 0), pil_file(u8[1], 50, subsampling, False, 3), pil_file(u8[2], 100, subsampling, True, 1),
                 pil_file(u8[0], 100, subsampling, True, 2)]
        _CLASSES[key] = (files, np.stack([jr.decode(f) for f in files]))
    return _CLASSES[key]


def as_layout(ref_u8, layout, dtype):
    """the reference frames [n, h, w, 3] as `JpegDecoder.decode` returns them"""
    r = torch.from_numpy(ref_u8) if dtype == torch.uint8 else torch.from_numpy(jr.to_float(ref_u8)).to(dtype)
    return {"hwc": r, "pose": r.permute(3, 0, 1, 2), "chw": r.permute(0, 3, 1, 2)}[layout].contiguous()


# ============================================================================================== coefficients
@pytest.mark.parametrize("subsampling", ["420", "444"])
@pytest.mark.parametrize("h,w,n", [(16, 16, 3), (48, 80, 3), (480, 832, 1)])
def test_coefficient_round_trip(dec, h, w, n, subsampling):
    x = torch.from_numpy(frames_u8(n, h, w, seed=h)).to(DEV)
    for quality, ri in ((100, 1), (90, None), (100, 7), (50, 60000)):       # 7 spans MCU rows (5 / 10 / 52 / 104 MCUs per row); 60000: one interval
        enc = sfa.JpegEncoder(quality, subsampling, restart_interval=ri, device=DEV)
        files = enc.encode(x)
        want = enc.coefficients(x)
        got = dec.coefficients(files)
        assert got.dtype == torch.int16 and got.shape == want.shape
        assert torch.equal(got, want), (quality, ri, int((got != want).sum()))
        assert dec.status == [0] * n
        assert dec.info(files[0]) == (h, w, subsampling, enc.restart_interval)


def test_coefficients_of_crafted_symbols(dec):
    """ZRL runs, a non-zero 63rd coefficient, the largest DC and AC categories, all-zero blocks: through the encoder's entropy
    coder and back."""
    c = torch.zeros(2, 24, 64, dtype=torch.int16)
    c[0, 0, 0], c[0, 0, 63] = 100, 3
    c[0, 1, 0], c[0, 1, 40] = -1024, -5
    c[0, 2, 0], c[0, 2, 1] = 1016, 1023
    c[1, :, 49] = torch.arange(-12, 12, dtype=torch.int16)
    c[1, 7, 63], c[1, 9, 0] = -1023, -1000
    enc = sfa.JpegEncoder(100, "420", restart_interval=3, device=DEV)
    files = enc.encode_coefficients(c.to(DEV), 32, 32)
    assert torch.equal(dec.coefficients(files).cpu(), c)
    assert np.array_equal(dec.decode(files).cpu().numpy(), np.stack([jr.decode(f) for f in files]))


# ============================================================================================== pixels
@pytest.mark.parametrize("h,w", [(16, 16), (64, 96), (50, 70)])
@pytest.mark.parametrize("subsampling", [0, 1, 2, "L"])
def test_pixels_equal_the_reference(dec, subsampling, h, w):
    files, ref = file_class(h, w, subsampling)              # one call mixes qualities, Huffman tables and restart intervals
    assert dec.info(files[0])[:3] == (h, w, SAMPLING[subsampling]) and {dec.info(f)[3] for f in files} != {0}
    for layout in ("hwc", "pose", "chw"):
        for dtype in (torch.uint8, torch.float32, torch.bfloat16):
            got = dec.decode(files, layout=layout, dtype=dtype)
            want = as_layout(ref, layout, dtype)
            assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got.cpu(), want), (layout, dtype)
    assert torch.equal(as_layout(ref, "chw", torch.float32), torch.from_numpy(ref).permute(0, 3, 1, 2).float() / 127.5 - 1)
    # the coefficients of a PIL file, padding MCUs included
    assert np.array_equal(dec.coefficients(files[:2]).cpu().numpy(), np.stack([jr.decode_coefficients(f) for f in files[:2]]))


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_pixels_of_encoder_files(dec, subsampling):
    """What the project writes it reads: the encoder's files at the default interval, and the reference encoder's."""
    u8 = frames_u8(3, 48, 80, seed=3)
    files = sfa.JpegEncoder(90, subsampling, device=DEV).encode(torch.from_numpy(u8).to(DEV)) + jr.encode(u8[:1], 75, subsampling, 4)
    ref = np.stack([jr.decode(f) for f in files])
    assert np.array_equal(dec.decode(files).cpu().numpy(), ref)
    assert np.abs(ref[1].astype(int) - u8[1]).mean() < 3                       # and it is the picture that went in
    frame = frames_u8(2, 480, 832, seed=9)[1:]               # the smooth one: the host definition decodes it in half a second
    big = sfa.JpegEncoder(90, subsampling, device=DEV).encode(torch.from_numpy(frame).to(DEV))
    assert np.array_equal(dec.decode(big).cpu().numpy()[0], jr.decode(big[0]))


# ============================================================================================== damaged files
def test_truncated_file_is_reported_and_harms_nothing(dec):
    u8 = frames_u8(3, 48, 80, seed=5)
    for ri in (None, 60000):                                # with restart markers and as a single interval
        files = sfa.JpegEncoder(90, "420", restart_interval=ri, device=DEV).encode(torch.from_numpy(u8).to(DEV))
        info = jr.parse(files[1])
        cut = files[1][:(info.scan_offset + info.scan_end) // 2] + b"\xff\xd9"
        whole = dec.decode(files)
        with pytest.raises(sfa._lib.SfHipError, match="file 1: a truncated restart interval"):
            dec.decode([files[0], cut, files[2]])
        with pytest.raises(sfa._lib.SfHipError, match="truncated"):
            dec.coefficients([cut])
        got = dec.decode([files[0], cut, files[2]], strict=False)
        assert dec.status[0] == 0 and dec.status[2] == 0 and dec.status[1] & 4 and bool(dec.status[1] & 8) == (ri is None)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[2], whole[2])
        # what lies in front of the cut is decoded: the first MCU row (its last rows blend in chroma of the row below)
        assert torch.equal(got[1, :12], whole[1, :12]) and not torch.equal(got[1], whole[1])
        assert torch.equal(dec.decode(files), whole)         # and the next call is what it was
    # bits that are no code: nine 1-bits start no code of the Annex K DC table (0xFF in front of 0xFF is data, not a marker)
    good = files[0]
    info = jr.parse(good)
    body = bytearray(good)
    body[info.scan_offset:info.scan_offset + 8] = b"\xff" * 8
    with pytest.raises(sfa._lib.SfHipError, match="file 0: a bit pattern that is no Huffman code"):
        dec.decode([bytes(body)])
    with pytest.raises(ValueError, match="bad Huffman code"):
        jr.decode(bytes(body))
    assert torch.equal(dec.decode(files), whole)


# ============================================================================================== where the frames go
def pose_files(n, h=64, w=96):
    """n skeleton pose frames as JPEG files (the reference encoder's), their clip [3, n, h, w] uint8 as the definition decodes it"""
    clip = pw.synth_pose_clip(92, n, h, w, "skeleton").permute(1, 2, 3, 0).contiguous().numpy()
    files = jr.encode(clip, 90, "420", 10)
    return files, torch.from_numpy(np.stack([jr.decode(f) for f in files])).permute(3, 0, 1, 2).contiguous()


def test_pose_embedder_takes_the_decoded_clip(dec):
    emb = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=DEV)
    files, ref = pose_files(9)
    got = dec.decode(files, layout="pose")
    assert got.dtype == torch.uint8 and got.shape == (3, 9, 64, 96) and torch.equal(got.cpu(), ref)
    tokens, fhw = emb.embed(got)
    want, fhw_ref = emb.embed(ref)
    assert fhw == fhw_ref == (3, 4, 6) and torch.equal(tokens, want)


@pytest.mark.parametrize("piece", [1, 5, 12])
def test_pose_feed_pieces_concatenate_to_the_clip(dec, piece):
    files, ref = pose_files(13)
    whole = dec.decode(files, layout="pose")
    feed = sfa.jpeg.pose_feed(iter(files), dec, piece)
    first = next(feed)                                      # decoded when pulled: one piece so far
    assert first.shape == (3, min(piece, 13), 64, 96)
    pieces = [first] + list(feed)
    assert [p.shape[1] for p in pieces] == [piece] * (13 // piece) + ([13 % piece] if 13 % piece else [])
    assert all(p.dtype == torch.uint8 and p.is_contiguous() for p in pieces)
    assert torch.equal(torch.cat(pieces, dim=1), whole) and torch.equal(whole.cpu(), ref)


def test_generate_reads_an_mjpeg_pose_clip(tmp_path):
    """generate.py --pose_path clip.avi --ref_pose_path ref.jpg writes the latents of the .pt dict that holds the same frames
    as the definition decodes them."""
    files, ref = pose_files(9)
    image = pw.synth_pose_image(93, 64, 96, "skeleton").numpy()
    ref_file = jr.encode(image[None], 95, "444", 21)[0]
    sfa.mjpeg.write_avi(str(tmp_path / "clip.avi"), files, 16, 96, 64)
    (tmp_path / "ref.jpg").write_bytes(ref_file)
    torch.save({"dwpose_data": ref, "random_ref_dwpose": torch.from_numpy(jr.decode(ref_file))}, tmp_path / "pose.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\n"
                   "independent_first_frame: false\nmodel_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n")
    (tmp_path / "p.txt").write_text("a red fox\n")
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", str(cfg), "--data_path", str(tmp_path / "p.txt"),
            "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height", "8", "--latent_width", "12", "--seed", "5",
            "--pose_random_init_seed", "0"]
    runs = {"avi": ["--pose_path", str(tmp_path / "clip.avi"), "--ref_pose_path", str(tmp_path / "ref.jpg")], "pt": ["--pose_path", str(tmp_path / "pose.pt")]}
    for folder, extra in runs.items():
        res = subprocess.run(base + extra + ["--output_folder", str(tmp_path / folder)], capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, res.stderr[-2000:]
    avi, pt = (torch.load(tmp_path / k / "0-0.pt") for k in runs)
    assert avi.shape == (3, 16, 8, 12) and bool(torch.isfinite(avi.float()).all()) and bool(avi.float().abs().sum() > 0)
    assert torch.equal(avi, pt)
