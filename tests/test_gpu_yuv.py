"""GPU tests of the raw YUV path (csrc/yuv.hip behind `YuvDecoder` / `YuvEncoder`), all exact against the integer host
definition `yuv_reference`: every format, chroma filter, layout and type at sizes that are one pixel, odd (so that the frames
of a batch start at unaligned bytes), one whole tile, and a row and two columns beyond one; the arithmetic over every (Y, U, V)
and every (R, G, B) with each of the four constant rows; chroma samples at the corners and edges of the planes; the encoder's
input forms; `size=`, `frame_feed`, `stream(frame_encoder=...)`, and the custom ops under torch.compile.  Run with `-m gpu`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import pose_weights as pw
from self_forcing_amd import taehv_weights as tw
from self_forcing_amd import yuv_reference as yr
from test_gpu_live_session import DEV, LAT_H, LAT_W, fix_noise, make_pipe, roll  # noqa: F401  (`roll` is a fixture)

pytestmark = pytest.mark.gpu

ROWS = [("bt601", "full"), ("bt601", "limited"), ("bt709", "full"), ("bt709", "limited")]
LAYOUTS = ("hwc", "pose", "chw")
DTYPES = (torch.uint8, torch.float32, torch.bfloat16)
SIZES = [(1, 1, 1), (2, 2, 2), (3, 19, 33), (2, 16, 64), (2, 17, 66), (1, 48, 136)]
PACKED_SIZES = [(2, 2, 2), (2, 16, 64), (2, 17, 66), (1, 48, 136), (3, 19, 34)]
ENCODE_SIZES = [(3, 19, 33), (2, 16, 64), (2, 17, 66), (1, 2, 2)]


@pytest.fixture(scope="module")
def dec():
    return sfa.YuvDecoder(DEV)


def random_frames(fmt, n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, yr.frame_bytes(fmt, h, w)), dtype=np.uint8)


def reference(raw, fmt, h, w, matrix="bt601", range_="limited", chroma="triangle"):
    """uint8 [n, h, w, 3] of the definition."""
    return np.stack([yr.decode(f.tobytes(), fmt, h, w, matrix, range_, chroma) for f in raw])


def as_layout(u8, layout, dtype):
    """The definition's uint8 [n, h, w, 3] in a layout and type of the decoder, on the host."""
    x = torch.from_numpy(u8 if dtype == torch.uint8 else jr.to_float(u8))
    x = x.permute({"hwc": (0, 1, 2, 3), "pose": (3, 0, 1, 2), "chw": (0, 3, 1, 2)}[layout]).contiguous()
    return x if dtype != torch.bfloat16 else x.bfloat16()


# ------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("chroma", ["nearest", "triangle"])
@pytest.mark.parametrize("fmt", list(yr.FORMATS))
def test_decode_equals_the_definition(dec, fmt, chroma):
    for n, h, w in (PACKED_SIZES if fmt in ("yuyv", "uyvy") else SIZES):
        raw = random_frames(fmt, n, h, w, seed=h * w)
        want = reference(raw, fmt, h, w, chroma=chroma)
        dev = torch.from_numpy(raw).to(DEV)
        for layout in LAYOUTS:
            for dtype in DTYPES:
                got = dec.decode(dev, fmt, (h, w), layout, dtype, chroma=chroma)
                ref = as_layout(want, layout, dtype)
                assert got.shape == ref.shape and got.dtype == dtype and torch.equal(got.cpu(), ref), (fmt, chroma, (n, h, w), layout, dtype)
        # host bytes take the same way, whole or one by one
        assert torch.equal(dec.decode([f.tobytes() for f in raw], fmt, (h, w), chroma=chroma).cpu(), torch.from_numpy(want))
    assert torch.equal(dec.decode(raw[0].tobytes(), fmt, (h, w), chroma=chroma).cpu(), torch.from_numpy(want[:1]))


def test_decode_of_an_unaligned_view(dec):
    n, h, w = 2, 16, 64
    need = yr.frame_bytes("nv12", h, w)
    raw = random_frames("nv12", n, h, w, seed=9)
    for shift in (1, 2, 3):
        buf = torch.zeros(n * need + 8, dtype=torch.uint8, device=DEV)
        view = buf[shift:shift + n * need].view(n, need)
        view.copy_(torch.from_numpy(raw))
        assert torch.equal(dec.decode(view, "nv12", (h, w)).cpu(), torch.from_numpy(reference(raw, "nv12", h, w)))


@pytest.fixture(scope="module")
def all_triples():
    """Every triple of bytes once, as three planes [4096, 4096]: (a, b, c) = (v >> 16, (v >> 8) & 255, v & 255)."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return ((v >> 16) & 255).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v & 255).astype(np.uint8)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(r))
def test_decode_arithmetic_over_every_triple(dec, all_triples, row):
    y, u, v = all_triples
    raw = torch.from_numpy(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])[None]).to(DEV)
    got = dec.decode(raw, "i444", (4096, 4096), matrix=row[0], range=row[1])
    want = yr.yuv_to_rgb(y, u, v, yr.constants(*row))
    assert torch.equal(got[0].cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(r))
def test_encode_arithmetic_over_every_colour(all_triples, row):
    rgb = np.stack(all_triples, -1)
    enc = sfa.YuvEncoder("i444", row[0], row[1], device=DEV)
    got = enc.encode_to_device(torch.from_numpy(rgb[None]).to(DEV))
    want = yr.rgb_to_yuv(rgb, yr.constants(*row))
    assert tuple(got.shape) == (1, 3 << 24)
    assert torch.equal(got[0].cpu().view(3, 4096, 4096), torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1))))


@pytest.mark.parametrize("h,w", [(17, 33), (16, 64)])
def test_chroma_at_the_corners_and_edges(dec, h, w):
    """Chroma planes that are 0 except at the corners and the middle of each edge: a lane that reads across a plane's or a
    frame's end, or replicates the wrong neighbour, changes a pixel.  Frame 1's luma is 255, so a chroma read of frame 0
    that runs on into it shows too."""
    ch, cw = yr.chroma_size("i420", h, w)
    frames = []
    for k, (luma, mark) in enumerate([(100, 255), (255, 200)]):
        c = np.zeros((2, ch, cw), np.uint8)
        for cy in (0, ch // 2, ch - 1):
            for cx in (0, cw // 2, cw - 1):
                if (cy, cx) != (ch // 2, cw // 2):
                    c[0, cy, cx], c[1, cy, cx] = mark, mark - 50
        frames.append(np.concatenate([np.full(h * w, luma, np.uint8), c.reshape(-1)]))
    raw = np.stack(frames)
    for fmt, data in (("i420", raw), ("nv12", np.stack([np.concatenate([f[:h * w], f[h * w:].reshape(2, -1).T.reshape(-1)]) for f in frames]))):
        want = reference(data, fmt, h, w)
        assert torch.equal(dec.decode(torch.from_numpy(data).to(DEV), fmt, (h, w)).cpu(), torch.from_numpy(want))
    assert not np.array_equal(want[0], reference(raw, "i420", h, w, chroma="nearest")[0])


# ------------------------------------------------------------------------------------------ encode
def encoder_inputs(n, h, w, seed):
    """(name, device frames, value_range, the uint8 [n, h, w, 3] they stand for)"""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    yield "uint8", torch.from_numpy(u8).to(DEV), (-1, 1), u8
    for vr in ((-1, 1), (0, 1)):
        lo, hi = (-1.2, 1.2) if vr == (-1, 1) else (-0.1, 1.1)
        x = torch.from_numpy(rng.uniform(lo, hi, (n, 3, h, w)).astype(np.float32))
        yield f"float32{vr}", x.to(DEV), vr, jr.to_uint8(x.numpy(), vr)
        xb = x.bfloat16()
        yield f"bfloat16{vr}", xb.to(DEV), vr, jr.to_uint8(xb.float().numpy(), vr)


@pytest.mark.parametrize("fmt", yr.ENCODE_FORMATS)
def test_encode_equals_the_definition(dec, fmt):
    for n, h, w in ENCODE_SIZES:
        for name, frames, vr, u8 in encoder_inputs(n, h, w, seed=h + w):
            enc = sfa.YuvEncoder(fmt, "bt709", "limited", value_range=vr, device=DEV)
            want = [yr.encode(f, fmt, "bt709", "limited") for f in u8]
            got = enc.encode_to_device(frames)
            assert tuple(got.shape) == (n, yr.frame_bytes(fmt, h, w)) and got.dtype == torch.uint8
            assert [bytes(g.cpu().numpy()) for g in got] == want, (fmt, (n, h, w), name)
            assert enc.encode(frames) == want
            # the way back on the device is the definition's decode of the definition's encode: no round-trip tolerance
            back = dec.decode(got, fmt, (h, w), matrix="bt709", range="limited")
            assert torch.equal(back.cpu(), torch.from_numpy(np.stack([yr.decode(f, fmt, h, w, "bt709", "limited") for f in want])))
    five = enc.encode(frames.reshape(1, *frames.shape))            # [B, T, ...] is flattened
    assert five == want


def test_resized_decode_equals_the_resizer(dec):
    n, h, w = 2, 90, 160
    raw = torch.from_numpy(random_frames("nv12", n, h, w, seed=4)).to(DEV)
    full = dec.decode(raw, "nv12", (h, w))
    resizer = sfa.FrameResizer(DEV)
    for layout, dtype, filter, fit in (("hwc", torch.uint8, "bilinear", "stretch"), ("pose", torch.uint8, "bicubic", "cover"), ("chw", torch.float32, "bilinear", "cover")):
        got = dec.decode(raw, "nv12", (h, w), layout, dtype, size=(48, 80), filter=filter, fit=fit)
        assert torch.equal(got, resizer.resize(full, (48, 80), filter, "hwc", layout, dtype, fit=fit))


# ------------------------------------------------------------------------------------------ feeds and the pipeline
@pytest.mark.parametrize("piece", [1, 5, 12])
def test_frame_feed_pieces_concatenate_to_the_clip(dec, piece):
    h, w = 64, 96
    raw = random_frames("i420", 13, h, w, seed=2)
    whole = dec.decode(torch.from_numpy(raw).to(DEV), "i420", (h, w), "pose")
    pulled = []

    def source():
        for f in raw:
            pulled.append(1)
            yield f.tobytes()
    feed = sfa.yuv.frame_feed(source(), dec, "i420", (h, w), piece)
    assert not pulled
    first = next(feed)                                             # decoded when pulled: one piece so far
    assert first.shape == (3, min(piece, 13), h, w) and len(pulled) == min(piece, 13)
    pieces = [first] + list(feed)
    assert [p.shape[1] for p in pieces] == [piece] * (13 // piece) + ([13 % piece] if 13 % piece else [])
    assert all(p.dtype == torch.uint8 and p.is_contiguous() for p in pieces)
    assert torch.equal(torch.cat(pieces, dim=1), whole)
    hwc = list(sfa.yuv.frame_feed(iter(f.tobytes() for f in raw), dec, "i420", (h, w), piece, layout="hwc"))
    assert torch.equal(torch.cat(hwc, dim=0), whole.permute(1, 2, 3, 0))


def test_frame_feed_drives_stream_as_the_clip_does(dec, roll):  # noqa: F811
    shape = sfa.WAN_REDUCED
    h, w = 8 * LAT_H, 8 * LAT_W
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0, pose=True), timestep_shift=5.0, is_causal=True,
                                  local_attn_size=3, sink_size=1, device=DEV)
    embedder = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=DEV)
    clip = pw.synth_pose_clip(92, 21, h, w, "skeleton")             # uint8 [3, 21, H, W]
    raw = [yr.encode(np.ascontiguousarray(f), "i420", "bt601", "full") for f in clip.permute(1, 2, 3, 0).cpu().numpy()]
    frames = torch.from_numpy(np.stack([yr.decode(f, "i420", h, w, "bt601", "full") for f in raw])).permute(3, 0, 1, 2).contiguous()
    image = pw.synth_pose_image(93, h, w, "skeleton")
    pipe = make_pipe(gen, roll.pe, pose_embedder=embedder)
    fix_noise(pipe, roll.eps)
    want = torch.cat([c[1] for c in pipe.stream(roll.noise, ["p"], dwpose_data=frames, random_ref_dwpose=image)], dim=1)
    q = fix_noise(pipe, roll.eps)
    feed = sfa.yuv.frame_feed(iter(raw), dec, "i420", (h, w), 5, range="full")
    mine = torch.cat([c[1] for c in pipe.stream(roll.noise, ["p"], pose_feed=feed)], dim=1)
    torch.cuda.synchronize()
    assert not q and torch.equal(mine, want)


def test_pipeline_stream_with_a_yuv_frame_encoder(dec):
    H, W = 8, 12
    g = torch.Generator().manual_seed(41)
    noise = torch.randn(1, 4, 16, H, W, generator=g).to(torch.bfloat16).to(DEV)
    pe = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=2, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0), timestep_shift=5.0,
                                  is_causal=True, device=DEV)
    vae = sfa.TAEHVWrapper(tw.synth_taehv_state_dict(0), device=DEV)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=vae)
    enc = sfa.YuvEncoder("i420", value_range=(0, 1), device=DEV)
    chunks = list(pipe.stream(noise, ["p"], frame_encoder=enc))
    assert len(chunks) == 2
    for i, x, p, frames in chunks:
        assert len(frames) == p.shape[0] * p.shape[1]
        u8 = jr.to_uint8(p[0].float().cpu().numpy(), (0, 1))
        hh, ww = u8.shape[1:3]
        assert frames == [yr.encode(f, "i420") for f in u8]
        # the frames decode to the definition's round trip of the yielded pixels, byte for byte
        assert torch.equal(dec.decode(frames, "i420", (hh, ww)).cpu(), torch.from_numpy(np.stack([yr.decode(yr.encode(f, "i420"), "i420", hh, ww) for f in u8])))


def test_custom_ops_trace_and_equal_the_ctypes_path(dec):
    n, h, w = 2, 17, 66
    raw = torch.from_numpy(random_frames("nv12", n, h, w, seed=6)).to(DEV)
    k = list(yr.constants("bt601", "limited"))

    def block(raw):
        x = torch.ops.sf_hip.yuv_decode_frames(raw, "nv12", h, w, k, "triangle", "chw", torch.float32)
        return x, torch.ops.sf_hip.yuv_encode_frames(x * 0.5, "i420", k, False)

    eager = block(raw)
    compiled = torch.compile(block, backend="aot_eager", fullgraph=True)(raw)
    assert all(torch.equal(a, b) for a, b in zip(eager, compiled))
    assert torch.equal(eager[0], dec.decode(raw, "nv12", (h, w), "chw", torch.float32))
    assert torch.equal(eager[1], sfa.YuvEncoder("i420", device=DEV).encode_to_device(eager[0] * 0.5))
    u8 = jr.to_uint8((eager[0] * 0.5).cpu().numpy())
    assert [bytes(f.cpu().numpy()) for f in eager[1]] == [yr.encode(f, "i420") for f in u8]


def test_generate_reads_and_writes_y4m(tmp_path):
    """generate.py --pose_path clip.y4m --ref_pose_path ref.jpg writes the latents of the .pt dict that holds the same frames as
    the definition decodes them, and --video_format y4m the definition's i420 frames of the default run's video."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h, w = 64, 96
    clip = pw.synth_pose_clip(92, 9, h, w, "skeleton").permute(1, 2, 3, 0).cpu().numpy()
    raw = [yr.encode(np.ascontiguousarray(f), "i420", "bt709", "limited") for f in clip]
    with sfa.y4m.Y4mWriter(str(tmp_path / "clip.y4m"), w, h, 16) as wr:
        wr.write(raw)
    frames = np.stack([yr.decode(f, "i420", h, w, "bt709", "limited", "nearest") for f in raw])
    image = pw.synth_pose_image(93, h, w, "skeleton").numpy()
    ref_file = jr.encode(image[None], 95, "444", 21)[0]
    (tmp_path / "ref.jpg").write_bytes(ref_file)
    torch.save({"dwpose_data": torch.from_numpy(frames).permute(3, 0, 1, 2).contiguous(), "random_ref_dwpose": torch.from_numpy(jr.decode(ref_file))},
               tmp_path / "pose.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\n"
                   "independent_first_frame: false\nmodel_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n")
    (tmp_path / "p.txt").write_text("a red fox\n")
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "generate.py"), "--config_path", str(cfg), "--data_path", str(tmp_path / "p.txt"),
            "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height", "8", "--latent_width", "12", "--seed", "5",
            "--pose_random_init_seed", "0", "--taehv_random_init_seed", "0"]
    runs = {"y4m": ["--pose_path", str(tmp_path / "clip.y4m"), "--ref_pose_path", str(tmp_path / "ref.jpg"), "--pose_yuv_matrix", "bt709",
                    "--pose_yuv_chroma", "nearest", "--video_format", "y4m", "--yuv_range", "full"],
            "pt": ["--pose_path", str(tmp_path / "pose.pt")]}
    for folder, extra in runs.items():
        res = subprocess.run(base + extra + ["--output_folder", str(tmp_path / folder)], capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, res.stderr[-2000:]
    mine, pt = (torch.load(tmp_path / k / "0-0.pt") for k in runs)
    assert mine.shape == (3, 16, 8, 12) and bool(torch.isfinite(mine.float()).all()) and torch.equal(mine, pt)
    video = torch.load(tmp_path / "pt" / "0-0.video.pt").numpy()               # uint8 [T, H, W, 3] = trunc(255 x)
    r = sfa.y4m.Y4mReader(str(tmp_path / "y4m" / "0-0.y4m"))
    assert (r.width, r.height, r.fps, r.fmt, r.range) == (video.shape[2], video.shape[1], 16, "i420", "full")
    assert list(r) == [yr.encode(f, "i420", "bt601", "full") for f in video]


def test_generate_open_length_from_a_y4m_clip_to_a_y4m_video(tmp_path):
    """generate.py --open_length with a y4m clip as the live source and --video_format y4m: the 17-frame clip decides the length (5
    latent frames, 17 video frames, written chunk by chunk), and the latents are those of the .pt dict that holds the same frames."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h, w = 64, 96
    clip = pw.synth_pose_clip(92, 17, h, w, "skeleton").permute(1, 2, 3, 0).cpu().numpy()
    raw = [yr.encode(np.ascontiguousarray(f), "i420") for f in clip]
    with sfa.y4m.Y4mWriter(str(tmp_path / "clip.y4m"), w, h, 16) as wr:
        wr.write(raw)
    frames = np.stack([yr.decode(f, "i420", h, w) for f in raw])
    ref_file = jr.encode(pw.synth_pose_image(93, h, w, "skeleton").numpy()[None], 95, "444", 21)[0]
    (tmp_path / "ref.jpg").write_bytes(ref_file)
    torch.save({"dwpose_data": torch.from_numpy(frames).permute(3, 0, 1, 2).contiguous(), "random_ref_dwpose": torch.from_numpy(jr.decode(ref_file))},
               tmp_path / "pose.pt")
    (tmp_path / "prompts.txt").write_text("a red fox\n")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\nindependent_first_frame: false\n"
                   "model_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n  local_attn_size: 3\n  sink_size: 1\n")
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "generate.py"), "--config_path", str(cfg), "--data_path",
            str(tmp_path / "prompts.txt"), "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height", "8", "--latent_width", "12", "--seed", "5",
            "--vae_random_init_seed", "0", "--pose_random_init_seed", "0", "--open_length"]
    runs = {"y4m": ["--pose_path", str(tmp_path / "clip.y4m"), "--ref_pose_path", str(tmp_path / "ref.jpg"), "--video_format", "y4m"],
            "pt": ["--pose_path", str(tmp_path / "pose.pt")]}
    for folder, extra in runs.items():
        res = subprocess.run(base + extra + ["--output_folder", str(tmp_path / folder)], capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, res.stderr[-2000:]
    mine, pt = (torch.load(tmp_path / k / "0-0.pt") for k in runs)
    assert mine.shape == (5, 16, 8, 12) and torch.equal(mine, pt)
    video = torch.load(tmp_path / "pt" / "0-0.video.pt").numpy()
    r = sfa.y4m.Y4mReader(str(tmp_path / "y4m" / "0-0.y4m"))
    assert (r.width, r.height, r.fmt, r.range) == (w, h, "i420", "limited") and video.shape == (17, h, w, 3)
    assert list(r) == [yr.encode(f, "i420") for f in video]
