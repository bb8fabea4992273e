"""GPU tests of the pose renderer (csrc/pose_render.hip behind `PoseRenderer`), all exact (`torch.equal`; the arithmetic is
integer): the kernel against the host definition `pose_render_reference.render` at the sizes where each mechanism can go
wrong (one tile, one pixel into a second tile on each axis, ragged quads, several tiles), with one, two (more primitives
than lanes) and eight people (the full list), hand-placed geometry on tile and frame edges, every layout and type,
`out=`, the pieces of `pose_feed` and their way into a `PoseStream`, a second device and two streams.  Run with `-m gpu`."""
import os
import sys

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_render_reference as pr
from self_forcing_amd import pose_weights as pw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TILE_H, TILE_W = 16, 64                     # csrc/pose_render.hip: TH, TW
SIZES = [(TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (50, 70), (96, 160)]


@pytest.fixture(scope="module")
def renderer():
    return sfa.PoseRenderer(device=DEV)


def skeletons(seed, frames, people):
    """Seeded keypoints: x, y in [-0.1, 1.25] (some points negative = invalid, some beyond the right and bottom edges),
    hands and faces as clusters, scores in [0.1, 1] (about one point in five below the threshold)"""
    rng = np.random.default_rng(seed)
    k = np.zeros((frames, people, 134, 3), np.float32)
    k[..., :24, :2] = rng.uniform(-0.1, 1.25, (frames, people, 24, 2))
    for lo, hi, spread in ((24, 92, 0.12), (92, 113, 0.15), (113, 134, 0.15)):
        centre = rng.uniform(0.0, 1.0, (frames, people, 1, 2))
        k[..., lo:hi, :2] = centre + rng.uniform(-spread, spread, (frames, people, hi - lo, 2))
    k[..., 2] = rng.uniform(0.1, 1.0, (frames, people, 134))
    return k


def empty(frames=1, people=1):
    k = np.full((frames, people, 134, 3), -1, np.float32)
    k[..., 2] = 1
    return k


def same(renderer, k, size, **kw):
    got = renderer.render(k, size, layout="hwc", **kw)
    want = torch.from_numpy(pr.render(k, size, **kw))
    assert got.dtype == torch.uint8 and got.shape == want.shape and got.is_contiguous() and got.device == torch.device(DEV)
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).any(-1).sum())
    return want


# ============================================================================================== sizes, people, frames
@pytest.mark.parametrize("frames,people", [(1, 1), (3, 2), (1, 8)], ids=lambda v: str(v))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_people_and_frames_equal_the_definition(renderer, size, frames, people):
    want = same(renderer, skeletons(size[1] + people, frames, people), size)
    assert want.any(-1).float().mean() > 0.05
    if frames > 1:
        assert not torch.equal(want[0], want[2])


# ============================================================================================== geometry on the edges
def test_geometry_on_tile_and_frame_edges(renderer):
    h, w = 96, 160
    k = empty(1, 4)
    k[0, 0, 1], k[0, 0, 2], k[0, 0, 5] = (60, 14, 1), (68, 18, 1), (66, 30, 1)        # limbs across the corner of four tiles
    k[0, 0, 8], k[0, 0, 9] = (120, 10, 1), (136, 38, 1)                               # ... and across a corner further right
    k[0, 1, 1], k[0, 1, 8] = (170, 40, 1), (40, 120, 1)                               # a limb longer than the frame, both ends outside it
    k[0, 1, 2], k[0, 1, 3] = (0, 0, 1), (8191, 8191, 1)                               # ... and one to the far corner of the coordinate range
    for j, c in enumerate(((64, 16), (63, 15), (128, 32), (159, 95), (0, 95), (159, 0), (64, 95), (159, 16))):
        k[0, 2, 24 + j] = (*c, 1)                                                     # face discs on tile edges and the last row and column
        k[0, 2, 92 + j] = (c[0], (c[1] + 40) % h, 1)                                  # hand discs and edges likewise
    k[0, 3, 4], k[0, 3, 7], k[0, 3, 10] = (162, 50, 1), (80, 98, 1), (163, 99, 1)     # joints off the right and bottom edges reach in
    k[0, 3, 113:118] = [(158, 60, 1), (170, 60, 1), (170, 80, 1), (158, 94, 1), (150, 100, 1)]      # a hand that leaves the frame
    want = same(renderer, k, (h, w), normalized=False)
    assert tuple(want[0, 50, 159].tolist()) == pr.COLORS[4] and tuple(want[0, 95, 80].tolist()) == pr.COLORS[7]
    assert tuple(want[0, 95, 159].tolist()) == (255, 255, 255) and want[0, 80, 105].any()


def test_all_points_invalid_gives_zeros(renderer):
    out = torch.full((2, 50, 70, 3), 255, dtype=torch.uint8, device=DEV)
    bad = skeletons(1, 2, 2)
    bad[..., 2] = 0.29
    assert renderer.render(bad, (50, 70), layout="hwc", out=out) is out and not out.any()
    out.fill_(255)
    renderer.render(empty(2, 1)[:, 0], (50, 70), layout="hwc", out=out)                # [F, 134, 3], every point -1
    assert not out.any()
    nan = np.full((1, 1, 134, 3), np.nan, np.float32)
    assert not renderer.render(nan, (17, 65)).any()


def test_one_tile_dense_with_every_primitive_of_eight_people(renderer):
    """All 8 x 185 primitives land in the tile at (64..127, 16..31) of a 48 x 192 frame: its list is full, the others' empty."""
    rng = np.random.default_rng(8)
    k = np.ones((1, 8, 134, 3), np.float32)
    k[..., 0] = rng.integers(70, 122, (1, 8, 134))
    k[..., 1] = rng.integers(21, 27, (1, 8, 134))
    want = same(renderer, k, (48, 192), normalized=False)
    assert not want[0, :, :64].any() and not want[0, :, 128:].any() and not want[0, 32:].any() and want[0, 21:27, 70:122].all()
    X, Y, ok = pr.quantize(k, (48, 192), False)
    assert len(pr.primitives(X[0], Y[0], ok[0])) > 8 * 185 - 8 * 17                   # only limbs of length 0 are missing


# ============================================================================================== layouts and types
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("layout", ["hwc", "pose", "chw"])
def test_layouts_and_dtypes(renderer, layout, dtype):
    for size in ((50, 70), (32, 72)):                                                 # ragged quads, and rows of whole quads (vector stores)
        k = skeletons(21, 2, 2)
        got = renderer.render(k, size, layout=layout, dtype=dtype)
        want = torch.from_numpy(pr.render(k, size, layout, np.uint8 if dtype == torch.uint8 else np.float32)).to(dtype)
        assert got.dtype == dtype and got.shape == want.shape and torch.equal(got.cpu(), want), (size, layout, dtype)


def test_keypoints_from_host_and_device_and_unnormalized(renderer):
    k = skeletons(5, 2, 1)
    want = torch.from_numpy(pr.render(k, (50, 70), "pose"))
    for kk in (k, torch.from_numpy(k), torch.from_numpy(k).to(DEV), torch.from_numpy(k).double(), k[:, 0], k[:, 0].tolist()):
        assert torch.equal(renderer.render(kk, (50, 70)).cpu(), want)
    px = k * np.float32([70, 50, 1])
    assert torch.equal(renderer.render(px, (50, 70), normalized=False).cpu(), torch.from_numpy(pr.render(px, (50, 70), "pose", normalized=False)))
    assert torch.equal(renderer.render(k, (50, 70), score_threshold=0.6).cpu(), torch.from_numpy(pr.render(k, (50, 70), "pose", score_threshold=0.6)))
    assert not torch.equal(renderer.render(k, (50, 70), score_threshold=0.6).cpu(), want)


# ============================================================================================== out= and views
def test_out_into_a_slice_of_a_larger_buffer(renderer):
    k = skeletons(6, 3, 1)
    want = torch.from_numpy(pr.render(k, (48, 64)))
    buf = torch.full((5, 48, 64, 3), 7, dtype=torch.uint8, device=DEV)
    got = renderer.render(k, (48, 64), layout="hwc", out=buf[1:4])
    assert got.data_ptr() == buf[1:4].data_ptr() and torch.equal(buf[1:4].cpu(), want) and (buf[0] == 7).all() and (buf[4] == 7).all()
    fbuf = torch.full((3, 5, 48, 64), 7.0, dtype=torch.float32, device=DEV)            # the pose layout's frames 1..3 are no contiguous slice
    with pytest.raises(ValueError, match="out must be"):
        renderer.render(k, (48, 64), dtype=torch.float32, out=fbuf[:, 1:4])
    with pytest.raises(ValueError, match="out must be"):
        renderer.render(k, (48, 64), layout="hwc", out=torch.empty(3 * 48 * 64 * 3 + 1, dtype=torch.uint8, device=DEV)[1:].view(3, 48, 64, 3))
    with pytest.raises(ValueError, match="out must be"):
        renderer.render(k, (48, 64), layout="hwc", out=buf[1:3])
    assert (fbuf == 7).all()


# ============================================================================================== pieces
F_CLIP = 13
STREAM_H, STREAM_W = 9, 9           # the smallest frames the pose stack takes: one token per latent frame, 8 x 8 gives none


@pytest.mark.parametrize("per_piece", [1, 5])
def test_pose_feed_pieces_concatenate_to_the_whole_render(renderer, per_piece):
    k = skeletons(9, F_CLIP, 2)
    whole = renderer.render(k, (50, 70))
    pulled = []

    def source():
        for i in range(F_CLIP):
            pulled.append(i)
            yield k[i]
    feed = sfa.pose_render.pose_feed(source(), renderer, (50, 70), per_piece)
    first = next(feed)
    assert pulled == list(range(per_piece)) and first.shape == (3, per_piece, 50, 70) and first.dtype == torch.uint8
    pieces = [first] + list(feed)
    assert [p.shape[1] for p in pieces] == [per_piece] * (F_CLIP // per_piece) + ([F_CLIP % per_piece] if F_CLIP % per_piece else [])
    assert torch.equal(torch.cat(pieces, dim=1), whole) and torch.equal(whole.cpu(), torch.from_numpy(pr.render(k, (50, 70), "pose")))


def test_pose_feed_into_a_pose_stream_gives_the_tokens_of_the_reference_frames(renderer):
    embedder = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=DEV)
    k = skeletons(10, F_CLIP, 1)
    frames = torch.from_numpy(pr.render(k, (STREAM_H, STREAM_W), "pose"))
    assert frames.any()
    want, fhw = embedder.embed(frames.to(DEV))
    want = want.clone()
    assert fhw == pw.pose_plan(F_CLIP, STREAM_H, STREAM_W) == (4, 1, 1)
    with pytest.raises(ValueError, match="no tokens"):
        pw.pose_plan(F_CLIP, STREAM_H - 1, STREAM_W - 1)
    for per_piece in (1, 5):
        stream = embedder.open_stream(STREAM_H, STREAM_W)
        rows = [stream.push(piece)[0] for piece in sfa.pose_render.pose_feed(k, renderer, (STREAM_H, STREAM_W), per_piece)]
        rows.append(stream.close()[0])
        assert torch.equal(torch.cat(rows, dim=1), want), per_piece


def test_generate_reads_and_renders_keypoint_files(tmp_path):
    sys.path.insert(0, ROOT)
    import generate
    k = skeletons(12, 5, 2)
    np.savez(tmp_path / "clip.npz", keypoints=k)
    np.save(tmp_path / "ref.npy", k[0, 0])
    clip, ref = generate.load_pose_keypoints(str(tmp_path / "clip.npz"), str(tmp_path / "ref.npy"), torch.device(DEV), (64, 96))
    assert torch.equal(clip.cpu(), torch.from_numpy(pr.render(k, (64, 96), "pose")))
    assert ref.shape == (64, 96, 3) and torch.equal(ref.cpu(), torch.from_numpy(pr.render(k[:1, :1], (64, 96))[0]))


# ============================================================================================== devices and streams
def test_second_device(renderer):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    k = skeletons(13, 2, 2)
    want = torch.from_numpy(pr.render(k, (50, 70), "pose"))
    other = sfa.PoseRenderer(device="cuda:1").render(k, (50, 70))
    assert other.device == torch.device("cuda:1") and torch.equal(other.cpu(), want)
    moved = renderer.render(torch.from_numpy(k).to("cuda:1"), (50, 70))                # device keypoints are rendered where they are
    assert moved.device == torch.device("cuda:1") and torch.equal(moved.cpu(), want)
    assert torch.equal(renderer.render(k, (50, 70)).cpu(), want)


def test_two_streams_give_the_same_bits(renderer):
    k = torch.from_numpy(skeletons(14, 3, 8)).to(DEV)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            outs.append(renderer.render(k, (96, 160)))
            outs.append(renderer.render(k, (96, 160), dtype=torch.bfloat16))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]) and outs[0].any()
    assert torch.equal(outs[0].cpu(), torch.from_numpy(pr.render(k.cpu().numpy(), (96, 160), "pose")))
