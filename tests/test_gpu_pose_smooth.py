"""GPU tests of the pose smoother (csrc/pose_smooth.hip behind `PoseSmoother`), all exact: the kernel against the host
definition `pose_smooth_reference` on the float32 BITS of the output, markers included, and on the bits of the packed state
it leaves on the device; the edge samples (NaN, inf, a re-seed near FLT_MAX, subnormals, scores at and just below the
threshold); the stream over partitions of a clip, from device and host pieces; the way into the retargeter and the renderer,
through `pose_feed` and through `generate.load_pose_keypoints`; and the current stream.  Run with `-m gpu`.  The shapes are
the smallest at which the kernel can go wrong: a lane is a (person, point), so what varies is the lane count and its ragged
last wave (1, 2, 8 people: 134, 268, 1072 lanes), the loop's trip count and its prefetch edge (1, 2, 7 frames) and the state
a launch starts from (the partitions); one clip of 151 frames gives a long chain."""
import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_render_reference as pr
from self_forcing_amd import pose_retarget_reference as rr
from self_forcing_amd import pose_smooth_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (96, 160)
F32 = np.float32
MARKER = np.array([-1, -1, 0], F32)


@pytest.fixture(scope="module")
def smoother():
    return sfa.PoseSmoother(device=DEV)


def clip(seed, frames, people, pixels=False):
    """Seeded keypoints [frames, people, 134, 3]: every point walks from a start in [0.1, 0.9]^2 with steps of up to 0.02 and
    jitter of 0.004; about 4 % of the points have a negative coordinate, 6 % of the scores are below 0.3 and 4 % of the
    samples start a run of up to three missing ones, so 10 to 20 % of the samples are invalid, alone and in runs"""
    rng = np.random.default_rng(seed)
    k = np.empty((frames, people, 134, 3), F32)
    start, drift = rng.uniform(0.1, 0.9, (people, 134, 2)), rng.uniform(-0.02, 0.02, (people, 134, 2))
    k[..., :2] = start + np.arange(frames)[:, None, None, None] * drift + rng.uniform(-0.004, 0.004, (frames, people, 134, 2))
    k[..., :2] = np.where(rng.random(k[..., :2].shape) < 0.02, -k[..., :2], np.abs(k[..., :2]))
    k[..., 2] = rng.uniform(0.255, 1.0, k.shape[:3])
    gone = rng.random(k.shape[:3]) < 0.04
    gone[1:] |= gone[:-1] & (rng.random(gone[1:].shape) < 0.5)
    gone[1:] |= gone[:-1] & (rng.random(gone[1:].shape) < 0.3)
    k[gone] = MARKER
    if pixels:
        k[..., :2] *= F32([SIZE[1], SIZE[0]])
    return k


def people(seed, frames, count):
    """Seeded normalised skeletons [frames, count, 134, 3], every point valid: a body of limbs 0.05..0.2 long around a neck
    near the centre that drifts from frame to frame, attached points near their anchors, jitter of 0.015"""
    rng = np.random.default_rng(seed)
    k = np.zeros((frames, count, 134, 3), F32)
    for q in range(count):
        xy = np.zeros((134, 2))
        xy[1] = rng.uniform(0.35, 0.65, 2)
        for a, b in pr.LIMBS:
            angle, length = rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 0.2)
            xy[b] = xy[a] + length * np.array([np.cos(angle), np.sin(angle)])
        for lo, hi, anchor, _ in rr.ATTACHED:
            xy[lo:hi] = xy[anchor] + rng.uniform(-0.08, 0.08, (hi - lo, 2))
        for f in range(frames):
            k[f, q, :, :2] = np.abs(xy + f * rng.uniform(-0.02, 0.02, 2) + rng.uniform(-0.015, 0.015, (134, 2)))
    k[..., 2] = rng.uniform(0.5, 1.0, k.shape[:3])
    return k


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def same(smoother, k, fps, counts=None, **kw):
    """`smooth` and a one-push stream against the definition: the output's bits and the bits of the state left on the device"""
    src = sr.as_source(k)
    state = sr.fresh_state(src.shape[1])
    want = sr.frames(src, state, sr.prepare(fps, **kw), counts)
    got = smoother.smooth(k, fps, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous() and got.device == torch.device(DEV)
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (int((bits(got) != bits(want)).sum()), fps, kw)
    stream = smoother.open_stream(fps, **kw)
    assert stream.state is None
    again = stream.push(k)
    assert stream.state.dtype == torch.int32 and tuple(stream.state.shape) == state.shape and stream.state.device == torch.device(DEV)
    assert np.array_equal(bits(again.cpu().numpy()), bits(want)) and stream.frames_in == len(src)
    assert np.array_equal(stream.state.cpu().numpy(), state), (int((stream.state.cpu().numpy() != state).sum()), fps, kw)
    return want


# ============================================================================================== kernel against reference
@pytest.mark.parametrize("count", [1, 2, 8])
def test_every_setting_equals_the_definition(smoother, count):
    counts = {}
    for frames in (1, 2, 7):
        for pixels in (False, True):
            k = clip(10 * frames + count, frames, count, pixels)
            if frames > 1:
                k[0, count - 1, 133], k[1, count - 1, 133] = (0.5, 0.5, 0.9), (3e38, 0.5, 0.9)      # valid, then huge: the filtered step overflows
            invalid = 1 - ((k[..., 2] >= F32(0.3)) & (k[..., 0] >= 0) & (k[..., 1] >= 0)).mean()
            assert frames * count < 10 or 0.05 < invalid < 0.25
            for fps in (16, 30, "30000/1001"):
                for beta in (0.0, 0.7):
                    for max_gap in (0, 1, 3):
                        fired = {}
                        same(smoother, k, fps, fired, beta=beta, max_gap=max_gap)
                        assert max_gap > 0 or fired["hold"] == 0
                        for name, hits in fired.items():
                            counts[name] = counts.get(name, 0) + hits
    # every rule of the definition fired for this number of people: no pass without filtered steps, seeds, holds and drops
    assert all(counts[name] > 0 for name in sr.RULES), counts
    assert counts["filter"] > 1000 * count and counts["hold"] > 50 * count and counts["reseed"] >= 72


def edge_clip(threshold=F32(0.3)):
    """[8, 1, 134, 3]: every point valid at (0.5 + j / 1000, 0.25, 0.9) but for the edge cases, one per point"""
    k = np.empty((8, 1, 134, 3), F32)
    k[..., 0], k[..., 1], k[..., 2] = 0.5 + np.arange(134, dtype=F32) / 1000, 0.25, 0.9
    below = np.nextafter(threshold, F32(-1))
    k[2, 0, 0, 2], k[2, 0, 1, 2] = threshold, below                                      # at the threshold; one ulp below
    k[3, 0, 2, 0], k[3, 0, 3, 1], k[3, 0, 4, 2] = -0.0, -0.0, -0.0                       # -0.0 >= 0: valid coordinates; a score of -0.0 is low
    for j, bad in zip((5, 8, 11), (np.nan, np.inf, -np.inf)):
        for c in range(3):
            k[4, 0, j + c, c] = bad
    k[1:3, 0, 14, 0], k[3:, 0, 14, 0] = 3e38, 0                                          # e = -3e38, dx overflows: re-seed
    k[1:3, 0, 15, 1], k[3:, 0, 15, 1] = 3e38, 0
    k[:, 0, 16, :2], k[:, 0, 17, :2] = 1e-42, 1e-45                                      # subnormal, constant
    k[:, 0, 18, 0] = np.array([1e-42, 3e-42, 1e-45, 0, 2e-40, 1e-38, 1e-42, 1e-45], F32)  # subnormal, moving
    k[5, 0, 19] = (3e38, 3e38, 3e38)                                                     # huge, finite: valid
    return k


def test_edge_samples_in_one_launch(smoother):
    for threshold in (0.3, 0.5, 0.0):
        k = edge_clip(F32(threshold))
        for kw in (dict(), dict(beta=0.7, max_gap=1)):
            fired = {}
            out = same(smoother, k, 30, fired, score_threshold=threshold, **kw)[:, 0]
            assert out[2, 0, 2] == F32(threshold) and ((out[2, 1] == MARKER).all() != bool(kw))
            assert fired["reseed"] >= 2 and out[3, 14, 0] == 0 and out[1, 14, 0] == F32(3e38)
            assert np.array_equal(bits(out[:, 16]), bits(k[:, 0, 16])) and np.array_equal(bits(out[:, 17]), bits(k[:, 0, 17]))      # subnormals are kept
            assert (out[1:, 18, 0] > 0).all() and np.isfinite(out).all()
    same(smoother, edge_clip(), "30000/1001", beta=0.7, max_gap=3, min_cutoff=0.2, d_cutoff=3.0)


def test_input_kinds_and_a_long_clip(smoother):
    k = clip(7, 5, 2)
    want = torch.from_numpy(sr.smooth(k, 24, beta=0.3, max_gap=1))
    for kk in (k, torch.from_numpy(k), torch.from_numpy(k).to(DEV), torch.from_numpy(k).double(), k.tolist()):
        assert torch.equal(smoother.smooth(kk, 24, beta=0.3, max_gap=1).cpu(), want)
    one = clip(9, 4, 1)
    assert torch.equal(smoother.smooth(one[:, 0], 16).cpu(), torch.from_numpy(sr.smooth(one, 16)))              # [F, 134, 3] is one person
    # 151 frames of one person, the bench tool's clip: a long chain per lane
    long = people(10, 1, 1).repeat(151, 0) + np.linspace(0, 0.2, 151, dtype=F32)[:, None, None, None] * F32([1, 0.5, 0])
    rng = np.random.default_rng(10)
    long[..., :2] += rng.uniform(-0.004, 0.004, long[..., :2].shape).astype(F32)
    long[rng.random(long.shape[:3]) < 0.05] = MARKER
    fired = {}
    same(smoother, long, 30, fired, beta=0.7, max_gap=2)
    assert fired["filter"] > 15000 and fired["hold"] > 500 and fired["drop"] > 0
    same(smoother, long, "30000/1001")


# ============================================================================================== stream and pipeline
@pytest.mark.parametrize("kw", [dict(), dict(beta=0.7, max_gap=2)], ids=["defaults", "beta-hold"])
def test_stream_partitions_equal_the_one_shot_call(smoother, kw):
    n = 7
    k = clip(11, n, 2)
    state = sr.fresh_state(2)
    want = sr.frames(k, state, sr.prepare(30, **kw))
    whole = smoother.smooth(k, 30, **kw)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want))
    dev = torch.from_numpy(k).to(DEV)
    for parts in ([1] * n, [5, 2], [3, 4], [n]):
        for pieces in (k, dev, torch.from_numpy(k)):
            stream = smoother.open_stream(30, **kw)
            got, at = [], 0
            for m in parts:
                got.append(stream.push(pieces[at:at + m]))
                assert got[-1].shape == (m, 2, 134, 3) and got[-1].device == torch.device(DEV) and got[-1].dtype == torch.float32
                at += m
                assert stream.frames_in == at
            assert stream.close() is None
            assert torch.equal(torch.cat(got), whole), (parts, type(pieces))
            assert np.array_equal(stream.state.cpu().numpy(), state), (parts, type(pieces))
            with pytest.raises(ValueError, match="closed"):
                stream.push(pieces[:1])
    stream = smoother.open_stream(30, **kw)
    first = dev[:3].clone()
    out = stream.push(first)
    first.zero_()                                                                        # the stream keeps nothing of the caller's
    rest = stream.push(dev[3:])
    assert torch.equal(torch.cat([out, rest]), whole)
    with pytest.raises(ValueError, match="holds 2 people, the piece 1"):
        stream.push(dev[:1, :1])


def dropped_elbow(seed, frames=7):
    """Two valid people and a reference; person 0's right elbow is missing in source frames 3 and 4"""
    k, ref = people(seed, frames, 2), people(seed + 1, 1, 1)[0]
    k[3:5, 0, 3] = MARKER
    return k, ref


def test_smoothed_keypoints_retarget_and_render_as_the_definitions_say(smoother):
    retargeter, renderer = sfa.PoseRetargeter(device=DEV), sfa.PoseRenderer(device=DEV)
    k, ref = dropped_elbow(13)
    kw = dict(min_cutoff=1.0, beta=0.7, max_gap=2)
    frames = renderer.render(retargeter.retarget(smoother.smooth(k, 30, **kw), ref, SIZE, source_fps=30), SIZE, layout="hwc", normalized=False)
    moved = rr.retarget(sr.smooth(k, 30, **kw), ref, SIZE, source_fps=30)
    want = pr.render(moved, SIZE, normalized=False)
    assert torch.equal(frames.cpu(), torch.from_numpy(want)) and want.any(-1).mean() > 0.02
    # output frame 2 sits at source position 3.75: without the smoother the elbow and its two limbs are gone there
    plain = rr.retarget(k, ref, SIZE, source_fps=30)
    assert (plain[2, 0, 3] == MARKER).all() and (moved[2, 0, 3] != MARKER).any()
    unsmoothed = renderer.render(retargeter.retarget(k, ref, SIZE, source_fps=30), SIZE, layout="hwc", normalized=False)
    assert torch.equal(unsmoothed.cpu(), torch.from_numpy(pr.render(plain, SIZE, normalized=False)))
    assert not torch.equal(frames[2], unsmoothed[2])
    assert not np.array_equal(want, pr.render(rr.retarget(sr.smooth(k, 30, min_cutoff=1.0, beta=0.7), ref, SIZE, source_fps=30), SIZE, normalized=False))


@pytest.mark.parametrize("per_piece", [1, 3])
def test_pose_feed_through_a_smoother_yields_the_pieces_of_the_one_shot_result(smoother, per_piece):
    retargeter, renderer = sfa.PoseRetargeter(device=DEV), sfa.PoseRenderer(device=DEV)
    n = 10
    k, ref = dropped_elbow(15, n)
    kw = dict(beta=0.7, max_gap=2)
    smoothed = smoother.smooth(k, 30, **kw)
    # smoother and retargeter: pieces of OUTPUT frames
    whole = renderer.render(retargeter.retarget(smoothed, ref, SIZE, source_fps=30), SIZE, normalized=False)
    assert whole.shape == (3, 5, *SIZE)
    for source in ([k[i] for i in range(n)], [torch.from_numpy(k[i]).to(DEV) for i in range(n)]):
        feed = sfa.pose_render.pose_feed(iter(source), renderer, SIZE, per_piece, retargeter=retargeter.open_stream(ref, SIZE, source_fps=30),
                                         smoother=smoother.open_stream(30, **kw))
        pieces = list(feed)
        assert [p.shape[1] for p in pieces] == [per_piece] * (5 // per_piece) + ([5 % per_piece] if 5 % per_piece else [])
        assert all(p.dtype == torch.uint8 and p.shape[0] == 3 for p in pieces) and torch.equal(torch.cat(pieces, dim=1), whole)
    # the smoother alone: pieces of source frames, drawn with the feed's `normalized`
    alone = renderer.render(smoothed, SIZE)
    assert not torch.equal(alone, renderer.render(k, SIZE))
    pieces = list(sfa.pose_render.pose_feed(iter(k), renderer, SIZE, per_piece, smoother=smoother.open_stream(30, **kw)))
    assert [p.shape[1] for p in pieces] == [per_piece] * (n // per_piece) + ([n % per_piece] if n % per_piece else [])
    assert torch.equal(torch.cat(pieces, dim=1), alone)
    pixels = k * F32([SIZE[1], SIZE[0], 1])
    pieces = list(sfa.pose_render.pose_feed(iter(pixels), renderer, SIZE, per_piece, normalized=False, smoother=smoother.open_stream(30, **kw)))
    assert torch.equal(torch.cat(pieces, dim=1).cpu(), torch.from_numpy(pr.render(sr.smooth(pixels, 30, **kw), SIZE, "pose", normalized=False)))
    # without a smoother: what the feed gave before, the frames of the keypoints as they are
    plain = list(sfa.pose_render.pose_feed(iter(k), renderer, SIZE, per_piece, smoother=None))
    assert torch.equal(torch.cat(plain, dim=1), renderer.render(k, SIZE)) and plain[0].shape[1] == per_piece
    assert torch.equal(torch.cat(plain, dim=1).cpu(), torch.from_numpy(pr.render(k, SIZE, "pose")))


def test_generate_smooths_keypoint_files(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import generate
    k, ref = dropped_elbow(17)
    ref = np.concatenate([ref, people(19, 1, 1)[0]])
    np.savez(tmp_path / "clip.npz", keypoints=k)
    np.save(tmp_path / "ref.npy", ref)
    paths = (str(tmp_path / "clip.npz"), str(tmp_path / "ref.npy"), torch.device(DEV), SIZE)
    ref_frame = torch.from_numpy(pr.render(ref[None], SIZE)[0])
    clip_frames, drawn = generate.load_pose_keypoints(*paths)                            # the defaults: as before
    assert torch.equal(clip_frames.cpu(), torch.from_numpy(pr.render(k, SIZE, "pose"))) and torch.equal(drawn.cpu(), ref_frame)
    clip_frames, drawn = generate.load_pose_keypoints(*paths, smooth=(1.0, 0.7), hold=2, source_fps="30", align=True)
    moved = rr.retarget(sr.smooth(k, "30", 1.0, 0.7, max_gap=2), ref, SIZE, source_fps="30", align=True)
    assert torch.equal(clip_frames.cpu(), torch.from_numpy(pr.render(moved, SIZE, "pose", normalized=False)))
    assert torch.equal(drawn.cpu(), ref_frame)                                           # the reference pose is never smoothed
    clip_frames, _ = generate.load_pose_keypoints(*paths, hold=2)                        # a hold alone: the filter at its defaults, at 16 frames/s, no retargeter
    assert torch.equal(clip_frames.cpu(), torch.from_numpy(pr.render(sr.smooth(k, 16, max_gap=2), SIZE, "pose")))


def test_the_current_stream_and_the_tensors_device(smoother):
    k = torch.from_numpy(clip(19, 7, 8)).to(DEV)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            outs.append(smoother.smooth(k, 24, beta=0.7, max_gap=2))
            stream = smoother.open_stream(24, beta=0.7, max_gap=2)
            outs.append(torch.cat([stream.push(k[:3]), stream.push(k[3:])]))
    torch.cuda.synchronize()
    want = torch.from_numpy(sr.smooth(k.cpu().numpy(), 24, beta=0.7, max_gap=2))
    for o in outs:
        assert o.device == k.device and torch.equal(o.cpu(), want)
