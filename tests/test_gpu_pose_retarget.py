"""GPU tests of the pose retargeter (csrc/pose_retarget.hip behind `PoseRetargeter`), all exact: the kernel against the host
definition `pose_retarget_reference` on the float32 BITS, markers included, at every frame count, people count, reference
broadcast, frame rate, input unit, source size and align setting; the missing-point rules (neck, wrist, nose, a whole hand,
gaps in frame 0 only) and scores at and just below the threshold; the stream over partitions of a clip, from device and host
pieces; the way into the renderer and through `pose_feed`; and the current stream.  Run with `-m gpu`.  The shapes are the
smallest at which the kernel can go wrong: one workgroup per (frame, person) handles all 134 points, so what varies is the
grid (1, 2, 7 frames x 1, 2, 8 people), the frame pair a workgroup reads (rem == 0 or not, the window's offset in a stream)
and the branches a person takes."""
import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_render_reference as pr
from self_forcing_amd import pose_retarget_reference as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (96, 160)
SOURCE_SIZE = (72, 128)
F32 = np.float32
MARKER = np.array([-1, -1, 0], F32)


@pytest.fixture(scope="module")
def retargeter():
    return sfa.PoseRetargeter(device=DEV)


def people(seed, frames, count):
    """Seeded normalised keypoints [frames, count, 134, 3]: a body of limbs 0.05..0.2 long around a neck near the centre
    that drifts from frame to frame, attached points near their anchors; about 3 % of the coordinates negative and 7 % of
    the scores below 0.3 (invalid points), so some people lose their neck in frame 0 and are not retargeted"""
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
            k[f, q, :, :2] = xy + f * rng.uniform(-0.02, 0.02, 2) + rng.uniform(-0.015, 0.015, (134, 2))
    k[..., :2] = np.where(rng.random(k[..., :2].shape) < 0.015, -k[..., :2], k[..., :2])
    k[..., 2] = rng.uniform(0.25, 1.0, k.shape[:3])
    return k


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def same(retargeter, k, ref, size=SIZE, **kw):
    got = retargeter.retarget(k, ref, size, **kw)
    want = rr.retarget(k, ref, size, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous() and got.device == torch.device(DEV)
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (int((bits(got) != bits(want)).sum()), kw)
    return want


# ============================================================================================== kernel against reference
@pytest.mark.parametrize("count", [1, 2, 8])
@pytest.mark.parametrize("frames", [1, 2, 7])
def test_every_setting_equals_the_definition(retargeter, frames, count):
    k = people(10 * frames + count, frames, count)
    ref = people(100 + count, 1, count)[0]
    k[0, 0, 1], ref[0, 1] = (abs(k[0, 0, 1, 0]), abs(k[0, 0, 1, 1]), 0.9), (abs(ref[0, 1, 0]), abs(ref[0, 1, 1]), 0.9)     # person 0 keeps its anchor
    retargeted = settings = 0
    for ref_people in sorted({1, count}):
        for source in (16, 30, 24, 15):
            for normalized in (True, False):
                unit = F32([1, 1, 1]) if normalized else F32([SIZE[1], SIZE[0], 1])
                for source_size in (None, SOURCE_SIZE):
                    src_unit = unit if normalized or source_size is None else F32([source_size[1], source_size[0], 1])
                    for align in (True, False):
                        kw = dict(source_fps=source, normalized=normalized, source_size=source_size)
                        want = same(retargeter, k * src_unit, ref[:ref_people] * unit, align=align, **kw)
                        assert want.shape[0] == rr.frames_out(frames, *rr.rate(source, 16))
                        if align:
                            settings += 1
                            retargeted += not np.array_equal(want, rr.retarget(k * src_unit, ref[:ref_people] * unit, SIZE, align=False, **kw))
    assert retargeted == settings == 16 * len({1, count})       # align does something wherever someone has an anchor


def test_missing_points(retargeter):
    """Eight people, each with one kind of gap, in one launch: the rules of the definition's `resample`, `fit` and `retarget_frame`"""
    k = people(3, 7, 8)
    k[..., 2] = np.maximum(k[..., 2], 0.5)
    k[..., :2] = np.abs(k[..., :2])                                                      # everything valid, then:
    ref = k[3, ::-1].copy()
    gone = (-1, -1, 0)
    k[0, 0, 1] = gone                       # person 0: no neck in frame 0 -> lifted and resampled only
    k[3, 1, 1] = gone                       # person 1: no neck in a later frame -> its children fall back to sim
    k[2:5, 2, 4] = gone                     # person 2: a wrist -> the right hand falls back to sim
    k[1:, 3, 0] = gone                      # person 3: the nose -> eyes and face fall back to sim
    k[:, 4, 92:113] = gone                  # person 4: a whole hand, all clip long
    k[0, 5, 3] = k[0, 5, 6] = gone          # person 5: both elbows in frame 0 only -> groups {2, 4}, {3, 5} take g
    k[0, 6, 3, :2] = k[0, 6, 2, :2]         # person 6: a limb of length 0 in frame 0 -> its group has one usable member
    ref[7, 1] = gone                        # person 7: no neck in the reference
    ref[2, 12] = gone                       # ... and a gap in person 2's reference
    for source in (16, 30, 24, 15):
        out = same(retargeter, k, ref, source_fps=source)
        plain = rr.retarget(k, ref, SIZE, source_fps=source, align=False)
        assert np.array_equal(out[:, 0], plain[:, 0]) and np.array_equal(out[:, 7], plain[:, 7])
        assert all(not np.array_equal(out[:, q], plain[:, q]) for q in range(1, 7))
        assert (out[:, 4, 92:113] == MARKER).all() and (out[0, 5, 3] == MARKER).all() and (out[-1, 5, 3] != MARKER).any()
    same(retargeter, k, ref[0], source_fps=30)
    same(retargeter, k, ref[7], source_fps=30)                                           # nobody has an anchor


def test_scores_at_the_threshold_and_just_below(retargeter):
    for threshold in (0.3, 0.5, 0.0):
        k = np.abs(people(4, 3, 2))
        k[..., 2] = 0.9
        t = F32(threshold)
        below = np.nextafter(t, F32(-1))
        k[0, 0, 5, 2], k[0, 0, 6, 2], k[1, 0, 7, 2], k[1, 0, 8, 2], k[2, 1, 1, 2], k[0, 1, 2, 2] = t, below, t, below, below, t
        ref = people(5, 1, 1)[0]
        ref[..., 2] = 0.9
        ref[0, 9, 2], ref[0, 10, 2] = t, below
        for source in (16, 24):
            out = same(retargeter, k, ref, source_fps=source, score_threshold=threshold)
            assert (out[0, 0, 6] == MARKER).all() and out[0, 0, 5, 2] == t
    odd = people(6, 2, 1)
    odd[..., 2] = 0.9
    odd[0, 0, 20], odd[0, 0, 21], odd[1, 0, 22], odd[1, 0, 23, 0] = (np.nan, 0.5, 1), (0.5, np.inf, 1), (0.5, 0.5, np.nan), -0.0
    out = same(retargeter, odd, odd[0], source_fps=16)
    assert (out[0, 0, 20:22] == MARKER).all() and (out[1, 0, 22] == MARKER).all() and (out[1, 0, 23] != MARKER).any()


def test_input_kinds_and_a_long_clip(retargeter):
    k, ref = people(7, 5, 2), people(8, 1, 1)[0, 0]
    want = torch.from_numpy(rr.retarget(k, ref, SIZE, source_fps=24))
    for kk, rf in ((k, ref), (torch.from_numpy(k), torch.from_numpy(ref)), (torch.from_numpy(k).to(DEV), ref), (k, torch.from_numpy(ref).to(DEV)),
                   (torch.from_numpy(k).double(), ref.tolist())):
        assert torch.equal(retargeter.retarget(kk, rf, SIZE, source_fps=24).cpu(), want)
    one = people(9, 4, 1)
    assert torch.equal(retargeter.retarget(one[:, 0], ref, SIZE).cpu(), torch.from_numpy(rr.retarget(one, ref, SIZE)))
    # 151 frames at 30 frames/s give 81: more workgroups than the card runs at once, and frame indices past the first piece
    long = people(10, 1, 1).repeat(151, 0) + np.linspace(0, 0.2, 151, dtype=F32)[:, None, None, None] * F32([1, 0.5, 0])
    assert same(retargeter, long, ref, source_fps=30).shape[0] == 81
    same(retargeter, long, ref, source_fps="30000/1001")


# ============================================================================================== stream and pipeline
@pytest.mark.parametrize("source", [16, 30, 24])
def test_stream_partitions_equal_the_one_shot_call(retargeter, source):
    n = 7
    k, ref = people(11, n, 2), people(12, 1, 2)[0]
    k[0, 1, 1, 2] = 0.9
    whole = retargeter.retarget(k, ref, SIZE, source_fps=source)
    assert torch.equal(whole.cpu(), torch.from_numpy(rr.retarget(k, ref, SIZE, source_fps=source)))
    dev = torch.from_numpy(k).to(DEV)
    for parts in ([1] * n, [5, 2], [3, 4], [n]):
        for pieces in (k, dev, torch.from_numpy(k)):
            stream = retargeter.open_stream(ref, SIZE, source_fps=source)
            got, at = [], 0
            for m in parts:
                got.append(stream.push(pieces[at:at + m]))
                assert got[-1].shape == (rr.plan(at, m, *rr.rate(source, 16))[1], 2, 134, 3) and got[-1].device == torch.device(DEV)
                assert got[-1].dtype == torch.float32
                at += m
            assert stream.close() is None and (stream.frames_in, stream.frames_out) == (n, whole.shape[0])
            assert torch.equal(torch.cat(got), whole), (parts, type(pieces))
            if source == 30 and parts == [1] * n:
                assert [g.shape[0] for g in got] == [1, 0, 1, 0, 1, 0, 1]                 # pushes that make no frame final return none
    stream = retargeter.open_stream(ref, SIZE, source_fps=source)
    first = dev[:3].clone()
    out = stream.push(first)
    first.zero_()                                                                        # the stream keeps its own frame 0 and last frame
    rest = stream.push(dev[3:])
    assert torch.equal(torch.cat([out, rest]), whole)


def test_retargeted_keypoints_render_as_the_definitions_say(retargeter):
    renderer = sfa.PoseRenderer(device=DEV)
    k, ref = people(13, 7, 2), people(14, 1, 1)[0]
    k[0, :, 1, 2] = ref[0, 1, 2] = 0.9
    k[..., :2], ref[..., :2] = np.abs(k[..., :2]), np.abs(ref[..., :2])
    moved = retargeter.retarget(k, ref, SIZE, source_fps=24)
    frames = renderer.render(moved, SIZE, layout="hwc", normalized=False)
    want = pr.render(rr.retarget(k, ref, SIZE, source_fps=24), SIZE, normalized=False)
    assert torch.equal(frames.cpu(), torch.from_numpy(want)) and want.any(-1).mean() > 0.02
    assert not np.array_equal(want, pr.render(rr.retarget(k, ref, SIZE, source_fps=24, align=False), SIZE, normalized=False))


@pytest.mark.parametrize("per_piece", [1, 3])
def test_pose_feed_through_a_retargeter_yields_the_pieces_of_the_one_shot_result(retargeter, per_piece):
    renderer = sfa.PoseRenderer(device=DEV)
    n = 10
    k, ref = people(15, n, 1), people(16, 1, 1)[0]
    whole = renderer.render(retargeter.retarget(k, ref, SIZE, source_fps=30), SIZE, normalized=False)
    assert whole.shape == (3, 5, *SIZE)
    pulled = []

    def source():
        for i in range(n):
            pulled.append(i)
            yield k[i]

    def host_source():
        return (k[i] for i in range(n))
    feed = sfa.pose_render.pose_feed(source(), renderer, SIZE, per_piece, retargeter=retargeter.open_stream(ref, SIZE, source_fps=30))
    first = next(feed)
    assert pulled == list(range(1 if per_piece == 1 else 5))                             # frame 0 is final at once; three frames need 0..4
    pieces = [first] + list(feed)
    assert [p.shape[1] for p in pieces] == [per_piece] * (5 // per_piece) + ([5 % per_piece] if 5 % per_piece else [])
    assert all(p.dtype == torch.uint8 and p.shape[0] == 3 for p in pieces) and torch.equal(torch.cat(pieces, dim=1), whole)
    dev = [torch.from_numpy(k[i]).to(DEV) for i in range(n)]
    again = list(sfa.pose_render.pose_feed(dev, renderer, SIZE, per_piece, retargeter=retargeter.open_stream(ref, SIZE, source_fps=30)))
    assert torch.equal(torch.cat(again, dim=1), whole)
    # without a retargeter: what it gave before, the frames of the keypoints as they are
    plain = list(sfa.pose_render.pose_feed(host_source(), renderer, SIZE, per_piece))
    assert torch.equal(torch.cat(plain, dim=1), renderer.render(k, SIZE)) and [p.shape[1] for p in plain][0] == per_piece
    assert torch.equal(torch.cat(plain, dim=1).cpu(), torch.from_numpy(pr.render(k, SIZE, "pose")))


def test_generate_retargets_keypoint_files(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import generate
    k, ref = people(17, 7, 2), people(18, 1, 2)[0]
    np.savez(tmp_path / "clip.npz", keypoints=k)
    np.save(tmp_path / "ref.npy", ref)
    paths = (str(tmp_path / "clip.npz"), str(tmp_path / "ref.npy"), torch.device(DEV), SIZE)
    ref_frame = torch.from_numpy(pr.render(ref[None], SIZE)[0])
    clip, drawn = generate.load_pose_keypoints(*paths)                                   # the defaults: as before
    assert torch.equal(clip.cpu(), torch.from_numpy(pr.render(k, SIZE, "pose"))) and torch.equal(drawn.cpu(), ref_frame)
    for kw in (dict(align=True), dict(source_fps="24"), dict(align=True, source_fps="30", source_size=SOURCE_SIZE)):
        clip, drawn = generate.load_pose_keypoints(*paths, **kw)
        moved = rr.retarget(k, ref, SIZE, source_fps=kw.get("source_fps", 16), align=kw.get("align", False), source_size=kw.get("source_size"))
        assert torch.equal(clip.cpu(), torch.from_numpy(pr.render(moved, SIZE, "pose", normalized=False))), kw
        assert torch.equal(drawn.cpu(), ref_frame)                                       # the reference pose is drawn as it is


def test_the_current_stream_and_the_tensors_device(retargeter):
    k, ref = torch.from_numpy(people(19, 7, 8)).to(DEV), torch.from_numpy(people(20, 1, 8)[0]).to(DEV)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            outs.append(retargeter.retarget(k, ref, SIZE, source_fps=24))
            stream = retargeter.open_stream(ref, SIZE, source_fps=24)
            outs.append(torch.cat([stream.push(k[:3]), stream.push(k[3:])]))
    torch.cuda.synchronize()
    want = torch.from_numpy(rr.retarget(k.cpu().numpy(), ref.cpu().numpy(), SIZE, source_fps=24))
    for o in outs:
        assert o.device == k.device and torch.equal(o.cpu(), want)
