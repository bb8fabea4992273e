"""GPU tests of the pose tracker (csrc/pose_track.hip behind `PoseTracker`), all exact: the kernels against the host
definition `pose_track_reference` on the float32 BITS of the output, markers included, on the ids and on the bits of the
packed state left on the device; the edge values; ties; the stream over partitions of a clip, from numpy, host and device
pieces; the way into the smoother, the retargeter and the renderer, through `pose_feed` and through
`generate.load_pose_keypoints`; and the current stream.  Run with `-m gpu`.  The shapes are the smallest at which the
kernels can go wrong: a lane of the assignment kernel is a (slot, detection) pair of an 8 x 8 grid, so what varies is which
lanes are inactive ((P, S) from (1, 1) to (8, 8), both ways ragged), the number of greedy rounds (0 .. 8), the loop's trip
count and its prefetch edge (1, 2, 7 frames), the state a launch starts from (the partitions) and the gather's ragged last
block (S * 402 * n elements in blocks of 256); one clip of 151 frames gives a long chain."""
import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_render_reference as pr
from self_forcing_amd import pose_retarget_reference as rr
from self_forcing_amd import pose_smooth_reference as sr
from self_forcing_amd import pose_track_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (96, 160)
F32 = np.float32
MARKER = np.array([-1, -1, 0], F32)
BODY = 18


@pytest.fixture(scope="module")
def tracker():
    return sfa.PoseTracker(device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def people(seed, frames, centers, limb=(0.03, 0.08)):
    """Seeded skeletons [frames, len(centers), 134, 3], every point valid: necks at x = centers, limbs `limb` long, the other
    points within 0.08 of the neck; each person drifts by a CONSTANT step of up to 0.004 per frame, with jitter of 0.004"""
    rng = np.random.default_rng(seed)
    k = np.zeros((frames, len(centers), 134, 3), F32)
    for q, cx in enumerate(centers):
        xy = np.zeros((134, 2))
        xy[1] = (cx, rng.uniform(0.4, 0.6))
        for a, b in pr.LIMBS:
            angle, length = rng.uniform(0, 2 * np.pi), rng.uniform(*limb)
            xy[b] = xy[a] + length * np.array([np.cos(angle), np.sin(angle)])
        xy[BODY:] = xy[1] + rng.uniform(-0.08, 0.08, (134 - BODY, 2))
        drift = rng.uniform(-0.004, 0.004, 2)
        for f in range(frames):
            k[f, q, :, :2] = np.abs(xy + f * drift + rng.uniform(-0.004, 0.004, (134, 2)))
    k[..., 2] = rng.uniform(0.5, 1.0, k.shape[:3])
    return k


def shuffled(k, rng, first=1):
    """The people of every frame from `first` on in a seeded random order"""
    out = k.copy()
    for f in range(first, len(k)):
        out[f] = k[f, rng.permutation(k.shape[1])]
    return out


def crowd(seed, frames, count, pixels=False, jump=0.12):
    """A clip for the tracker to go wrong on: `count` people 0.8 / count apart, 5 % of the points dropped, people who leave for
    one to four frames, people who jump by 0.15..0.4 (a new person to the tracker; a share `jump` of the samples) and by
    0.03..0.06 (the gate decides), the order shuffled in every frame"""
    rng = np.random.default_rng(seed)
    k = people(seed, frames, tuple(0.1 + 0.8 * (q + 0.5) / count for q in range(count)))
    for q in range(count):
        shift = np.zeros(2)
        for f in range(1, frames):
            u = rng.random()
            if u < jump:
                shift = shift + rng.uniform(0.15, 0.4, 2) * rng.choice([-1, 1], 2)
            elif u < jump + 0.18:
                shift = shift + rng.uniform(0.03, 0.06, 2) * rng.choice([-1, 1], 2)
            k[f, q, :, :2] = np.abs(k[f, q, :, :2] + shift.astype(F32))
    k[rng.random(k.shape[:3]) < 0.05] = MARKER
    gone = rng.random(k.shape[:2]) < 0.1
    for _ in range(3):
        gone[1:] |= gone[:-1] & (rng.random(gone[1:].shape) < 0.5)
    k[gone] = MARKER
    if pixels:
        k[..., :2] *= F32([SIZE[1], SIZE[0]])
    return shuffled(k, rng, 0)


def same(tracker, k, counts=None, **kw):
    """`track` and a one-push stream against the definition: the bits of the output, the ids, and the bits of the state left
    on the device"""
    src = tr.as_source(k)
    p = tr.prepare(**kw)
    slots = src.shape[1] if p.slots is None else p.slots
    state = tr.fresh_state(slots)
    want, want_ids = tr.frames(src, state, p, counts)
    got = tracker.track(k, **kw)
    assert isinstance(got, tuple) and got.keypoints is got[0] and got.ids is got[1]
    assert got.keypoints.dtype == torch.float32 and tuple(got.keypoints.shape) == want.shape and got.keypoints.is_contiguous()
    assert got.ids.dtype == torch.int32 and tuple(got.ids.shape) == want_ids.shape and got.ids.device == got.keypoints.device == torch.device(DEV)
    out, ids = got.keypoints.cpu().numpy(), got.ids.cpu().numpy()
    assert np.array_equal(ids, want_ids), (np.argwhere(ids != want_ids)[:4].tolist(), kw)
    assert np.array_equal(bits(out), bits(want)), (int((bits(out) != bits(want)).sum()), kw)
    stream = tracker.open_stream(**kw)
    assert stream.state is None and stream.ids is None
    again = stream.push(k)
    assert stream.state.dtype == torch.int32 and tuple(stream.state.shape) == state.shape and stream.state.device == torch.device(DEV)
    assert np.array_equal(bits(again.cpu().numpy()), bits(want)) and np.array_equal(stream.ids.cpu().numpy(), want_ids) and stream.frames_in == len(src)
    left = stream.state.cpu().numpy()
    assert np.array_equal(left, state), (np.argwhere(left != state)[:4].tolist(), kw)
    return want, want_ids


def settings(count, slots):
    """Every (clip, arguments) of one (P, S): clips of 1, 2 and 7 frames in normalised and pixel coordinates, max_age 0, 1
    and 3 and two gates; and 12 frames in which everybody keeps jumping while no slot is freed, so that the slots run out"""
    for frames in (1, 2, 7):
        for pixels in (False, True):
            k = crowd(1000 * count + 100 * slots + 10 * frames + pixels, frames, count, pixels)
            for max_age in (0, 1, 3):
                for gate in (0.5, 0.25):
                    yield k, dict(slots=slots, max_age=max_age, gate=gate)
    yield crowd(1000 * count + 100 * slots, 12, count, jump=0.9), dict(slots=slots, max_age=20)


# ============================================================================================== kernels against reference
@pytest.mark.parametrize("count,slots", [(1, 1), (2, 2), (3, 2), (2, 3), (8, 8), (8, 1), (1, 8), (5, 8)])
def test_every_setting_equals_the_definition(tracker, count, slots):
    counts = {}
    for k, kw in settings(count, slots):
        fired = {}
        same(tracker, k, fired, **kw)
        assert kw["max_age"] > 0 or fired["lost"] == 0
        for name, hits in fired.items():
            counts[name] = counts.get(name, 0) + hits
    # every rule of the definition fired for this grid: no pass without matches, births, tracks that wait and tracks that
    # die, people dropped for want of a slot and pairs that only the gate kept apart
    assert all(counts[name] > 0 for name in tr.RULES), counts
    assert counts["match"] >= 40 and counts["birth"] >= 20


def edge_clip(threshold=F32(0.3)):
    """[6, 6, 134, 3] for 8 slots and what its rows are for; every row starts as a person at its own place"""
    k = people(11, 6, tuple(0.1 + 0.15 * q for q in range(6)))
    below = np.nextafter(threshold, F32(-1))
    k[:, 0, :BODY, 2] = below                                                            # row 0: four points AT the threshold, the rest one ulp below
    k[:, 0, :4, 2] = threshold
    k[2:, 0, 3, 2] = below                                                               # ... then three: no person any more
    k[:, 1, 4:BODY] = MARKER                                                             # row 1: four points, two of them at -0.0 (valid) ...
    k[:, 1, 0, 0], k[:, 1, 1, 1] = -0.0, -0.0
    k[3, 1, 2, 2] = -0.0                                                                 # ... and a score of -0.0 (low) in frame 3: three points, no person
    for c, bad in enumerate((np.nan, np.inf, -np.inf)):                                  # row 2: NaN and inf in each field of points 5..13 in frame 2
        for field in range(3):
            k[2, 2, 5 + 3 * c + field, field] = bad
    k[2, 3, :BODY, 0] = 3e38                                                             # row 3: huge in frame 2: acc overflows against the track
    k[:, 4, 0, 0], k[:, 4, 2, 1], k[:, 4, 5, :2] = 1e-42, 1e-45, (3e-39, 0)              # row 4: subnormal coordinates on a body of normal size
    k[:, 5, :BODY, :2] = k[0, 5, 1, :2]                                                  # row 5: all valid points coincide: s2 = 0, never matched
    return k


def test_edge_values_in_one_launch(tracker):
    for threshold in (0.3, 0.5, 0.0):
        k = edge_clip(F32(threshold))
        fired = {}
        out, ids = same(tracker, k, fired, slots=8, score_threshold=threshold)
        assert ids[:, 3].tolist() == [3, 3, -1, 3, 3, 3] and ids[2, 7] == 7 and np.array_equal(bits(out[2, 7]), bits(k[2, 3]))      # 3e38: never picked
        assert (ids[:, 4] == 4).all() and np.array_equal(bits(out[:, 4]), bits(k[:, 4]))                                            # subnormals are kept
        assert (ids[:, 2] == 2).all() and fired["overflow"] > 0 and fired["freed"] > 0
        same(tracker, k, slots=8, score_threshold=threshold, min_common=1, min_points=1, max_age=0, gate=2.0)
    huge = people(12, 3, (0.5,))                                                         # a box of infinite extent: s2 = inf is not admissible
    huge[:, 0, 0, 0] = 3e38
    assert same(tracker, huge, slots=2)[1].tolist() == [[0, -1], [-1, 1], [-1, -1]]
    few = people(13, 2, (0.5,))
    few[0, 0, 9:BODY], few[1, 0, :7] = MARKER, MARKER                                    # points 7 and 8 in common
    assert same(tracker, few, slots=2)[1].tolist() == [[0, -1], [-1, 1]]
    assert same(tracker, few, slots=2, min_common=2)[1].tolist() == [[0, -1], [0, -1]]
    assert same(tracker, few, slots=2, min_common=2, min_points=12)[1].tolist() == [[-1, -1], [-1, -1]]


def test_ties_resolve_by_slot_then_detection(tracker):
    one = people(9, 1, (0.5,))[0, 0]
    k = np.stack([np.stack([one] * 8)] * 3)                                              # the same detection in all 8 rows
    k[..., 2] = np.linspace(0.5, 0.9, 8, dtype=F32)[None, :, None]                       # told apart by score alone, which matching never reads
    fired = {}
    out, ids = same(tracker, k, fired)
    assert (ids == np.arange(8)).all() and np.array_equal(bits(out), bits(k)) and fired["match"] == 16
    k[1] = k[1, ::-1]                                                                    # reversed in frame 1: still by index, so the scores reverse
    out, ids = same(tracker, k)
    assert (ids == np.arange(8)).all() and np.array_equal(bits(out[1]), bits(k[1])) and np.array_equal(bits(out[2]), bits(k[2]))
    for slots in (3, 1):
        out, ids = same(tracker, k, slots=slots)
        assert (ids == np.arange(slots)).all() and np.array_equal(bits(out), bits(k[:, :slots]))


def test_input_kinds_and_a_long_clip(tracker):
    k = crowd(7, 5, 2)
    want, want_ids = tr.track(k, slots=3, max_age=1)
    for kk in (k, torch.from_numpy(k), torch.from_numpy(k).to(DEV), torch.from_numpy(k).double(), k.tolist()):
        got = tracker.track(kk, slots=3, max_age=1)
        assert torch.equal(got.keypoints.cpu(), torch.from_numpy(want)) and torch.equal(got.ids.cpu(), torch.from_numpy(want_ids))
    one = crowd(9, 4, 1)
    got = tracker.track(one[:, 0])                                                       # [F, 134, 3] is one person
    assert torch.equal(got.keypoints.cpu(), torch.from_numpy(tr.track(one)[0])) and got.ids.shape == (4, 1)
    # 151 frames of three people, the bench tool's kind of clip: a long chain, and ids far beyond the slots
    fired = {}
    _, ids = same(tracker, crowd(10, 151, 3), fired, max_age=2)
    assert all(fired[name] > 0 for name in tr.RULES) and fired["match"] > 200 and ids.max() > 20
    # a shuffled clip of steady people comes back in order
    steady = people(3, 31, (0.2, 0.5, 0.8))
    rng = np.random.default_rng(103)
    steady[rng.random(steady.shape[:3]) < 0.05] = MARKER
    out, ids = same(tracker, shuffled(steady, rng))
    assert np.array_equal(bits(out), bits(steady)) and (ids == np.arange(3)).all()


# ============================================================================================== stream and pipeline
@pytest.mark.parametrize("kw", [dict(), dict(slots=3, max_age=1, gate=0.3)], ids=["defaults", "three-slots"])
def test_stream_partitions_equal_the_one_shot_call(tracker, kw):
    n = 7
    k = crowd(11, n, 4)
    slots = kw.get("slots", 4)
    state = tr.fresh_state(slots)
    want, want_ids = tr.frames(k, state, tr.prepare(**kw))
    whole = tracker.track(k, **kw)
    assert np.array_equal(bits(whole.keypoints.cpu().numpy()), bits(want)) and np.array_equal(whole.ids.cpu().numpy(), want_ids)
    dev = torch.from_numpy(k).to(DEV)
    for parts in ([1] * n, [5, 2], [3, 4], [n]):
        for pieces in (k, dev, torch.from_numpy(k)):
            stream = tracker.open_stream(**kw)
            got, got_ids, at = [], [], 0
            for m in parts:
                got.append(stream.push(pieces[at:at + m]))
                got_ids.append(stream.ids)
                assert got[-1].shape == (m, slots, 134, 3) and got[-1].device == torch.device(DEV) and got[-1].dtype == torch.float32
                assert stream.ids.shape == (m, slots) and stream.ids.dtype == torch.int32
                at += m
                assert stream.frames_in == at
            assert stream.close() is None
            assert torch.equal(torch.cat(got), whole.keypoints) and torch.equal(torch.cat(got_ids), whole.ids), (parts, type(pieces))
            assert np.array_equal(stream.state.cpu().numpy(), state), (parts, type(pieces))
            with pytest.raises(ValueError, match="closed"):
                stream.push(pieces[:1])
    stream = tracker.open_stream(**kw)
    first = dev[:3].clone()
    out = stream.push(first)
    first.zero_()                                                                        # the stream keeps nothing of the caller's
    rest = stream.push(dev[3:])
    assert torch.equal(torch.cat([out, rest]), whole.keypoints) and torch.equal(stream.ids, whole.ids[3:])
    with pytest.raises(ValueError, match="holds 4 people, the piece 1"):
        stream.push(dev[:1, :1])


def swapping_pair(seed, frames=10):
    """Two steady people of a size the renderer shows, a reference, and the clip with their order swapped in frames 3, 4 and 7"""
    k, ref = people(seed, frames, (0.3, 0.7), (0.06, 0.15)), people(seed + 1, 1, (0.5,), (0.06, 0.15))[0]
    mixed = k.copy()
    for f in (3, 4, 7):
        mixed[f] = k[f, ::-1]
    return k, mixed, ref


def test_tracked_keypoints_smooth_retarget_and_render_as_the_definitions_say(tracker):
    smoother, retargeter, renderer = sfa.PoseSmoother(device=DEV), sfa.PoseRetargeter(device=DEV), sfa.PoseRenderer(device=DEV)
    k, mixed, ref = swapping_pair(13)
    kw = dict(min_cutoff=1.0, beta=0.7, max_gap=2)

    def chain(source, track):
        if track:
            source = tracker.track(source).keypoints
        return renderer.render(retargeter.retarget(smoother.smooth(source, 30, **kw), ref, SIZE, source_fps=30), SIZE, layout="hwc", normalized=False)
    tracked, ids = tr.track(mixed)
    assert np.array_equal(bits(tracked), bits(k)) and (ids == [0, 1]).all()
    want = pr.render(rr.retarget(sr.smooth(tracked, 30, **kw), ref, SIZE, source_fps=30), SIZE, normalized=False)
    frames = chain(mixed, True)
    assert torch.equal(frames.cpu(), torch.from_numpy(want)) and want.any(-1).mean() > 0.005
    assert torch.equal(frames, chain(k, False))                                          # what a source that tracks would have given
    untracked = chain(mixed, False)                                                      # each person smoothed towards the other and fitted as the other
    assert torch.equal(untracked.cpu(), torch.from_numpy(pr.render(rr.retarget(sr.smooth(mixed, 30, **kw), ref, SIZE, source_fps=30), SIZE, normalized=False)))
    assert not torch.equal(frames, untracked)


@pytest.mark.parametrize("per_piece", [1, 3])
def test_pose_feed_through_a_tracker_yields_the_pieces_of_the_one_shot_result(tracker, per_piece):
    smoother, retargeter, renderer = sfa.PoseSmoother(device=DEV), sfa.PoseRetargeter(device=DEV), sfa.PoseRenderer(device=DEV)
    n = 10
    k, mixed, ref = swapping_pair(15, n)
    kw = dict(beta=0.7, max_gap=2)
    whole = renderer.render(retargeter.retarget(smoother.smooth(tracker.track(mixed).keypoints, 30, **kw), ref, SIZE, source_fps=30), SIZE, normalized=False)
    assert whole.shape == (3, 5, *SIZE)
    assert torch.equal(whole, renderer.render(retargeter.retarget(smoother.smooth(k, 30, **kw), ref, SIZE, source_fps=30), SIZE, normalized=False))
    for source in ([mixed[i] for i in range(n)], [torch.from_numpy(mixed[i]).to(DEV) for i in range(n)]):
        live = tracker.open_stream()
        feed = sfa.pose_render.pose_feed(iter(source), renderer, SIZE, per_piece, retargeter=retargeter.open_stream(ref, SIZE, source_fps=30),
                                         smoother=smoother.open_stream(30, **kw), tracker=live)
        pieces = list(feed)
        assert [p.shape[1] for p in pieces] == [per_piece] * (5 // per_piece) + ([5 % per_piece] if 5 % per_piece else [])
        assert all(p.dtype == torch.uint8 and p.shape[0] == 3 for p in pieces) and torch.equal(torch.cat(pieces, dim=1), whole)
        assert live.frames_in == n
    # the tracker alone, and the tracker and the smoother: pieces of source frames, drawn with the feed's `normalized`
    pieces = list(sfa.pose_render.pose_feed(iter(mixed), renderer, SIZE, per_piece, tracker=tracker.open_stream()))
    assert [p.shape[1] for p in pieces] == [per_piece] * (n // per_piece) + ([n % per_piece] if n % per_piece else [])
    assert torch.equal(torch.cat(pieces, dim=1).cpu(), torch.from_numpy(pr.render(k, SIZE, "pose")))
    pieces = list(sfa.pose_render.pose_feed(iter(mixed), renderer, SIZE, per_piece, tracker=tracker.open_stream(), smoother=smoother.open_stream(30, **kw)))
    assert torch.equal(torch.cat(pieces, dim=1).cpu(), torch.from_numpy(pr.render(sr.smooth(k, 30, **kw), SIZE, "pose")))
    # without a tracker: what the feed gave before
    plain = list(sfa.pose_render.pose_feed(iter(mixed), renderer, SIZE, per_piece, smoother=smoother.open_stream(30, **kw), tracker=None))
    assert torch.equal(torch.cat(plain, dim=1).cpu(), torch.from_numpy(pr.render(sr.smooth(mixed, 30, **kw), SIZE, "pose")))
    # a smoother that bridges more frames than the tracker keeps a slot empty
    feed = sfa.pose_render.pose_feed(iter(mixed), renderer, SIZE, per_piece, tracker=tracker.open_stream(max_age=1), smoother=smoother.open_stream(30, **kw))
    with pytest.raises(ValueError, match="max_gap = 2 .* max_age \\+ 1 = 2 .* one person towards another"):
        next(feed)


def test_generate_tracks_keypoint_files(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import generate
    k, mixed, ref = swapping_pair(17)
    ref = np.concatenate([ref, people(19, 1, (0.4,), (0.06, 0.15))[0]])
    np.savez(tmp_path / "clip.npz", keypoints=mixed)
    np.save(tmp_path / "ref.npy", ref[::-1])                                             # a reference in any order: it is never tracked
    paths = (str(tmp_path / "clip.npz"), str(tmp_path / "ref.npy"), torch.device(DEV), SIZE)
    ref_frame = torch.from_numpy(pr.render(ref[None, ::-1], SIZE)[0])
    clip_frames, drawn = generate.load_pose_keypoints(*paths)                            # the defaults: as before
    assert torch.equal(clip_frames.cpu(), torch.from_numpy(pr.render(mixed, SIZE, "pose"))) and torch.equal(drawn.cpu(), ref_frame)
    clip_frames, drawn = generate.load_pose_keypoints(*paths, smooth=(1.0, 0.7), hold=2, source_fps="30", align=True, track={})
    moved = rr.retarget(sr.smooth(k, "30", 1.0, 0.7, max_gap=2), ref[::-1], SIZE, source_fps="30", align=True)
    assert torch.equal(clip_frames.cpu(), torch.from_numpy(pr.render(moved, SIZE, "pose", normalized=False)))
    assert torch.equal(drawn.cpu(), ref_frame)
    unmoved = rr.retarget(sr.smooth(mixed, "30", 1.0, 0.7, max_gap=2), ref[::-1], SIZE, source_fps="30", align=True)
    assert not np.array_equal(moved, unmoved)
    clip_frames, _ = generate.load_pose_keypoints(*paths, track=dict(slots=1, gate=0.4, max_age=0))      # one slot: the first person alone
    assert torch.equal(clip_frames.cpu(), torch.from_numpy(pr.render(k[:, :1], SIZE, "pose")))


def test_the_current_stream_and_the_tensors_device(tracker):
    k = torch.from_numpy(crowd(19, 7, 8)).to(DEV)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            outs.append(tuple(tracker.track(k, max_age=1)))
            stream = tracker.open_stream(max_age=1)
            a, a_ids = stream.push(k[:3]), stream.ids
            b, b_ids = stream.push(k[3:]), stream.ids
            outs.append((torch.cat([a, b]), torch.cat([a_ids, b_ids])))
    torch.cuda.synchronize()
    want, want_ids = tr.track(k.cpu().numpy(), max_age=1)
    for o, i in outs:
        assert o.device == k.device and torch.equal(o.cpu(), torch.from_numpy(want)) and torch.equal(i.cpu(), torch.from_numpy(want_ids))
