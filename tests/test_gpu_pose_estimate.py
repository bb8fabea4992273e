"""The DWPose glue on the device (csrc/pose_estimate.hip) against its definition (pose_estimate_reference.py): boxes, person
crops and SimCC keypoints, every float32 compared by its bits, at the smallest shapes at which the kernels can go wrong, and
`PoseEstimator` end to end with stub networks."""
import itertools

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_estimate_reference as er
from self_forcing_amd import pose_render_reference as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ============================================================================================== boxes
def same_boxes(head, ratio, people, **kw):
    p = er.box_params(**kw)
    want_b, want_c = er.decode_boxes(head, ratio, people, p)
    boxes, count = sfa.ops.decode_boxes(dev(head), float(F32(ratio)), people, **kw)
    assert boxes.dtype == torch.float32 and count.dtype == torch.int32
    got_b, got_c = boxes.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(got_c, want_c), (got_c, want_c)
    assert np.array_equal(bits(got_b), bits(want_b)), (got_b, want_b)
    return want_b, want_c


def quiet_head(frames, p: er.BoxParams, classes):
    """A head with no candidate: objectness 0.05, class scores 0.5."""
    head = np.zeros((frames, p.anchors, 5 + classes), F32)
    head[..., 4], head[..., 5:] = 0.05, 0.5
    return head


def plant(head, f, anchor, score, size=(0.0, 0.0), cls=0, offset=(0.5, 0.5)):
    """An undecoded box on `anchor`: its centre `offset` cells into the cell, w, h = exp(size) strides."""
    head[f, anchor, :4] = (offset[0], offset[1], size[0], size[1])
    head[f, anchor, 4], head[f, anchor, 5 + cls] = score, 1.0


def random_head(seed, frames, p: er.BoxParams, classes):
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1, (frames, p.anchors, 5 + classes)).astype(F32)
    head[..., 4:] = rng.uniform(0, 1, (frames, p.anchors, 1 + classes))
    return head


@pytest.mark.parametrize("input_size,classes,frames", [((64, 64), 1, 1), ((64, 64), 3, 3), ((96, 64), 3, 1), ((96, 64), 1, 3)])
@pytest.mark.parametrize("people", [1, 3, 8])
def test_boxes_of_random_heads(input_size, classes, frames, people):
    kw = dict(input_size=input_size, class_index=classes - 1)
    p = er.box_params(**kw)
    assert p.anchors == (84 if input_size == (64, 64) else 126)
    head = random_head(people * 7 + classes, frames, p, classes)
    _, count = same_boxes(head, 1.0, people, **kw)
    assert count.max() == people                                        # more survivors than P in some frame
    same_boxes(head, 0.7692308, people, iou_threshold=0.1, score_threshold=0.6, **kw)
    same_boxes(head * F32(8), 1.3, people, decoded=True, **kw)


def test_boxes_counts_ties_and_non_finite_values():
    kw = dict(input_size=(64, 64), class_index=2)
    p = er.box_params(**kw)
    people = 3
    head = quiet_head(6, p, 3)
    # frame 0: no candidate.  frame 1: exactly P, far apart, on three levels.  frame 2: P + 2 far apart
    for a, s in ((0, 0.9), (69, 0.5), (83, 0.7)):
        plant(head, 1, a, s, cls=2)
    for a, s in ((0, 0.4), (7, 0.5), (56, 0.8), (63, 0.7), (36, 0.6)):
        plant(head, 2, a, s, cls=2)
    # frame 3: two equal scores far apart (the lower anchor first), and two equal scores on one spot (the lower anchor alone)
    for a in (5, 58):
        plant(head, 3, a, 0.75, cls=2)
    plant(head, 3, 27, 0.5, size=(1.0, 1.0), cls=2), plant(head, 3, 28, 0.5, size=(1.0, 1.0), cls=2, offset=(-0.5, 0.5))
    # frame 4: NaN and infinite scores and corners are no candidates; an enormous finite box is one
    plant(head, 4, 1, np.nan, cls=2), plant(head, 4, 2, np.inf, cls=2), plant(head, 4, 3, -np.inf, cls=2)
    plant(head, 4, 10, 0.9, cls=2, offset=(np.nan, 0.5)), plant(head, 4, 11, 0.9, cls=2, offset=(0.5, np.inf))
    plant(head, 4, 12, 0.9, size=(np.nan, 0.0), cls=2), plant(head, 4, 13, 0.8, size=(np.inf, -np.inf), cls=2)
    plant(head, 4, 14, 0.9, cls=2, offset=(3e38, 0.5)), plant(head, 4, 40, 0.6, cls=2)
    head[4, 41, 4], head[4, 41, 7] = 0.9, np.nan
    # frame 5: the other classes do not count
    plant(head, 5, 20, 0.9, cls=0), plant(head, 5, 21, 0.9, cls=1)
    head[5, 20, 7] = head[5, 21, 7] = 0.1
    boxes, count = same_boxes(head, 1.0, people, **kw)
    assert count.tolist() == [0, 3, 3, 3, 2, 0]
    assert np.array_equal(boxes[0], np.tile(er.EMPTY_BOX, (3, 1))) and boxes[1, :, 4].tolist() == [F32(0.9), F32(0.7), F32(0.5)]
    assert boxes[2, :, 4].tolist() == [F32(0.8), F32(0.7), F32(0.6)]
    assert boxes[3, :, 4].tolist() == [F32(0.75), F32(0.75), F32(0.5)] and boxes[3, 0, 1] < boxes[3, 1, 1]    # anchor 5 lies above anchor 58
    corners, live = er.candidates(head, 1.0, p)
    assert np.array_equal(boxes[3, 2, :4], corners[3, 27]) and np.array_equal(corners[3, 27], corners[3, 28])
    assert sorted(np.nonzero(live[4])[0].tolist()) == [13, 40] and boxes[4, 0, 2] > 1e9
    same_boxes(head, 0.5, 8, **kw)


@pytest.mark.parametrize("threshold,kept", [(F32(0.5), 2), (np.nextafter(F32(0.5), F32(0)), 1)])
def test_an_iou_equal_to_the_threshold_keeps_the_box_and_one_ulp_above_removes_it(threshold, kept):
    kw = dict(input_size=(64, 64), decoded=True, iou_threshold=float(threshold))
    head = quiet_head(1, er.box_params(**kw), 1)
    # integers: (0, 0, 9, 9) has area 100 with the + 1, (0, 0, 9, 4) area 50 and lies inside it: iou = 50 / 100
    head[0, 3] = (4.5, 4.5, 9, 9, 0.9, 1.0)
    head[0, 70] = (4.5, 2.0, 9, 4, 0.8, 1.0)
    assert er.iou(np.array([0, 0, 9, 9], F32), np.array([0, 0, 9, 4], F32)) == F32(0.5)
    boxes, count = same_boxes(head, 1.0, 3, **kw)
    assert count.tolist() == [kept] and boxes[0, 0].tolist() == [0, 0, 9, 9, F32(0.9)]


def test_boxes_at_the_real_head_size():
    p = er.box_params()
    assert p.anchors == 8400
    head = random_head(3, 1, p, 80)
    head[0, :, 2:4] *= F32(0.3)
    boxes, count = same_boxes(head, float(er.letterbox_ratio((480, 832), (640, 640))), 8)
    assert count.tolist() == [8] and (np.diff(boxes[0, :, 4]) <= 0).all()


# ============================================================================================== crops
H, W = 20, 27
CASES = np.array([[3, 4, 20, 15, .9],                   # inside the frame
                  [-6, 5, 9, 14, .9],                   # over the left edge
                  [5, -7, 16, 6, .9],                   # over the top edge
                  [18, 3, 33, 17, .9],                  # over the right edge
                  [6, 12, 21, 29, .9],                  # over the bottom edge
                  [40, 30, 52, 44, .9],                 # wholly outside
                  [10, 5, 10, 15, .9],                  # zero width: the aspect fix gives it one
                  [np.nan, 2, 12, 14, .9]], F32)        # not finite: no window, a row of zeros
ODD = np.array([[5, 5, 5, 5, .9], [2, 3, np.inf, 9, .9], [9, 9, 3, 3, .9], [-3e38, 0, 3e38, 10, .9], [0, 0, 26, 19, .9],
                [-100, -100, 200, 200, .9], [26.5, 19.5, 27.5, 20.5, .9], [-1.5, -1.5, 0.5, 0.5, .9]], F32)


def crop_inputs(people):
    """Three frames with 0, 1 and P people listed, the boxes rotated so that every case is a listed person somewhere."""
    rng = np.random.default_rng(people)
    frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    boxes = np.stack([np.roll(CASES, -f, 0)[:people] for f in range(3)])
    return frames, boxes, np.array([0, 1, people], np.int32)


def in_layout(frames, layout):
    return np.ascontiguousarray(frames.transpose({"hwc": (0, 1, 2, 3), "pose": (3, 0, 1, 2), "chw": (0, 3, 1, 2)}[layout]))


def same_crops(frames, boxes, count, layout, dtype, **kw):
    want = er.crop_people(frames, boxes, count, layout, **kw)
    got = sfa.ops.crop_people(dev(frames), dev(boxes), dev(count), layout, dtype=dtype, **kw)
    assert got.dtype == dtype and tuple(got.shape) == want.shape
    if dtype == torch.bfloat16:
        assert torch.equal(got.cpu().view(torch.int16), torch.from_numpy(want).to(torch.bfloat16).view(torch.int16))
    else:
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    return want


@pytest.mark.parametrize("layout", ["hwc", "pose", "chw"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("channels", ["rgb", "bgr"])
def test_small_crops_in_every_layout_type_and_channel_order(layout, dtype, channels):
    frames, boxes, count = crop_inputs(8)
    want = same_crops(in_layout(frames, layout), boxes, count, layout, dtype, out_size=(8, 6), channels=channels)
    want = want.reshape(3, 8, 3, 8, 6)
    assert not want[0].any() and not want[1, 1:].any() and want[1, 0].any()            # count 0, and 1 of 8
    assert not want[2, 5].any() and np.delete(want[2], 5, 0).any(axis=(1, 2, 3)).all()    # frame 2 lists the box that is not finite sixth
    border = (F32(0) - np.array(er.MEAN, F32)) / np.array(er.STD, F32)
    assert np.array_equal(want[2, 3], np.broadcast_to(border.reshape(3, 1, 1), (3, 8, 6)))       # wholly outside: frame 2 lists case 5 fourth


@pytest.mark.parametrize("people", [1, 3, 8])
def test_crop_counts_and_odd_boxes(people):
    frames, boxes, count = crop_inputs(people)
    same_crops(frames, boxes, count, "hwc", torch.float32, out_size=(8, 6))
    same_crops(frames, boxes, count, "hwc", torch.float32, out_size=(5, 9), padding=1.0, mean=(0, 1, 2), std=(1, 2, 255))
    for dtype in (torch.float32, torch.bfloat16):                       # rows of whole quads: the vector stores
        same_crops(frames, boxes, count, "hwc", dtype, out_size=(6, 8), mean=(0, 0, 0))
    odd = np.stack([np.roll(ODD, -f, 0)[:people] for f in range(3)])
    same_crops(frames, odd, np.array([people, people, people], np.int32), "hwc", torch.float32, out_size=(8, 6))


@pytest.mark.parametrize("people,layout,dtype", [(1, "hwc", torch.float32), (3, "pose", torch.bfloat16), (3, "chw", torch.float32)])
def test_crops_at_the_default_size(people, layout, dtype):
    frames, boxes, count = crop_inputs(people)
    want = same_crops(in_layout(frames, layout), boxes, count, layout, dtype)
    assert want.shape == (3 * people, 3, 384, 288)


def test_a_unit_window_copies_the_pixels():
    """A box whose window is the frame at one source pixel per output pixel samples at whole pixels: the crop is the frame."""
    frames = np.random.default_rng(1).integers(0, 256, (1, 8, 6, 3), dtype=np.uint8)
    boxes, count = np.array([[[0, 0, 6, 8, 1]]], F32), np.array([1], np.int32)
    want = same_crops(frames, boxes, count, "hwc", torch.float32, out_size=(8, 6), padding=1.0, mean=(0, 0, 0), std=(1, 1, 1))
    assert np.array_equal(want[0], frames[0].transpose(2, 0, 1).astype(F32))


# ============================================================================================== keypoints
def simcc_inputs(seed, wx, wy, np_dtype):
    """Two frames of three slots, count (3, 1): person (1, 1) and (1, 2) are absent; the cases are planted on frame 0."""
    rng = np.random.default_rng(seed)
    x, y = rng.normal(0, 1, (6, 133, wx)).astype(np_dtype), rng.normal(0, 1, (6, 133, wy)).astype(np_dtype)
    x[0, 0, :], x[0, 0, 0] = -1, 2                       # the maximum at index 0
    y[0, 0, :], y[0, 0, -1] = -1, 2                      # ... and at the last index
    x[0, 1, :], x[0, 1, [3, 7]] = 0.5, 1.5               # a tie: the first index wins
    y[0, 1, :], y[0, 1, [wy - 1, 2]] = 0.25, 1.25
    x[0, 2, :] = -np.abs(x[0, 2, :]) - 0.01              # all negative: the marker
    y[0, 3, :] = np.nan                                  # all NaN: the marker
    x[0, 4, ::2] = np.nan                                # NaN among numbers: skipped
    x[0, 7, 2], y[0, 7, 1] = np.inf, np.inf              # both maxima infinite: the marker
    y[0, 10, 1] = np.inf                                 # one of them: the other is the score
    x[0, 8, :] = 0                                       # zero is not a score
    x[0, 9, :], x[0, 9, [1, 2]] = -0.0, 0.0
    x[1, 5, :], x[1, 5, 4] = 0, 0.2                      # person 1: one shoulder below the neck's threshold, itself still a point
    y[1, 5, :], y[1, 5, 2] = 0, 0.9
    x[1, 6, :], x[1, 6, 1] = 0, 0.9
    y[1, 6, :], y[1, 6, 0] = 0, 0.9
    x[2, 6, :] = -1                                      # person 2: one shoulder missing
    x[0, 5, :], x[0, 5, 2] = 0, 0.9                      # person 0: both shoulders there
    y[0, 5, :], y[0, 5, 3] = 0, 0.8
    x[0, 6, :], x[0, 6, 9] = 0, 0.7
    y[0, 6, :], y[0, 6, 5] = 0, 0.6
    boxes = np.array([[[30, 20, 90, 140, .9], [100.5, 10.25, 150.75, 90, .8], [-20, -30, 50, 60, .7]],
                      [[5, 5, 60, 70, .9], [1, 1, 2, 2, .5], [np.nan, 0, 1, 1, .4]]], F32)
    return x, y, boxes, np.array([3, 1], np.int32)


def same_keypoints(x, y, boxes, count, frame_size=(96, 160), gx=None, gy=None, **kw):
    want = er.decode_simcc(x, y, boxes, count, frame_size, **kw)
    got = sfa.ops.decode_simcc(dev(x) if gx is None else gx, dev(y) if gy is None else gy, dev(boxes), dev(count), frame_size, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (boxes.shape[0], boxes.shape[1], 134, 3)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    return want


@pytest.mark.parametrize("wx,wy", [(12, 16), (13, 70), (576, 768), (1031, 2056), (1032, 2056)])
@pytest.mark.parametrize("np_dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_keypoints_and_their_edges(wx, wy, np_dtype):
    x, y, boxes, count = simcc_inputs(wx, wx, wy, np_dtype)
    kw = dict(out_size=(384, 288)) if wx == 576 else dict(out_size=(8, 6))
    k = same_keypoints(x, y, boxes, count, **kw)
    marker = er.MARKER.tolist()
    assert (k[1, 1:] == er.MARKER).all()                                # absent people
    # COCO 0 is OpenPose 0; COCO 1..4 are OpenPose 15, 14, 17, 16; COCO 7, 8, 9 are OpenPose 6, 3, 7
    assert k[0, 0, 0, 2] == 2 and k[0, 0, 15, 2] == F32(1.25) and k[0, 0, 14].tolist() == marker and k[0, 0, 17].tolist() == marker
    assert not np.isnan(k).any() and k[0, 0, 6].tolist() == marker and k[0, 0, 3].tolist() == marker and k[0, 0, 7].tolist() == marker
    assert k[0, 0, 1, 2] == 1 and k[0, 1, 1].tolist() == marker and k[0, 2, 1].tolist() == marker
    assert k[0, 1, 5, 2] == F32(np_dtype(0.2)) and k[0, 2, 2].tolist() == marker
    win = er.person_window(boxes[0, 0], kw["out_size"][0], kw["out_size"][1], er.PADDING)
    left = win.cx - F32(kw["out_size"][1]) * F32(0.5) * win.ax                                   # index 0 is the window's left edge
    assert k[0, 0, 0, 0] == left / F32(160) and k[0, 0, 15, 0] == (win.cx + (F32(1.5) - F32(kw["out_size"][1]) * F32(0.5)) * win.ax) / F32(160)
    pixels = same_keypoints(x, y, boxes, count, normalized=False, split_ratio=1.5, neck_threshold=0.65, padding=1.0, **kw)
    assert pixels[0, 0, 0, 0] == er.person_window(boxes[0, 0], kw["out_size"][0], kw["out_size"][1], 1.0).cx - F32(kw["out_size"][1]) * F32(0.5) * \
        er.person_window(boxes[0, 0], kw["out_size"][0], kw["out_size"][1], 1.0).ax
    assert pixels[0, 0, 1].tolist() == marker                           # 0.6 is below this threshold


def test_keypoints_from_logits_that_start_inside_a_16_byte_line():
    x, y, boxes, count = simcc_inputs(5, 12, 16, np.float32)
    gx, gy = torch.empty(x.size + 1, device=DEV)[1:].view(x.shape), torch.empty(y.size + 3, device=DEV)[3:].view(y.shape)
    gx.copy_(torch.from_numpy(x)), gy.copy_(torch.from_numpy(y))
    assert gx.data_ptr() % 16 == 4 and gy.data_ptr() % 16 == 12 and gx.is_contiguous()
    same_keypoints(x, y, boxes, count, gx=gx, gy=gy, out_size=(8, 6))


# ============================================================================================== end to end
SIZE = (96, 160)


class Stubs:
    """Two stub networks that return fixed tensors and keep what they were given."""

    def __init__(self, seed, frames, people, input_size=(64, 64), bins=(12, 16)):
        p = er.box_params(input_size=input_size)
        rng = np.random.default_rng(seed)
        head = quiet_head(frames, p, 1)
        for f in range(frames):                          # person-sized boxes in letterbox pixels, f + 2 of them
            for q in range(f + 2):
                plant(head, f, 64 + 3 * q + f, 0.9 - 0.1 * q, size=(0.3, 0.9))
        self.head = head
        self.x = rng.normal(0, 1, (frames * people, 133, bins[0])).astype(F32)
        self.y = rng.normal(0, 1, (frames * people, 133, bins[1])).astype(F32)
        self.seen = []

    def detector(self, x):
        self.seen.append(("detector", x))
        return dev(self.head[:x.shape[0]])

    def pose_net(self, crops):
        self.seen.append(("pose_net", crops))
        return dev(self.x[:crops.shape[0]]), dev(self.y[:crops.shape[0]])

    def simcc(self, crops):
        return self.x[:crops.shape[0]], self.y[:crops.shape[0]]


def clip(seed, frames):
    return np.random.default_rng(seed).integers(0, 256, (frames,) + SIZE + (3,), dtype=np.uint8)


KW = dict(input_size=(64, 64), out_size=(8, 6))


def reference(stubs, frames, people, **kw):
    kw = {**KW, **kw}
    box = er.box_params(kw["input_size"])
    return er.estimate(frames, "hwc", stubs.head[:frames.shape[0]], stubs.simcc, people, box, er.crop_params(kw["out_size"]),
                       er.simcc_params(kw["out_size"]))


def test_the_estimator_equals_the_chained_definition_and_feeds_the_tracker_and_the_renderer():
    frames, stubs = clip(0, 2), Stubs(0, 2, 3)
    est = sfa.PoseEstimator(stubs.detector, stubs.pose_net, DEV, **KW)
    got = est.estimate(dev(frames), 3)
    want = reference(stubs, frames, 3)
    assert want.count.tolist() == [2, 3] and (want.keypoints[..., 2] > 0).sum() > 300
    assert got.keypoints.device == got.boxes.device == got.count.device == torch.device(DEV)
    for g, w in zip(got[:2], want[:2]):
        assert np.array_equal(bits(g.cpu().numpy()), bits(w))
    assert np.array_equal(got.count.cpu().numpy(), want.count)
    (_, x), (_, crops) = stubs.seen
    letterboxed, ratio = er.letterbox(frames, "hwc", (64, 64))
    assert ratio == F32(0.4) and np.array_equal(x.cpu().numpy(), letterboxed) and (letterboxed[:, :, 38:] == 114).all()
    assert np.array_equal(bits(crops.cpu().numpy()), bits(er.crop_people(frames, want.boxes, want.count, "hwc", out_size=(8, 6))))
    tracked = sfa.PoseTracker(DEV).track(got.keypoints)
    assert tuple(tracked.keypoints.shape) == (2, 3, 134, 3) and tuple(tracked.ids.shape) == (2, 3)
    drawn = sfa.PoseRenderer(DEV).render(got.keypoints, SIZE)
    assert torch.equal(drawn.cpu(), torch.from_numpy(pr.render(want.keypoints, SIZE, "pose"))) and drawn.any()
    # what a network returns in another shape is refused by name
    with pytest.raises(ValueError, match=r"head \[2, 84, 5 \+ C\]"):
        sfa.PoseEstimator(lambda x: dev(stubs.head[:1]), stubs.pose_net, DEV, **KW).estimate(dev(frames), 3)
    with pytest.raises(ValueError, match="simcc_x must be"):
        sfa.PoseEstimator(stubs.detector, lambda c: (dev(stubs.x[:5]), dev(stubs.y)), DEV, **KW).estimate(dev(frames), 3)
    # the other layouts give the same people
    for layout in ("pose", "chw"):
        again = est.estimate(dev(in_layout(frames, layout)), 3, layout)
        assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_keypoint_feed_over_a_partition_gives_the_whole_clips_bits():
    frames = clip(1, 5)
    stubs = Stubs(1, 5, 2)
    whole = reference(stubs, frames, 2).keypoints
    outs, at = [], 0
    for n in (2, 1, 2):
        part = Stubs(1, 5, 2)
        part.head, part.x, part.y = stubs.head[at:at + n], stubs.x[2 * at:2 * (at + n)], stubs.y[2 * at:2 * (at + n)]
        est = sfa.PoseEstimator(part.detector, part.pose_net, DEV, **KW)
        outs += list(sfa.keypoint_feed([dev(frames[at:at + n])], est, 2))
        at += n
    assert [o.shape[0] for o in outs] == [2, 1, 2]
    assert np.array_equal(bits(torch.cat(outs).cpu().numpy()), bits(whole))
    per_frame = list(itertools.chain.from_iterable(outs))
    assert len(per_frame) == 5 and tuple(per_frame[0].shape) == (2, 134, 3)
    drawn = list(sfa.pose_render.pose_feed(per_frame, sfa.PoseRenderer(DEV), SIZE, frames_per_piece=5))
    assert torch.equal(drawn[0].cpu(), torch.from_numpy(pr.render(whole, SIZE, "pose")))


def test_the_launches_land_on_the_current_stream():
    frames, stubs = clip(2, 2), Stubs(2, 2, 3)
    est = sfa.PoseEstimator(stubs.detector, stubs.pose_net, DEV, **KW)
    g = dev(frames)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            outs.append(est.estimate(g, 3))
        s.synchronize()                                  # this stream alone: work put on another one would not be waited for
    want = reference(stubs, frames, 3)
    for o in outs:
        assert np.array_equal(bits(o.keypoints.cpu().numpy()), bits(want.keypoints)) and np.array_equal(o.count.cpu().numpy(), want.count)
