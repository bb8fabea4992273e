"""The DWPose glue without a GPU: the numpy definition (pose_estimate_reference.py) against its own claims, the C entry
points' refusals, the ctypes mirror and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_estimate_reference as er
from self_forcing_amd import pose_render_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ============================================================================================== the definition
def test_exp32_is_within_2_to_the_minus_20_of_exp_over_its_range():
    x = np.linspace(-20, 20, 4_000_001).astype(F32)
    x = np.concatenate([x, np.arange(-29, 30, dtype=F32) * F32(np.log(2)), np.arange(-29, 30, dtype=F32) * F32(np.log(2) / 2)])
    x = x[np.abs(x) <= 20]
    got, want = er.exp32(x).astype(np.float64), np.exp(x.astype(np.float64))
    worst = np.max(np.abs(got - want) / want)
    print(f"exp32: worst relative error {worst:.3e} = {worst / 2.0 ** -23:.2f} ulp over {x.size} points")
    assert worst <= 2.0 ** -20
    # the clamp, and what is no number
    assert er.exp32(F32(-1000)) == er.exp32(F32(-20)) and er.exp32(F32(np.inf)) == er.exp32(F32(20)) and np.isnan(er.exp32(F32(np.nan)))
    assert er.exp32(F32(0)) == 1 and er.exp32(np.zeros((2, 3), F32)).dtype == F32


def random_candidates(seed, anchors, ties):
    rng = np.random.default_rng(seed)
    centre, size = rng.uniform(0, 100, (anchors, 2)), rng.uniform(5, 60, (anchors, 2))
    corners = np.concatenate([centre - size / 2, centre + size / 2], 1).astype(F32)
    live = rng.uniform(0.05, 1, anchors).astype(F32)
    if ties:
        live = np.round(live * 8).astype(F32) / F32(8)               # nine values: most scores are shared
        corners[1::3] = corners[::3][:corners[1::3].shape[0]]         # and a third of the boxes are copies
    live[rng.random(anchors) < 0.3] = 0
    return corners, live


@pytest.mark.parametrize("ties", [False, True])
def test_p_rounds_of_arg_max_equal_full_nms_cut_to_p(ties):
    more = 0
    for seed in range(16):
        corners, live = random_candidates(seed, 30 + 3 * seed, ties)
        everyone, total = er.nms_full(corners, live, 1000, F32(0.45))
        for people in (1, 3, 8):
            a, na = er.nms_rounds(corners, live, people, F32(0.45))
            b, nb = er.nms_full(corners, live, people, F32(0.45))
            assert na == nb == min(total, people) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(a[:na], everyone[:na]) and (a[na:] == er.EMPTY_BOX).all()
            more += total > people
    assert more >= 30                                                   # more survivors than P is the usual case here


def test_ties_go_to_the_lowest_anchor_and_nan_never_suppresses():
    corners = np.array([[0, 0, 10, 10], [50, 50, 60, 60], [0, 0, 10, 10], [np.inf, 0, np.inf, 10], [0, 0, 3e38, 3e38]], F32)
    live = np.array([0.5, 0.5, 0.5, 0, 0.4], F32)
    boxes, n = er.nms_rounds(corners, live, 8, F32(0.45))
    assert n == 3 and np.array_equal(boxes[:3, :4], corners[[0, 1, 4]])           # anchor 2 is a copy of anchor 0; the huge box has iou NaN
    assert np.isnan(er.iou(corners[4], corners[4]))
    head = np.zeros((1, 84, 6), F32)
    p = er.box_params((64, 64))
    boxes, count = er.decode_boxes(head, 1.0, 2, p)
    assert count.tolist() == [0] and (boxes == er.EMPTY_BOX).all() and boxes.shape == (1, 2, 5) and count.dtype == np.int32


def test_the_anchor_grid_is_stride_major_then_row_major():
    gx, gy, s = er.anchor_grid(er.box_params((96, 64)))
    assert gx.shape == (12 * 8 + 6 * 4 + 3 * 2,) and s[:96].tolist() == [8] * 96 and s[96:120].tolist() == [16] * 24 and s[120:].tolist() == [32] * 6
    assert gx[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0] and gy[:9].tolist() == [0] * 8 + [1] and (gx[96:104].tolist(), gy[100]) == ([0, 1, 2, 3] * 2, 1)
    head = np.zeros((1, 126, 6), F32)
    head[0, 97] = (0.5, 0.25, np.log(2), 0, 1, 1)                       # level 1, cell (0, 1): centre (24, 4), 32 x 16
    corners, live = er.candidates(head, 0.5, er.box_params((96, 64)))
    assert live[0, 97] == 1 and np.allclose(corners[0, 97], [16, -8, 80, 24], atol=1e-4)


def test_the_reorder_table_gives_openpose_names():
    table = er.reorder_table()
    tmp_names = list(er.COCO_NAMES) + ["neck"] + [f"point{i}" for i in range(17, 133)]
    out_names = [tmp_names[t] for t in table]
    assert tuple(out_names[:18]) == er.OPENPOSE_NAMES
    assert out_names[18:] == tmp_names[18:] and table.dtype == np.uint8 and table.shape == (134,)
    assert sorted(table.tolist()) == list(range(134))                   # a permutation: nothing is lost
    assert (pr.KEYPOINTS, len(er.BODY_DST), len(er.BODY_SRC)) == (134, 15, 15)
    with pytest.raises(ValueError, match="body_dst"):
        er.reorder_table((1, 1), (2, 3))
    with pytest.raises(ValueError, match="body_src"):
        er.reorder_table((1,), (134,))


def test_planted_keypoints_come_back_within_half_a_bin():
    rng = np.random.default_rng(4)
    frame, out_size, split = (480, 832), (384, 288), 2.0
    boxes = np.array([[[100, 50, 260, 420, .9], [400, 100, 700, 300, .8], [-40, 200, 90, 470, .7]],
                      [[10, 10, 200, 400, .9], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]], F32)
    count = np.array([3, 1], np.int32)
    win, here = er.present(boxes, count, out_size[0], out_size[1], er.PADDING)
    assert here.tolist() == [[True, True, True], [True, False, False]]
    lo, hi = boxes[..., None, :2], boxes[..., None, 2:4]
    truth = (lo + (hi - lo) * rng.uniform(0, 1, (2, 3, 133, 2))).astype(F32)                  # source pixels, inside each box
    bins = (int(out_size[1] * split), int(out_size[0] * split))
    sx, sy = np.zeros((6, 133, bins[0]), F32), np.zeros((6, 133, bins[1]), F32)
    with np.errstate(all="ignore"):
        u = np.rint(((truth[..., 0] - win.cx[..., None]) / win.ax[..., None] + out_size[1] / 2) * split).astype(np.int64).reshape(6, 133)
        v = np.rint(((truth[..., 1] - win.cy[..., None]) / win.ay[..., None] + out_size[0] / 2) * split).astype(np.int64).reshape(6, 133)
    rows = np.repeat(here.reshape(6), 133).reshape(6, 133)
    assert (u[rows] >= 0).all() and (u[rows] < bins[0]).all() and (v[rows] >= 0).all() and (v[rows] < bins[1]).all()
    n, k = np.nonzero(rows)
    sx[n, k, u[n, k]] = 0.9
    sy[n, k, v[n, k]] = 0.8
    got = er.decode_simcc(sx, sy, boxes, count, frame, out_size=out_size, split_ratio=split, normalized=False)
    assert got.shape == (2, 3, 134, 3) and (got[~here] == er.MARKER).all()
    tmp = np.concatenate([truth[..., :17, :], (truth[..., 5:6, :] + truth[..., 6:7, :]) / 2, truth[..., 17:, :]], -2)[..., er.reorder_table(), :]
    bound_x = F32(0.5 / split) * win.ax[here][:, None] + F32(1e-3)
    bound_y = F32(0.5 / split) * win.ay[here][:, None] + F32(1e-3)
    neck = np.arange(134) == 1                                           # the mean of two points, each within the bound
    assert (np.abs(got[here][..., 0] - tmp[here][..., 0]) <= bound_x).all() and (np.abs(got[here][..., 1] - tmp[here][..., 1]) <= bound_y).all()
    assert (got[here][:, ~neck, 2] == F32(0.8)).all() and (got[here][:, neck, 2] == 1).all()
    normalized = er.decode_simcc(sx, sy, boxes, count, frame, out_size=out_size, split_ratio=split)
    assert np.array_equal(normalized[here][:, ~neck, 0], got[here][:, ~neck, 0] / F32(832))            # the neck is the mean of the normalised points
    assert np.array_equal(normalized[here][:, ~neck, 1], got[here][:, ~neck, 1] / F32(480))


def test_person_window_refusals_and_the_aspect_fix():
    w = er.person_window(np.array([[10, 20, 50, 120],                    # tall: the width grows to 3 / 4 of the padded height
                                   [10, 20, 210, 40],                    # wide: the height grows
                                   [5, 5, 5, 5], [9, 9, 3, 3], [5, 5, 5, 4],           # no extent, negative extent
                                   [np.nan, 0, 1, 1], [0, 0, np.inf, 1], [-3e38, 0, 3e38, 1], [0, -np.inf, 1, np.inf],
                                   [10, 5, 10, 15]], F32), 384, 288, 1.25)             # no width: the aspect fix gives it one
    assert w.valid.tolist() == [True, True, False, False, False, False, False, False, False, True]
    assert (w.cx[0], w.cy[0], w.ay[0]) == (30, 70, F32(125) / F32(384)) and w.ax[0] == F32(125) * F32(0.75) / F32(288)
    assert (w.cx[1], w.ax[1]) == (110, F32(250) / F32(288)) and w.ay[1] == F32(250) / F32(0.75) / F32(384)
    assert w.ax[9] > 0 and er.person_window(np.array([0, 0, 1, 1], F32), 8, 6, 1.0).valid.shape == ()
    win, here = er.present(np.array([[[0, 0, 4, 4, 1], [0, 0, 4, 4, 1]]], F32), np.array([1], np.int32), 8, 6, 1.25)
    assert here.tolist() == [[True, False]]


def test_crops_of_the_definition():
    frames = np.random.default_rng(0).integers(0, 256, (1, 8, 6, 3), dtype=np.uint8)
    boxes, count = np.array([[[0, 0, 6, 8, 1], [0, 0, 6, 8, 1]]], F32), np.array([1], np.int32)
    plain = dict(out_size=(8, 6), padding=1.0, mean=(0, 0, 0), std=(1, 1, 1))
    out = er.crop_people(frames, boxes, count, **plain)
    assert out.shape == (2, 3, 8, 6) and out.dtype == F32 and np.array_equal(out[0], frames[0].transpose(2, 0, 1)) and not out[1].any()
    assert np.array_equal(er.crop_people(frames, boxes, count, channels="bgr", **plain)[0], out[0, ::-1])
    for layout, axes in (("pose", (3, 0, 1, 2)), ("chw", (0, 3, 1, 2))):
        assert np.array_equal(er.crop_people(np.ascontiguousarray(frames.transpose(axes)), boxes, count, layout, **plain), out)
    half = er.crop_people(frames, np.array([[[0.5, 0.5, 6.5, 8.5, 1]]], F32), count, **plain)[0]          # half a pixel on: means of four taps
    f = frames[0].astype(F32).transpose(2, 0, 1)
    assert np.array_equal(half[:, :-1, :-1], (f[:, :-1, :-1] + f[:, :-1, 1:] + f[:, 1:, :-1] + f[:, 1:, 1:]) / 4)
    assert np.array_equal(half[:, -1, :-1], (f[:, -1, :-1] + f[:, -1, 1:]) / 4)                             # the taps below the frame are 0
    scaled = er.crop_people(frames, boxes, count, out_size=(8, 6), padding=1.0)
    assert np.array_equal(scaled[0], (out[0] - np.array(er.MEAN, F32).reshape(3, 1, 1)) / np.array(er.STD, F32).reshape(3, 1, 1))
    for bad in (dict(out_size=(0, 6)), dict(out_size=(8, 1025)), dict(padding=0), dict(std=(1, 0, 1)), dict(mean=(1, 2)), dict(channels="gbr"),
                dict(padding=float("nan"))):
        with pytest.raises(ValueError):
            er.crop_params(**bad)


def test_the_letterbox_of_the_definition():
    assert er.letterbox_ratio((480, 832), (640, 640)) == F32(640) / F32(832) and er.letterbox_ratio((96, 160), (64, 64)) == F32(0.4)
    assert er.letterbox_size((96, 160), F32(0.4)) == (38, 64) and er.letterbox_size((3, 4000), er.letterbox_ratio((3, 4000), (64, 64))) == (1, 64)
    frames = np.random.default_rng(0).integers(0, 256, (2, 96, 160, 3), dtype=np.uint8)
    x, ratio = er.letterbox(frames, "hwc", (64, 64))
    assert x.shape == (2, 3, 64, 64) and x.dtype == F32 and (x[:, :, 38:] == 114).all() and (x[:, :, :38] != 114).any() and ratio == F32(0.4)
    small = sfa.resize_reference.resize(frames, (38, 64), "bilinear")
    assert np.array_equal(x[:, :, :38], small.transpose(0, 3, 1, 2).astype(F32))


def test_parameter_checks_name_the_parameter():
    for kw, match in ((dict(input_size=(64, 60)), "multiple of every stride"), (dict(input_size=(1024, 1024)), "anchors"), (dict(strides=()), "strides"),
                      (dict(strides=(8, 16, 32, 64, 128)), "strides"), (dict(class_index=-1), "class_index"), (dict(score_threshold=-0.1), "score_threshold"),
                      (dict(score_threshold=float("nan")), "score_threshold"), (dict(iou_threshold=float("inf")), "iou_threshold"),
                      (dict(input_size=(640,)), "input_size")):
        with pytest.raises(ValueError, match=match):
            er.box_params(**kw)
    p = er.box_params()
    assert (p.anchors, p.strides, p.score_threshold, p.iou_threshold) == (8400, (8, 16, 32), F32(0.3), F32(0.45))
    for shape in ((8400, 85), (1, 8399, 85), (1, 8400, 5), (0, 8400, 85)):
        with pytest.raises(ValueError, match="head must be"):
            er.check_head(shape, p)
    with pytest.raises(ValueError, match="class_index"):
        er.check_head((1, 8400, 6), er.box_params(class_index=1))
    for bad in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match="max_people"):
            er.check_people(bad)
    for kw, match in ((dict(split_ratio=0), "split_ratio"), (dict(neck_threshold=float("nan")), "neck_threshold"), (dict(out_size=(384,)), "out_size")):
        with pytest.raises(ValueError, match=match):
            er.simcc_params(**kw)
    with pytest.raises(ValueError, match="ratio"):
        er.decode_boxes(np.zeros((1, 8400, 6), F32), 0.0, 1, p)


# ============================================================================================== the C entry points
NEW = ("sf_pose_boxes_decode", "sf_pose_boxes_scratch_bytes", "sf_pose_crop_people", "sf_pose_simcc_decode")


def test_the_abi_is_still_11_and_every_new_prototype_has_its_mirror():
    lib, L = sfa._lib.lib(), sfa._lib
    assert lib.sf_abi_version() == 11 == L.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert "#define SF_HIP_ABI_VERSION 11" in header
    declared = re.findall(r"^(?:int|size_t) (sf_pose_(?:boxes|crop|simcc)\w+)\(", header, re.M)
    assert tuple(declared) == NEW and all(name in L.SIGNATURES and hasattr(lib, name) for name in NEW)
    # the new section stands after everything that was there: nothing existing moved
    assert header.index("sf_pose_track_state_bytes(int slots);") < header.index("typedef struct sf_pose_boxes_args")
    for name, value in (("SF_POSE_BOXES_MAX_ANCHORS", L.POSE_BOXES_MAX_ANCHORS), ("SF_POSE_BOXES_MAX_STRIDES", L.POSE_BOXES_MAX_STRIDES),
                        ("SF_POSE_BOXES_MAX_CLASSES", L.POSE_BOXES_MAX_CLASSES), ("SF_POSE_BOXES_MAX_FRAMES", L.POSE_BOXES_MAX_FRAMES),
                        ("SF_POSE_CROP_MAX_SIZE", L.POSE_CROP_MAX_SIZE), ("SF_POSE_CROP_MAX_FRAME", L.POSE_CROP_MAX_FRAME),
                        ("SF_POSE_SIMCC_POINTS", L.POSE_SIMCC_POINTS), ("SF_POSE_SIMCC_MAX_BINS", L.POSE_SIMCC_MAX_BINS)):
        assert f"#define {name} {value}\n" in header
    assert (L.POSE_BOXES_MAX_ANCHORS, L.POSE_BOXES_MAX_STRIDES, L.POSE_BOXES_MAX_CLASSES, L.POSE_BOXES_MAX_FRAMES) == \
        (er.MAX_ANCHORS, er.MAX_STRIDES, er.MAX_CLASSES, er.MAX_FRAMES)
    assert (L.POSE_CROP_MAX_SIZE, L.POSE_CROP_MAX_FRAME, L.POSE_SIMCC_POINTS, L.POSE_SIMCC_MAX_BINS) == (er.MAX_CROP, er.MAX_FRAME_SIZE, er.SIMCC_POINTS, er.MAX_BINS)
    assert "SF_POSE_SIMCC_F32 = 0, SF_POSE_SIMCC_F16 = 1" in header and L.POSE_SIMCC_DTYPES == {"float32": 0, "float16": 1}
    B, K, S = L.PoseBoxesArgs, L.PoseCropArgs, L.PoseSimccArgs
    assert C.sizeof(B) == 4 * 8 + 7 * 4 + 4 * 4 + 2 * 4 + 3 * 4 == 96 and B.F.offset == 32 and B.strides.offset == 60 and B.ratio.offset == 84
    assert C.sizeof(K) == 4 * 8 + 9 * 4 + 4 + 24 == 96 and K.F.offset == 32 and K.padding.offset == 68 and K.mean.offset == 72 and K.std.offset == 84
    assert C.sizeof(S) == 6 * 8 + 10 * 4 + 3 * 4 + 4 == 104 and S.F.offset == 48 and S.padding.offset == 88 and S.neck_threshold.offset == 96
    for f in range(1, 4):
        assert lib.sf_pose_boxes_scratch_bytes(f, 8400) == f * 8400 * 20 == sfa.ops.pose_boxes_scratch_bytes(f, 8400)
    for f, a in ((0, 84), (65536, 84), (1, 0), (1, 16385), (-1, -1)):
        assert lib.sf_pose_boxes_scratch_bytes(f, a) == 0


def overlaps(call, err, ok, size, align=16):
    """every pair of the ranges: the second placed over the first's last bytes, and the first's start inside the second"""
    names = list(size)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for at in (ok[a] + (size[a] - 1) // align * align, ok[a]):
                assert call(**{b: at}) != 0 and b"%s and %s overlap" % (a.encode(), b.encode()) in err(), (a, b, at)


def test_boxes_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib, A = sfa._lib.lib(), sfa._lib.PoseBoxesArgs
    err = lib.sf_last_error
    strides = (C.c_int32 * 4)(8, 16, 32, 0)
    ok = dict(head=1 << 24, boxes=2 << 24, count=3 << 24, scratch=4 << 24, F=2, A=84, C=3, P=3, in_h=64, in_w=64, n_strides=3, strides=strides,
              class_index=2, decoded=0, ratio=0.5, score_threshold=0.3, iou_threshold=0.45)
    size = dict(head=2 * 84 * 8 * 4, boxes=2 * 3 * 5 * 4, count=2 * 4, scratch=2 * 84 * 20)

    def call(**kw):
        return lib.sf_pose_boxes_decode(C.byref(A(**{**ok, **kw})), None)
    assert lib.sf_pose_boxes_decode(None, None) != 0 and b"null args" in err()
    for name in size:
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
        assert call(**{name: ok[name] + 2}) != 0 and b"must be 4-byte aligned" in err(), name
    for bad in (0, 9, -1):
        assert call(P=bad) != 0 and b"P=%d (1..8)" % bad in err()
    for bad in (0, 65536):
        assert call(F=bad) != 0 and b"F=%d (1..65535)" % bad in err()
    for bad in (0, 256):
        assert call(C=bad) != 0 and b"C=%d (1..255)" % bad in err()
    for bad in (-1, 3):
        assert call(class_index=bad) != 0 and b"class_index=%d (0..2)" % bad in err()
    for bad in (0, 5):
        assert call(n_strides=bad) != 0 and b"n_strides=%d (1..4)" % bad in err()
    assert call(A=85) != 0 and b"A=85, the input size and the strides give 84" in err()
    assert call(in_h=60) != 0 and b"stride 8 does not divide the input size 60 x 64" in err()
    assert call(strides=(C.c_int32 * 4)(8, 16, 0, 0)) != 0 and b"stride 0 does not divide" in err()
    assert call(strides=(C.c_int32 * 4)(8, 16, 24, 0)) != 0 and b"stride 24 does not divide" in err()
    assert call(in_h=1024, in_w=1024, A=16385) != 0 and b"more than 16384 anchors" in err()        # A > 16384
    assert call(in_h=0) != 0 and b"input_size" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(ratio=bad) != 0 and b"ratio must be finite and > 0" in err()
    for bad in (-0.1, float("nan"), float("inf")):
        assert call(score_threshold=bad) != 0 and b"score_threshold must be finite and >= 0" in err()
    for bad in (float("nan"), float("inf")):
        assert call(iou_threshold=bad) != 0 and b"iou_threshold must be finite" in err()
    overlaps(call, err, ok, size, 4)


def test_crop_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib, A = sfa._lib.lib(), sfa._lib.PoseCropArgs
    err = lib.sf_last_error
    three = lambda *v: (C.c_float * 3)(*v)                                                                       # noqa: E731
    ok = dict(frames=1 << 24, boxes=2 << 24, count=3 << 24, out=4 << 24, F=2, P=3, H=20, W=27, layout=0, out_h=8, out_w=6, dtype=1, bgr=0, padding=1.25,
              mean=three(1, 2, 3), std=three(1, 2, 3))
    size = dict(frames=2 * 3 * 20 * 27, boxes=2 * 3 * 5 * 4, count=2 * 4, out=6 * 3 * 8 * 6 * 4)

    def call(**kw):
        return lib.sf_pose_crop_people(C.byref(A(**{**ok, **kw})), None)
    assert lib.sf_pose_crop_people(None, None) != 0 and b"null args" in err()
    for name in size:
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
    for name in ("boxes", "count", "out"):
        assert call(**{name: ok[name] + 2}) != 0 and b"4-byte aligned" in err(), name
    assert call(out=ok["out"] + 1, dtype=2) != 0 and b"aligned" in err()
    for bad in (0, 9):
        assert call(P=bad) != 0 and b"P=%d (1..8)" % bad in err()
    for bad in (0, 65536):
        assert call(F=bad) != 0 and b"F=%d (1..65535)" % bad in err()
    for kw in (dict(H=0), dict(W=16385)):
        assert call(**kw) != 0 and b"(1..16384)" in err()
    for kw in (dict(out_h=0), dict(out_w=1025)):
        assert call(**kw) != 0 and b"(1..1024)" in err()
    for bad in (-1, 3):
        assert call(layout=bad) != 0 and b"layout=%d" % bad in err()
    for bad in (0, 3):                                                     # uint8 crops are not on offer
        assert call(dtype=bad) != 0 and b"dtype=%d" % bad in err()
    for bad in (0.0, float("nan"), float("inf")):
        assert call(padding=bad) != 0 and b"padding must be finite and > 0" in err()
    assert call(mean=three(1, float("nan"), 3)) != 0 and b"mean must be finite" in err()
    for bad in (0.0, -1.0, float("inf")):
        assert call(std=three(1, 2, bad)) != 0 and b"std must be finite and > 0" in err()
    overlaps(call, err, ok, size, 4)


def test_simcc_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib, A = sfa._lib.lib(), sfa._lib.PoseSimccArgs
    err = lib.sf_last_error
    table = (C.c_uint8 * 134)(*er.reorder_table().tolist())
    ok = dict(simcc_x=1 << 24, simcc_y=2 << 24, boxes=3 << 24, count=4 << 24, out=5 << 24, order=C.addressof(table), F=2, P=3, H=96, W=160, Wx=12, Wy=16,
              dtype=0, out_h=8, out_w=6, normalized=1, padding=1.25, split_ratio=2.0, neck_threshold=0.3)
    size = dict(simcc_x=6 * 133 * 12 * 4, simcc_y=6 * 133 * 16 * 4, boxes=6 * 5 * 4, count=2 * 4, out=6 * 134 * 12)

    def call(**kw):
        return lib.sf_pose_simcc_decode(C.byref(A(**{**ok, **kw})), None)
    assert lib.sf_pose_simcc_decode(None, None) != 0 and b"null args" in err()
    for name in list(size) + ["order"]:
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
    for name in ("simcc_x", "simcc_y"):
        assert call(**{name: ok[name] + 2}) != 0 and b"aligned to their element" in err(), name
        assert call(**{name: ok[name] + 1, "dtype": 1}) != 0 and b"aligned to their element" in err(), name
    for name in ("boxes", "count", "out"):
        assert call(**{name: ok[name] + 2}) != 0 and b"4-byte aligned" in err(), name
    for bad in (0, 9):
        assert call(P=bad) != 0 and b"P=%d (1..8)" % bad in err()
    for kw in (dict(Wx=0), dict(Wy=65537)):
        assert call(**kw) != 0 and b"(1..65536)" in err()
    for bad in (-1, 2):
        assert call(dtype=bad) != 0 and b"dtype=%d" % bad in err()
    for kw in (dict(H=0), dict(out_w=0), dict(padding=0.0)):
        assert call(**kw) != 0
    for bad in (0.0, float("nan")):
        assert call(split_ratio=bad) != 0 and b"split_ratio must be finite and > 0" in err()
    assert call(neck_threshold=float("nan")) != 0 and b"neck_threshold must be finite" in err()
    wrong = (C.c_uint8 * 134)(*([0] * 133 + [134]))
    assert call(order=C.addressof(wrong)) != 0 and b"order[133]=134 (0..133)" in err()
    overlaps(call, err, ok, size, 4)


# ============================================================================================== the Python surface
def test_operator_schemas_and_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("pose_boxes_decode", "pose_crop_people", "pose_simcc_decode"):
        assert name in sfa.torch_ops.OPS and "!" not in str(getattr(torch.ops.sf_hip, name).default._schema)
    with FakeTensorMode():
        order = torch.zeros(134, dtype=torch.uint8)                      # the reorder table stays on the host
        head = torch.empty(2, 84, 6, device="cuda")
        boxes, count = torch.ops.sf_hip.pose_boxes_decode(head, 64, 64, [8, 16, 32], 1.0, 3)
        assert tuple(boxes.shape) == (2, 3, 5) and boxes.dtype == torch.float32 and tuple(count.shape) == (2,) and count.dtype == torch.int32
        frames = torch.empty(2, 20, 27, 3, dtype=torch.uint8, device="cuda")
        crops = torch.ops.sf_hip.pose_crop_people(frames, boxes, count, "hwc", 8, 6, 1.25, [0., 0., 0.], [1., 1., 1.], False, torch.bfloat16)
        assert tuple(crops.shape) == (6, 3, 8, 6) and crops.dtype == torch.bfloat16
        sx, sy = torch.empty(6, 133, 12, device="cuda", dtype=torch.float16), torch.empty(6, 133, 16, device="cuda", dtype=torch.float16)
        k = torch.ops.sf_hip.pose_simcc_decode(sx, sy, boxes, count, 20, 27, 8, 6, 1.25, 2.0, True, 0.3, order)
        assert tuple(k.shape) == (2, 3, 134, 3) and k.dtype == torch.float32
        with pytest.raises(Exception, match="head must be"):
            torch.ops.sf_hip.pose_boxes_decode(head[:, :80], 64, 64, [8, 16, 32], 1.0, 3)
        with pytest.raises(Exception, match="strides must be"):
            torch.ops.sf_hip.pose_boxes_decode(head, 64, 64, [8, 16, 24], 1.0, 3)
        with pytest.raises(Exception, match="max_people must be"):
            torch.ops.sf_hip.pose_boxes_decode(head, 64, 64, [8, 16, 32], 1.0, 9)
        with pytest.raises(Exception, match="count must be"):
            torch.ops.sf_hip.pose_crop_people(frames, boxes, count[:1], "hwc", 8, 6, 1.25, [0., 0., 0.], [1., 1., 1.], False, torch.float32)
        with pytest.raises(Exception, match="dtype must be"):
            torch.ops.sf_hip.pose_crop_people(frames, boxes, count, "hwc", 8, 6, 1.25, [0., 0., 0.], [1., 1., 1.], False, torch.uint8)
        with pytest.raises(Exception, match="simcc_y must be"):
            torch.ops.sf_hip.pose_simcc_decode(sx, sy[:5], boxes, count, 20, 27, 8, 6, 1.25, 2.0, True, 0.3, order)
        with pytest.raises(Exception, match="both be float32 or both float16"):
            torch.ops.sf_hip.pose_simcc_decode(sx, sy.float(), boxes, count, 20, 27, 8, 6, 1.25, 2.0, True, 0.3, order)
        with pytest.raises(Exception, match="order must be"):
            torch.ops.sf_hip.pose_simcc_decode(sx, sy, boxes, count, 20, 27, 8, 6, 1.25, 2.0, True, 0.3, order[:100])
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.ops.decode_boxes(torch.zeros(1, 84, 6), 1.0, 1, (64, 64))
    boxes, count = torch.zeros(1, 1, 5), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.ops.crop_people(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), boxes, count)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.ops.decode_simcc(torch.zeros(1, 133, 4), torch.zeros(1, 133, 4), boxes, count, (4, 4))
    with pytest.raises(ValueError, match="channels"):
        sfa.ops.crop_people(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), boxes, count, channels="gbr")


def test_pose_estimator_checks_that_need_no_device():
    assert sfa.PoseEstimator is sfa.pose_estimate.PoseEstimator and sfa.keypoint_feed is sfa.pose_estimate.keypoint_feed
    assert {"PoseEstimator", "keypoint_feed", "pose_estimate", "pose_estimate_reference"} <= set(sfa.__all__)
    calls = []
    est = sfa.PoseEstimator(lambda x: calls.append("detector"), lambda c: calls.append("pose_net"), input_size=(64, 64), out_size=(8, 6))
    assert (est.box.anchors, est.crop.out_h, est.simcc.order.tolist()) == (84, 8, er.reorder_table().tolist())
    frames = torch.zeros(2, 96, 160, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        est.estimate(frames, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        next(sfa.keypoint_feed([frames], est, 3))
    for bad in (frames.float(), frames[0], torch.zeros(2, 96, 160, 4, dtype=torch.uint8), frames.numpy(), torch.zeros(0, 96, 160, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="frames must be"):
            est.estimate(bad, 3)
    with pytest.raises(ValueError, match="frames must be"):
        est.estimate(frames, 3, "chw")
    for bad in (0, 9):
        with pytest.raises(ValueError, match="max_people"):
            est.estimate(frames, bad)
    assert calls == []
    assert est.check_head(torch.zeros(2, 84, 6), 2).shape == (2, 84, 6)
    for bad in (torch.zeros(2, 85, 6), torch.zeros(1, 84, 6), torch.zeros(2, 84, 5), torch.zeros(84, 6), None, torch.zeros(2, 84, 5 + 256)):
        with pytest.raises(ValueError, match=r"head \[2, 84, 5 \+ C\]"):
            est.check_head(bad, 2)
    sx, sy = torch.zeros(6, 133, 12), torch.zeros(6, 133, 16)
    assert est.check_simcc((sx, sy), 6)[1] is sy
    for bad, match in (((sx, sy[:5]), "simcc_y must be"), ((sx[:, :17], sy), "simcc_x must be"), ((sx, sy.half()), "both be float32 or both float16"),
                       ((sx.double(), sy.double()), "both be float32"), (sx, "the pair"), ((sx, sy, sy), "the pair"), ((sx, None), "the pair")):
        with pytest.raises(ValueError, match=match):
            est.check_simcc(bad, 6)
    for kw, match in ((dict(layout="nhwc"), "layout"), (dict(crop_dtype=torch.float16), "crop_dtype"), (dict(input_size=(64, 60)), "stride"),
                      (dict(channels="gbr"), "channels"), (dict(split_ratio=-1), "split_ratio"), (dict(body_dst=(1, 1), body_src=(1, 2)), "body_dst")):
        with pytest.raises(ValueError, match=match):
            sfa.PoseEstimator(len, len, **kw)
    with pytest.raises(ValueError, match="callables"):
        sfa.PoseEstimator(None, len)
