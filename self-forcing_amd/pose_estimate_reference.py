"""The definition of the numbers of the DWPose glue (numpy, no GPU): everything DWPose does around its two networks
(YOLOX-L for person boxes, RTMPose for SimCC whole-body keypoints) in numpy and OpenCV on the host.  The formulas and
the style are DWPose's; the bits are THIS PROJECT'S definition: float32, every operation (add, sub, mul, div) rounded on its
own and never fused, so the device (csrc/pose_estimate.hip) equals this file bit for bit.  Nothing here is OpenCV's
fixed-point arithmetic.  The default constants (640 x 640, strides 8 / 16 / 32, 0.3, 0.45, 1.25, 384 x 288, split ratio 2,
the mean / std, the two index lists) are DWPose's published pipeline as remembered; they were NOT checked against a DWPose
checkout, which is why every one is a parameter.

1 boxes      `decode_boxes`: head float32 [F, A, 5 + C] in YOLOX's anchor order (stride-major, then row-major (gy, gx)).
             Per anchor, with gx, gy, s as fp32:  cx = (o0 + gx) * s;  cy = (o1 + gy) * s;  w = exp32(o2) * s;
             h = exp32(o3) * s   (decoded=True: cx, cy, w, h = o0..o3);  x1 = cx - w * 0.5;  x2 = cx + w * 0.5;  y likewise;
             each corner / ratio;  score = o4 * o[5 + class_index].  A CANDIDATE iff score and the corners are finite and
             score > score_threshold (which is >= 0, so a candidate's score is positive and its float bits order as it does).
             Greedy NMS, at most P rounds: the live candidate with the largest score (ties: the lowest anchor) is emitted and
             removed with every live candidate whose iou with it exceeds iou_threshold (false for NaN):
               area = (x2 - x1 + 1) * (y2 - y1 + 1);  iw = max(0, min(x2a, x2b) - max(x1a, x1b) + 1);  ih likewise;
               inter = iw * ih;  iou = inter / (area_a + area_b - inter)       (a = the emitted box; min / max as selects)
             -> boxes float32 [F, P, 5] = (x1, y1, x2, y2, score) in descending score, then (-1, -1, -1, -1, 0); count int32 [F].
             `decode_boxes_full` is full greedy NMS cut to its first P survivors: the same thing.
  exp32      explicit fp32 arithmetic: x clamped to [-20, 20] by selects (NaN passes); n = rint(x * log2e);
             r = x - n * LN2_HI;  r = r - n * LN2_LO;  a degree-6 Taylor polynomial by Horner;  ldexp(p, n).
2 window     `person_window`: the padded, aspect-fixed window of a box, shared by the crop and its inverse:
               cx = (x1 + x2) * 0.5;  bw = (x2 - x1) * padding;  aspect = fp32(out_w) / fp32(out_h);
               bw > bh * aspect ? bh = bw / aspect : bw = bh * aspect;  ax = bw / out_w;  ay = bh / out_h
             valid iff cx, cy, bw, bh, ax, ay are finite and bw > 0 and bh > 0.
3 crops      `crop_people`: element (c, j, i) of person (f, p), p < count[f], valid window:
               sx = cx + (i - out_w * 0.5) * ax;  x0 = floor(sx);  fx = sx - x0   (y likewise); a tap outside the frame is 0;
               a = p00 + (p01 - p00) * fx;  b = p10 + (p11 - p10) * fx;  v = a + (b - a) * fy;  out = (v - mean[c]) / std[c]
             with v = 0 and no tap read unless -1 <= sx <= W and -1 <= sy <= H.  Unfiltered bilinear sampling with a zero
             border, as cv2.warpAffine(INTER_LINEAR), in plain fp32.  Other rows are 0.0.  -> float32 [F * P, 3, out_h, out_w];
             bfloat16 is the round-to-nearest-even of that (torch's `.to(torch.bfloat16)`).
4 keypoints  `decode_simcc`: simcc_x [N, 133, Wx], simcc_y [N, 133, Wy], N = F * P.  ix = the first index of the maximum over
             the non-NaN entries (scan upward with >, start (-inf, 0)), mx its value; s = mx if mx < my else my; the point is
             valid iff the person is present with a valid window, s is finite and s > 0;  u = fp32(ix) / split_ratio;
             x = cx + (u - out_w * 0.5) * ax  (y likewise);  normalized: x / fp32(W), y / fp32(H).  Invalid: (-1, -1, 0).
             Neck from COCO 5 and 6: both valid and both scores > neck_threshold -> ((x5 + x6) * 0.5, (y5 + y6) * 0.5, 1).
             tmp = 17 body points, the neck, the other 116; out = tmp, out[BODY_DST] = tmp[BODY_SRC]: OpenPose-18, feet
             18-23, face 24-91, hands 92-112 and 113-133 (pose_render_reference).  -> float32 [F, P, 134, 3]."""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple, Sequence, Tuple

import numpy as np

from .pose_render_reference import KEYPOINTS, MAX_PEOPLE

F32 = np.float32
MAX_ANCHORS, MAX_STRIDES, MAX_CLASSES, MAX_FRAMES = 16384, 4, 255, 65535
MAX_CROP, MAX_FRAME_SIZE, MAX_BINS = 1024, 16384, 65536
SIMCC_POINTS = 133
INPUT_SIZE, STRIDES = (640, 640), (8, 16, 32)
SCORE_THRESHOLD, IOU_THRESHOLD = 0.3, 0.45
OUT_SIZE, PADDING = (384, 288), 1.25
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
SPLIT_RATIO, NECK_THRESHOLD = 2.0, 0.3
LETTERBOX_FILL = 114.0
BODY_DST = (1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17)
BODY_SRC = (17, 6, 8, 10, 7, 9, 12, 14, 16, 13, 15, 2, 1, 4, 3)
COCO_NAMES = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
              "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle")
OPENPOSE_NAMES = ("nose", "neck", "right_shoulder", "right_elbow", "right_wrist", "left_shoulder", "left_elbow", "left_wrist", "right_hip",
                  "right_knee", "right_ankle", "left_hip", "left_knee", "left_ankle", "right_eye", "left_eye", "right_ear", "left_ear")
MARKER = np.array([-1, -1, 0], F32)
EMPTY_BOX = np.array([-1, -1, -1, -1, 0], F32)

# exp32
EXP_CLAMP = F32(20.0)
LOG2E = F32(1.4426950408889634)
LN2_HI = F32(0.693145751953125)
LN2_LO = F32(1.428606765330187e-06)
EXP_POLY = tuple(F32(1.0 / math.factorial(k)) for k in range(6, -1, -1))     # Horner, the highest degree first


# ------------------------------------------------------------------------------------------ checks
def _integer(value, name: str, lo: int, hi: int) -> int:
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {value!r}")
    return int(value)


def _real(value, name: str, positive: bool = False, non_negative: bool = False) -> np.float32:
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise ValueError(f"{name} must be a number, got {value!r}")
    v = F32(value)
    if not np.isfinite(v) or (positive and not v > 0) or (non_negative and not v >= 0):
        raise ValueError(f"{name} must be finite{' and > 0' if positive else ' and >= 0' if non_negative else ''}, got {value!r}")
    return v


def _pair(value, name: str, lo: int, hi: int) -> Tuple[int, int]:
    if isinstance(value, (str, bytes)) or not isinstance(value, Sequence) or len(value) != 2:
        raise ValueError(f"{name} must be (height, width), got {value!r}")
    return _integer(value[0], f"{name}[0]", lo, hi), _integer(value[1], f"{name}[1]", lo, hi)


def check_people(max_people) -> int:
    return _integer(max_people, "max_people", 1, MAX_PEOPLE)


class BoxParams(NamedTuple):
    in_h: int
    in_w: int
    strides: Tuple[int, ...]
    anchors: int
    class_index: int
    score_threshold: np.float32
    iou_threshold: np.float32
    decoded: bool


def box_params(input_size=INPUT_SIZE, strides=STRIDES, class_index=0, score_threshold=SCORE_THRESHOLD, iou_threshold=IOU_THRESHOLD,
               decoded=False) -> BoxParams:
    in_h, in_w = _pair(input_size, "input_size", 1, 1 << 20)
    if isinstance(strides, (str, bytes)) or not isinstance(strides, Sequence) or not 1 <= len(strides) <= MAX_STRIDES:
        raise ValueError(f"strides must be 1..{MAX_STRIDES} integers, got {strides!r}")
    strides = tuple(_integer(s, "strides[]", 1, 1 << 20) for s in strides)
    for s in strides:
        if in_h % s or in_w % s:
            raise ValueError(f"input_size {in_h} x {in_w} must be a multiple of every stride, got stride {s}")
    anchors = sum((in_h // s) * (in_w // s) for s in strides)
    if anchors > MAX_ANCHORS:
        raise ValueError(f"input_size and strides give {anchors} anchors, at most {MAX_ANCHORS}")
    return BoxParams(in_h, in_w, strides, anchors, _integer(class_index, "class_index", 0, MAX_CLASSES - 1),
                     _real(score_threshold, "score_threshold", non_negative=True), _real(iou_threshold, "iou_threshold"), bool(decoded))


class CropParams(NamedTuple):
    out_h: int
    out_w: int
    padding: np.float32
    mean: Tuple[np.float32, np.float32, np.float32]
    std: Tuple[np.float32, np.float32, np.float32]
    bgr: bool


def _triple(value, name: str, positive: bool):
    if isinstance(value, (str, bytes)) or not isinstance(value, Sequence) or len(value) != 3:
        raise ValueError(f"{name} must be three numbers, got {value!r}")
    return tuple(_real(v, name, positive=positive) for v in value)


def crop_params(out_size=OUT_SIZE, padding=PADDING, mean=MEAN, std=STD, channels="rgb") -> CropParams:
    out_h, out_w = _pair(out_size, "out_size", 1, MAX_CROP)
    if channels not in ("rgb", "bgr"):
        raise ValueError(f"channels must be 'rgb' or 'bgr', got {channels!r}")
    return CropParams(out_h, out_w, _real(padding, "padding", positive=True), _triple(mean, "mean", False), _triple(std, "std", True),
                      channels == "bgr")


class SimccParams(NamedTuple):
    out_h: int
    out_w: int
    padding: np.float32
    split_ratio: np.float32
    normalized: bool
    neck_threshold: np.float32
    order: np.ndarray            # uint8 [134]: the index into tmp of every output point


def reorder_table(body_dst=BODY_DST, body_src=BODY_SRC) -> np.ndarray:
    """uint8 [134]: out[i] = tmp[table[i]]."""
    dst, src = list(body_dst), list(body_src)
    if len(dst) != len(src) or len(set(dst)) != len(dst):
        raise ValueError("body_dst and body_src must be two index lists of one length, body_dst without repeats")
    table = np.arange(KEYPOINTS, dtype=np.uint8)
    for d, s in zip(dst, src):
        table[_integer(d, "body_dst[]", 0, KEYPOINTS - 1)] = _integer(s, "body_src[]", 0, KEYPOINTS - 1)
    return table


def simcc_params(out_size=OUT_SIZE, padding=PADDING, split_ratio=SPLIT_RATIO, normalized=True, neck_threshold=NECK_THRESHOLD, body_dst=BODY_DST,
                 body_src=BODY_SRC) -> SimccParams:
    out_h, out_w = _pair(out_size, "out_size", 1, MAX_CROP)
    return SimccParams(out_h, out_w, _real(padding, "padding", positive=True), _real(split_ratio, "split_ratio", positive=True), bool(normalized),
                       _real(neck_threshold, "neck_threshold"), reorder_table(body_dst, body_src))


def check_head(shape, p: BoxParams) -> Tuple[int, int]:
    """(F, C) of a head [F, A, 5 + C]."""
    if len(shape) != 3 or not 1 <= shape[0] <= MAX_FRAMES or shape[1] != p.anchors or not 6 <= shape[2] <= 5 + MAX_CLASSES:
        raise ValueError(f"head must be [F, {p.anchors}, 5 + C] with 1 <= F <= {MAX_FRAMES} and 1 <= C <= {MAX_CLASSES}, got {tuple(shape)}")
    if p.class_index >= shape[2] - 5:
        raise ValueError(f"class_index {p.class_index} is outside the head's {shape[2] - 5} classes")
    return int(shape[0]), int(shape[2]) - 5


def check_boxes(boxes_shape, count_shape) -> Tuple[int, int]:
    """(F, P) of boxes [F, P, 5] and count [F]."""
    if len(boxes_shape) != 3 or boxes_shape[2] != 5 or not 1 <= boxes_shape[0] <= MAX_FRAMES or not 1 <= boxes_shape[1] <= MAX_PEOPLE:
        raise ValueError(f"boxes must be [F, P, 5] with 1 <= F <= {MAX_FRAMES} and 1 <= P <= {MAX_PEOPLE}, got {tuple(boxes_shape)}")
    if tuple(count_shape) != (boxes_shape[0],):
        raise ValueError(f"count must be [{boxes_shape[0]}], got {tuple(count_shape)}")
    return int(boxes_shape[0]), int(boxes_shape[1])


def check_frame_size(size) -> Tuple[int, int]:
    return _pair(size, "frame size", 1, MAX_FRAME_SIZE)


def check_simcc(x_shape, y_shape, n: int) -> Tuple[int, int]:
    """(Wx, Wy) of simcc_x [N, 133, Wx] and simcc_y [N, 133, Wy]."""
    for name, s in (("simcc_x", x_shape), ("simcc_y", y_shape)):
        if len(s) != 3 or s[0] != n or s[1] != SIMCC_POINTS or not 1 <= s[2] <= MAX_BINS:
            raise ValueError(f"{name} must be [{n}, {SIMCC_POINTS}, bins] with 1 <= bins <= {MAX_BINS}, got {tuple(s)}")
    return int(x_shape[2]), int(y_shape[2])


# ------------------------------------------------------------------------------------------ 1 boxes
def exp32(x) -> np.ndarray:
    """e^x of float32 values clamped to [-20, 20], as the explicit fp32 operations the kernel repeats; NaN gives NaN."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        x = np.where(x < -EXP_CLAMP, -EXP_CLAMP, np.where(x > EXP_CLAMP, EXP_CLAMP, x)).astype(F32)
        n = np.rint(x * LOG2E).astype(F32)
        r = x - n * LN2_HI
        r = r - n * LN2_LO
        p = np.full(x.shape, EXP_POLY[0], F32)
        for c in EXP_POLY[1:]:
            p = p * r
            p = p + c
        return np.ldexp(p, np.where(np.isnan(n), 0, n).astype(np.int32)).astype(F32)


def anchor_grid(p: BoxParams) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(gx, gy, s) float32 [A] in YOLOX's order."""
    gx, gy, ss = [], [], []
    for s in p.strides:
        hs, ws = p.in_h // s, p.in_w // s
        yy, xx = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
        gx.append(xx.ravel()), gy.append(yy.ravel()), ss.append(np.full(hs * ws, s))
    return np.concatenate(gx).astype(F32), np.concatenate(gy).astype(F32), np.concatenate(ss).astype(F32)


def candidates(head: np.ndarray, ratio, p: BoxParams) -> Tuple[np.ndarray, np.ndarray]:
    """(corners float32 [F, A, 4] = (x1, y1, x2, y2) in source pixels, live float32 [F, A] = the score of a candidate, 0 of
    any other anchor)."""
    head = np.asarray(head, F32)
    check_head(head.shape, p)
    ratio = _real(ratio, "ratio", positive=True)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        if p.decoded:
            cx, cy, w, h = (head[..., k] for k in range(4))
        else:
            gx, gy, s = anchor_grid(p)
            cx, cy = (head[..., 0] + gx) * s, (head[..., 1] + gy) * s
            w, h = exp32(head[..., 2]) * s, exp32(head[..., 3]) * s
        hw, hh = w * half, h * half
        corners = np.stack([(cx - hw) / ratio, (cy - hh) / ratio, (cx + hw) / ratio, (cy + hh) / ratio], -1).astype(F32)
        score = (head[..., 4] * head[..., 5 + p.class_index]).astype(F32)
        ok = np.isfinite(score) & np.isfinite(corners).all(-1) & (score > p.score_threshold)
    return corners, np.where(ok, score, F32(0)).astype(F32)


def iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The iou of box a [4] with boxes b [..., 4], the + 1 of DWPose's numpy NMS included; min / max are selects."""
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        area_a = (a[2] - a[0] + one) * (a[3] - a[1] + one)
        area_b = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)
        iw = np.where(a[2] < b[..., 2], a[2], b[..., 2]) - np.where(a[0] > b[..., 0], a[0], b[..., 0]) + one
        ih = np.where(a[3] < b[..., 3], a[3], b[..., 3]) - np.where(a[1] > b[..., 1], a[1], b[..., 1]) + one
        iw, ih = np.where(iw > zero, iw, zero), np.where(ih > zero, ih, zero)
        inter = iw * ih
        return (inter / (area_a + area_b - inter)).astype(F32)


def nms_rounds(corners: np.ndarray, live: np.ndarray, people: int, iou_threshold) -> Tuple[np.ndarray, int]:
    """One frame, the kernel's form: at most `people` rounds of arg-max, emit, suppress."""
    live = live.copy()
    boxes = np.tile(EMPTY_BOX, (people, 1))
    n = 0
    for _ in range(people):
        w = int(np.argmax(live))                       # the first index of the maximum
        if not live[w] > 0:
            break
        boxes[n, :4], boxes[n, 4] = corners[w], live[w]
        n += 1
        with np.errstate(all="ignore"):
            gone = (live > 0) & (iou(corners[w], corners) > iou_threshold)
        live[gone] = 0
        live[w] = 0
    return boxes, n


def nms_full(corners: np.ndarray, live: np.ndarray, people: int, iou_threshold) -> Tuple[np.ndarray, int]:
    """One frame, DWPose's form: sort by score (stable, descending), full greedy NMS, the first `people` survivors."""
    order = [int(i) for i in np.argsort(-live.astype(np.float64), kind="stable") if live[i] > 0]
    keep = []
    while order:
        w = order.pop(0)
        keep.append(w)
        with np.errstate(all="ignore"):
            order = [i for i in order if not iou(corners[w], corners[i]) > iou_threshold]
    boxes = np.tile(EMPTY_BOX, (people, 1))
    for n, w in enumerate(keep[:people]):
        boxes[n, :4], boxes[n, 4] = corners[w], live[w]
    return boxes, min(len(keep), people)


def _decode(head, ratio, max_people, p: BoxParams, nms) -> Tuple[np.ndarray, np.ndarray]:
    people = check_people(max_people)
    corners, live = candidates(head, ratio, p)
    frames = [nms(corners[f], live[f], people, p.iou_threshold) for f in range(corners.shape[0])]
    return np.stack([b for b, _ in frames]).astype(F32), np.array([n for _, n in frames], np.int32)


def decode_boxes(head, ratio, max_people, params: BoxParams = None, **kw) -> Tuple[np.ndarray, np.ndarray]:
    """head [F, A, 5 + C] -> (boxes float32 [F, P, 5], count int32 [F])."""
    return _decode(head, ratio, max_people, box_params(**kw) if params is None else params, nms_rounds)


def decode_boxes_full(head, ratio, max_people, params: BoxParams = None, **kw) -> Tuple[np.ndarray, np.ndarray]:
    return _decode(head, ratio, max_people, box_params(**kw) if params is None else params, nms_full)


# ------------------------------------------------------------------------------------------ 2 window
class Window(NamedTuple):
    cx: np.ndarray
    cy: np.ndarray
    ax: np.ndarray
    ay: np.ndarray
    valid: np.ndarray


def person_window(boxes: np.ndarray, out_h: int, out_w: int, padding) -> Window:
    """The windows of boxes [..., >= 4] = (x1, y1, x2, y2, ...)."""
    b = np.asarray(boxes, F32)
    half, padding = F32(0.5), F32(padding)
    with np.errstate(all="ignore"):
        cx, cy = (b[..., 0] + b[..., 2]) * half, (b[..., 1] + b[..., 3]) * half
        bw, bh = (b[..., 2] - b[..., 0]) * padding, (b[..., 3] - b[..., 1]) * padding
        aspect = F32(out_w) / F32(out_h)
        wide = bw > bh * aspect
        bh, bw = np.where(wide, bw / aspect, bh).astype(F32), np.where(wide, bw, bh * aspect).astype(F32)
        ax, ay = bw / F32(out_w), bh / F32(out_h)
        valid = np.isfinite(cx) & np.isfinite(cy) & np.isfinite(bw) & np.isfinite(bh) & np.isfinite(ax) & np.isfinite(ay) & (bw > 0) & (bh > 0)
    return Window(cx.astype(F32), cy.astype(F32), ax.astype(F32), ay.astype(F32), valid)


def present(boxes: np.ndarray, count: np.ndarray, out_h: int, out_w: int, padding) -> Tuple[Window, np.ndarray]:
    """The windows of boxes [F, P, 5] and which (f, p) are people: p < count[f] and a valid window."""
    w = person_window(boxes, out_h, out_w, padding)
    return w, w.valid & (np.arange(boxes.shape[1])[None, :] < np.asarray(count)[:, None])


# ------------------------------------------------------------------------------------------ 3 crops
def to_chw(frames: np.ndarray, layout: str) -> np.ndarray:
    """uint8 frames in a decoder layout -> [F, 3, H, W]."""
    frames = np.asarray(frames)
    if layout not in ("hwc", "pose", "chw") or frames.ndim != 4 or frames.dtype != np.uint8:
        raise ValueError(f"frames must be uint8 in layout 'hwc', 'pose' or 'chw', got {frames.dtype} {frames.shape} {layout!r}")
    return frames.transpose({"hwc": (0, 3, 1, 2), "pose": (1, 0, 2, 3), "chw": (0, 1, 2, 3)}[layout])


def crop_people(frames, boxes, count, layout: str = "hwc", params: CropParams = None, **kw) -> np.ndarray:
    """-> float32 [F * P, 3, out_h, out_w]."""
    p = crop_params(**kw) if params is None else params
    src = to_chw(frames, layout)
    boxes, count = np.asarray(boxes, F32), np.asarray(count, np.int32)
    nf, people = check_boxes(boxes.shape, count.shape)
    if src.shape[0] != nf or src.shape[1] != 3:
        raise ValueError(f"frames hold {src.shape[0]} frames of {src.shape[1]} channels, boxes {nf} frames")
    H, W = check_frame_size(src.shape[2:])
    win, here = present(boxes, count, p.out_h, p.out_w, p.padding)
    out = np.zeros((nf, people, 3, p.out_h, p.out_w), F32)
    half = F32(0.5)
    di = np.arange(p.out_w, dtype=F32) - F32(p.out_w) * half
    dj = np.arange(p.out_h, dtype=F32) - F32(p.out_h) * half
    mean, std = np.array(p.mean, F32).reshape(3, 1, 1), np.array(p.std, F32).reshape(3, 1, 1)
    for f, q in zip(*np.nonzero(here)):
        with np.errstate(all="ignore"):
            sx = (win.cx[f, q] + di * win.ax[f, q]).astype(F32)
            sy = (win.cy[f, q] + dj * win.ay[f, q]).astype(F32)
            in_x, in_y = (sx >= -1) & (sx <= W), (sy >= -1) & (sy <= H)
            sx, sy = np.where(in_x, sx, F32(0)), np.where(in_y, sy, F32(0))
            x0, y0 = np.floor(sx), np.floor(sy)
            fx, fy = (sx - x0).astype(F32)[None, None, :], (sy - y0).astype(F32)[None, :, None]
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        img = src[f, ::-1] if p.bgr else src[f]
        padded = np.zeros((3, H + 3, W + 3), F32)                     # rows / columns -1 .. H + 1 / W + 1
        padded[:, 1:H + 1, 1:W + 1] = img

        def tap(dy, dx):
            return padded[:, (y0 + 1 + dy)[:, None], (x0 + 1 + dx)[None, :]]
        a = tap(0, 0) + (tap(0, 1) - tap(0, 0)) * fx
        b = tap(1, 0) + (tap(1, 1) - tap(1, 0)) * fx
        v = a + (b - a) * fy
        v = np.where((in_y[:, None] & in_x[None, :])[None], v, F32(0)).astype(F32)
        out[f, q] = (v - mean) / std
    return out.reshape(nf * people, 3, p.out_h, p.out_w)


# ------------------------------------------------------------------------------------------ 4 keypoints
def first_max(v: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(index, value) along the last axis: the first index of the maximum over the non-NaN entries; (0, -inf) without any."""
    v = np.asarray(v).astype(F32)                               # float16 widens exactly
    clean = np.where(np.isnan(v), F32(-np.inf), v)
    idx = np.argmax(clean, -1)                                  # the first index of the maximum; +0 and -0 compare equal
    return idx, np.take_along_axis(clean, idx[..., None], -1)[..., 0]


def decode_simcc(simcc_x, simcc_y, boxes, count, frame_size, params: SimccParams = None, **kw) -> np.ndarray:
    """-> float32 [F, P, 134, 3]."""
    p = simcc_params(**kw) if params is None else params
    boxes, count = np.asarray(boxes, F32), np.asarray(count, np.int32)
    nf, people = check_boxes(boxes.shape, count.shape)
    H, W = check_frame_size(frame_size)
    simcc_x, simcc_y = np.asarray(simcc_x), np.asarray(simcc_y)
    check_simcc(simcc_x.shape, simcc_y.shape, nf * people)
    win, here = present(boxes, count, p.out_h, p.out_w, p.padding)
    ix, mx = first_max(simcc_x.reshape(nf, people, SIMCC_POINTS, -1))
    iy, my = first_max(simcc_y.reshape(nf, people, SIMCC_POINTS, -1))
    half = F32(0.5)
    with np.errstate(all="ignore"):
        s = np.where(mx < my, mx, my).astype(F32)
        valid = here[..., None] & np.isfinite(s) & (s > 0)
        u, v = ix.astype(F32) / p.split_ratio, iy.astype(F32) / p.split_ratio
        x = win.cx[..., None] + (u - F32(p.out_w) * half) * win.ax[..., None]
        y = win.cy[..., None] + (v - F32(p.out_h) * half) * win.ay[..., None]
        if p.normalized:
            x, y = x / F32(W), y / F32(H)
        pts = np.where(valid[..., None], np.stack([x, y, s], -1), MARKER).astype(F32)            # [F, P, 133, 3]
        both = valid[..., 5] & valid[..., 6] & (s[..., 5] > p.neck_threshold) & (s[..., 6] > p.neck_threshold)
        neck = np.stack([(pts[..., 5, 0] + pts[..., 6, 0]) * half, (pts[..., 5, 1] + pts[..., 6, 1]) * half, np.ones_like(s[..., 0])], -1)
        neck = np.where(both[..., None], neck, MARKER).astype(F32)
    tmp = np.concatenate([pts[..., :17, :], neck[..., None, :], pts[..., 17:, :]], -2)
    return np.ascontiguousarray(tmp[..., p.order.astype(np.int64), :])


# ------------------------------------------------------------------------------------------ the letterbox and the whole chain
def letterbox_ratio(frame_size, input_size) -> np.float32:
    """fp32 min(in_h / H, in_w / W), each quotient an fp32 division."""
    (H, W), (in_h, in_w) = check_frame_size(frame_size), input_size
    return min(F32(in_h) / F32(H), F32(in_w) / F32(W))


def letterbox_size(frame_size, ratio) -> Tuple[int, int]:
    """(int(H * r), int(W * r)), the products in fp32, at least 1 and at most the input size by construction."""
    return max(int(F32(frame_size[0]) * ratio), 1), max(int(F32(frame_size[1]) * ratio), 1)


def letterbox(frames, layout: str, input_size=INPUT_SIZE, fill=LETTERBOX_FILL) -> Tuple[np.ndarray, np.float32]:
    """(float32 [F, 3, in_h, in_w] of values 0..255, ratio): the frames stretched to `letterbox_size` by
    `resize_reference.resize` (Pillow's antialiased bilinear, not cv2.resize) in the top-left corner, `fill` elsewhere."""
    from . import resize_reference
    src = to_chw(frames, layout)
    ratio = letterbox_ratio(src.shape[2:], input_size)
    nh, nw = letterbox_size(src.shape[2:], ratio)
    small = resize_reference.resize(np.ascontiguousarray(src.transpose(0, 2, 3, 1)), (nh, nw), "bilinear")
    x = np.full((src.shape[0], 3, input_size[0], input_size[1]), fill, F32)
    x[:, :, :nh, :nw] = small.transpose(0, 3, 1, 2)
    return x, ratio


class Estimate(NamedTuple):
    keypoints: np.ndarray
    boxes: np.ndarray
    count: np.ndarray


def estimate(frames, layout, head, simcc, max_people, box: BoxParams, crop: CropParams, simcc_p: SimccParams) -> Estimate:
    """The chain on the host with the networks' outputs given: `head` of the letterboxed frames and `simcc(crops)` ->
    (simcc_x, simcc_y)."""
    src = to_chw(frames, layout)
    size = src.shape[2:]
    boxes, count = decode_boxes(head, letterbox_ratio(size, (box.in_h, box.in_w)), max_people, box)
    sx, sy = simcc(crop_people(frames, boxes, count, layout, crop))
    return Estimate(decode_simcc(sx, sy, boxes, count, size, simcc_p), boxes, count)
