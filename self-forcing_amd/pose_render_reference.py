"""The definition of the pose renderer's pixels (numpy, no GPU): DWPose whole-body keypoints -> skeleton frames.

The reference has no renderer: its `dwpose_data` arrives already drawn, in the DWPose style of UniAnimate-DiT (limbs as
filled ellipses dimmed to 60 %, joints as discs, hands as coloured edges and blue discs, faces as white discs).  These are
THIS PROJECT'S definitions in that style, in exact integer arithmetic, so that the device (csrc/pose_render.hip) and this
file agree to the bit.  They are not OpenCV's bits: OpenCV is not a dependency and its rasteriser is not restated here.
What differs from a cv2 drawing: boundary pixels (cv2.ellipse2Poly / fillConvexPoly and cv2.circle round their outlines
their own way), and hand edges, which are capsules of half-width 1 here -- three pixels wide on an axis -- where
cv2.line(thickness=2) draws two or three.  The dimming is `c * 3 // 5` of the limb's colour instead of `canvas * 0.6`
after all limbs, which is the same number for every palette entry (all multiples of 5).

keypoints  float32 [F, P, 134, 3] = (x, y, score) in DWPose's whole-body order: 0-17 the OpenPose-18 body, 18-23 feet
           (ignored), 24-91 the 68 face points, 92-112 the left hand, 113-133 the right hand.  [F, 134, 3] is P = 1.
pixel      normalized: X = int(x * W), Y = int(y * H), one fp32 multiply and a truncation; else X = int(x), Y = int(y).
valid      x, y, score finite; score >= score_threshold (compared in fp32); x >= 0 and y >= 0 (DWPose marks a missing
           point with -1); X <= 8191 and Y <= 8191.
Pixel centres are integer (px, py); later primitives overwrite earlier ones; the background is 0.
  limb      between valid P0, P1: the ellipse with centre at the midpoint and semi-axes (length / 2, 4).  d = P1 - P0,
            L2 = d.d, q = 2 p - (P0 + P1), u = q.d, v = q.x d.y - q.y d.x; inside iff v^2 <= 64 L2 and u^2 <= L2^2 and
            64 u^2 + v^2 L2 <= 64 L2^2 (the first two are implied by the third and keep it inside int64).  L2 == 0: nothing.
  disc      radius r at a valid point: dx^2 + dy^2 <= r^2 + r.
  hand edge between valid P0, P1, a capsule of half-width 1: s = (p - P0).d, c = (p - P0) x d; s <= 0: |p - P0|^2 <= 1;
            s >= L2: |p - P1|^2 <= 1; else c^2 <= L2.
Order (`primitives`): the 17 limbs (limb-major, person-minor) in LIMB_COLORS; the 18 body joints (joint-major,
person-minor), r = 4, in COLORS; the hands per person, left then right, each 20 edges in HAND_EDGE_COLORS then 21 discs
r = 4 in (0, 0, 255); the faces per person, 68 discs r = 3 in white.  185 primitives per person.
With 1 <= H, W <= 4096 and coordinates <= 8191 every expression fits int64 (the kernel uses int32 where that is enough).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import jpeg_reference as jr

KEYPOINTS = 134
MAX_PEOPLE = 8                 # SF_POSE_RENDER_MAX_PEOPLE
MAX_SIZE = 4096                # SF_POSE_RENDER_MAX_SIZE: H and W
MAX_COORD = 8191               # SF_POSE_RENDER_MAX_COORD: a point beyond it is invalid
PRIMS_PER_PERSON = 185
LIMB, DISC, EDGE = 0, 1, 2     # primitive kinds, the kernel's codes

LIMBS = ((1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 0), (0, 14), (14, 16), (0, 15),
         (15, 17))
COLORS = ((255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0), (0, 255, 85), (0, 255, 170),
          (0, 255, 255), (0, 170, 255), (0, 85, 255), (0, 0, 255), (85, 0, 255), (170, 0, 255), (255, 0, 255), (255, 0, 170), (255, 0, 85))
LIMB_COLORS = tuple(tuple(c * 3 // 5 for c in rgb) for rgb in COLORS[:17])
HAND_EDGES = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12), (0, 13), (13, 14), (14, 15),
              (15, 16), (0, 17), (17, 18), (18, 19), (19, 20))
# int(255 * channel) of colorsys.hsv_to_rgb(e / 20, 1, 1), e = 0..19
HAND_EDGE_COLORS = ((255, 0, 0), (255, 76, 0), (255, 153, 0), (255, 229, 0), (203, 255, 0), (127, 255, 0), (51, 255, 0), (0, 255, 25), (0, 255, 102),
                    (0, 255, 178), (0, 255, 255), (0, 178, 255), (0, 102, 255), (0, 25, 255), (50, 0, 255), (127, 0, 255), (204, 0, 255),
                    (255, 0, 229), (255, 0, 152), (255, 0, 76))
HAND_COLOR = (0, 0, 255)
FACE_COLOR = (255, 255, 255)
JOINT_RADIUS, HAND_RADIUS, FACE_RADIUS = 4, 4, 3
FACE0, HANDS0 = 24, (92, 113)
LAYOUTS = ("hwc", "pose", "chw")


def check_size(size) -> Tuple[int, int]:
    if len(size) != 2 or any(int(v) != v for v in size) or min(size) < 1 or max(size) > MAX_SIZE:
        raise ValueError(f"size must be (height, width), both 1..{MAX_SIZE}, got {size!r}")
    return int(size[0]), int(size[1])


def check_threshold(score_threshold) -> float:
    t = float(score_threshold)
    if not np.isfinite(t):
        raise ValueError(f"score_threshold must be finite, got {score_threshold!r}")
    return t


def check_keypoints_shape(shape: Sequence[int]) -> Tuple[int, int]:
    """(F, P) of a keypoint array's shape, [F, P, 134, 3] or [F, 134, 3]."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 3:
        shape = (shape[0], 1) + shape[1:]
    if len(shape) != 4 or shape[2:] != (KEYPOINTS, 3) or shape[0] < 1 or not 1 <= shape[1] <= MAX_PEOPLE:
        raise ValueError(f"keypoints must be [F, P, {KEYPOINTS}, 3] or [F, {KEYPOINTS}, 3] with F >= 1 and 1 <= P <= {MAX_PEOPLE}, got {shape}")
    return shape[0], shape[1]


def as_source(keypoints) -> np.ndarray:
    """Keypoints [F, P, 134, 3] or [F, 134, 3] -> float32 [F, P, 134, 3]."""
    k = np.asarray(keypoints, dtype=np.float32)
    f, people = check_keypoints_shape(k.shape)
    return k.reshape(f, people, KEYPOINTS, 3)


def quantize(keypoints: np.ndarray, size: Tuple[int, int], normalized: bool = True, score_threshold: float = 0.3):
    """float32 [..., 3] -> (X int64 [...], Y int64 [...], valid bool [...]); X and Y are 0 where the point is invalid."""
    k = np.asarray(keypoints, dtype=np.float32)
    h, w = size
    x, y, s = k[..., 0], k[..., 1], k[..., 2]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(s)
    ok &= np.where(ok, s, 0) >= np.float32(score_threshold)
    ok &= (np.where(ok, x, 0) >= 0) & (np.where(ok, y, 0) >= 0)
    with np.errstate(over="ignore"):
        px = np.where(ok, x, 0) * (np.float32(w) if normalized else np.float32(1))          # one fp32 multiply
        py = np.where(ok, y, 0) * (np.float32(h) if normalized else np.float32(1))
    ok &= (px < np.float32(MAX_COORD + 1)) & (py < np.float32(MAX_COORD + 1))               # trunc(p) <= 8191; inf fails
    return np.where(ok, px, 0).astype(np.int64), np.where(ok, py, 0).astype(np.int64), ok


def primitives(X: np.ndarray, Y: np.ndarray, valid: np.ndarray) -> List[tuple]:
    """One frame's primitives in painter's order from quantised points [P, 134]: (kind, x0, y0, x1, y1, r, rgb).  Invalid
    ones are left out (a limb of length 0 too); discs have (x1, y1) = (x0, y0)."""
    people = X.shape[0]
    out: List[tuple] = []

    def edge(kind, p, a, b, rgb):
        if valid[p, a] and valid[p, b] and not (kind == LIMB and X[p, a] == X[p, b] and Y[p, a] == Y[p, b]):
            out.append((kind, int(X[p, a]), int(Y[p, a]), int(X[p, b]), int(Y[p, b]), 0, rgb))

    def disc(p, a, r, rgb):
        if valid[p, a]:
            out.append((DISC, int(X[p, a]), int(Y[p, a]), int(X[p, a]), int(Y[p, a]), r, rgb))

    for i, (a, b) in enumerate(LIMBS):
        for p in range(people):
            edge(LIMB, p, a, b, LIMB_COLORS[i])
    for j in range(18):
        for p in range(people):
            disc(p, j, JOINT_RADIUS, COLORS[j])
    for p in range(people):
        for base in HANDS0:
            for e, (a, b) in enumerate(HAND_EDGES):
                edge(EDGE, p, base + a, base + b, HAND_EDGE_COLORS[e])
            for j in range(21):
                disc(p, base + j, HAND_RADIUS, HAND_COLOR)
    for p in range(people):
        for j in range(68):
            disc(p, FACE0 + j, FACE_RADIUS, FACE_COLOR)
    return out


def inside(kind: int, x0: int, y0: int, x1: int, y1: int, r: int, px: np.ndarray, py: np.ndarray) -> np.ndarray:
    """The coverage test of one primitive at the integer pixel centres (px, py) (int64 arrays that broadcast)."""
    px, py = px.astype(np.int64), py.astype(np.int64)
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    if kind == DISC:
        ex, ey = px - x0, py - y0
        return ex * ex + ey * ey <= r * r + r
    if kind == LIMB:
        if L2 == 0:
            return np.zeros(np.broadcast(px, py).shape, bool)
        qx, qy = 2 * px - (x0 + x1), 2 * py - (y0 + y1)
        u, v = qx * dx + qy * dy, qx * dy - qy * dx
        first = (v * v <= 64 * L2) & (u * u <= L2 * L2)
        u, v = np.where(first, u, 0), np.where(first, v, 0)                    # the third test only where it fits int64
        return first & (64 * u * u + v * v * L2 <= 64 * L2 * L2)
    ex, ey = px - x0, py - y0
    s, c = ex * dx + ey * dy, ex * dy - ey * dx
    fx, fy = px - x1, py - y1
    return np.where(s <= 0, ex * ex + ey * ey <= 1, np.where(s >= L2, fx * fx + fy * fy <= 1, c * c <= L2))


def extent(kind: int, x0: int, y0: int, x1: int, y1: int, r: int) -> Tuple[int, int, int, int]:
    """(xmin, ymin, xmax, ymax), inclusive: a box no pixel of the primitive lies outside (the ellipse reaches at most
    |d.x| / 2 + 4 from its centre along x; the kernel tests the same box against its tiles)."""
    pad = 4 if kind == LIMB else (r if kind == DISC else 1)
    return min(x0, x1) - pad, min(y0, y1) - pad, max(x0, x1) + pad, max(y0, y1) + pad


def render(keypoints, size: Sequence[int], layout: str = "hwc", dtype=np.uint8, normalized: bool = True, score_threshold: float = 0.3) -> np.ndarray:
    """keypoints [F, P, 134, 3] or [F, 134, 3] -> frames in `layout` ("hwc" [F, H, W, 3], "pose" [3, F, H, W], "chw"
    [F, 3, H, W]); dtype np.uint8 or np.float32 (= jpeg_reference.to_float of the uint8 frames).  bfloat16 is torch's:
    round the float32 result with `torch.from_numpy(...).to(torch.bfloat16)`."""
    h, w = check_size(size)
    thr = check_threshold(score_threshold)
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
    if np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise ValueError(f"dtype must be uint8 or float32, got {dtype}")
    k = np.asarray(keypoints, dtype=np.float32)
    frames, people = check_keypoints_shape(k.shape)
    k = k.reshape(frames, people, KEYPOINTS, 3)
    X, Y, ok = quantize(k, (h, w), normalized, thr)
    out = np.zeros((frames, h, w, 3), np.uint8)
    for f in range(frames):
        for kind, x0, y0, x1, y1, r, rgb in primitives(X[f], Y[f], ok[f]):
            bx0, by0, bx1, by1 = extent(kind, x0, y0, x1, y1, r)
            bx0, by0, bx1, by1 = max(bx0, 0), max(by0, 0), min(bx1, w - 1), min(by1, h - 1)
            if bx0 > bx1 or by0 > by1:
                continue
            m = inside(kind, x0, y0, x1, y1, r, np.arange(bx0, bx1 + 1)[None, :], np.arange(by0, by1 + 1)[:, None])
            out[f, by0:by1 + 1, bx0:bx1 + 1][m] = rgb
    if layout == "pose":
        out = out.transpose(3, 0, 1, 2)
    elif layout == "chw":
        out = out.transpose(0, 3, 1, 2)
    out = np.ascontiguousarray(out)
    return out if np.dtype(dtype) == np.dtype(np.uint8) else jr.to_float(out)
