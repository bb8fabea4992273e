"""Host-side tests of the pose renderer (no GPU): the definition `pose_render_reference` on hand-computed pixels, its colour
tables and painter's order, the validity rules, the float outputs, a sanity check against an independent Pillow drawing of
the same skeletons, the argument checks of sf_pose_render_frames, the torch operator's fake implementation, and the
ValueErrors of `PoseRenderer`, `pose_render.pose_feed` and generate.py's keypoint file types that need no device."""
import colorsys
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import pose_render_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# DWPose's tables, typed here a second time: the Pillow drawing below and the table tests do not read the module's
LIMBS = [(1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 0), (0, 14), (14, 16), (0, 15), (15, 17)]
PALETTE = [(255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0), (0, 255, 85), (0, 255, 170), (0, 255, 255),
           (0, 170, 255), (0, 85, 255), (0, 0, 255), (85, 0, 255), (170, 0, 255), (255, 0, 255), (255, 0, 170), (255, 0, 85)]
HAND_EDGES = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12), (0, 13), (13, 14), (14, 15), (15, 16),
              (0, 17), (17, 18), (18, 19), (19, 20)]


def empty(frames=1, people=1):
    """keypoints with every point missing as DWPose marks it (-1), score 1"""
    k = np.full((frames, people, 134, 3), -1, np.float32)
    k[..., 2] = 1
    return k


def lit(img):
    """{(x, y)} of the pixels of one hwc frame that are not background"""
    ys, xs = np.nonzero(img.any(-1))
    return set(zip(xs.tolist(), ys.tolist()))


def mask(kind, x0, y0, x1, y1, r, h=40, w=40):
    return pr.inside(kind, x0, y0, x1, y1, r, np.arange(w)[None, :], np.arange(h)[:, None])


# ============================================================================================== the primitives, by hand
def test_limb_is_the_ellipse_with_semi_axes_half_length_and_4():
    m = mask(pr.LIMB, 10, 10, 20, 10, 0)
    assert m[10, 10] and m[14, 15] and m[6, 15] and m[10, 20]
    assert not m[10, 9] and not m[15, 15] and not m[10, 21] and not m[5, 15]
    # through the renderer: the limb's own pixels beside the two joint discs, in the dimmed colour
    k = empty()
    k[0, 0, 1], k[0, 0, 2] = (10, 10, 1), (20, 10, 1)
    img = pr.render(k, (40, 40), normalized=False)[0]
    assert tuple(img[14, 15]) == (153, 0, 0) and tuple(img[15, 15]) == (0, 0, 0) and tuple(img[10, 15]) == (153, 0, 0)
    assert tuple(img[10, 10]) == (255, 85, 0) and tuple(img[10, 20]) == (255, 170, 0)          # joints 1 and 2 over the limb's ends
    # the same ellipse turned by 90 degrees and reversed
    assert np.array_equal(mask(pr.LIMB, 10, 20, 10, 10, 0), m.T)
    # a diagonal one is symmetric about its centre and about its axis
    d = mask(pr.LIMB, 8, 8, 30, 30, 0)
    assert np.array_equal(d, d.T) and np.array_equal(d[8:31, 8:31], d[8:31, 8:31][::-1, ::-1]) and d[19, 19] and d[8, 8] and not d[7, 7]
    assert d[16, 21] and not d[16, 22]                                                     # 5 / sqrt(2) = 3.5 from the axis is in, 6 / sqrt(2) = 4.2 out
    assert not mask(pr.LIMB, 10, 10, 10, 10, 0).any()                                      # L2 == 0


def test_discs():
    for x, y in ((20, 20), (0, 0)):
        m = lambda r: {(px - x, py - y) for px, py in zip(*np.nonzero(mask(pr.DISC, x, y, x, y, r).T))}     # noqa: E731
        if (x, y) == (20, 20):
            four, three = m(4), m(3)
            assert {(4, 0), (-4, 0), (0, 4), (0, -4), (4, 2), (-4, -2), (3, 3)} <= four
            assert not {(5, 0), (-5, 0), (4, 3), (4, -3), (-4, 3), (-4, -3), (0, 5)} & four
            assert {(3, 1), (3, -1), (-3, 1), (-3, -1), (3, 0)} <= three and not {(3, 2), (3, -2), (-3, 2), (-3, -2), (4, 0)} & three
            assert len(four) == 69 and len(three) == 37
        else:
            assert m(4) == {(a, b) for a in range(5) for b in range(5) if a * a + b * b <= 20}


def test_hand_edge_is_three_rows_with_one_pixel_more_at_each_end():
    m = mask(pr.EDGE, 10, 20, 17, 20, 0)
    want = {(x, y) for x in range(10, 18) for y in (19, 20, 21)} | {(9, 20), (18, 20)}
    assert {(int(x), int(y)) for y, x in zip(*np.nonzero(m))} == want
    assert np.array_equal(mask(pr.EDGE, 20, 10, 20, 17, 0), m.T) and np.array_equal(mask(pr.EDGE, 17, 20, 10, 20, 0), m)
    # a diagonal: |c| <= |d| keeps the pixels within one pixel of the axis
    d = mask(pr.EDGE, 5, 5, 15, 15, 0)
    assert d[10, 10] and d[10, 11] and d[11, 10] and not d[10, 12] and d[5, 4] and not d[4, 4] and d[15, 16] and not d[16, 16]


def test_the_box_holds_every_pixel_of_its_primitive():
    rng = np.random.default_rng(5)
    for _ in range(200):
        kind = int(rng.integers(0, 3))
        x0, y0, x1, y1 = (int(v) for v in rng.integers(20, 100, 4))
        r = int(rng.integers(3, 5))
        if kind == pr.DISC:
            x1, y1 = x0, y0
        m = mask(kind, x0, y0, x1, y1, r, 120, 120)
        bx0, by0, bx1, by1 = pr.extent(kind, x0, y0, x1, y1, r)
        ys, xs = np.nonzero(m)
        if len(xs):
            assert bx0 <= xs.min() and xs.max() <= bx1 and by0 <= ys.min() and ys.max() <= by1, (kind, x0, y0, x1, y1, r)


def test_the_largest_coordinates_stay_inside_int64():
    """Points at the corners of the coordinate range against the far corner of the largest frame: python's unbounded integers
    and the int64 arithmetic agree."""
    for x0, y0, x1, y1 in ((0, 0, 8191, 8191), (8191, 0, 0, 8191), (8191, 8191, 0, 1)):
        for px, py in ((4095, 4095), (0, 4095), (4095, 0), (0, 0), (2048, 2047)):
            dx, dy = x1 - x0, y1 - y0
            L2 = dx * dx + dy * dy
            qx, qy = 2 * px - (x0 + x1), 2 * py - (y0 + y1)
            u, v = qx * dx + qy * dy, qx * dy - qy * dx
            want = 64 * u * u + v * v * L2 <= 64 * L2 * L2
            assert bool(pr.inside(pr.LIMB, x0, y0, x1, y1, 0, np.array([px]), np.array([py]))[0]) == want
            assert max(abs(u), abs(v)) < 2 ** 31 and L2 < 2 ** 31                  # what the kernel keeps in int32


# ============================================================================================== colours and order
def test_tables():
    assert list(pr.LIMBS) == LIMBS and list(pr.COLORS) == PALETTE and list(pr.HAND_EDGES) == HAND_EDGES
    assert list(pr.HAND_EDGE_COLORS) == [tuple(int(255 * c) for c in colorsys.hsv_to_rgb(e / 20, 1, 1)) for e in range(20)]
    assert pr.HAND_EDGE_COLORS[1] == (255, 76, 0)
    assert list(pr.LIMB_COLORS) == [tuple(c * 3 // 5 for c in rgb) for rgb in PALETTE[:17]]
    assert all(c % 5 == 0 for rgb in PALETTE for c in rgb)                          # so c * 3 // 5 == c * 0.6 exactly
    assert pr.PRIMS_PER_PERSON == 17 + 18 + 2 * (20 + 21) + 68 == 185
    k = np.random.default_rng(0).random((1, 3, 134, 3)).astype(np.float32)
    k[..., 2] = 1
    X, Y, ok = pr.quantize(k, (64, 64))
    assert ok.all() and len(pr.primitives(X[0], Y[0], ok[0])) == 3 * 185           # (random points: no limb of length 0)


def test_painters_order():
    k = empty(1, 2)
    k[0, 0, 1], k[0, 0, 2] = (10, 10, 1), (30, 10, 1)                       # a limb and its two joints
    k[0, 0, 92], k[0, 0, 24] = (20, 30, 1), (20, 30, 1)                     # a hand point and a face point on one spot
    k[0, 1, 113], k[0, 0, 30] = (40, 30, 1), (42, 30, 1)                    # person 1's hand point beside person 0's face point
    img = pr.render(k, (48, 64), normalized=False)[0]
    assert tuple(img[10, 10]) == PALETTE[1] and tuple(img[10, 30]) == PALETTE[2] and tuple(img[10, 20]) == (153, 0, 0)   # joints over the limb
    assert tuple(img[30, 20]) == (255, 255, 255) and tuple(img[30, 24]) == (0, 0, 255)      # the face disc (r = 3) over the hand disc (r = 4)
    assert tuple(img[30, 40]) == (255, 255, 255) and tuple(img[30, 38]) == (0, 0, 255)      # the class decides, not the person
    # limb-major: limb 1 (points 1-5) lies over limb 0 (points 1-2) whichever person holds which
    for first, second in ((0, 1), (1, 0)):
        two = empty(1, 2)
        two[0, first, 1], two[0, first, 2], two[0, second, 1], two[0, second, 5] = (10, 10, 1), (30, 10, 1), (20, 0, 1), (20, 20, 1)
        img = pr.render(two, (48, 64), normalized=False)[0]
        assert tuple(img[10, 20]) == (153, 51, 0) and tuple(img[10, 15]) == (153, 0, 0) and tuple(img[15, 20]) == (153, 51, 0)
    # joint-major: joint 4 lies over joint 3 whichever person holds which
    for first, second in ((0, 1), (1, 0)):
        two = empty(1, 2)
        two[0, first, 3], two[0, second, 4] = (20, 20, 1), (22, 20, 1)
        assert tuple(pr.render(two, (40, 40), normalized=False)[0][20, 21]) == PALETTE[4]


def test_person_one_lies_over_person_zero_within_a_class():
    """The hands are painted person by person: person 1's hand EDGE lies over person 0's hand DISC, and person 0's edge under
    person 1's disc, while within one person the discs lie over the edges."""
    k = empty(1, 2)
    k[0, 1, 92], k[0, 1, 93] = (10, 20, 1), (30, 20, 1)            # person 1: hand edge 0 (red) along row 20
    k[0, 0, 100] = (20, 20, 1)                                     # person 0: a hand disc in its way
    img = pr.render(k, (40, 40), normalized=False)[0]
    assert tuple(img[20, 20]) == (255, 0, 0) and tuple(img[23, 20]) == (0, 0, 255) and tuple(img[20, 10]) == (0, 0, 255)
    img = pr.render(k[:, ::-1], (40, 40), normalized=False)[0]     # the people swapped: the disc is person 1's now
    assert tuple(img[20, 20]) == (0, 0, 255) and tuple(img[20, 25]) == (255, 0, 0)
    one = empty()
    one[0, 0, 92], one[0, 0, 93], one[0, 0, 100] = (10, 20, 1), (30, 20, 1), (20, 20, 1)
    assert tuple(pr.render(one, (40, 40), normalized=False)[0][20, 20]) == (0, 0, 255)
    # the same joint of two people: both discs are there
    both = empty(1, 2)
    both[0, 0, 3], both[0, 1, 3] = (20, 20, 1), (22, 20, 1)
    assert lit(pr.render(both, (40, 40), normalized=False)[0]) == {(x, y) for x in range(40) for y in range(40)
                                                                  if min((x - 20) ** 2, (x - 22) ** 2) + (y - 20) ** 2 <= 20}


def test_every_colour_is_in_the_palette():
    k = np.random.default_rng(3).random((2, 3, 134, 3)).astype(np.float32)
    img = pr.render(k, (96, 160))
    allowed = {(0, 0, 0), (0, 0, 255), (255, 255, 255)} | set(PALETTE) | set(pr.LIMB_COLORS) | set(pr.HAND_EDGE_COLORS)
    seen = {tuple(c) for c in np.unique(img.reshape(-1, 3), axis=0).tolist()}
    assert seen <= allowed and len(seen) > 30


# ============================================================================================== validity
def test_invalid_points_draw_nothing():
    base = empty()
    base[0, 0, 1], base[0, 0, 2] = (0.25, 0.25, 1), (0.5, 0.25, 1)
    assert lit(pr.render(base, (40, 40))[0])
    for bad in ((0.25, 0.25, 0.29), (-0.01, 0.25, 1), (0.25, -1, 1), (np.nan, 0.25, 1), (0.25, np.inf, 1), (0.25, 0.25, np.nan), (0.25, 0.25, -np.inf),
                (8192 / 40, 0.25, 1), (0.25, 1e30, 1), (3e38, 3e38, 1)):
        k = empty()
        k[0, 0, 1] = bad
        assert not lit(pr.render(k, (40, 40))[0]), bad
        k[0, 0, 2] = (0.5, 0.25, 1)                                 # the limb to a valid point is not drawn either: only joint 2's disc
        assert lit(pr.render(k, (40, 40))[0]) == {(20 + a, 10 + b) for a in range(-4, 5) for b in range(-4, 5) if a * a + b * b <= 20}, bad
    k = empty()
    k[0, 0, 1] = (0.25, 0.25, 0.3)                                  # the threshold itself counts, compared in fp32
    assert lit(pr.render(k, (40, 40))[0]) and not lit(pr.render(k, (40, 40), score_threshold=0.31)[0])
    assert lit(pr.render(base * np.float32([1, 1, 0.1]), (40, 40), score_threshold=0.05)[0])
    k = empty()
    k[0, 0, 1] = k[0, 0, 2] = (0.25, 0.25, 1)                       # a limb of length 0: the two discs alone
    k[0, 0, 2, 0] = 0.26                                            # (0.26 * 40 = 10.4 -> the same pixel)
    assert len(lit(pr.render(k, (40, 40))[0])) == 69
    X, Y, ok = pr.quantize(np.float32([[8191.9, 0.99, 1], [8192, 0, 1], [0.999, 0.999, 1]]), (7, 9), normalized=False)
    assert ok.tolist() == [True, False, True] and X.tolist() == [8191, 0, 0] and Y.tolist() == [0, 0, 0]
    X, Y, ok = pr.quantize(np.float32([[0.999, 0.5, 1], [1.0, 1.0, 1]]), (7, 9))
    assert ok.all() and X.tolist() == [8, 9] and Y.tolist() == [3, 7]        # int(x * W): 1.0 is the first pixel outside the frame


def test_points_beyond_the_edges_clip_in_and_feet_are_ignored():
    k = empty()
    k[0, 0, 1], k[0, 0, 2] = (30, 20, 1), (60, 20, 1)               # joint 2 lies 20 pixels right of a 40-pixel frame
    img = pr.render(k, (40, 40), normalized=False)[0]
    assert tuple(img[20, 39]) == (153, 0, 0) and tuple(img[20, 30]) == PALETTE[1]
    k[0, 0, 1] = (42, 41, 1)                                        # a disc centred just outside the corner reaches in
    assert lit(pr.render(k, (40, 40), normalized=False)[0]) >= {(39, 39)}
    feet = empty()
    feet[0, 0, 18:24] = (0.5, 0.5, 1)
    assert not lit(pr.render(feet, (40, 40))[0])
    assert np.array_equal(pr.render(empty()[:, 0], (8, 8)), np.zeros((1, 8, 8, 3), np.uint8))       # [F, 134, 3] is one person


# ============================================================================================== outputs
def test_layouts_and_float_outputs():
    k = np.random.default_rng(4).random((2, 2, 134, 3)).astype(np.float32)
    hwc = pr.render(k, (50, 70))
    assert hwc.shape == (2, 50, 70, 3) and hwc.dtype == np.uint8
    assert np.array_equal(pr.render(k, (50, 70), "pose"), hwc.transpose(3, 0, 1, 2))
    assert np.array_equal(pr.render(k, (50, 70), "chw"), hwc.transpose(0, 3, 1, 2))
    f = pr.render(k, (50, 70), "chw", np.float32)
    assert f.dtype == np.float32 and np.array_equal(f, jr.to_float(hwc.transpose(0, 3, 1, 2))) and f.min() == -1 and f.max() == 1
    for bad, what in ((dict(size=(0, 8)), "size"), (dict(size=(8, 4097)), "size"), (dict(size=(8,)), "size"), (dict(layout="nhwc"), "layout"),
                      (dict(dtype=np.float64), "dtype"), (dict(score_threshold=float("nan")), "score_threshold")):
        with pytest.raises(ValueError, match=what):
            pr.render(k, **{"size": (8, 8), **bad})
    for shape in ((2, 9, 134, 3), (2, 133, 3), (134, 3), (0, 1, 134, 3), (2, 0, 134, 3), (2, 1, 134, 2)):
        with pytest.raises(ValueError, match="keypoints must be"):
            pr.render(np.zeros(shape, np.float32), (8, 8))


# ============================================================================================== against an independent drawing
def skeletons(seed, frames, people):
    """Seeded skeletons in [0, 1]: body points anywhere in the middle 80 %, each hand and face a cluster, some points missing"""
    rng = np.random.default_rng(seed)
    k = np.zeros((frames, people, 134, 3), np.float32)
    k[..., :24, :2] = rng.uniform(0.1, 0.9, (frames, people, 24, 2))
    for lo, hi, spread in ((24, 92, 0.05), (92, 113, 0.06), (113, 134, 0.06)):
        centre = rng.uniform(0.15, 0.85, (frames, people, 1, 2))
        k[..., lo:hi, :2] = centre + rng.uniform(-spread, spread, (frames, people, hi - lo, 2))
    k[..., 2] = rng.uniform(0.2, 1.0, (frames, people, 134))             # about one point in eight is below the threshold
    return k


def pillow_render(k, h, w):
    """The same skeletons drawn by Pillow from the tables above: a 360-point ellipse polygon per limb, `ellipse` per disc,
    `line(width=2)` per hand edge.  An independent rasteriser, not a bit specification."""
    out = np.zeros((k.shape[0], h, w, 3), np.uint8)
    for f in range(k.shape[0]):
        im = Image.new("RGB", (w, h))
        d = ImageDraw.Draw(im)
        pt = lambda p, j: (int(k[f, p, j, 0] * np.float32(w)), int(k[f, p, j, 1] * np.float32(h)))     # noqa: E731
        ok = lambda p, j: k[f, p, j, 2] >= np.float32(0.3) and k[f, p, j, 0] >= 0 and k[f, p, j, 1] >= 0   # noqa: E731
        people = range(k.shape[1])
        for i, (a, b) in enumerate(LIMBS):
            for p in people:
                if ok(p, a) and ok(p, b):
                    (x0, y0), (x1, y1) = pt(p, a), pt(p, b)
                    cx, cy, half, ang = (x0 + x1) / 2, (y0 + y1) / 2, math.hypot(x1 - x0, y1 - y0) / 2, math.atan2(y1 - y0, x1 - x0)
                    poly = [(cx + half * math.cos(t) * math.cos(ang) - 4 * math.sin(t) * math.sin(ang),
                             cy + half * math.cos(t) * math.sin(ang) + 4 * math.sin(t) * math.cos(ang)) for t in np.linspace(0, 2 * math.pi, 360, False)]
                    if half > 0:
                        d.polygon(poly, fill=tuple(c * 3 // 5 for c in PALETTE[i]))
        disc = lambda c, r, rgb: d.ellipse([c[0] - r, c[1] - r, c[0] + r, c[1] + r], fill=rgb)      # noqa: E731
        for j in range(18):
            for p in people:
                if ok(p, j):
                    disc(pt(p, j), 4, PALETTE[j])
        for p in people:
            for base in (92, 113):
                for e, (a, b) in enumerate(HAND_EDGES):
                    if ok(p, base + a) and ok(p, base + b):
                        d.line([pt(p, base + a), pt(p, base + b)], fill=tuple(int(255 * c) for c in colorsys.hsv_to_rgb(e / 20, 1, 1)), width=2)
                for j in range(21):
                    if ok(p, base + j):
                        disc(pt(p, base + j), 4, (0, 0, 255))
        for p in people:
            for j in range(68):
                if ok(p, 24 + j):
                    disc(pt(p, 24 + j), 3, (255, 255, 255))
        out[f] = np.asarray(im)
    return out


# The share of all pixels in which `pose_render_reference.render` and the Pillow drawing above differ, measured on these seeded
# inputs with Pillow 12.2: 4.334 % at 96 x 160 (3 frames of one person; 12.6 % of the drawn pixels) and
# 2.146 % at 480 x 832 (2 frames of two people; 14.2 % of the drawn ones), all of them outline pixels and hand-edge widths.
# The bound is 1.5 x that share, because Pillow versions move boundary pixels; x and y swapped differ in 44 % and 23 %, a limb
# table rotated by one entry in 22 % and 12 %.
PILLOW_CASES = {(96, 160): (11, 3, 1, 0.04334), (480, 832): (12, 2, 2, 0.02146)}          # size -> (seed, frames, people, the measured share)


@pytest.mark.parametrize("size", list(PILLOW_CASES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_sanity_against_a_pillow_drawing(size):
    seed, frames, people, measured = PILLOW_CASES[size]
    k = skeletons(seed, frames, people)
    ours, theirs = pr.render(k, size), pillow_render(k, *size)
    differ = (ours != theirs).any(-1)
    drawn = ours.any(-1) | theirs.any(-1)
    share = differ.mean()
    print(f"pose renderer vs Pillow at {size[0]}x{size[1]}: {share:.5f} of all pixels differ, {differ.sum() / drawn.sum():.4f} of the drawn ones "
          f"({drawn.mean():.4f} of the frame is drawn)")
    assert drawn.mean() > 0.02
    assert share <= 1.5 * measured
    # what a gross error looks like on the same input: x and y swapped differs in far more
    swapped = pr.render(k[..., [1, 0, 2]], size)
    assert (swapped != theirs).any(-1).mean() > 4 * 1.5 * measured


# ============================================================================================== the C entry point
def test_c_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    assert lib.sf_abi_version() == 11 == sfa._lib.ABI_VERSION
    L = sfa._lib
    assert C.sizeof(L.PoseRenderArgs) == 2 * 8 + 7 * 4 + 4 == 48 and L.PoseRenderArgs.F.offset == 16 and L.PoseRenderArgs.score_threshold.offset == 44
    assert (L.POSE_RENDER_MAX_PEOPLE, L.POSE_RENDER_MAX_SIZE, L.POSE_RENDER_MAX_COORD) == (pr.MAX_PEOPLE, pr.MAX_SIZE, pr.MAX_COORD) == (8, 4096, 8191)
    header = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    for name, value in (("MAX_PEOPLE", 8), ("MAX_SIZE", 4096), ("MAX_COORD", 8191)):
        assert f"#define SF_POSE_RENDER_{name} {value}\n" in header
    ok = dict(keypoints=4096, out=4096, F=2, P=1, H=48, W=64, layout=1, dtype=0, normalized=1, score_threshold=0.3)

    def call(**kw):
        return lib.sf_pose_render_frames(C.byref(L.PoseRenderArgs(**{**ok, **kw})), None)
    err = lib.sf_last_error
    assert lib.sf_pose_render_frames(None, None) != 0 and b"null args" in err()
    for name in ("keypoints", "out"):
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
    for bad in (0, -1, 65536):
        assert call(F=bad) != 0 and b"F=%d frames" % bad in err()
    for bad in (0, 9, -2):
        assert call(P=bad) != 0 and b"P=%d people (1..8)" % bad in err()
    assert call(H=0) != 0 and b"frame 0x64" in err()
    assert call(H=4097) != 0 and b"frame 4097x64 (1..4096)" in err()
    assert call(W=0) != 0 and b"frame 48x0" in err()
    assert call(W=4097) != 0 and b"frame 48x4097" in err()
    assert call(layout=3) != 0 and b"unknown layout 3" in err()
    assert call(layout=-1) != 0 and b"unknown layout -1" in err()
    assert call(dtype=3) != 0 and b"unknown dtype 3" in err()
    assert call(dtype=-1) != 0 and b"unknown dtype -1" in err()
    assert call(normalized=2) != 0 and b"normalized=2" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(score_threshold=bad) != 0 and b"score_threshold must be finite" in err()
    assert call(keypoints=4098) != 0 and b"aligned" in err()
    assert call(out=4104) != 0 and b"aligned" in err()


# ============================================================================================== the Python surface
def test_operator_schema_and_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert {"pose_render_frames", "pose_render_frames_out"} <= set(sfa.torch_ops.OPS)
    assert "!" not in str(torch.ops.sf_hip.pose_render_frames.default._schema)
    assert "Tensor(a0!) out" in str(torch.ops.sf_hip.pose_render_frames_out.default._schema)
    with FakeTensorMode():
        k = torch.empty(5, 2, 134, 3, device="cuda")
        for layout, shape in (("hwc", (5, 48, 64, 3)), ("pose", (3, 5, 48, 64)), ("chw", (5, 3, 48, 64))):
            o = torch.ops.sf_hip.pose_render_frames(k, 48, 64, layout, torch.bfloat16)
            assert tuple(o.shape) == shape and o.dtype == torch.bfloat16
        assert torch.ops.sf_hip.pose_render_frames_out(torch.empty(3, 5, 48, 64, dtype=torch.uint8, device="cuda"), k, "pose") is None
        with pytest.raises(Exception, match="keypoints must be"):
            torch.ops.sf_hip.pose_render_frames(torch.empty(5, 9, 134, 3, device="cuda"), 48, 64, "pose", torch.uint8)
        with pytest.raises(Exception, match="layout"):
            torch.ops.sf_hip.pose_render_frames(k, 48, 64, "nhwc", torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        torch.ops.sf_hip.pose_render_frames(torch.zeros(1, 1, 134, 3), 8, 8, "pose", torch.uint8)


def test_pose_renderer_checks_that_need_no_device():
    assert sfa.PoseRenderer is sfa.pose_render.PoseRenderer and "PoseRenderer" in sfa.__all__ and "pose_render_reference" in sfa.__all__
    r = sfa.PoseRenderer()
    k = np.zeros((2, 1, 134, 3), np.float32)
    for size in ((0, 40), (24, -1), (24,), (24.5, 40), (4097, 8)):
        with pytest.raises(ValueError, match="size"):
            r.render(k, size)
    with pytest.raises(ValueError, match="layout"):
        r.render(k, (24, 40), layout="nhwc")
    with pytest.raises(ValueError, match="dtype"):
        r.render(k, (24, 40), dtype=torch.float16)
    with pytest.raises(ValueError, match="score_threshold"):
        r.render(k, (24, 40), score_threshold=float("inf"))
    for bad in (k[0, 0], np.zeros((2, 9, 134, 3), np.float32), np.zeros((2, 1, 133, 3), np.float32), np.zeros((0, 1, 134, 3), np.float32),
                torch.zeros(2, 134, 2)):
        with pytest.raises(ValueError, match="keypoints must be"):
            r.render(bad, (24, 40))
    with pytest.raises(ValueError, match="numbers"):
        r.render(np.zeros((2, 134, 3), object), (24, 40))
    with pytest.raises(ValueError, match="numbers"):
        r.render(torch.zeros(2, 134, 3, dtype=torch.bool), (24, 40))
    for kk in (k, torch.from_numpy(k), k[:, 0].tolist()):
        with pytest.raises(ValueError, match="no CPU fallback"):
            sfa.PoseRenderer(device="cpu").render(kk, (24, 40))
    with pytest.raises(ValueError, match="out must be"):
        r.render(k, (24, 40), out=torch.zeros(3, 2, 24, 40, dtype=torch.uint8))           # a host tensor


def test_pose_feed_checks_that_need_no_device():
    r = sfa.PoseRenderer(device="cpu")
    k = np.zeros((3, 1, 134, 3), np.float32)
    with pytest.raises(ValueError, match="frames_per_piece"):
        next(sfa.pose_render.pose_feed(k, r, (24, 40), 0))
    with pytest.raises(ValueError, match="size"):
        next(sfa.pose_render.pose_feed(k, r, (24,)))
    with pytest.raises(ValueError, match="score_threshold"):
        next(sfa.pose_render.pose_feed(k, r, (24, 40), score_threshold=float("nan")))
    with pytest.raises(ValueError, match="no CPU fallback"):                 # the first piece is rendered when it is asked for
        next(sfa.pose_render.pose_feed(k, r, (24, 40), 2))
    with pytest.raises(ValueError, match="keypoints must be"):
        next(sfa.pose_render.pose_feed(iter([np.zeros((134, 2), np.float32)]), r, (24, 40), 1))
    pulled = []

    def source():
        for i in range(5):
            pulled.append(i)
            yield k[0]
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2)
    assert pulled == []                                                      # nothing is read before a piece is asked for
    with pytest.raises(ValueError, match="no CPU fallback"):
        next(feed)
    assert pulled == [0, 1]


def test_generate_keypoint_file_types(tmp_path):
    sys.path.insert(0, ROOT)
    import generate
    k = np.random.default_rng(0).random((5, 2, 134, 3)).astype(np.float32)
    np.savez(tmp_path / "clip.npz", keypoints=k)
    np.save(tmp_path / "clip.npy", k[:, 0])
    np.savez(tmp_path / "ref.npz", keypoints=k[0])
    np.save(tmp_path / "ref.npy", k[0, 0])
    np.save(tmp_path / "dict.npy", {"dwpose_data": np.zeros((3, 1, 8, 8), np.uint8), "random_ref_dwpose": np.zeros((8, 8, 3), np.uint8)}, allow_pickle=True)
    np.savez(tmp_path / "other.npz", points=k)
    (tmp_path / "pose.pt").write_bytes(b"")
    (tmp_path / "clip.avi").write_bytes(b"")
    kinds = {n: generate.pose_file_kind(str(tmp_path / n)) for n in ("clip.npz", "clip.npy", "ref.npy", "dict.npy", "pose.pt", "clip.avi")}
    assert kinds == {"clip.npz": "keypoints", "clip.npy": "keypoints", "ref.npy": "keypoints", "dict.npy": "dict", "pose.pt": "dict", "clip.avi": "mjpeg"}
    assert np.array_equal(generate.read_keypoints(str(tmp_path / "clip.npz")), k)
    assert np.array_equal(generate.read_keypoints(str(tmp_path / "clip.npy")), k[:, :1])
    assert np.array_equal(generate.read_keypoints(str(tmp_path / "ref.npz"), one_frame=True), k[:1])
    assert np.array_equal(generate.read_keypoints(str(tmp_path / "ref.npy"), one_frame=True), k[:1, :1])
    with pytest.raises(SystemExit, match="one frame"):
        generate.read_keypoints(str(tmp_path / "clip.npz"), one_frame=True)
    with pytest.raises(SystemExit, match="no array 'keypoints'"):
        generate.read_keypoints(str(tmp_path / "other.npz"))
    d, ref = generate.load_pose(str(tmp_path / "dict.npy"))                   # the pickled dict is read as before
    assert tuple(d.shape) == (3, 1, 8, 8) and tuple(ref.shape) == (8, 8, 3)

    base = [sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", "c", "--data_path", "d", "--output_folder", "o", "--pose_random_init_seed", "0"]
    run = lambda *more: subprocess.run(base + list(more), capture_output=True, text=True)       # noqa: E731
    r = run("--pose_path", str(tmp_path / "clip.npz"))
    assert r.returncode == 2 and "--ref_pose_path" in r.stderr and "keypoints" in r.stderr
    r = run("--pose_path", str(tmp_path / "clip.npz"), "--ref_pose_path", str(tmp_path / "missing.npz"))
    assert r.returncode == 2 and "no such file" in r.stderr
    r = run("--pose_path", str(tmp_path / "clip.npy"), "--ref_pose_path", str(tmp_path / "pose.pt"))
    assert r.returncode == 2 and "keypoints (.npz / .npy array) expected" in r.stderr
    r = run("--pose_path", str(tmp_path / "clip.npz"), "--ref_pose_path", str(tmp_path / "ref.npz"), "--pose_resize", "cover")
    assert r.returncode == 2 and "--pose_resize" in r.stderr and "keypoints are drawn at the output size" in r.stderr
    r = run("--pose_path", str(tmp_path / "dict.npy"), "--ref_pose_path", str(tmp_path / "ref.npz"))
    assert r.returncode == 2 and "holds its own" in r.stderr
    r = run("--pose_path", str(tmp_path / "dict.npy"), "--pose_pixel_coords")
    assert r.returncode == 2 and "--pose_pixel_coords" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "Does not apply to keypoints" in " ".join(r.stdout.split())
