"""Host tests of the pose retargeter (no GPU): analytic properties of the definition `pose_retarget_reference` that do not
depend on how it is written (a similarity of the reference is recovered, bones keep their direction and take the fitted
length, a point moving linearly stays on its line, missing points follow the nearer-neighbour and fall-back rules), the
partition invariance of its stream, the C plan against its Python mirror, the argument checks of the C entry points through
ctypes (they return before any device call), the `ValueError`s of the Python surface and the `generate.py` flag errors."""
import ctypes as C
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_render_reference as pr
from self_forcing_amd import pose_retarget_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (480, 832)
F32 = np.float32
RATES = [(16, 16, 1, 1), (30, 16, 15, 8), (24, 16, 3, 2), (60, 16, 15, 4), (15, 16, 15, 16), ("30000/1001", 16, 1875, 1001)]


def person(rng, lo=(40.0, 40.0), hi=(792.0, 440.0)):
    """One person, every point valid, x and y uniform in a box inside 832 x 480 (pixels), scores in [0.5, 1]"""
    k = np.empty((134, 3), F32)
    k[:, 0], k[:, 1] = rng.uniform(lo[0], hi[0], 134), rng.uniform(lo[1], hi[1], 134)
    k[:, 2] = rng.uniform(0.5, 1.0, 134)
    return k


def skeleton(rng):
    """One person with plausible proportions, every point valid and inside 832 x 480: limbs of 25..50 px at random angles
    from a neck near the centre, feet, face and hands within 25 px of their anchors.  Limb ratios between two of these stay
    in [0.5, 2], so retargeted coordinates stay below 1024 in size and the tolerances below can be absolute."""
    k = np.empty((134, 3), F32)
    xy = np.zeros((134, 2))
    xy[1] = rng.uniform((330, 230), (500, 250))
    for a, b in pr.LIMBS:
        angle, length = rng.uniform(0, 2 * np.pi), rng.uniform(25, 50)
        xy[b] = xy[a] + length * np.array([np.cos(angle), np.sin(angle)])
    for lo, hi, anchor, _ in rr.ATTACHED:
        xy[lo:hi] = xy[anchor] + rng.uniform(-25, 25, (hi - lo, 2))
    k[:, :2], k[:, 2] = xy, rng.uniform(0.5, 1.0, 134)
    assert (k[:, :2] > 0).all()
    return k


def similar(rng, r):
    """S0 = (R - R[1]) / s + R[1] + d with s in [0.4, 2.5]; d also moves every point to a positive coordinate"""
    s = rng.uniform(0.4, 2.5)
    xy = (r[:, :2].astype(np.float64) - r[1, :2]) / s + r[1, :2]
    xy += np.maximum(0, -xy.min(0)) + rng.uniform(1, 60, 2)
    return np.concatenate([xy, r[:, 2:]], axis=1).astype(F32), s


def px(k, ref, **kw):
    """retarget in pixel units at SIZE"""
    return rr.retarget(k, ref, SIZE, normalized=False, **kw)


# ============================================================================================== the fit and the retarget
def test_a_similarity_of_the_reference_is_recovered():
    # measured with this file's reference: worst |out - R| over 300 draws = 1.1e-3 px (the construction of S0 rounds to
    # fp32 at coordinates up to about 3000, an ulp of 2.4e-4, and the chain adds up to four steps); the bound is 2^-7 px
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(300):
        r = person(rng)
        s0, _ = similar(rng, r)
        out = px(s0[None], r)
        assert out.shape == (1, 1, 134, 3) and out.dtype == F32 and np.array_equal(out[0, 0, :, 2], s0[:, 2])
        worst = max(worst, float(np.abs(out[0, 0, :, :2].astype(np.float64) - r[:, :2]).max()))
    print(f"similarity recovery: worst {worst:.3e} px")
    assert worst <= 2.0 ** -7


def limb_vectors(xy):
    xy = xy.astype(np.float64)
    return np.stack([xy[b] - xy[a] for a, b in pr.LIMBS])


def test_bones_take_the_fitted_length_and_keep_their_direction():
    # measured: worst relative length error 1.4e-6, worst |cross| / (|u| |v|) 2.7e-6 over 100 draws; the bound is 1e-5
    rng = np.random.default_rng(1)
    worst_len = worst_cross = 0.0
    for _ in range(100):
        r, s0, q = skeleton(rng), skeleton(rng), skeleton(rng)
        out = px(np.stack([s0, q])[:, None], r)
        p = rr.prepare(SIZE, normalized=False)
        f = rr.fit(rr.lift(s0, p.src_sx, p.src_sy, p.threshold), rr.lift(r, p.ref_sx, p.ref_sy, p.threshold))
        assert f.retarget
        for frame, src in ((0, s0), (1, q)):
            u, v = limb_vectors(out[frame, 0, :, :2]), limb_vectors(src[:, :2])
            lu, lv = np.hypot(u[:, 0], u[:, 1]), np.hypot(v[:, 0], v[:, 1])
            ratio = np.array([float(f.ratio[rr.GROUP_OF[e]]) for e in range(17)])
            worst_len = max(worst_len, float(np.abs(lu / (ratio * lv) - 1).max()))
            worst_cross = max(worst_cross, float(np.abs(u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]).max() / (lu * lv).min()))
            assert (np.einsum("ij,ij->i", u, v) > 0).all()                      # the same way round, not mirrored
    print(f"bone lengths: worst relative {worst_len:.3e}; directions: worst cross {worst_cross:.3e}")
    assert worst_len <= 1e-5 and worst_cross <= 1e-5


def test_frame_0_has_the_reference_lengths_when_symmetric_limbs_share_a_ratio():
    # S0 is R with every limb of group k shortened by its own factor c[k]: both members of a group then have the ratio
    # c[k], so frame 0 comes out with R's lengths (measured: 1.5e-6 relative; the bound is 1e-5)
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(50):
        r = skeleton(rng)
        c = rng.uniform(0.6, 1.8, len(rr.GROUPS))
        xy = r[:, :2].astype(np.float64).copy()
        for e, (a, b) in enumerate(pr.LIMBS):
            xy[b] = xy[a] + (r[b, :2].astype(np.float64) - r[a, :2]) / c[rr.GROUP_OF[e]]
        xy += np.maximum(0, -xy.min(0)) + 5
        s0 = np.concatenate([xy, r[:, 2:]], axis=1).astype(F32)
        out = px(s0[None], r)
        u, v = limb_vectors(out[0, 0, :, :2]), limb_vectors(r[:, :2])
        worst = max(worst, float(np.abs(np.hypot(u[:, 0], u[:, 1]) / np.hypot(v[:, 0], v[:, 1]) - 1).max()))
        assert np.abs(out[0, 0, :18, :2].astype(np.float64) - r[:18, :2]).max() < 2.0 ** -7      # and the body is R itself
    print(f"frame 0 lengths: worst relative {worst:.3e}")
    assert worst <= 1e-5


def test_attached_points_follow_their_anchor_at_their_ratio():
    rng = np.random.default_rng(3)
    r, s0, q = skeleton(rng), skeleton(rng), skeleton(rng)
    out = px(np.stack([s0, q])[:, None], r)[1, 0, :, :2].astype(np.float64)
    p = rr.prepare(SIZE, normalized=False)
    f = rr.fit(rr.lift(s0, p.src_sx, p.src_sy, p.threshold), rr.lift(r, p.ref_sx, p.ref_sy, p.threshold))
    table = {(18, 21): (13, f.g), (21, 24): (10, f.g), (24, 92): (0, f.ratio[7]), (92, 113): (7, f.ratio[2]), (113, 134): (4, f.ratio[2])}
    assert f.ratio[2] != f.ratio[7] != f.g
    for (lo, hi), (anchor, ratio) in table.items():
        want = out[anchor] + float(ratio) * (q[lo:hi, :2].astype(np.float64) - q[anchor, :2])
        assert np.abs(out[lo:hi] - want).max() < 2.0 ** -9, (lo, hi)                 # three roundings at coordinates below 2048
    # the hand ratio is the forearms', the face ratio nose-eye: the mean of the two sides
    length = lambda k, a, b: math.hypot(*(k[b, :2].astype(np.float64) - k[a, :2]))      # noqa: E731
    for grp, (e0, e1) in ((2, (3, 5)), (7, (13, 15))):
        mean = sum(length(r, *pr.LIMBS[e]) / length(s0, *pr.LIMBS[e]) for e in (e0, e1)) / 2
        assert abs(float(f.ratio[grp]) / mean - 1) < 1e-6
    total = sum(length(r, a, b) for a, b in pr.LIMBS) / sum(length(s0, a, b) for a, b in pr.LIMBS)
    assert abs(float(f.g) / total - 1) < 1e-6


# ============================================================================================== resampling
@pytest.mark.parametrize("source,target,num,den", RATES, ids=lambda v: str(v).replace("/", "_"))
def test_frame_count_and_linear_motion(source, target, num, den):
    assert rr.rate(source, target) == (num, den)
    for frames in (1, 2, 3, 7, 16, 31, 151):
        brute = sum(1 for j in range(frames * den + 2) if -((-j * num) // den) <= frames - 1)      # i1(j) = ceil(j num / den)
        assert rr.frames_out(frames, num, den) == ((frames - 1) * den) // num + 1 == brute
    frames = 31
    rng = np.random.default_rng(4)
    p0, v = rng.uniform(100, 300, (134, 2)), rng.uniform(-3, 20, (134, 2))         # coordinates stay below 1024
    k = np.ones((frames, 134, 3), F32)
    k[..., :2] = (p0 + v * np.arange(frames)[:, None, None]).astype(F32)
    out = px(k, k[0], source_fps=source, target_fps=target, align=False)
    assert out.shape == (rr.frames_out(frames, num, den), 1, 134, 3) and (out[..., 2] == 1).all()
    at = np.arange(len(out))[:, None, None] * (num / den)
    # the source itself is rounded to fp32 (half an ulp of 2^-14 each end), then three roundings: 2^-10 px holds both
    assert np.abs(out[:, 0, :, :2].astype(np.float64) - (p0 + v * at)).max() <= 2.0 ** -10
    copies = [j for j in range(len(out)) if (j * num) % den == 0]
    assert len(copies) >= 2 or den > frames
    for j in copies:
        assert np.array_equal(out[j, 0], k[j * num // den])                         # rem == 0: the bits of the source frame


def test_fps_forms_and_errors():
    assert rr.rate(30, 16) == rr.rate("30", "16") == rr.rate(Fraction(30), Fraction(16)) == rr.rate(" 60 / 2 ", 16) == (15, 8)
    assert rr.rate(Fraction(30000, 1001), 16) == (1875, 1001) and rr.rate(np.int64(24), 16) == (3, 2)
    assert rr.rate(65535, 1) == (65535, 1) and rr.rate(1, 65535) == (1, 65535)
    for bad in (0, -5, 30.0, "30.0", "a/b", "30/0", "", None, True, Fraction(0), "1/2/3"):
        with pytest.raises(ValueError, match="fps"):
            rr.rate(bad, 16)
        with pytest.raises(ValueError, match="fps"):
            rr.rate(16, bad)
    for bad in ((65536, 1), (1, 65536), ("65537/65536", 1)):
        with pytest.raises(ValueError, match="1..65535"):
            rr.rate(*bad)


# ============================================================================================== missing points
def test_one_missing_neighbour_takes_the_nearer_one_and_the_tie_goes_to_the_earlier():
    rng = np.random.default_rng(5)
    k = np.stack([skeleton(rng) for _ in range(10)])
    gone = lambda i, pt: k.__setitem__((i, pt), (-1, -1, 0))                             # noqa: E731
    # 30 -> 16 is 15/8: frame 1 sits at 1 + 7/8, 2 at 3 + 6/8, 4 at 7 + 4/8 (the tie), 5 at 9 + 3/8 (no frame 10: it does not exist)
    gone(1, 20), gone(2, 21)           # frame 1: a missing (b nearer: taken), b missing (a farther: invalid)
    gone(7, 30), gone(8, 31)           # frame 4, the tie: a missing -> invalid; b missing -> a taken
    gone(5, 40), gone(6, 40)           # frame 3 (5 + 5/8): both missing
    gone(4, 50)                        # frame 2 (3 + 6/8): a valid, b missing, b nearer -> invalid
    out = px(k[:, None], k[0], source_fps=30, align=False)[:, 0]
    assert len(out) == 5
    marker = np.array([-1, -1, 0], F32)
    assert np.array_equal(out[1, 20], k[2, 20]) and np.array_equal(out[1, 21], marker)
    assert np.array_equal(out[4, 30], marker) and np.array_equal(out[4, 31], k[7, 31])
    assert np.array_equal(out[3, 40], marker) and np.array_equal(out[2, 50], marker)
    mid = out[1, 22].astype(np.float64)                                                  # an untouched point: both valid
    want = k[1, 22].astype(np.float64) + 7 / 8 * (k[2, 22].astype(np.float64) - k[1, 22])
    assert np.abs(mid[:2] - want[:2]).max() < 2.0 ** -10 and out[1, 22, 2] == min(k[1, 22, 2], k[2, 22, 2])
    for bad in ((np.nan, 5, 1), (5, np.inf, 1), (5, 5, np.nan), (-0.5, 5, 1), (5, -1e-9, 1), (5, 5, 0.29)):
        one = k[:1].copy()
        one[0, 60] = bad
        assert np.array_equal(px(one[:, None], k[0], align=False)[0, 0, 60], marker), bad
    edge = k[:1].copy()
    edge[0, 60], edge[0, 61] = (0, 0, 0.3), (7, 7, np.nextafter(F32(0.3), F32(0)))       # at the threshold, and just below it
    got = px(edge[:, None], k[0], align=False)[0, 0]
    assert np.array_equal(got[60], edge[0, 60]) and np.array_equal(got[61], marker)


def test_no_neck_no_retarget():
    rng = np.random.default_rng(6)
    r, k = skeleton(rng), np.stack([skeleton(rng) for _ in range(4)])
    plain = px(k[:, None], r, source_fps=24, align=False)
    assert not np.array_equal(px(k[:, None], r, source_fps=24), plain)
    no_s0 = k.copy()
    no_s0[0, 1, 2] = 0.1                                                                 # the neck of S0 below the threshold
    assert np.array_equal(px(no_s0[:, None], r, source_fps=24), px(no_s0[:, None], r, source_fps=24, align=False))
    no_r = r.copy()
    no_r[1, 0] = -1
    assert np.array_equal(px(k[:, None], no_r, source_fps=24), plain)
    two = np.stack([k, no_s0], axis=1)                                                   # per person: person 1 has no anchor, person 0 has
    out = px(two, r, source_fps=24)
    assert np.array_equal(out[:, 0], px(k[:, None], r, source_fps=24)[:, 0])
    assert np.array_equal(out[:, 1], px(no_s0[:, None], r, source_fps=24, align=False)[:, 0])


def test_a_broken_chain_falls_back_to_the_similarity():
    rng = np.random.default_rng(7)
    r, s0, q = skeleton(rng), skeleton(rng), skeleton(rng)
    q[3] = (-1, -1, 0)                                                                   # the right elbow: wrist 4 loses its parent
    q[0, 2] = 0.0                                                                        # the nose: eyes 14, 15 and the face lose theirs
    out = px(np.stack([s0, q])[:, None], r)[1, 0]
    p = rr.prepare(SIZE, normalized=False)
    f = rr.fit(rr.lift(s0, p.src_sx, p.src_sy, p.threshold), rr.lift(r, p.ref_sx, p.ref_sy, p.threshold))
    sim = lambda pt: r[1, :2].astype(np.float64) + float(f.g) * (pt[:2].astype(np.float64) - s0[1, :2])      # noqa: E731
    marker = np.array([-1, -1, 0], F32)
    assert np.array_equal(out[3], marker) and np.array_equal(out[0], marker)
    for pt in (4, 14, 15, 24, 60, 91):
        assert np.abs(out[pt, :2] - sim(q[pt])).max() < 2.0 ** -9 and out[pt, 2] == q[pt, 2], pt
    want = out[4, :2].astype(np.float64) + float(f.ratio[2]) * (q[113:, :2].astype(np.float64) - q[4, :2])   # the hand hangs on the wrist
    assert np.abs(out[113:, :2] - want).max() < 2.0 ** -9
    want = out[14, :2].astype(np.float64) + float(f.ratio[8]) * (q[16, :2].astype(np.float64) - q[14, :2])   # the ear on the eye
    assert np.abs(out[16, :2] - want).max() < 2.0 ** -9
    no_neck = q.copy()
    no_neck[1] = (-1, -1, 0)                                                             # the neck missing in a LATER frame: its children use sim
    out = px(np.stack([s0, no_neck])[:, None], r)[1, 0]
    for pt in (2, 5, 8, 11):
        assert np.abs(out[pt, :2] - sim(no_neck[pt])).max() < 2.0 ** -9
    assert np.array_equal(out[1], marker)


def test_unusable_edges_and_group_ratios():
    rng = np.random.default_rng(8)
    r, s0 = skeleton(rng), skeleton(rng)
    p = rr.prepare(SIZE, normalized=False)
    lift = lambda k, ref=False: rr.lift(k, p.ref_sx if ref else p.src_sx, p.ref_sy if ref else p.src_sy, p.threshold)      # noqa: E731
    length = lambda k, a, b: math.hypot(*(k[b, :2].astype(np.float64) - k[a, :2]))      # noqa: E731
    full = rr.fit(lift(s0), lift(r, True))
    flat = s0.copy()
    flat[3, :2] = flat[2, :2]                                                            # limb 2 = (2, 3) has length 0 in S0: unusable
    f = rr.fit(lift(flat), lift(r, True))
    assert abs(float(f.ratio[1]) / (length(r, 5, 6) / length(flat, 5, 6)) - 1) < 1e-6    # group {2, 4}: its other member alone
    others = [e for e in range(17) if e != 2]
    g = sum(length(r, *pr.LIMBS[e]) for e in others) / sum(length(flat, *pr.LIMBS[e]) for e in others)
    assert abs(float(f.g) / g - 1) < 1e-6 and f.g != full.g and np.isfinite(f.ratio).all()
    none = s0.copy()
    none[3, 2] = none[6, 2] = 0.0                                                        # both elbows: limbs 2, 3, 4, 5 unusable
    f = rr.fit(lift(none), lift(r, True))
    assert f.ratio[1] == f.g and f.ratio[2] == f.g and f.ratio[0] == full.ratio[0] and f.retarget
    ref_gap = r.copy()
    ref_gap[6, 0] = np.nan                                                               # ... and a gap in the reference counts the same
    f = rr.fit(lift(s0), lift(ref_gap, True))
    assert abs(float(f.ratio[1]) / (length(r, 2, 3) / length(s0, 2, 3)) - 1) < 1e-6 and abs(float(f.ratio[2]) / (length(r, 3, 4) / length(s0, 3, 4)) - 1) < 1e-6
    # the hand then scales by g although its forearm is there in a later frame
    q = skeleton(rng)
    out = px(np.stack([none, q])[:, None], r)[1, 0, :, :2].astype(np.float64)
    f = rr.fit(lift(none), lift(r, True))
    assert np.abs(out[92:113] - (out[7] + float(f.g) * (q[92:113, :2].astype(np.float64) - q[7, :2]))).max() < 2.0 ** -9
    empty = np.full((134, 3), -1, F32)
    empty[1] = s0[1]                                                                     # only the neck: no usable edge, g = 1
    f = rr.fit(lift(empty), lift(r, True))
    assert f.g == 1 and all(v == 1 for v in f.ratio) and f.retarget


# ============================================================================================== lift, people
def test_lift_source_size_and_pixel_input():
    p = rr.prepare(SIZE)
    assert (p.src_sx, p.src_sy, p.ref_sx, p.ref_sy) == (832, 480, 832, 480) and (p.num, p.den, p.align) == (1, 1, True) and p.threshold == F32(0.3)
    p = rr.prepare(SIZE, source_size=(720, 1280))
    assert (p.src_sx, p.src_sy, p.ref_sx, p.ref_sy) == (F32(480 * 1280 / 720), 480, 832, 480)
    p = rr.prepare(SIZE, normalized=False, source_size=(720, 1280))
    assert (p.src_sx, p.src_sy, p.ref_sx, p.ref_sy) == (F32(480 / 720), F32(480 / 720), 1, 1)
    p = rr.prepare(SIZE, normalized=False)
    assert (p.src_sx, p.src_sy, p.ref_sx, p.ref_sy) == (1, 1, 1, 1)
    rng = np.random.default_rng(9)
    k = rng.uniform(0.05, 0.95, (3, 2, 134, 3)).astype(F32)
    k[..., 2] = 1
    out = rr.retarget(k, k[0], SIZE, align=False, source_size=(720, 1280))
    assert np.array_equal(out[..., 0], k[..., 0] * F32(480 * 1280 / 720)) and np.array_equal(out[..., 1], k[..., 1] * F32(480))
    out = rr.retarget(k * F32([1280, 720, 1]), k[0], SIZE, align=False, normalized=False, source_size=(720, 1280))
    assert np.array_equal(out[..., :2], (k * F32([1280, 720, 1]))[..., :2] * F32(480 / 720))
    # a source of another aspect and scale, retargeted: a similarity of the reference comes back as the reference
    r = skeleton(rng)
    s0, _ = similar(rng, r)
    big = s0 * F32([1.5, 1.5, 1])
    assert np.abs(px(big[None], r, source_size=(720, 1280))[0, 0, :, :2].astype(np.float64) - r[:, :2]).max() < 2.0 ** -7
    norm = rr.retarget((s0 / F32([1280, 720, 1]))[None], r / F32([832, 480, 1]), SIZE, source_size=(720, 1280))
    assert np.abs(norm[0, 0, :, :2].astype(np.float64) - r[:, :2]).max() < 2.0 ** -5       # the normalised inputs round once more
    for bad in ((0, 5), (5,), (5, -1), (5, float("nan")), "ab", 7):
        with pytest.raises(ValueError, match="source_size"):
            rr.prepare(SIZE, source_size=bad)


def test_reference_broadcast_and_eight_people():
    rng = np.random.default_rng(10)
    k = np.stack([np.stack([skeleton(rng) for _ in range(8)]) for _ in range(3)])          # [3, 8, 134, 3]
    k[1, 3, 7], k[0, 5, 1] = (-1, -1, 0), (-1, -1, 0)
    r = np.stack([skeleton(rng) for _ in range(8)])
    out = px(k, r, source_fps=24)
    assert out.shape == (2, 8, 134, 3)
    for q in range(8):
        assert np.array_equal(out[:, q], px(k[:, q], r[q], source_fps=24)[:, 0]), q
    one = px(k, r[0], source_fps=24)
    assert np.array_equal(one, px(k, r[:1], source_fps=24)) and np.array_equal(one, px(k, np.broadcast_to(r[:1], r.shape), source_fps=24))
    assert not np.array_equal(one, out)
    for bad in (r[:2], r[0, :100], np.zeros((9, 134, 3), F32), np.zeros((1, 8, 134, 3), F32)):
        with pytest.raises(ValueError, match="ref_keypoints"):
            px(k, bad)
    with pytest.raises(ValueError, match="keypoints must be"):
        px(np.zeros((2, 9, 134, 3), F32), r[0])


# ============================================================================================== the stream
@pytest.mark.parametrize("source", [16, 30, 24, 15])
def test_reference_stream_partitions_give_the_whole_clip(source):
    rng = np.random.default_rng(11)
    n = 12
    k = np.stack([np.stack([skeleton(rng), skeleton(rng)]) for _ in range(n)])
    k[4, 0, 9], k[0, 1, 30] = (-1, -1, 0), (-1, -1, 0)
    r = skeleton(rng)
    whole = rr.retarget(k, r, SIZE, source_fps=source, normalized=False)
    for parts in ([1] * n, [5, 2, 4, 1], [n], [1, n - 1], [n - 1, 1]):
        s = rr.Stream(r, SIZE, source_fps=source, normalized=False)
        got, at = [], 0
        for m in parts:
            got.append(s.push(k[at:at + m]))
            assert got[-1].shape[0] == rr.plan(at, m, *rr.rate(source, 16))[1]
            at += m
        assert s.close() is None and (s.frames_in, s.frames_out) == (n, len(whole))
        assert np.array_equal(np.concatenate(got), whole), parts
        with pytest.raises(ValueError, match="closed"):
            s.push(k[:1])
    if source == 30:
        s = rr.Stream(r, SIZE, source_fps=30, normalized=False)
        assert [s.push(k[i:i + 1]).shape[0] for i in range(5)] == [1, 0, 1, 0, 1]        # frames 0, 15/8, 30/8: pushes with nothing final
    with pytest.raises(ValueError, match="people"):
        s = rr.Stream(r, SIZE)
        s.push(k[:1])
        s.push(k[1:2, :1])


# ============================================================================================== the C entry points
def test_c_plan_equals_its_python_mirror():
    lib = sfa._lib.lib()
    assert lib.sf_abi_version() == 11 == sfa._lib.ABI_VERSION
    for num, den in ((1, 1), (15, 8), (3, 2), (15, 4), (15, 16), (1875, 1001), (65535, 1), (1, 65535), (65535, 65534)):
        for before in (0, 1, 2, 7, 150, 99999):
            for n in (0, 1, 2, 5, 151):
                assert sfa.ops.pose_retarget_plan(before, n, num, den) == rr.plan(before, n, num, den), (before, n, num, den)
        total, at = 0, 0
        for n in (1, 3, 1, 8, 2):                                                       # the plans of a partition tile the clip's frames
            first, count = sfa.ops.pose_retarget_plan(at, n, num, den)
            assert first == total
            total, at = total + count, at + n
        assert total == rr.frames_out(at, num, den)
    first, count = C.c_int64(), C.c_int64()
    err = lib.sf_last_error
    assert lib.sf_pose_retarget_plan(0, 1, 1, 1, None, C.byref(count)) != 0 and b"null result" in err()
    for bad in ((-1, 1, 1, 1), (0, -1, 1, 1), (1 << 41, 1, 1, 1)):
        assert lib.sf_pose_retarget_plan(*bad, C.byref(first), C.byref(count)) != 0 and b"frames_before=" in err()
    for bad in ((0, 1, 0, 1), (0, 1, 1, 0), (0, 1, 65536, 1), (0, 1, 1, 65536)):
        assert lib.sf_pose_retarget_plan(*bad, C.byref(first), C.byref(count)) != 0 and b"rate %d/%d" % bad[2:] in err()
        with pytest.raises(ValueError, match="plan"):
            rr.plan(*bad)
    with pytest.raises(sfa._lib.SfHipError, match="sf_pose_retarget_plan"):
        sfa.ops.pose_retarget_plan(-1, 1, 1, 1)


def test_c_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib, L = sfa._lib.lib(), sfa._lib
    A = L.PoseRetargetArgs
    assert C.sizeof(A) == 4 * 8 + 2 * 8 + 6 * 4 + 5 * 4 + 4 == 96 and A.src0.offset == 32 and A.n_src.offset == 48 and A.align.offset == 92
    assert (L.POSE_RETARGET_MAX_RATE, L.POSE_RETARGET_MAX_FRAMES) == (rr.MAX_RATE, 1 << 20)
    header = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert "#define SF_POSE_RETARGET_MAX_RATE 65535\n" in header and "#define SF_POSE_RETARGET_MAX_FRAMES 1048576\n" in header
    ok = dict(src=4096, first=4096, ref=8192, out=16384, src0=0, out0=0, n_src=10, n_out=5, people=2, ref_people=1, num=15, den=8, src_sx=832,
              src_sy=480, ref_sx=832, ref_sy=480, score_threshold=0.3, align=1)

    def call(**kw):
        return lib.sf_pose_retarget_frames(C.byref(A(**{**ok, **kw})), None)
    err = lib.sf_last_error
    assert lib.sf_pose_retarget_frames(None, None) != 0 and b"null args" in err()
    for name in ("src", "first", "ref", "out"):
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
        assert call(**{name: 4098}) != 0 and b"aligned" in err(), name
    for bad in (0, 9, -1):
        assert call(people=bad) != 0 and b"people=%d (1..8)" % bad in err()
    for bad in (0, 3, 8):
        assert call(ref_people=bad) != 0 and b"ref_people=%d (1 or people=2)" % bad in err()
    assert call(people=8, ref_people=8, n_out=0) != 0 and b"n_out=0" in err()
    for num, den in ((0, 8), (65536, 8), (15, 0), (15, 65536), (-1, -1)):
        assert call(num=num, den=den) != 0 and b"rate %d/%d (both 1..65535)" % (num, den) in err()
    assert call(n_src=0) != 0 and b"n_src=0" in err()
    assert call(n_out=(1 << 20) + 1) != 0 and b"n_out=1048577" in err()
    assert call(src0=-1) != 0 and b"src0=-1" in err()
    assert call(out0=-1) != 0 and b"out0=-1" in err()
    assert call(out0=(1 << 40) + 1) != 0 and b"out0=" in err()
    for name in ("src_sx", "src_sy", "ref_sx", "ref_sy"):
        for bad in (float("nan"), float("inf")):
            assert call(**{name: bad}) != 0 and b"scale factors must be finite" in err(), name
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(score_threshold=bad) != 0 and b"score_threshold must be finite" in err()
    assert call(align=2) != 0 and b"align=2" in err()
    # the source range: 10 source frames at 15/8 give frames 0..4 (frame 4 reads 7 and 8; frame 5 would read 9 and 10)
    assert call(n_out=6) != 0 and b"output frames [0, 5] read source frames [0, 10], the piece holds [0, 9]" in err()
    assert call(n_src=8) != 0 and b"read source frames [0, 8], the piece holds [0, 7]" in err()
    assert call(src0=1) != 0 and b"read source frames [0, 8], the piece holds [1, 10]" in err()
    assert call(out0=3, n_out=2, src0=6, n_src=3) != 0 and b"output frames [3, 4] read source frames [5, 8], the piece holds [6, 8]" in err()
    assert call(out0=4, n_out=2, src0=7, n_src=3) != 0 and b"read source frames [7, 10], the piece holds [7, 9]" in err()


# ============================================================================================== the Python surface
def test_operator_schema_and_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "pose_retarget_frames" in sfa.torch_ops.OPS
    assert "!" not in str(torch.ops.sf_hip.pose_retarget_frames.default._schema)
    with FakeTensorMode():
        k, r = torch.empty(5, 2, 134, 3, device="cuda"), torch.empty(1, 134, 3, device="cuda")
        o = torch.ops.sf_hip.pose_retarget_frames(k, k[0], r, 0, 0, 3, 15, 8, 832.0, 480.0, 832.0, 480.0)
        assert tuple(o.shape) == (3, 2, 134, 3) and o.dtype == torch.float32
        with pytest.raises(Exception, match="ref must be"):
            torch.ops.sf_hip.pose_retarget_frames(k, k[0], torch.empty(3, 134, 3, device="cuda"), 0, 0, 3, 15, 8, 1.0, 1.0, 1.0, 1.0)
        with pytest.raises(Exception, match="first must be"):
            torch.ops.sf_hip.pose_retarget_frames(k, k[0, :1], r, 0, 0, 3, 15, 8, 1.0, 1.0, 1.0, 1.0)
        with pytest.raises(Exception, match="n_out=0"):
            torch.ops.sf_hip.pose_retarget_frames(k, k[0], r, 0, 0, 0, 15, 8, 1.0, 1.0, 1.0, 1.0)
    z = torch.zeros(2, 1, 134, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        torch.ops.sf_hip.pose_retarget_frames(z, z[0], z[0], 0, 0, 2, 1, 1, 1.0, 1.0, 1.0, 1.0)


def test_pose_retargeter_checks_that_need_no_device():
    assert sfa.PoseRetargeter is sfa.pose_retarget.PoseRetargeter and sfa.PoseRetargetStream is sfa.pose_retarget.PoseRetargetStream
    assert {"PoseRetargeter", "PoseRetargetStream", "pose_retarget", "pose_retarget_reference"} <= set(sfa.__all__)
    assert (rr.KEYPOINTS, rr.LIMBS, rr.MAX_PEOPLE) == (pr.KEYPOINTS, pr.LIMBS, pr.MAX_PEOPLE)
    t = sfa.PoseRetargeter()
    k, r = np.zeros((3, 2, 134, 3), F32), np.zeros((134, 3), F32)
    for size in ((0, 40), (24,), (24.5, 40), (4097, 8)):
        with pytest.raises(ValueError, match="size"):
            t.retarget(k, r, size)
        with pytest.raises(ValueError, match="size"):
            t.open_stream(r, size)
    for kw, match in ((dict(source_fps=0), "fps"), (dict(target_fps="x"), "fps"), (dict(source_fps=65537, target_fps=65536), "1..65535"),
                      (dict(score_threshold=float("nan")), "score_threshold"), (dict(source_size=(0, 4)), "source_size")):
        with pytest.raises(ValueError, match=match):
            t.retarget(k, r, (24, 40), **kw)
        with pytest.raises(ValueError, match=match):
            t.open_stream(r, (24, 40), **kw)
    for bad in (k[0, 0], np.zeros((2, 9, 134, 3), F32), np.zeros((0, 1, 134, 3), F32), torch.zeros(2, 134, 2)):
        with pytest.raises(ValueError, match="keypoints must be"):
            t.retarget(bad, r, (24, 40))
    for bad in (np.zeros((3, 134, 3), F32), np.zeros((133, 3), F32), torch.zeros(1, 1, 134, 3)):
        with pytest.raises(ValueError, match="ref_keypoints must be"):
            t.retarget(k, bad, (24, 40))
    with pytest.raises(ValueError, match="ref_keypoints must be"):
        t.open_stream(np.zeros((9, 134, 3), F32), (24, 40))
    with pytest.raises(ValueError, match="numbers"):
        t.retarget(np.zeros((2, 134, 3), object), r, (24, 40))
    with pytest.raises(ValueError, match="numbers"):
        t.retarget(k, torch.zeros(134, 3, dtype=torch.bool), (24, 40))
    cpu = sfa.PoseRetargeter(device="cpu")
    for kk in (k, torch.from_numpy(k), k[:, 0].tolist()):
        with pytest.raises(ValueError, match="no CPU fallback"):
            cpu.retarget(kk, r, (24, 40))
    s = cpu.open_stream(r, (24, 40), source_fps=30)
    assert isinstance(s, sfa.PoseRetargetStream) and (s.params.num, s.params.den, s.frames_in, s.frames_out) == (15, 8, 0, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        s.push(k)
    with pytest.raises(ValueError, match="ref_keypoints must be"):
        cpu.open_stream(np.zeros((3, 134, 3), F32), (24, 40)).push(k)                    # 3 reference people, 2 in the piece
    assert s.close() is None
    with pytest.raises(ValueError, match="closed"):
        s.push(k)


def test_pose_feed_with_a_retargeter_checks_that_need_no_device():
    r = sfa.PoseRenderer(device="cpu")
    k = np.zeros((5, 1, 134, 3), F32)
    stream = sfa.PoseRetargeter(device="cpu").open_stream(k[0], (24, 40), source_fps=30)
    with pytest.raises(ValueError, match="opened for"):
        next(sfa.pose_render.pose_feed(k, r, (48, 40), 2, retargeter=stream))
    with pytest.raises(ValueError, match="frames_per_piece"):
        next(sfa.pose_render.pose_feed(k, r, (24, 40), 0, retargeter=stream))
    pulled = []

    def source():
        for i in range(5):
            pulled.append(i)
            yield k[i]
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, retargeter=stream)
    assert pulled == []                                                                  # nothing is read before a piece is asked for
    with pytest.raises(ValueError, match="no CPU fallback"):
        next(feed)
    assert pulled == [0, 1, 2]                                                           # two output frames at 15/8 need source frames 0..2


def test_generate_flags(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import generate
    k = np.random.default_rng(0).random((5, 2, 134, 3)).astype(F32)
    np.savez(tmp_path / "clip.npz", keypoints=k)
    np.savez(tmp_path / "ref.npz", keypoints=k[0])
    np.save(tmp_path / "dict.npy", {"dwpose_data": np.zeros((3, 1, 8, 8), np.uint8), "random_ref_dwpose": np.zeros((8, 8, 3), np.uint8)}, allow_pickle=True)
    (tmp_path / "clip.avi").write_bytes(b"")
    (tmp_path / "ref.jpg").write_bytes(b"")
    base = ["generate.py", "--config_path", "c", "--data_path", "d", "--output_folder", "o"]

    def run(*more):
        """the parser's error text: every one of these ends in ap.error, before any file of the config is opened"""
        monkeypatch.setattr(sys, "argv", base + list(more))
        with pytest.raises(SystemExit) as e:
            generate.main()
        assert e.value.code == 2
        return capsys.readouterr().err
    seeded = ("--pose_random_init_seed", "0")
    for flag in (("--pose_align",), ("--pose_fps", "30"), ("--pose_source_size", "720x1280")):
        assert f"{flag[0]} needs a keypoint --pose_path" in run(*flag), flag
        assert f"{flag[0]} goes with a keypoint --pose_path" in run(*seeded, "--pose_path", str(tmp_path / "dict.npy"), *flag), flag
        assert f"{flag[0]} goes with a keypoint --pose_path" in run(*seeded, "--pose_path", str(tmp_path / "clip.avi"), "--ref_pose_path",
                                                                    str(tmp_path / "ref.jpg"), *flag), flag
    keypoints = (*seeded, "--pose_path", str(tmp_path / "clip.npz"), "--ref_pose_path", str(tmp_path / "ref.npz"))
    for bad in ("0", "thirty", "30/0", "65537/65536", "30.0"):
        assert f"--pose_fps {bad}" in run(*keypoints, "--pose_fps", bad), bad
    for bad in ("720", "720x", "0x1280", "720X1280", "a x b"):
        err = run(*keypoints, "--pose_source_size", bad)
        assert "--pose_source_size" in err and "HxW expected" in err, bad
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--pose_align", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--pose_align", "--pose_fps N[/D]", "--pose_source_size HxW"))
