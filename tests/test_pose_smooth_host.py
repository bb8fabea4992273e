"""Host tests of the pose smoother (no GPU): the vectorised definition `pose_smooth_reference` against a scalar transcription of
the formulas written here, the partition invariance of `frames` and `Stream` on output and packed state, the hold rules on
hand-made sequences, the edges (threshold, -0.0, NaN, inf, a re-seed near FLT_MAX, subnormals, a constant clip), what the
filter is for (jitter and lag), `prepare`'s checks, the C entry points' argument checks through ctypes (they return before
any device call), the `ValueError`s of the Python surface and the `generate.py` flag errors."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_smooth_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MARKER = np.array([-1, -1, 0], F32)
TWO_PI = F32(2 * np.pi)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


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
    gone = rng.random(k.shape[:3]) < 0.04                                                # runs of two and three missing samples
    gone[1:] |= gone[:-1] & (rng.random(gone[1:].shape) < 0.5)
    gone[1:] |= gone[:-1] & (rng.random(gone[1:].shape) < 0.3)
    k[gone] = MARKER
    if pixels:
        k[..., :2] *= F32([832, 480])
    return k


# ============================================================================================== a scalar transcription
def coordinate(v, h, d, te, p):
    """One coordinate of one point of one frame, as the definition's docstring lists the formulas: (h', d')"""
    e = F32(v - h)
    dx = F32(e / te)
    rd = F32(p.kd * te)
    ad = F32(rd / F32(rd + F32(1)))
    t = F32(dx - d)
    t = F32(ad * t)
    dn = F32(d + t)
    fc = F32(p.beta * F32(abs(dn)))
    fc = F32(p.min_cutoff + fc)
    r = F32(TWO_PI * fc)
    r = F32(r * te)
    a = F32(r / F32(r + F32(1)))
    t = F32(a * e)
    return F32(h + t), dn


def scalar_point(samples, p, log=None):
    """One point's samples [F, 3] from a fresh state -> (its outputs [F, 3], its packed state [8] int32), in a plain loop"""
    seen, gap, h, d, s = False, 0, [F32(0), F32(0)], [F32(0), F32(0)], F32(0)
    out = np.empty((len(samples), 3), F32)
    with np.errstate(all="ignore"):
        for f, (x, y, score) in enumerate(samples):
            valid = bool(np.isfinite(x) and np.isfinite(y) and np.isfinite(score) and score >= p.threshold and x >= 0 and y >= 0)
            te = F32(F32(gap + 1) * p.period)
            if valid:
                new = [coordinate(v, h[c], d[c], te, p) for c, v in enumerate((x, y))] if seen else None
                if new is not None and all(np.isfinite(v) for pair in new for v in pair):
                    h, d = [new[0][0], new[1][0]], [new[0][1], new[1][1]]
                    if log is not None:
                        log.append((f, float(te)))
                else:
                    h, d = [F32(x), F32(y)], [F32(0), F32(0)]
                s, gap, seen = F32(score), 0, True
                out[f] = (h[0], h[1], s)
            elif seen and gap < p.max_gap:
                gap += 1
                out[f] = (h[0], h[1], s)
            else:
                seen, gap = False, 0
                out[f] = MARKER
    state = np.zeros(8, np.int32)
    state[:5] = bits(np.array([h[0], h[1], d[0], d[1], s], F32))
    state[5:7] = gap, seen
    return out, state


@pytest.mark.parametrize("beta", [0.0, 0.7])
@pytest.mark.parametrize("fps", [30, 16, "30000/1001"])
def test_the_vectorised_definition_equals_a_scalar_transcription(fps, beta):
    for seed, people, max_gap, pixels in ((1, 2, 0, False), (2, 1, 2, True)):
        k = clip(seed, 12, people, pixels)
        p = sr.prepare(fps, 1.0, beta, 1.0, max_gap)
        state, counts = sr.fresh_state(people), {}
        out = sr.frames(k, state, p, counts)
        assert out.dtype == F32 and out.shape == k.shape
        assert np.array_equal(bits(out), bits(sr.smooth(k, fps, beta=beta, max_gap=max_gap)))
        for q in range(people):
            for j in range(134):
                want, want_state = scalar_point(k[:, q, j], p)
                assert np.array_equal(bits(out[:, q, j]), bits(want)), (q, j)
                assert np.array_equal(state[q, j], want_state), (q, j)
        assert counts["filter"] > 1000 and counts["seed"] >= 134 * people and counts["drop"] > 20 and (counts["hold"] > 20) == (max_gap > 0)
        assert sum(counts.values()) == k[..., 0].size


def test_constants_are_formed_in_double_and_rounded_once():
    p = sr.prepare("30000/1001", 1.5, 0.25, 2.0, 3, 0.4)
    assert (p.num, p.den, p.max_gap) == (30000, 1001, 3) and p.period == F32(1001 / 30000) and p.kd == F32(2 * np.pi * 2.0)
    assert p.two_pi == TWO_PI and bits(p.two_pi) == 0x40C90FDB and (p.min_cutoff, p.beta, p.threshold) == (F32(1.5), F32(0.25), F32(0.4))
    assert all(isinstance(v, F32) for v in (p.period, p.min_cutoff, p.beta, p.kd, p.two_pi, p.threshold))
    assert sr.prepare(Fraction(25, 2)).period == F32(2 / 25) and sr.prepare(16) == sr.prepare("16", 1.0, 0.0, 1.0, 0, 0.3)


# ============================================================================================== partitions
def test_any_partition_gives_the_whole_clips_bits():
    n = 7
    k = clip(3, n, 2)
    for kw in (dict(), dict(beta=0.7, max_gap=2), dict(min_cutoff=0.3, d_cutoff=2.0, max_gap=1)):
        p = sr.prepare(30, **kw)
        whole_state = sr.fresh_state(2)
        whole = sr.frames(k, whole_state, p)
        assert np.array_equal(bits(whole), bits(sr.smooth(k, 30, **kw))) and whole_state.any()
        for parts in ([1] * n, [5, 2], [3, 4], [n]):
            state, stream = sr.fresh_state(2), sr.Stream(30, **kw)
            got, pushed, at = [], [], 0
            for m in parts:
                got.append(sr.frames(k[at:at + m], state, p))
                pushed.append(stream.push(k[at:at + m]))
                assert pushed[-1].shape == (m, 2, 134, 3)                                # nothing is held back
                at += m
            assert stream.close() is None and stream.frames_in == n
            assert np.array_equal(bits(np.concatenate(got)), bits(whole)) and np.array_equal(state, whole_state), parts
            assert np.array_equal(bits(np.concatenate(pushed)), bits(whole)) and np.array_equal(stream.state, whole_state), parts
            with pytest.raises(ValueError, match="closed"):
                stream.push(k[:1])
    stream = sr.Stream(30)
    assert stream.state is None
    assert stream.push(k[:2, 0]).shape == (2, 1, 134, 3) and stream.state.shape == (1, 134, 8)      # [n, 134, 3] is one person
    with pytest.raises(ValueError, match="people"):
        stream.push(k[2:3])
    with pytest.raises(ValueError, match="state must be"):
        sr.frames(k, sr.fresh_state(1), sr.prepare(30))


# ============================================================================================== the hold rules
def one_point(samples):
    """[F, 3] samples of point 0 of one person -> a clip [F, 1, 134, 3] whose other points are missing"""
    k = np.tile(MARKER, (len(samples), 1, 134, 1))
    k[:, 0, 0] = samples
    return k


@pytest.mark.parametrize("max_gap", [0, 1, 3])
def test_a_gap_of_max_gap_is_bridged_and_a_longer_one_ends_in_markers(max_gap):
    gone = (-1, -1, 0)
    lead = [(100, 50, 0.9), (104, 52, 0.8), (103, 55, 0.7)]
    p = sr.prepare(30, 1.0, 0.1, 1.0, max_gap)
    # a gap of exactly max_gap frames, then a valid sample: bridged with the last filtered position and the last valid score
    k = one_point(lead + [gone] * max_gap + [(110, 60, 0.6), (111, 61, 0.5)])
    out = sr.smooth(k, 30, beta=0.1, max_gap=max_gap)[:, 0, 0]
    log = []
    want, _ = scalar_point(k[:, 0, 0], p, log)
    assert np.array_equal(bits(out), bits(want))
    for g in range(max_gap):
        assert np.array_equal(bits(out[3 + g]), bits(out[2])) and out[3 + g, 2] == F32(0.7)
    assert (out[:, :2] >= 0).all() and not (out == MARKER).all(-1).any()
    # after the bridged gap of g frames the filter ran with te = (g + 1) * period, and with period elsewhere
    assert log == [(1, float(p.period)), (2, float(p.period)), (3 + max_gap, float(F32(max_gap + 1) * p.period)), (4 + max_gap, float(p.period))]
    assert not np.array_equal(out[3 + max_gap], k[3 + max_gap, 0, 0]) and out[3 + max_gap, 2] == F32(0.6)      # filtered, not seeded
    # a gap one longer: the hold runs out, markers follow, and the next valid sample seeds (its output is its input)
    k = one_point(lead + [gone] * (max_gap + 1) + [(110, 60, 0.6), (111, 61, 0.5)])
    state, counts = sr.fresh_state(1), {}
    out = sr.frames(k, state, p, counts)[:, 0, 0]
    assert np.array_equal(bits(out), bits(scalar_point(k[:, 0, 0], p)[0]))
    for g in range(max_gap):
        assert np.array_equal(bits(out[3 + g]), bits(out[2]))
    assert np.array_equal(out[3 + max_gap], MARKER)
    assert np.array_equal(bits(out[4 + max_gap]), bits(k[4 + max_gap, 0, 0]))
    assert not np.array_equal(out[5 + max_gap], k[5 + max_gap, 0, 0])
    assert counts == dict(filter=3, seed=2, reseed=0, hold=max_gap, drop=133 * len(k) + 1)
    assert (state[0, 0, sr.GAP], state[0, 0, sr.SEEN]) == (0, 1) and not state[0, 1:, sr.SEEN].any()
    # a clip that ends inside a hold leaves the gap in the state; a point never seen is never held
    if max_gap:
        state = sr.fresh_state(1)
        sr.frames(one_point(lead + [gone]), state, p)
        assert (state[0, 0, sr.GAP], state[0, 0, sr.SEEN]) == (1, 1)
    assert (sr.smooth(one_point([gone] * 3 + lead), 30, max_gap=max_gap)[:3] == MARKER).all()


def test_max_gap_zero_never_invents_a_point():
    k = clip(4, 9, 2)
    out = sr.smooth(k, 30, beta=0.3)
    valid = (k[..., 2] >= F32(0.3)) & (k[..., 0] >= 0) & (k[..., 1] >= 0)
    assert np.array_equal((out != MARKER).any(-1), valid) and 0.05 < 1 - valid.mean() < 0.25
    held = sr.smooth(k, 30, beta=0.3, max_gap=2)
    assert ((held != MARKER).any(-1) & ~valid).sum() > 50
    assert np.array_equal(held[..., 2][valid], k[..., 2][valid])                          # scores pass


# ============================================================================================== edges
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


def test_edges():
    t = F32(0.3)
    k = edge_clip(t)
    for kw in (dict(), dict(beta=0.7, max_gap=1), dict(beta=0.7, max_gap=1, fps="30000/1001")):
        kw = {"fps": 30, **kw}
        p = sr.prepare(kw["fps"], 1.0, kw.get("beta", 0.0), 1.0, kw.get("max_gap", 0))
        counts = {}
        out = sr.frames(k, sr.fresh_state(1), p, counts)[:, 0]
        assert np.array_equal(bits(out), bits(sr.smooth(k, **kw)[:, 0]))
        for j in range(20):
            assert np.array_equal(bits(out[:, j]), bits(scalar_point(k[:, 0, j], p)[0])), j
        held = p.max_gap > 0
        assert out[2, 0, 2] == t and ((out[2, 1] == MARKER).all() != held)
        assert (out[3, 2] != MARKER).any() and (out[3, 3] != MARKER).any() and ((out[3, 4] == MARKER).all() != held)
        assert ((out[4, 5:14] == MARKER).all(-1) != held).all() and np.isfinite(out).all()
        # 3e38 then 0: the filtered step overflows, the point is seeded afresh at the sample itself
        assert counts["reseed"] >= 2 and out[3, 14, 0] == 0 and out[3, 15, 1] == 0 and out[1, 14, 0] == F32(3e38)
        assert np.array_equal(bits(out[:, 16]), bits(k[:, 0, 16])) and np.array_equal(bits(out[:, 17]), bits(k[:, 0, 17]))      # subnormals survive
        assert (out[1:, 18, 0] > 0).all() and (out[1:, 18, 0] < F32(1.2e-38)).all() and len(set(out[:, 18, 0].tolist())) == 8
        live = (out != MARKER).any(-1)
        assert np.isfinite(out[live]).all() and (out[live][:, :2] >= 0).all() and (out[live][:, 2] >= t).all()
    for threshold in (0.5, 0.0):
        k = edge_clip(F32(threshold))
        out = sr.smooth(k, 30, score_threshold=threshold)[:, 0]
        assert out[2, 0, 2] == F32(threshold) and (out[2, 1] == MARKER).all()


def test_a_constant_clip_returns_its_bits():
    rng = np.random.default_rng(5)
    frame = np.concatenate([rng.uniform(0, 1, (2, 134, 2)) * [832, 480], rng.uniform(0.3, 1, (2, 134, 1))], -1).astype(F32)
    k = np.repeat(frame[None], 9, 0)
    for kw in (dict(), dict(beta=0.7, min_cutoff=0.05, d_cutoff=3.0), dict(max_gap=3)):
        for fps in (30, 16, "30000/1001"):
            assert np.array_equal(bits(sr.smooth(k, fps, **kw)), bits(k)), (fps, kw)


def test_every_live_output_is_a_point_the_next_stage_reads_as_valid():
    for seed, pixels, threshold in ((6, False, 0.3), (7, True, 0.5), (8, True, 0.0)):
        k = clip(seed, 25, 2, pixels)
        k[3, 0, 7, 0], k[5, 1, 9, 1], k[8, 1, 3, 2] = 3e38, np.inf, np.nan
        out = sr.smooth(k, 30, beta=0.7, max_gap=3, score_threshold=threshold)
        live = (out != MARKER).any(-1)
        assert 0.5 < live.mean() < 1 and (out[~live] == MARKER).all()
        assert np.isfinite(out[live]).all() and (out[live][:, :2] >= 0).all() and (out[live][:, 2] >= F32(threshold)).all()
        from self_forcing_amd import pose_retarget_reference as rr
        assert np.array_equal(rr.lift(out, F32(1), F32(1), F32(threshold))[2], live)      # the retargeter's and the renderer's rule


# ============================================================================================== what the filter is for
def test_jitter_is_halved_and_beta_cuts_the_lag():
    frames = 151
    rng = np.random.default_rng(0)
    still = np.tile(F32([400, 300, 0.9]), (frames, 1))
    still[:, 0] += rng.uniform(-2, 2, frames)
    out = sr.smooth(one_point(still), 30, min_cutoff=1.0, beta=0.0)[:, 0, 0]

    def jitter(x):
        return float(np.sqrt(np.mean(np.diff(x.astype(np.float64)) ** 2)))
    print(f"jitter: output {jitter(out[:, 0]):.3f} px, input {jitter(still[:, 0]):.3f} px")
    assert jitter(out[:, 0]) < 0.5 * jitter(still[:, 0]) and abs(float(out[-1, 0]) - 400) < 2
    ramp = np.tile(F32([0, 300, 0.9]), (frames, 1))
    ramp[:, 0] = 10 * np.arange(frames)
    lag = [float(ramp[-1, 0] - sr.smooth(one_point(ramp), 30, min_cutoff=1.0, beta=beta)[-1, 0, 0, 0]) for beta in (0.0, 0.05)]
    print(f"lag on a ramp of 10 px per frame: {lag[0]:.2f} px at beta 0, {lag[1]:.2f} px at beta 0.05")
    assert 0 < lag[1] < 0.25 * lag[0]


# ============================================================================================== prepare
def test_prepare_rejects_each_bad_parameter_by_name():
    for bad in (0, -30, "x", "30/0", 30.0, None, True, 65536, "1/65536", Fraction(65537, 65536)):
        with pytest.raises(ValueError, match="fps"):
            sr.prepare(bad)
    for name, values in (("min_cutoff", (0, -1.0, np.nan, np.inf, "1", None, 1e-50, 1e39, True)),
                         ("beta", (-0.1, np.nan, np.inf, "0", None, 1e39, False)),
                         ("d_cutoff", (0, -1.0, np.nan, np.inf, "1", None, 1e-50, 1e38))):
        for bad in values:
            with pytest.raises(ValueError, match=name):
                sr.prepare(30, **{name: bad})
            with pytest.raises(ValueError, match=name):
                sr.Stream(30, **{name: bad})
    for bad in (-1, 65536, 1.0, "2", None, True):
        with pytest.raises(ValueError, match="max_gap"):
            sr.prepare(30, max_gap=bad)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="score_threshold"):
            sr.prepare(30, score_threshold=bad)
    assert sr.prepare(65535, max_gap=65535, beta=0).max_gap == 65535 and sr.prepare("1/65535").period == F32(65535)
    for bad in (0, 9, -1, 1.0, True):
        with pytest.raises(ValueError, match="people"):
            sr.fresh_state(bad)
    for bad in (np.zeros((134, 3)), np.zeros((2, 9, 134, 3)), np.zeros((0, 1, 134, 3)), np.zeros((2, 1, 133, 3))):
        with pytest.raises(ValueError, match="keypoints must be"):
            sr.smooth(bad, 30)


# ============================================================================================== the C entry points
def test_state_bytes():
    lib = sfa._lib.lib()
    assert lib.sf_abi_version() == 11 == sfa._lib.ABI_VERSION
    for people in range(1, 9):
        assert lib.sf_pose_smooth_state_bytes(people) == people * 134 * 32 == sr.state_bytes(people) == sr.fresh_state(people).nbytes
        assert sfa.ops.pose_smooth_state_bytes(people) == people * 134 * 32
    for people in (0, 9, -1, 1 << 20):
        assert lib.sf_pose_smooth_state_bytes(people) == 0 == sr.state_bytes(people)


def test_c_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib, L = sfa._lib.lib(), sfa._lib
    A = L.PoseSmoothArgs
    assert C.sizeof(A) == 3 * 8 + 2 * 4 + 5 * 4 + 4 == 56 and A.n.offset == 24 and A.period.offset == 32 and A.max_gap.offset == 52
    assert L.POSE_SMOOTH_MAX_GAP == sr.MAX_GAP == 65535
    frame = 2 * 134 * 12                                                                 # bytes of one frame of two people
    ok = dict(src=1 << 20, out=2 << 20, state=3 << 20, n=10, people=2, period=1 / 30, min_cutoff=1.0, beta=0.0, kd=6.2831855, score_threshold=0.3,
              max_gap=2)

    def call(**kw):
        return lib.sf_pose_smooth_frames(C.byref(A(**{**ok, **kw})), None)
    err = lib.sf_last_error
    assert lib.sf_pose_smooth_frames(None, None) != 0 and b"null args" in err()
    for name in ("src", "out", "state"):
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
    for name in ("src", "out"):
        assert call(**{name: ok[name] + 2}) != 0 and b"4-byte aligned" in err(), name
    for off in (4, 8, 12):
        assert call(state=ok["state"] + off) != 0 and b"state must be 16-byte aligned" in err()
    for bad in (0, 9, -1):
        assert call(people=bad) != 0 and b"people=%d (1..8)" % bad in err()
    for bad in (0, -1, (1 << 20) + 1):
        assert call(n=bad) != 0 and b"n=%d (1..1048576)" % bad in err()
    for bad in (-1, 65536):
        assert call(max_gap=bad) != 0 and b"max_gap=%d (0..65535)" % bad in err()
    for name in ("period", "min_cutoff", "kd"):
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            assert call(**{name: bad}) != 0 and b"%s must be finite and > 0" % name.encode() in err(), (name, bad)
    for bad in (float("nan"), float("inf"), -1e-6):
        assert call(beta=bad) != 0 and b"beta must be finite and >= 0" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(score_threshold=bad) != 0 and b"score_threshold must be finite" in err()
    # overlapping ranges: src and out hold n frames each, state people * 134 * 32 bytes
    src, out, state = ok["src"], ok["out"], ok["state"]
    for bad in (src, src + 10 * frame - 4, src - 10 * frame + 4):
        assert call(out=bad) != 0 and b"src and out overlap" in err(), bad
    for bad in (src - 2 * 134 * 32 + 16, src + 10 * frame - 16):
        assert call(state=bad) != 0 and b"src and state overlap" in err(), bad
    for bad in (out - 2 * 134 * 32 + 16, out + 10 * frame - 16):
        assert call(state=bad) != 0 and b"out and state overlap" in err(), bad


# ============================================================================================== the Python surface
def test_operator_schema_and_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "pose_smooth_frames" in sfa.torch_ops.OPS
    schema = str(torch.ops.sf_hip.pose_smooth_frames.default._schema)
    assert "Tensor(a1!) state" in schema and schema.count("!") == 1                       # it says that it mutates state, and only state
    with FakeTensorMode():
        k, s = torch.empty(5, 2, 134, 3, device="cuda"), torch.empty(2, 134, 8, dtype=torch.int32, device="cuda")
        o = torch.ops.sf_hip.pose_smooth_frames(k, s, 1 / 30, 1.0, 0.0, 6.28)
        assert tuple(o.shape) == (5, 2, 134, 3) and o.dtype == torch.float32
        with pytest.raises(Exception, match="state must be"):
            torch.ops.sf_hip.pose_smooth_frames(k, s[:1], 1 / 30, 1.0, 0.0, 6.28)
        with pytest.raises(Exception, match="state must be"):
            torch.ops.sf_hip.pose_smooth_frames(k, s.float(), 1 / 30, 1.0, 0.0, 6.28)
        with pytest.raises(Exception, match="src must be"):
            torch.ops.sf_hip.pose_smooth_frames(k[0], s, 1 / 30, 1.0, 0.0, 6.28)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.ops.pose_smooth_frames(torch.zeros(2, 1, 134, 3), torch.zeros(1, 134, 8, dtype=torch.int32), 1 / 30, 1.0, 0.0, 6.28, 0.3, 0)


def test_pose_smoother_checks_that_need_no_device():
    assert sfa.PoseSmoother is sfa.pose_smooth.PoseSmoother and sfa.PoseSmoothStream is sfa.pose_smooth.PoseSmoothStream
    assert {"PoseSmoother", "PoseSmoothStream", "pose_smooth", "pose_smooth_reference"} <= set(sfa.__all__)
    t = sfa.PoseSmoother()
    k = np.zeros((3, 2, 134, 3), F32)
    for kw, match in ((dict(fps=0), "fps"), (dict(fps="x"), "fps"), (dict(min_cutoff=0), "min_cutoff"), (dict(beta=-1), "beta"),
                      (dict(d_cutoff=float("nan")), "d_cutoff"), (dict(max_gap=-1), "max_gap"), (dict(max_gap=1.5), "max_gap"),
                      (dict(score_threshold=float("nan")), "score_threshold")):
        kw = {"fps": 30, **kw}
        with pytest.raises(ValueError, match=match):
            t.smooth(k, **kw)
        with pytest.raises(ValueError, match=match):
            t.open_stream(**kw)
    for bad in (k[0, 0], np.zeros((2, 9, 134, 3), F32), np.zeros((0, 1, 134, 3), F32), torch.zeros(2, 134, 2)):
        with pytest.raises(ValueError, match="keypoints must be"):
            t.smooth(bad, 30)
    with pytest.raises(ValueError, match="numbers"):
        t.smooth(np.zeros((2, 134, 3), object), 30)
    with pytest.raises(ValueError, match="numbers"):
        t.smooth(torch.zeros(2, 134, 3, dtype=torch.bool), 30)
    cpu = sfa.PoseSmoother(device="cpu")
    for kk in (k, torch.from_numpy(k), k[:, 0].tolist()):
        with pytest.raises(ValueError, match="no CPU fallback"):
            cpu.smooth(kk, 30)
    s = cpu.open_stream("30000/1001", beta=0.5, max_gap=2)
    assert isinstance(s, sfa.PoseSmoothStream) and (s.params.num, s.params.den, s.params.max_gap, s.frames_in, s.state) == (30000, 1001, 2, 0, None)
    with pytest.raises(ValueError, match="no CPU fallback"):
        s.push(k)
    assert s.state is None and s.frames_in == 0
    s.state = torch.zeros(2, 134, 8, dtype=torch.int32)                                  # a stream that has seen two people
    with pytest.raises(ValueError, match="holds 2 people, the piece 1"):
        s.push(k[:, :1])
    with pytest.raises(ValueError, match="keypoints must be"):
        s.push(k[0, 0])
    assert s.close() is None
    with pytest.raises(ValueError, match="closed"):
        s.push(k)


def test_pose_feed_with_a_smoother_pulls_no_more_than_a_piece():
    r = sfa.PoseRenderer(device="cpu")
    k = np.zeros((5, 1, 134, 3), F32)
    pulled = []

    def source():
        for i in range(5):
            pulled.append(i)
            yield k[i]
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, smoother=sfa.PoseSmoother(device="cpu").open_stream(30))
    assert pulled == []
    with pytest.raises(ValueError, match="PoseSmoother: expected a CUDA/ROCm device"):
        next(feed)
    assert pulled == [0, 1]
    pulled.clear()
    live = sfa.PoseRetargeter(device="cpu").open_stream(k[0], (24, 40), source_fps=30)
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, retargeter=live, smoother=sfa.PoseSmoother(device="cpu").open_stream(30))
    with pytest.raises(ValueError, match="PoseSmoother: expected a CUDA/ROCm device"):   # the smoother comes first
        next(feed)
    assert pulled == [0, 1, 2]


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
    for flag in (("--pose_smooth", "1.0"), ("--pose_hold", "2")):
        assert f"{flag[0]} needs a keypoint --pose_path" in run(*flag), flag
        assert f"{flag[0]} goes with a keypoint --pose_path" in run(*seeded, "--pose_path", str(tmp_path / "dict.npy"), *flag), flag
        assert f"{flag[0]} goes with a keypoint --pose_path" in run(*seeded, "--pose_path", str(tmp_path / "clip.avi"), "--ref_pose_path",
                                                                    str(tmp_path / "ref.jpg"), *flag), flag
    keypoints = (*seeded, "--pose_path", str(tmp_path / "clip.npz"), "--ref_pose_path", str(tmp_path / "ref.npz"))
    for bad in ("one", "1.0,", "1,2,3,4", "", "1.0;0.5"):
        err = run(*keypoints, "--pose_smooth", bad)
        assert "--pose_smooth" in err and "MIN_CUTOFF[,BETA[,D_CUTOFF]] expected" in err, bad
    for bad, name in (("0", "min_cutoff"), ("-1,0", "min_cutoff"), ("1,-0.5", "beta"), ("1,0,0", "d_cutoff"), ("nan", "min_cutoff"), ("1,inf", "beta")):
        err = run(*keypoints, f"--pose_smooth={bad}")                                    # (= lets a value begin with a minus sign)
        assert f"--pose_smooth {bad}" in err and name in err, bad
    for bad in ("-1", "65536"):
        err = run(*keypoints, f"--pose_hold={bad}")
        assert f"--pose_hold {bad}" in err and "max_gap" in err, bad
    assert "--pose_hold" in run(*keypoints, "--pose_hold", "two")                        # argparse's own: an integer is expected
    assert "--pose_fps 0" in run(*keypoints, "--pose_smooth", "1.0", "--pose_fps", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--pose_smooth MIN_CUTOFF[,BETA[,D_CUTOFF]]", "--pose_hold N"))
