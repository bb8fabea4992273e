"""The definition of the pose smoother's numbers (numpy, no GPU): jittery keypoints with dropped points -> keypoints a
One-Euro filter has smoothed and a bounded hold has carried across short gaps.  The reference project has no counterpart
(its poses arrive drawn); this is THIS PROJECT'S definition, after Casiez, Roussel and Vogel's 1-euro filter (CHI 2012).
All arithmetic is float32 and every operation (sub, mul, add, div) is rounded on its own, never fused, so the device
(csrc/pose_smooth.hip) equals this file bit for bit.

source     float32 [F, P, 134, 3] or [F, 134, 3] = (x, y, score), DWPose's whole-body order, in the caller's units
           (normalised or pixels): the smoother does not lift them.
valid      the renderer's rule on the raw values: x, y, score finite; score >= score_threshold (fp32); x >= 0, y >= 0.
constants  formed in double and rounded once: period = fp32(den / num) of fps = num / den (both 1..65535),
           kd = fp32(2 pi d_cutoff), two_pi = fp32(2 pi); min_cutoff, beta and the threshold as fp32.
state      per (person, point): seen, gap (frames since the last valid sample), h[2] and d[2] (filtered position and
           speed), s (the last valid score).  Packed as the device holds it: int32 words [P][134][8] = hx, hy, dx, dy, s
           (float bits), gap, seen, 0; zero-filled is fresh.
one frame  of one point, with te = fp32(gap + 1) * period (one rounding):
  valid and seen        per coordinate with sample v:  e = v - h;  dx = e / te;  rd = kd * te;  ad = rd / (rd + 1);
                        t = dx - d;  t = ad * t;  d' = d + t;  fc = beta * |d'|;  fc = min_cutoff + fc;  r = two_pi * fc;
                        r = r * te;  a = r / (r + 1);  t = a * e;  h' = h + t.  Where h'x, h'y, d'x, d'y are all finite they
                        become the state; else the point is seeded afresh (a coordinate near FLT_MAX cannot poison it).
  valid and not seen    (or seeded afresh) h = (x, y), d = 0.
  either valid case     s = score, gap = 0, seen = 1; the output is (hx, hy, s).
  invalid, seen and gap < max_gap (hold)   gap += 1; the output is (hx, hy, s): the last filtered position and valid score.
  invalid otherwise     seen = 0, gap = 0; the output is the marker (-1, -1, 0).  h, d and s keep their bits, dead until
                        the next seed.
The filter is causal: frame f's output depends on frames <= f alone, so a live source loses no frame to it, and any
partition of a clip into pieces gives the whole clip's bits once the state is carried from piece to piece.  An output point
is either the marker or finite with x, y >= 0 and score >= threshold (h' lies between h and v: a <= 1 and rounding is
monotone), so the retargeter and the renderer read it as the smoother meant it."""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple, Optional

import numpy as np

from .pose_render_reference import KEYPOINTS, MAX_PEOPLE, as_source, check_keypoints_shape, check_threshold
from .pose_retarget_reference import MAX_RATE, parse_fps

F32 = np.float32
MAX_GAP = 65535
STATE_WORDS = 8                # 32 bytes per point: hx, hy, dx, dy, s, gap, seen, 0
HX, HY, DX, DY, S, GAP, SEEN = range(7)
RULES = ("filter", "seed", "reseed", "hold", "drop")


class Params(NamedTuple):
    num: int
    den: int
    period: np.float32
    min_cutoff: np.float32
    beta: np.float32
    kd: np.float32
    two_pi: np.float32
    threshold: np.float32
    max_gap: int


def _number(value, name: str) -> float:
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise ValueError(f"{name} must be a number, got {value!r}")
    return float(value)


def prepare(fps, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, max_gap=0, score_threshold=0.3) -> Params:
    """Every check that needs no keypoints, and the numbers the kernel is handed."""
    f = parse_fps(fps)
    if not (1 <= f.numerator <= MAX_RATE and 1 <= f.denominator <= MAX_RATE):
        raise ValueError(f"fps = {f.numerator}/{f.denominator}: both terms must be 1..{MAX_RATE}")
    mc, b, dc = _number(min_cutoff, "min_cutoff"), _number(beta, "beta"), _number(d_cutoff, "d_cutoff")
    with np.errstate(over="ignore"):
        mc32, b32, kd = F32(mc), F32(b), F32(2.0 * math.pi * dc) if math.isfinite(dc) else F32(np.nan)
    if not (math.isfinite(mc) and np.isfinite(mc32) and mc32 > 0):
        raise ValueError(f"min_cutoff must be finite and > 0 as a float32 (Hz), got {min_cutoff!r}")
    if not (math.isfinite(b) and np.isfinite(b32) and b32 >= 0):
        raise ValueError(f"beta must be finite and >= 0 as a float32, got {beta!r}")
    if not (math.isfinite(dc) and dc > 0 and np.isfinite(kd) and kd > 0):
        raise ValueError(f"d_cutoff must be finite and > 0 (Hz), with 2 pi d_cutoff a positive float32, got {d_cutoff!r}")
    if isinstance(max_gap, bool) or not isinstance(max_gap, numbers.Integral) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in 0..{MAX_GAP}, got {max_gap!r}")
    thr = check_threshold(score_threshold)
    return Params(f.numerator, f.denominator, F32(f.denominator / f.numerator), mc32, b32, kd, F32(2.0 * math.pi), F32(thr), int(max_gap))


def check_people(people) -> int:
    if isinstance(people, bool) or not isinstance(people, numbers.Integral) or not 1 <= people <= MAX_PEOPLE:
        raise ValueError(f"people must be 1..{MAX_PEOPLE}, got {people!r}")
    return int(people)


def fresh_state(people: int) -> np.ndarray:
    """The packed state of `people` people before their first frame: int32 [P, 134, 8], all zero."""
    return np.zeros((check_people(people), KEYPOINTS, STATE_WORDS), np.int32)


def state_bytes(people: int) -> int:
    """sf_pose_smooth_state_bytes: 32 bytes per point, 0 for people out of range."""
    return people * KEYPOINTS * STATE_WORDS * 4 if 1 <= people <= MAX_PEOPLE else 0


# ---------------------------------------------------------------------------------------------- the arithmetic
def frames(src: np.ndarray, state: np.ndarray, p: Params, counts: Optional[dict] = None) -> np.ndarray:
    """What one launch of the kernel computes: the piece's frames float32 [n, P, 134, 3] smoothed, from the packed `state`
    int32 [P, 134, 8], which it advances in place.  `counts`, a dict, gains how often each of RULES fired."""
    src = np.asarray(src, dtype=F32)
    if src.ndim != 4 or src.shape[2:] != (KEYPOINTS, 3):
        raise ValueError(f"src must be [n, P, {KEYPOINTS}, 3], got {src.shape}")
    people = src.shape[1]
    if state.dtype != np.int32 or state.shape != (people, KEYPOINTS, STATE_WORDS) or not state.flags.c_contiguous:
        raise ValueError(f"state must be contiguous int32 [{people}, {KEYPOINTS}, {STATE_WORDS}], got {state.dtype} {state.shape}")
    fl = state.view(F32)
    h, d, s = fl[..., HX:HY + 1].copy(), fl[..., DX:DY + 1].copy(), fl[..., S].copy()
    gap, seen = state[..., GAP].copy(), state[..., SEEN] != 0
    out = np.empty(src.shape, F32)
    tally = dict.fromkeys(RULES, 0)
    for f in range(src.shape[0]):
        x, y, sc = src[f, ..., 0], src[f, ..., 1], src[f, ..., 2]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(sc)
        ok &= np.where(ok, sc, 0) >= p.threshold
        ok &= (np.where(ok, x, 0) >= 0) & (np.where(ok, y, 0) >= 0)
        v = np.where(ok[..., None], src[f, ..., :2], F32(0)).astype(F32)
        te = ((gap + 1).astype(F32) * p.period)[..., None]
        with np.errstate(over="ignore", invalid="ignore"):
            e = v - h
            dx = e / te
            rd = p.kd * te
            ad = rd / (rd + F32(1))
            t = dx - d
            t = ad * t
            dn = d + t
            fc = p.beta * np.abs(dn)
            fc = p.min_cutoff + fc
            r = p.two_pi * fc
            r = r * te
            a = r / (r + F32(1))
            t = a * e
            hn = h + t
        assert hn.dtype == dn.dtype == F32
        filt = ok & seen & np.isfinite(hn).all(-1) & np.isfinite(dn).all(-1)
        seed = ok & ~filt
        hold = ~ok & seen & (gap < p.max_gap)
        for name, hit in zip(RULES, (filt, seed & ~seen, seed & seen, hold, ~ok & ~hold)):
            tally[name] += int(hit.sum())
        h = np.where(filt[..., None], hn, np.where(seed[..., None], v, h))
        d = np.where(filt[..., None], dn, np.where(seed[..., None], F32(0), d))
        s = np.where(ok, sc, s)
        gap = np.where(hold, gap + 1, 0).astype(np.int32)
        seen = ok | hold
        out[f, ..., :2] = np.where(seen[..., None], h, F32(-1))
        out[f, ..., 2] = np.where(seen, s, F32(0))
    fl[..., HX:HY + 1], fl[..., DX:DY + 1], fl[..., S] = h, d, s
    state[..., GAP], state[..., SEEN] = gap, seen
    if counts is not None:
        for name in RULES:
            counts[name] = counts.get(name, 0) + tally[name]
    return out


def smooth(keypoints, fps, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, max_gap=0, score_threshold=0.3) -> np.ndarray:
    """Keypoints [F, P, 134, 3] or [F, 134, 3] recorded at `fps` -> float32 [F, P, 134, 3], smoothed from a fresh state."""
    p = prepare(fps, min_cutoff, beta, d_cutoff, max_gap, score_threshold)
    k = as_source(keypoints)
    return frames(k, fresh_state(k.shape[1]), p)


class Stream:
    """`smooth` piece by piece: `push(piece)` returns the piece's frames smoothed, exactly len(piece) of them (the filter
    is causal, nothing is held back).  Any partition of a clip gives the bits of `smooth` on the whole clip."""

    def __init__(self, fps, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, max_gap=0, score_threshold=0.3):
        self.params = prepare(fps, min_cutoff, beta, d_cutoff, max_gap, score_threshold)
        self.frames_in = 0
        self.closed = False
        self.state: Optional[np.ndarray] = None

    def push(self, piece) -> np.ndarray:
        if self.closed:
            raise ValueError("the stream is closed")
        k = as_source(piece)
        if self.state is None:
            self.state = fresh_state(k.shape[1])
        elif k.shape[1] != self.state.shape[0]:
            raise ValueError(f"the stream holds {self.state.shape[0]} people, the piece {k.shape[1]}")
        out = frames(k, self.state, self.params)
        self.frames_in += len(k)
        return out

    def close(self) -> None:
        """Ends the stream.  Nothing further comes out: every frame has been returned by its push."""
        self.closed = True
