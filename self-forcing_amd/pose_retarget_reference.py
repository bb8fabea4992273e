"""The definition of the pose retargeter's numbers (numpy, no GPU): driving keypoints -> keypoints of the reference person's
proportions and position, on the generator's timeline.  The reference project has no counterpart (its poses arrive drawn and
aligned); this is THIS PROJECT'S definition, in the spirit of the pose alignment of UniAnimate-style pipelines.  All
arithmetic is float32 and every operation (sub, mul, add, div, sqrt) is rounded on its own, never fused, so the device
(csrc/pose_retarget.hip) equals this file bit for bit.

source     float32 [F, P, 134, 3] or [F, 134, 3] = (x, y, score), DWPose's whole-body order (pose_render_reference).
reference  float32 [Pr, 134, 3] or [134, 3], Pr = P or 1 (one reference person serves every source person).
valid      the renderer's rule on the raw values: x, y, score finite; score >= score_threshold (fp32); x >= 0, y >= 0.
           An invalid output point is written as (-1, -1, 0).
lift       to pixels of the (H, W) output, one fp32 multiply per coordinate by factors formed in double and rounded once:
           reference (W, H) when normalized else (1, 1); source normalized (W, H), or (H * ws / hs, H) with
           source_size = (hs, ws) (another aspect is not stretched); source in pixels (1, 1), or (H / hs, H / hs).
resample   source_fps / target_fps = num / den in lowest terms, 1 <= num, den <= 65535.  Output frame j sits at source
           position j * num / den: i0 = j * num // den, rem = j * num % den, i1 = i0 + (rem != 0); it exists iff i1 <= F - 1,
           so F_out = (F - 1) * den // num + 1.  Per point, lifted: rem == 0 copies frame i0; both ends valid:
           w = fp32(rem) / fp32(den), p = a + w * (b - a) (three roundings), score = the smaller one; one end valid: it is
           taken when it is the nearer one (a when 2 rem <= den, b when 2 rem > den), else the point is invalid.
fit        per person, from the lifted source frame 0 (S0) and the lifted reference (R), over the 17 LIMBS:
           len(X, a, b) = sqrt(fp32(dx * dx) + fp32(dy * dy)); an edge is usable iff both ends are valid in S0 and in R and
           len(S0) > 0.  g = sum len(R) / sum len(S0) over the usable edges in LIMBS order (1 with none).  The ratio of a
           symmetric GROUP of edges is (r0 + r1) * 0.5f of its usable members' len(R) / len(S0), the one usable member's,
           or g; hands scale by the forearms' ratio, faces by the nose-eye ratio, feet by g.  The anchor is the neck
           (point 1): where it is invalid in S0 or in R the person is not retargeted (lifted and resampled only).
retarget   of a resampled frame Q, sim(q) = R[1] + g * (q - S0[1]): new[1] = sim(Q[1]); along LIMBS (a tree rooted at the
           neck, parents first) new[b] = new[a] + r_e * (Q[b] - Q[a]) when Q[a] and Q[b] are valid, sim(Q[b]) when only
           Q[b] is, invalid when Q[b] is; the attached points (ATTACHED) by the same rule from their anchor.  Scores pass.
The output is float32 [F_out, P, 134, 3] in output pixels, to be drawn with normalized=False; a retargeted point that lands
at a negative coordinate is what the renderer already calls missing."""
from __future__ import annotations

import numbers
import re
from fractions import Fraction
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .pose_render_reference import KEYPOINTS, LIMBS, MAX_PEOPLE, as_source, check_keypoints_shape, check_size, check_threshold

F32 = np.float32
MAX_RATE = 65535               # SF_POSE_RETARGET_MAX_RATE: num and den of source_fps / target_fps
NECK = 1
GROUPS = ((0, 1), (2, 4), (3, 5), (6, 9), (7, 10), (8, 11), (12,), (13, 15), (14, 16))      # symmetric LIMBS indices
GROUP_OF = tuple(next(g for g, members in enumerate(GROUPS) if e in members) for e in range(len(LIMBS)))
HAND_GROUP, FACE_GROUP = 2, 7  # the forearms {3, 5}, nose-eye {13, 15}
# (first point, one past the last, anchor, ratio: a GROUPS index or -1 for g)
ATTACHED = ((18, 21, 13, -1), (21, 24, 10, -1), (24, 92, 0, FACE_GROUP), (92, 113, 7, HAND_GROUP), (113, 134, 4, HAND_GROUP))


class Params(NamedTuple):
    h: int
    w: int
    num: int
    den: int
    src_sx: np.float32
    src_sy: np.float32
    ref_sx: np.float32
    ref_sy: np.float32
    threshold: np.float32
    align: bool


# ---------------------------------------------------------------------------------------------- arguments
def parse_fps(value) -> Fraction:
    """An int, a Fraction or a string "30" / "30000/1001" -> a positive Fraction."""
    if isinstance(value, str):
        m = re.fullmatch(r"\s*(\d+)\s*(?:/\s*(\d+)\s*)?", value)
        if not m or (m.group(2) is not None and int(m.group(2)) == 0):
            raise ValueError(f"fps must be N or N/D with positive integers, got {value!r}")
        f = Fraction(int(m.group(1)), int(m.group(2) or 1))
    elif isinstance(value, Fraction) or (isinstance(value, numbers.Integral) and not isinstance(value, bool)):
        f = Fraction(value)
    else:
        raise ValueError(f"fps must be an int, a fractions.Fraction or a string N/D, got {value!r}")
    if f <= 0:
        raise ValueError(f"fps must be positive, got {value!r}")
    return f


def rate(source_fps, target_fps) -> Tuple[int, int]:
    """(num, den) of source_fps / target_fps in lowest terms."""
    r = parse_fps(source_fps) / parse_fps(target_fps)
    if not (1 <= r.numerator <= MAX_RATE and 1 <= r.denominator <= MAX_RATE):
        raise ValueError(f"source_fps / target_fps = {r.numerator}/{r.denominator}: both terms must be 1..{MAX_RATE}")
    return r.numerator, r.denominator


def frames_out(frames: int, num: int, den: int) -> int:
    """The output frames a clip of `frames` source frames gives: those whose later neighbour i1 exists."""
    return 0 if frames <= 0 else ((frames - 1) * den) // num + 1


def plan(frames_before: int, n: int, num: int, den: int) -> Tuple[int, int]:
    """(first_out, n_out): the output frames that become final once n more source frames follow `frames_before`
    (sf_pose_retarget_plan)."""
    if frames_before < 0 or n < 0 or not (1 <= num <= MAX_RATE and 1 <= den <= MAX_RATE):
        raise ValueError(f"plan: frames_before={frames_before}, n={n} (>= 0), num={num}, den={den} (1..{MAX_RATE})")
    first = frames_out(frames_before, num, den)
    return first, frames_out(frames_before + n, num, den) - first


def check_source_size(source_size) -> Optional[Tuple[float, float]]:
    if source_size is None:
        return None
    try:
        ok = len(source_size) == 2 and all(np.isfinite(float(v)) and float(v) > 0 for v in source_size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"source_size must be (height, width), both positive, got {source_size!r}")
    return float(source_size[0]), float(source_size[1])


def prepare(size, source_fps=16, target_fps=16, align: bool = True, normalized: bool = True, score_threshold: float = 0.3, source_size=None) -> Params:
    """Every check that needs no keypoints, and the numbers the kernel is handed."""
    h, w = check_size(size)
    thr = check_threshold(score_threshold)
    num, den = rate(source_fps, target_fps)
    ss = check_source_size(source_size)
    if normalized:
        ref = (float(w), float(h))
        src = ref if ss is None else (h * ss[1] / ss[0], float(h))
    else:
        ref = (1.0, 1.0)
        src = ref if ss is None else (h / ss[0], h / ss[0])
    return Params(h, w, num, den, F32(src[0]), F32(src[1]), F32(ref[0]), F32(ref[1]), F32(thr), bool(align))


def check_reference_shape(shape: Sequence[int], people: Optional[int] = None) -> int:
    """Pr of a reference array's shape, [Pr, 134, 3] or [134, 3]; with `people`, against the source's P."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[1:] != (KEYPOINTS, 3) or not 1 <= shape[0] <= MAX_PEOPLE or (people is not None and shape[0] not in (1, people)):
        raise ValueError(f"ref_keypoints must be [Pr, {KEYPOINTS}, 3] or [{KEYPOINTS}, 3] with Pr = 1 or the source's "
                         f"{'P' if people is None else people} people (at most {MAX_PEOPLE}), got {shape}")
    return shape[0]


# ---------------------------------------------------------------------------------------------- the arithmetic
def lift(k: np.ndarray, sx: np.float32, sy: np.float32, threshold: np.float32):
    """float32 [..., 3] -> (xy float32 [..., 2] lifted, score [...], valid [...]); xy and score are 0 where invalid."""
    x, y, s = k[..., 0], k[..., 1], k[..., 2]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(s)
    ok &= np.where(ok, s, 0) >= threshold
    ok &= (np.where(ok, x, 0) >= 0) & (np.where(ok, y, 0) >= 0)
    with np.errstate(over="ignore"):
        xy = np.stack([np.where(ok, x, 0).astype(F32) * sx, np.where(ok, y, 0).astype(F32) * sy], axis=-1)
    return xy, np.where(ok, s, 0).astype(F32), ok


def resample(a, b, rem: int, den: int):
    """Two lifted frames (xy, score, valid) -> the frame at rem / den of the way from a to b."""
    (axy, asc, aok), (bxy, bsc, bok) = a, b
    if rem == 0:
        return axy, asc, aok
    w = F32(rem) / F32(den)
    with np.errstate(over="ignore", invalid="ignore"):
        t = bxy - axy
        t = w * t
        mid = axy + t
    both = aok & bok
    take_a = aok & ~bok & (2 * rem <= den)
    take_b = bok & ~aok & (2 * rem > den)
    xy = np.where(both[..., None], mid, np.where(take_a[..., None], axy, np.where(take_b[..., None], bxy, F32(0))))
    sc = np.where(both, np.where(bsc < asc, bsc, asc), np.where(take_a, asc, np.where(take_b, bsc, F32(0))))
    return xy.astype(F32), sc.astype(F32), both | take_a | take_b


def length(xy: np.ndarray, a: int, b: int) -> np.float32:
    dx, dy = xy[b, 0] - xy[a, 0], xy[b, 1] - xy[a, 1]
    return np.sqrt(F32(dx * dx) + F32(dy * dy))


class Fit(NamedTuple):
    retarget: bool             # the neck is valid in S0 and in R
    g: np.float32
    ratio: Tuple[np.float32, ...]      # per GROUPS entry


def fit(s0, r) -> Fit:
    """One person's fit from the lifted (xy [134, 2], score, valid [134]) of source frame 0 and of the reference."""
    (sxy, _, sok), (rxy, _, rok) = s0, r
    sum_r = sum_s = F32(0)
    usable, ratios = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for a, b in LIMBS:
            ok = bool(sok[a] and sok[b] and rok[a] and rok[b])
            ls = length(sxy, a, b) if ok else F32(0)
            ok = ok and bool(ls > 0)
            lr = length(rxy, a, b) if ok else F32(0)
            if ok:
                sum_r, sum_s = F32(sum_r + lr), F32(sum_s + ls)
            usable.append(ok)
            ratios.append(F32(lr / ls) if ok else F32(0))
        g = F32(sum_r / sum_s) if any(usable) else F32(1)
        group = []
        for members in GROUPS:
            have = [ratios[e] for e in members if usable[e]]
            group.append(F32(F32(have[0] + have[1]) * F32(0.5)) if len(have) == 2 else (have[0] if have else g))
    return Fit(bool(sok[NECK] and rok[NECK]), g, tuple(group))


def retarget_frame(q, f: Fit, s0_neck: np.ndarray, r_neck: np.ndarray) -> np.ndarray:
    """One person's resampled frame (xy [134, 2], score, valid) -> the retargeted xy [134, 2] (the validity is Q's)."""
    qxy, _, qok = q
    new = np.zeros_like(qxy)
    with np.errstate(over="ignore", invalid="ignore"):
        def sim(p):
            t = p - s0_neck
            t = f.g * t
            return (r_neck + t).astype(F32)

        def step(first, last, a, ratio):
            pts = slice(first, last)
            if qok[a]:
                t = qxy[pts] - qxy[a]
                t = ratio * t
                new[pts] = new[a] + t
            else:
                new[pts] = sim(qxy[pts])

        new[NECK] = sim(qxy[NECK])
        for e, (a, b) in enumerate(LIMBS):
            step(b, b + 1, a, f.ratio[GROUP_OF[e]])
        for first, last, a, grp in ATTACHED:
            step(first, last, a, f.g if grp < 0 else f.ratio[grp])
    return new


def frames(src: np.ndarray, src0: int, first: np.ndarray, ref: np.ndarray, out0: int, n_out: int, p: Params) -> np.ndarray:
    """What one launch of the kernel computes: output frames [out0, out0 + n_out) from the source frames
    [src0, src0 + len(src)) (float32 [n, P, 134, 3]), the clip's frame 0 `first` [P, 134, 3] and the reference [Pr, 134, 3]."""
    people = src.shape[1]
    out = np.empty((n_out, people, KEYPOINTS, 3), F32)
    if n_out == 0:
        return out
    i_lo, i_hi = (out0 * p.num) // p.den, -((-(out0 + n_out - 1) * p.num) // p.den)
    if i_lo < src0 or i_hi > src0 + len(src) - 1:
        raise ValueError(f"output frames [{out0}, {out0 + n_out}) read source frames [{i_lo}, {i_hi}], the piece holds [{src0}, {src0 + len(src)})")
    s0 = lift(first, p.src_sx, p.src_sy, p.threshold)
    r = lift(np.broadcast_to(ref, (people,) + ref.shape[1:]), p.ref_sx, p.ref_sy, p.threshold)
    fits = [fit(tuple(v[q] for v in s0), tuple(v[q] for v in r)) for q in range(people)] if p.align else None
    for j in range(out0, out0 + n_out):
        i0, rem = divmod(j * p.num, p.den)
        a = lift(src[i0 - src0], p.src_sx, p.src_sy, p.threshold)
        b = lift(src[i0 + (rem != 0) - src0], p.src_sx, p.src_sy, p.threshold)
        xy, sc, ok = resample(a, b, rem, p.den)
        if p.align:
            xy = xy.copy()
            for q in range(people):
                if fits[q].retarget:
                    xy[q] = retarget_frame((xy[q], sc[q], ok[q]), fits[q], s0[0][q, NECK], r[0][q, NECK])
        o = out[j - out0]
        o[..., :2] = np.where(ok[..., None], xy, F32(-1))
        o[..., 2] = np.where(ok, sc, F32(0))
    return out


def as_reference(ref_keypoints, people: int) -> np.ndarray:
    r = np.asarray(ref_keypoints, dtype=F32)
    return r.reshape(check_reference_shape(r.shape, people), KEYPOINTS, 3)


def retarget(keypoints, ref_keypoints, size, source_fps=16, target_fps=16, align: bool = True, normalized: bool = True,
             score_threshold: float = 0.3, source_size=None) -> np.ndarray:
    """Source keypoints [F, P, 134, 3] or [F, 134, 3] -> float32 [F_out, P, 134, 3] in pixels of the (H, W) output."""
    p = prepare(size, source_fps, target_fps, align, normalized, score_threshold, source_size)
    k = as_source(keypoints)
    ref = as_reference(ref_keypoints, k.shape[1])
    return frames(k, 0, k[0], ref, 0, frames_out(len(k), p.num, p.den), p)


class Stream:
    """`retarget` piece by piece: `push(piece)` returns the output frames that became final (frame j is final once source
    frame i1(j) is in), possibly none.  Any partition of a clip gives the bits of `retarget` on the whole clip."""

    def __init__(self, ref_keypoints, size, source_fps=16, target_fps=16, align: bool = True, normalized: bool = True,
                 score_threshold: float = 0.3, source_size=None):
        self.params = prepare(size, source_fps, target_fps, align, normalized, score_threshold, source_size)
        self._ref_in = np.array(ref_keypoints, dtype=F32)
        check_reference_shape(self._ref_in.shape)
        self.frames_in = self.frames_out = 0
        self.closed = False
        self._first = self._last = self._ref = None

    def push(self, piece) -> np.ndarray:
        if self.closed:
            raise ValueError("the stream is closed")
        k = as_source(piece)
        if self._first is None:
            self._ref = as_reference(self._ref_in, k.shape[1])
            self._first = k[0].copy()
        elif k.shape[1] != self._first.shape[0]:
            raise ValueError(f"the stream holds {self._first.shape[0]} people, the piece {k.shape[1]}")
        window, src0 = (k, 0) if self._last is None else (np.concatenate([self._last[None], k]), self.frames_in - 1)
        out0, n_out = plan(self.frames_in, len(k), self.params.num, self.params.den)
        assert out0 == self.frames_out
        out = frames(window, src0, self._first, self._ref, out0, n_out, self.params)
        self._last = k[-1].copy()
        self.frames_in += len(k)
        self.frames_out += n_out
        return out

    def close(self) -> None:
        """Ends the stream.  Nothing further comes out: every frame that can be computed has been returned."""
        self.closed = True
