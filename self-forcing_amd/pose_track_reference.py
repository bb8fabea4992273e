"""The definition of the pose tracker's numbers (numpy, no GPU): the people a detector lists per frame, in any order ->
each person in one stable SLOT across frames, with a track id.  The reference project has no counterpart (its poses arrive
drawn); this is THIS PROJECT'S definition.  All arithmetic is float32 and every operation (sub, mul, add, div) is rounded
on its own, never fused, so the device (csrc/pose_track.hip) equals this file bit for bit.  The tracker does no arithmetic
on what it passes on: a slot's row is the matched detection's 134 x 3 floats, copied bit for bit.

source     float32 [F, P, 134, 3] or [F, 134, 3] = (x, y, score), DWPose's whole-body order, in the caller's units: the
           detections of each frame, in any order, P <= 8.
output     out float32 [F, S, 134, 3] and ids int32 [F, S], S = slots (1..8, default P).  Where a slot has no detection in
           a frame its row is the marker (-1, -1, 0) at all 134 points and its id is -1.
valid      a point, by the renderer's rule on the raw values: x, y, score finite; score >= score_threshold (fp32); x >= 0,
           y >= 0.  Only the 18 body points (0..17) take part in matching.  A detection is a PERSON iff at least min_points
           of its body points are valid; other rows (all markers, a lone hand) are ignored.
track      lives in a slot: the x, y and validity of the 18 body points of the last detection matched to it (replaced
           wholesale at each match, the bits of invalid points included), age = frames since that match, and its id.
cost       of (track t, person d), over the body points j = 0..17 in ascending order that are valid in both (n of them):
             dx = xd - xt;  dy = yd - yt;  q = dx * dx + dy * dy;  acc = acc + q       (acc starts at +0)
           w, h = max - min of the track's valid remembered x and y;  s2 = w * w + h * h;  cost = (acc / fp32(n)) / s2.
           The pair is ADMISSIBLE iff n >= min_common, s2 > 0 and finite, cost finite and cost <= gate2, where
           gate2 = fp32(gate * gate) is formed in double and rounded once.  Anything that overflows or is NaN is
           inadmissible (a box of infinite extent would otherwise match everything at cost 0).
one frame  1 match   repeat: among the admissible pairs of unassigned live tracks and unassigned persons take the smallest
                     key (the cost's float bits as unsigned, t, d) and assign it; stop when none is left.  A cost is finite
                     and >= +0, so its bits order as it does; ties go to the lower slot, then to the lower detection.
           2 age     a matched track gets age = 0; an unmatched live one age += 1 and dies (alive = 0) if age > max_age.
           3 birth   each unassigned person, in ascending detection order, takes the lowest slot that was free AT THE START
                     of this frame, with id = next_id & 0x7fffffff, next_id += 1 (mod 2^32); a person with no free slot is
                     dropped from this frame.
           4 emit    rows and ids; the memory of every slot that has a detection is replaced.
state      packed as the device holds it: int32 [S + 1, 40], zero-filled is fresh.  Row s < S: words 0..35 the float bits
           of x, y of the 18 remembered points, 36 the validity mask (bit j for point j), 37 age, 38 id, 39 alive.  Row S:
           next_id in word 0; its other words are not touched.  Dead slots keep their old bits.
A slot freed in frame f is not reused in frame f, so a slot is empty for at least max_age + 1 frames between two different
people, and a smoother with max_gap <= max_age never filters one person towards another.  Frame f's output depends on
frames <= f alone, so any partition of a clip into pieces gives the whole clip's bits once the state is carried along."""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple, Optional, Tuple

import numpy as np

from .pose_render_reference import KEYPOINTS, MAX_PEOPLE, as_source, check_keypoints_shape, check_threshold

F32 = np.float32
BODY = 18                      # the body points 0..17 are what is matched
MAX_AGE = 65535
STATE_WORDS = 40               # per slot: 36 float bits, mask, age, id, alive
MASK, AGE, ID, ALIVE = 36, 37, 38, 39
RULES = ("match", "birth", "lost", "freed", "overflow", "gated")
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


class Params(NamedTuple):
    slots: Optional[int]       # None: the P of the first piece
    gate2: np.float32
    max_age: int
    min_points: int
    min_common: int
    threshold: np.float32


def _integer(value, name: str, lo: int, hi: int) -> int:
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {value!r}")
    return int(value)


def check_slots(slots) -> int:
    return _integer(slots, "slots", 1, MAX_PEOPLE)


def prepare(slots=None, gate=0.5, max_age=2, min_points=4, min_common=3, score_threshold=0.3) -> Params:
    """Every check that needs no keypoints, and the numbers the kernel is handed."""
    if slots is not None:
        slots = check_slots(slots)
    if isinstance(gate, bool) or not isinstance(gate, numbers.Real):
        raise ValueError(f"gate must be a number, got {gate!r}")
    g = float(gate)
    with np.errstate(over="ignore"):
        gate2 = F32(g * g) if math.isfinite(g) else F32(np.nan)
    if not (math.isfinite(g) and g > 0 and np.isfinite(gate2) and gate2 > 0):
        raise ValueError(f"gate must be finite and > 0, with gate * gate a positive float32, got {gate!r}")
    max_age = _integer(max_age, "max_age", 0, MAX_AGE)
    min_points = _integer(min_points, "min_points", 1, BODY)
    min_common = _integer(min_common, "min_common", 1, BODY)
    thr = check_threshold(score_threshold)
    return Params(slots, gate2, max_age, min_points, min_common, F32(thr))


def fresh_state(slots: int) -> np.ndarray:
    """The packed state of `slots` slots before their first frame: int32 [S + 1, 40], all zero."""
    return np.zeros((check_slots(slots) + 1, STATE_WORDS), np.int32)


def state_bytes(slots: int) -> int:
    """sf_pose_track_state_bytes: 160 bytes per slot and 160 for next_id, 0 for slots out of range."""
    return (slots + 1) * STATE_WORDS * 4 if 1 <= slots <= MAX_PEOPLE else 0


def valid_points(body: np.ndarray, threshold) -> np.ndarray:
    """The renderer's rule on points [..., 3]."""
    x, y, sc = body[..., 0], body[..., 1], body[..., 2]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(sc)
    ok &= np.where(ok, sc, 0) >= threshold
    ok &= (np.where(ok, x, 0) >= 0) & (np.where(ok, y, 0) >= 0)
    return ok


def costs(mem: np.ndarray, body: np.ndarray, ok: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(cost float32 [S, P], n int [S, P], s2 float32 [S]) of the slots' memory int32 [S, 40] against a frame's body
    points [P, 18, 3] with validity `ok` [P, 18]."""
    fl = mem.view(F32)
    tx, ty = fl[:, 0:2 * BODY:2], fl[:, 1:2 * BODY:2]
    tm = (mem[:, MASK, None] >> np.arange(BODY)) & 1 != 0
    common = tm[:, None, :] & ok[None, :, :]
    x, y = body[..., 0], body[..., 1]
    acc = np.zeros(common.shape[:2], F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(BODY):
            dx = x[None, :, j] - tx[:, None, j]
            dy = y[None, :, j] - ty[:, None, j]
            q = dx * dx + dy * dy
            acc = np.where(common[..., j], acc + q, acc)
        w = np.where(tm, tx, F32(-np.inf)).max(1) - np.where(tm, tx, F32(np.inf)).min(1)
        h = np.where(tm, ty, F32(-np.inf)).max(1) - np.where(tm, ty, F32(np.inf)).min(1)
        s2 = w * w + h * h
        n = common.sum(-1)
        cost = (acc / n.astype(F32)) / s2[:, None]
    assert acc.dtype == s2.dtype == cost.dtype == F32
    return cost, n, s2


# ---------------------------------------------------------------------------------------------- one piece
def frames(src: np.ndarray, state: np.ndarray, p: Params, counts: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """What one call of the kernels computes: the piece's detections float32 [n, P, 134, 3] put into slots, (out float32
    [n, S, 134, 3], ids int32 [n, S]), from the packed `state` int32 [S + 1, 40], which it advances in place.  `counts`, a
    dict, gains how often each of RULES fired: matches, births, tracks that went unmatched and lived on, tracks that died,
    persons dropped for want of a free slot, and pairs of a live track and a person that only the gate kept apart."""
    src = np.asarray(src, dtype=F32)
    if src.ndim != 4 or src.shape[2:] != (KEYPOINTS, 3) or not 1 <= src.shape[1] <= MAX_PEOPLE:
        raise ValueError(f"src must be [n, P, {KEYPOINTS}, 3] with P <= {MAX_PEOPLE}, got {src.shape}")
    if not isinstance(state, np.ndarray) or state.dtype != np.int32 or state.ndim != 2 or state.shape[1] != STATE_WORDS \
            or not 2 <= state.shape[0] <= MAX_PEOPLE + 1 or not state.flags.c_contiguous:
        raise ValueError(f"state must be contiguous int32 [S + 1, {STATE_WORDS}] with S <= {MAX_PEOPLE}")
    slots, people = state.shape[0] - 1, src.shape[1]
    if p.slots is not None and p.slots != slots:
        raise ValueError(f"the state holds {slots} slots, the parameters say {p.slots}")
    mem = state[:slots]
    out = np.empty((src.shape[0], slots, KEYPOINTS, 3), F32)
    ids = np.empty((src.shape[0], slots), np.int32)
    tally = dict.fromkeys(RULES, 0)
    pair = (np.arange(slots, dtype=np.uint64)[:, None] << np.uint64(3)) | np.arange(people, dtype=np.uint64)[None, :]
    for f in range(src.shape[0]):
        body = src[f, :, :BODY]
        ok = valid_points(body, p.threshold)
        person = ok.sum(1) >= p.min_points
        alive = mem[:, ALIVE] != 0
        cost, n, s2 = costs(mem, body, ok)
        with np.errstate(invalid="ignore"):
            near = alive[:, None] & person[None, :] & (n >= p.min_common) & ((s2 > 0) & np.isfinite(s2))[:, None] & np.isfinite(cost)
            admissible = near & (cost <= p.gate2)
        tally["gated"] += int((near & ~admissible).sum())
        key = np.where(admissible, (cost.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pair, _NONE)
        assigned = np.full(slots, -1)
        taken = np.zeros(people, bool)
        while True:                                                  # 1 match
            t, d = np.unravel_index(np.argmin(key), key.shape)
            if key[t, d] == _NONE:
                break
            assigned[t], taken[d] = d, True
            key[t, :], key[:, d] = _NONE, _NONE
            tally["match"] += 1
        for t in range(slots):                                       # 2 age
            if alive[t] and assigned[t] < 0:
                mem[t, AGE] += 1
                if mem[t, AGE] > p.max_age:
                    mem[t, ALIVE] = 0
                    tally["freed"] += 1
                else:
                    tally["lost"] += 1
        free = [t for t in range(slots) if not alive[t]]             # 3 birth: free at the start of this frame
        for d in range(people):
            if person[d] and not taken[d]:
                if not free:
                    tally["overflow"] += 1
                    continue
                t = free.pop(0)
                next_id = int(state[slots, 0]) & 0xFFFFFFFF
                assigned[t] = d
                mem[t, ID] = next_id & 0x7FFFFFFF
                state[slots, 0] = np.uint32((next_id + 1) & 0xFFFFFFFF).view(np.int32)
                tally["birth"] += 1
        for t in range(slots):                                       # 4 emit
            d = assigned[t]
            if d < 0:
                out[f, t], ids[f, t] = F32([-1, -1, 0]), -1
                continue
            out[f, t], ids[f, t] = src[f, d], mem[t, ID]
            mem[t, :2 * BODY] = body[d, :, :2].reshape(-1).view(np.int32)
            mem[t, MASK] = int((ok[d] << np.arange(BODY)).sum())
            mem[t, AGE], mem[t, ALIVE] = 0, 1
    if counts is not None:
        for name in RULES:
            counts[name] = counts.get(name, 0) + tally[name]
    return out, ids


def track(keypoints, slots=None, gate=0.5, max_age=2, min_points=4, min_common=3, score_threshold=0.3,
          counts: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Keypoints [F, P, 134, 3] or [F, 134, 3] -> (float32 [F, S, 134, 3], int32 [F, S]), tracked from a fresh state."""
    p = prepare(slots, gate, max_age, min_points, min_common, score_threshold)
    k = as_source(keypoints)
    return frames(k, fresh_state(k.shape[1] if p.slots is None else p.slots), p, counts)


class Stream:
    """`track` piece by piece: `push(piece)` returns the piece's frames in slots and leaves their ids in `ids`.  Any
    partition of a clip gives the bits of `track` on the whole clip."""

    def __init__(self, slots=None, gate=0.5, max_age=2, min_points=4, min_common=3, score_threshold=0.3):
        self.params = prepare(slots, gate, max_age, min_points, min_common, score_threshold)
        self.frames_in = 0
        self.closed = False
        self.people: Optional[int] = None
        self.state: Optional[np.ndarray] = None
        self.ids: Optional[np.ndarray] = None

    def push(self, piece) -> np.ndarray:
        if self.closed:
            raise ValueError("the stream is closed")
        k = as_source(piece)
        if self.state is None:
            self.people = k.shape[1]
            self.state = fresh_state(self.people if self.params.slots is None else self.params.slots)
        elif k.shape[1] != self.people:
            raise ValueError(f"the stream holds {self.people} people, the piece {k.shape[1]}")
        out, self.ids = frames(k, self.state, self.params)
        self.frames_in += len(k)
        return out

    def close(self) -> None:
        """Ends the stream.  Nothing further comes out: every frame has been returned by its push."""
        self.closed = True
