"""Host tests of the pose tracker: the definition `pose_track_reference` against a scalar transcription of its rules, what
it promises (a shuffled clip comes back in order; the life of a track; ties; edge values; invariants over random clips;
partition invariance), `prepare`'s refusals, the C entry points' argument checks (they return before any launch), and the
Python surface as far as it needs no device.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_render_reference as pr
from self_forcing_amd import pose_track_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MARKER = np.array([-1, -1, 0], F32)
BODY = 18


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def people(seed, frames, centers):
    """Seeded skeletons [frames, len(centers), 134, 3], every point valid: necks at x = centers, limbs 0.03..0.08 long, the
    other points within 0.08 of the neck; each person drifts by a CONSTANT step of up to 0.004 per frame, with jitter of 0.004"""
    rng = np.random.default_rng(seed)
    k = np.zeros((frames, len(centers), 134, 3), F32)
    for q, cx in enumerate(centers):
        xy = np.zeros((134, 2))
        xy[1] = (cx, rng.uniform(0.4, 0.6))
        for a, b in pr.LIMBS:
            angle, length = rng.uniform(0, 2 * np.pi), rng.uniform(0.03, 0.08)
            xy[b] = xy[a] + length * np.array([np.cos(angle), np.sin(angle)])
        xy[BODY:] = xy[1] + rng.uniform(-0.08, 0.08, (134 - BODY, 2))
        drift = rng.uniform(-0.004, 0.004, 2)
        for f in range(frames):
            k[f, q, :, :2] = np.abs(xy + f * drift + rng.uniform(-0.004, 0.004, (134, 2)))
    k[..., 2] = rng.uniform(0.5, 1.0, k.shape[:3])
    return k


def shuffled(k, rng, first=1):
    """The people of every frame from `first` on in a seeded random order"""
    out = k.copy()
    for f in range(first, len(k)):
        out[f] = k[f, rng.permutation(k.shape[1])]
    return out


def crowd(seed, frames, count, pixels=False):
    """A clip for the tracker to go wrong on: `count` people 0.8 / count apart, 5 % of the points dropped, people who leave for
    one to four frames, people who jump by 0.15..0.4 (a new person to the tracker) and by 0.03..0.06 (the gate decides), the
    order shuffled in every frame"""
    rng = np.random.default_rng(seed)
    k = people(seed, frames, tuple(0.1 + 0.8 * (q + 0.5) / count for q in range(count)))
    for q in range(count):
        shift = np.zeros(2)
        for f in range(1, frames):
            u = rng.random()
            if u < 0.12:
                shift = shift + rng.uniform(0.15, 0.4, 2) * rng.choice([-1, 1], 2)
            elif u < 0.3:
                shift = shift + rng.uniform(0.03, 0.06, 2) * rng.choice([-1, 1], 2)
            k[f, q, :, :2] = np.abs(k[f, q, :, :2] + shift.astype(F32))
    k[rng.random(k.shape[:3]) < 0.05] = MARKER
    gone = rng.random(k.shape[:2]) < 0.1
    for _ in range(3):
        gone[1:] |= gone[:-1] & (rng.random(gone[1:].shape) < 0.5)
    k[gone] = MARKER
    if pixels:
        k[..., :2] *= F32([160, 96])
    return shuffled(k, rng, 0)


# ============================================================================================== a scalar transcription
def scalar_valid(pt, thr):
    x, y, s = (F32(v) for v in pt)
    return bool(np.isfinite(x) and np.isfinite(y) and np.isfinite(s) and s >= thr and x >= 0 and y >= 0)


def scalar_track(src, slots, gate=0.5, max_age=2, min_points=4, min_common=3, thr=0.3, counts=None):
    """The issue's rules one number at a time: (out, ids, packed state)"""
    thr, gate2 = F32(thr), F32(float(gate) * float(gate))
    n_frames, count = src.shape[:2]
    alive, age, tid = [False] * slots, [0] * slots, [0] * slots
    mem = [[(F32(0), F32(0), False)] * BODY for _ in range(slots)]
    next_id = 0
    out, ids = np.empty((n_frames, slots, 134, 3), F32), np.empty((n_frames, slots), np.int32)
    c = dict.fromkeys(tr.RULES, 0)
    for f in range(n_frames):
        det = src[f]
        ok = [[scalar_valid(det[d, j], thr) for j in range(BODY)] for d in range(count)]
        person = [sum(ok[d]) >= min_points for d in range(count)]
        keys = {}
        for t in range(slots):
            if not alive[t]:
                continue
            xs, ys = [m[0] for m in mem[t] if m[2]], [m[1] for m in mem[t] if m[2]]
            w, h = F32(max(xs) - min(xs)), F32(max(ys) - min(ys))
            with np.errstate(all="ignore"):
                s2 = F32(F32(w * w) + F32(h * h))
            for d in range(count):
                if not person[d]:
                    continue
                acc, n = F32(0), 0
                with np.errstate(all="ignore"):
                    for j in range(BODY):
                        if mem[t][j][2] and ok[d][j]:
                            dx, dy = F32(det[d, j, 0] - mem[t][j][0]), F32(det[d, j, 1] - mem[t][j][1])
                            acc = F32(acc + F32(F32(dx * dx) + F32(dy * dy)))
                            n += 1
                    if n < min_common or not (s2 > 0 and np.isfinite(s2)):
                        continue
                    cost = F32(F32(acc / F32(n)) / s2)
                if not np.isfinite(cost):
                    continue
                if cost <= gate2:
                    keys[(int(cost.view(np.uint32)), t, d)] = None
                else:
                    c["gated"] += 1
        assign, used = [-1] * slots, [False] * count
        while True:
            left = [k for k in keys if assign[k[1]] < 0 and not used[k[2]]]
            if not left:
                break
            _, t, d = min(left)
            assign[t], used[d] = d, True
            c["match"] += 1
        free = [t for t in range(slots) if not alive[t]]
        for t in range(slots):
            if alive[t] and assign[t] < 0:
                age[t] += 1
                if age[t] > max_age:
                    alive[t] = False
                    c["freed"] += 1
                else:
                    c["lost"] += 1
        for d in range(count):
            if person[d] and not used[d]:
                if not free:
                    c["overflow"] += 1
                    continue
                t = free.pop(0)
                assign[t], used[d], tid[t] = d, True, next_id & 0x7FFFFFFF
                next_id = (next_id + 1) & 0xFFFFFFFF
                c["birth"] += 1
        for t in range(slots):
            d = assign[t]
            if d < 0:
                out[f, t], ids[f, t] = MARKER, -1
                continue
            out[f, t], ids[f, t] = det[d], tid[t]
            mem[t] = [(det[d, j, 0], det[d, j, 1], ok[d][j]) for j in range(BODY)]
            alive[t], age[t] = True, 0
    state = np.zeros((slots + 1, 40), np.int32)
    for t in range(slots):
        state[t, :36] = np.array([v for m in mem[t] for v in m[:2]], F32).view(np.int32)
        state[t, 36:] = sum(1 << j for j in range(BODY) if mem[t][j][2]), age[t], tid[t], alive[t]
    state[slots, 0] = np.uint32(next_id).view(np.int32)
    if counts is not None:
        counts.update(c)
    return out, ids, state


@pytest.mark.parametrize("count,slots", [(1, 1), (2, 2), (3, 2), (2, 3), (5, 8), (8, 8)])
def test_the_vectorised_definition_equals_a_scalar_transcription(count, slots):
    total = dict.fromkeys(tr.RULES, 0)
    for pixels, max_age, gate in ((False, 2, 0.5), (True, 0, 0.25), (False, 1, 1.0)):
        k = crowd(100 * count + slots, 12, count, pixels)
        want_counts, got_counts = {}, {}
        want, want_ids, want_state = scalar_track(k, slots, gate, max_age, counts=want_counts)
        state = tr.fresh_state(slots)
        got, got_ids = tr.frames(k, state, tr.prepare(slots, gate, max_age), got_counts)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_ids, want_ids) and got_ids.dtype == np.int32
        assert np.array_equal(state, want_state), np.argwhere(state != want_state)
        assert got_counts == want_counts
        for name in tr.RULES:
            total[name] += got_counts[name]
        again, again_ids = tr.track(k, slots, gate, max_age)
        assert np.array_equal(bits(again), bits(want)) and np.array_equal(again_ids, want_ids)
    assert total["match"] > 0 and total["birth"] > 0 and total["freed"] > 0 and total["gated"] > 0, total


def test_gate_is_squared_in_double_and_rounded_once():
    for gate in (0.5, 0.1, 1 / 3, 2.0, 1e-3):
        assert tr.prepare(gate=gate).gate2 == F32(float(gate) * float(gate)) and tr.prepare(gate=gate).gate2.dtype == F32
    assert tr.prepare(gate=0.1).gate2 != F32(F32(0.1) * F32(0.1))
    p = tr.prepare()
    assert (p.slots, p.gate2, p.max_age, p.min_points, p.min_common, p.threshold) == (None, F32(0.25), 2, 4, 3, F32(0.3))


# ============================================================================================== what it is for
@pytest.mark.parametrize("seed", range(20))
def test_a_shuffled_clip_comes_back_in_order(seed):
    k = people(seed, 31, (0.2, 0.5, 0.8))
    rng = np.random.default_rng(100 + seed)
    k[rng.random(k.shape[:3]) < 0.05] = MARKER
    counts = {}
    out, ids = tr.track(shuffled(k, rng), counts=counts)
    assert np.array_equal(bits(out), bits(k)) and (ids == np.arange(3)).all()
    assert counts == dict(match=90, birth=3, lost=0, freed=0, overflow=0, gated=counts["gated"])


def lifecycle_clip(seed=3):
    k = people(seed, 31, (0.2, 0.5, 0.8))
    k[10:12, 1] = MARKER                                                                 # gone for 2 frames
    k[20:23, 2] = MARKER                                                                 # gone for 3
    return k


def test_a_person_gone_for_max_age_frames_keeps_slot_and_id_and_a_longer_absence_ends_the_track():
    k = lifecycle_clip()
    rng = np.random.default_rng(5)
    counts = {}
    out, ids = tr.track(shuffled(k, rng), slots=4, max_age=2, counts=counts)
    assert np.array_equal(bits(out[:, :3]), bits(k)) and (out[:, 3] == MARKER).all() and (ids[:, 3] == -1).all()
    assert (ids[:, 0] == 0).all() and (ids[:10, 1] == 1).all() and (ids[10:12, 1] == -1).all() and (ids[12:, 1] == 1).all()
    # three frames away: markers for exactly those frames, then a new id in the lowest free slot, which is the old one
    assert (ids[:20, 2] == 2).all() and (ids[20:23, 2] == -1).all() and (ids[23:, 2] == 3).all()
    assert (out[20:23, 2] == MARKER).all()
    assert counts["birth"] == 4 and counts["freed"] == 1 and counts["lost"] == 4 and counts["overflow"] == 0


def test_a_newcomer_in_the_frame_that_frees_a_slot_takes_the_next_free_slot():
    k = lifecycle_clip()
    k[22:, 2] = k[23, 2]                                                                 # someone stands still from frame 22 on ...
    k[22:, 2, :, 0] += F32(0.3)                                                          # ... far from where person 2 was
    out, ids = tr.track(k, slots=4, max_age=2)
    assert ids[21, 2] == -1 and ids[22, 2] == -1 and ids[22, 3] == 3                     # slot 2 is freed in frame 22 and not reused in it
    assert (ids[22:, 3] == 3).all() and (ids[23:, 2] == -1).all() and np.array_equal(bits(out[22:, 3]), bits(k[22:, 2]))
    out, ids = tr.track(k, slots=3, max_age=2)                                           # with no other slot the newcomer waits a frame
    assert ids[22, 2] == -1 and (ids[23:, 2] == 3).all() and (out[22, 2] == MARKER).all()


def test_more_people_than_slots_and_max_age_zero():
    k = people(7, 6, (0.1, 0.3, 0.5, 0.7, 0.9))
    counts = {}
    out, ids = tr.track(k, slots=3, counts=counts)
    assert np.array_equal(bits(out), bits(k[:, :3])) and (ids == np.arange(3)).all()     # the later detections are dropped, in every frame
    assert counts["overflow"] == 2 * 6 and counts["birth"] == 3 and counts["match"] == 3 * 5
    # max_age = 0: an unmatched track dies at once, its slot is empty for one frame
    k = people(8, 6, (0.2, 0.6))
    k[2, 0] = MARKER
    counts = {}
    out, ids = tr.track(k, max_age=0, counts=counts)
    assert ids[:, 0].tolist() == [0, 0, -1, 2, 2, 2] and (ids[:, 1] == 1).all() and counts["lost"] == 0 and counts["freed"] == 1
    k[3, 0] = MARKER
    assert tr.track(k, max_age=0)[1][:, 0].tolist() == [0, 0, -1, -1, 2, 2]
    assert tr.track(k, max_age=1)[1][:, 0].tolist() == [0, 0, -1, -1, 2, 2]
    assert tr.track(k, max_age=2)[1][:, 0].tolist() == [0, 0, -1, -1, 0, 0]


# ============================================================================================== ties and edges
def test_ties_resolve_by_slot_then_detection():
    one = people(9, 1, (0.5,))[0, 0]
    k = np.stack([np.stack([one, one])] * 3)                                             # two identical detections, three frames
    counts = {}
    out, ids = tr.track(k, counts=counts)
    assert (ids == [0, 1]).all() and np.array_equal(bits(out), bits(k)) and counts["match"] == 4
    # told apart by score alone (matching never reads a valid score): slot 0 keeps taking detection 0
    k[:, 0, :, 2], k[:, 1, :, 2] = 0.75, 0.5
    out, _ = tr.track(k)
    assert (out[:, 0, :, 2] == 0.75).all() and (out[:, 1, :, 2] == 0.5).all()
    k[1] = k[1, ::-1]                                                                    # swapped in frame 1: still by index, so the scores swap
    out, ids = tr.track(k)
    assert (out[1, 0, :, 2] == 0.5).all() and (out[1, 1, :, 2] == 0.75).all() and (ids == [0, 1]).all()
    # all eight rows the same person
    k = np.stack([np.stack([one] * 8)] * 2)
    k[..., 2] = np.linspace(0.5, 0.9, 8, dtype=F32)[None, :, None]
    out, ids = tr.track(k)
    assert (ids == np.arange(8)).all() and np.array_equal(bits(out), bits(k))


def edge_clip(threshold=F32(0.3)):
    """[6, 6, 134, 3] for 8 slots and what its rows are for; every row starts as a person at its own place"""
    k = people(11, 6, tuple(0.1 + 0.15 * q for q in range(6)))
    below = np.nextafter(threshold, F32(-1))
    k[:, 0, :BODY, 2] = below                                                            # row 0: four points AT the threshold, the rest one ulp below
    k[:, 0, :4, 2] = threshold
    k[2:, 0, 3, 2] = below                                                               # ... then three: no person any more
    k[:, 1, 4:BODY] = MARKER                                                             # row 1: four points, two of them at -0.0 (valid) ...
    k[:, 1, 0, 0], k[:, 1, 1, 1] = -0.0, -0.0
    k[3, 1, 2, 2] = -0.0                                                                 # ... and a score of -0.0 (low) in frame 3: three points, no person
    for c, bad in enumerate((np.nan, np.inf, -np.inf)):                                  # row 2: NaN and inf in each field of points 5..13 in frame 2
        for field in range(3):
            k[2, 2, 5 + 3 * c + field, field] = bad
    k[2, 3, :BODY, 0] = 3e38                                                             # row 3: huge in frame 2: acc overflows against the track
    k[:, 4, 0, 0], k[:, 4, 2, 1], k[:, 4, 5, :2] = 1e-42, 1e-45, (3e-39, 0)              # row 4: subnormal coordinates on a body of normal size
    k[:, 5, :BODY, :2] = k[0, 5, 1, :2]                                                  # row 5: all valid points coincide: s2 = 0, never matched
    return k


def test_edges():
    for threshold in (0.3, 0.5, 0.0):
        k = edge_clip(F32(threshold))
        counts = {}
        out, ids = tr.track(k, slots=8, score_threshold=threshold, counts=counts)
        want = scalar_track(k, 8, thr=threshold)
        assert np.array_equal(bits(out), bits(want[0])) and np.array_equal(ids, want[1])
        rows = [{int(i) for i in np.flatnonzero((bits(out[f]) == bits(k[f, d])).all((1, 2)))} for f in range(6) for d in range(6)]
        where = lambda f, d: rows[6 * f + d]                                             # noqa: E731  the slots that hold detection d of frame f
        assert where(0, 0) == where(1, 0) == {0} and not where(2, 0) and not where(5, 0)  # at the threshold: a person; one point fewer: none
        # -0.0 coordinates count; a score of -0.0 does too where the threshold is 0, and is low elsewhere
        assert where(2, 1) == {1} and where(3, 1) == ({1} if threshold == 0 else set()) and where(4, 1) == {1} and (ids[[0, 1, 2, 4, 5], 1] == 1).all()
        assert where(2, 2) == where(1, 2) == {2} and (ids[:, 2] == 2).all()              # nine bad points: the other nine still match
        # 3e38 overflows acc: inadmissible, never picked; it is a newcomer in the last free slot, and the old track waits for its person
        assert where(1, 3) == {3} and where(2, 3) == {7} and where(3, 3) == {3} and ids[:, 3].tolist() == [3, 3, -1, 3, 3, 3] and ids[2, 7] == 7
        assert all(where(f, 4) == {4} for f in range(6)) and (ids[:, 4] == 4).all()      # subnormals are kept and matched
        born = [int(ids[f, min(where(f, 5))]) for f in range(6) if where(f, 5)]          # s2 = 0: a new track whenever a slot is free
        assert len(born) >= 3 and len(set(born)) == len(born)
        assert counts["overflow"] > 0 and counts["freed"] > 0 and counts["lost"] > 0
    huge = people(12, 3, (0.5,))                                                         # a box of infinite extent: s2 = inf is not admissible
    huge[:, 0, 0, 0] = 3e38
    assert tr.track(huge, slots=2)[1].tolist() == [[0, -1], [-1, 1], [-1, -1]]           # both slots wait for a person they can never match


def test_fewer_common_points_than_min_common_do_not_match():
    k = people(13, 2, (0.5,))
    k[0, 0, 9:BODY], k[1, 0, :7] = MARKER, MARKER                                        # points 7 and 8 in common
    assert tr.track(k, slots=2)[1].tolist() == [[0, -1], [-1, 1]]
    assert tr.track(k, slots=2, min_common=2)[1].tolist() == [[0, -1], [0, -1]]
    assert tr.track(k, slots=2, min_common=2, min_points=12)[1].tolist() == [[-1, -1], [-1, -1]]


# ============================================================================================== invariants
@pytest.mark.parametrize("seed", range(6))
def test_invariants_over_random_clips(seed):
    count, slots, max_age = ((3, 3, 2), (5, 4, 1), (8, 8, 0), (2, 3, 3), (4, 8, 2), (8, 2, 1))[seed]
    k = crowd(40 + seed, 40, count, pixels=bool(seed % 2))
    out, ids = tr.track(k, slots=slots, max_age=max_age)
    last_seen, in_slot = {}, {}
    for f in range(len(k)):
        used = []
        for s in range(slots):
            if ids[f, s] < 0:
                assert (out[f, s] == MARKER).all()
                continue
            same = [d for d in range(count) if np.array_equal(bits(out[f, s]), bits(k[f, d]))]
            assert same, (f, s)                                                          # a bit copy of an input row of the same frame
            used.append(same)
            i = int(ids[f, s])
            assert i not in last_seen or (in_slot[i] == s and f - last_seen[i] - 1 <= max_age)      # an id keeps its slot and never returns after a longer gap
            last_seen[i], in_slot[i] = f, s
        assert len(used) <= len({d for same in used for d in same})                      # no input row appears twice
        assert sorted(i for i in ids[f] if i >= 0) == sorted(set(i for i in ids[f] if i >= 0))
    for s in range(slots):                                                               # between two ids in one slot: at least max_age + 1 empty frames
        held = [(f, int(ids[f, s])) for f in range(len(k)) if ids[f, s] >= 0]
        for (f0, a), (f1, b) in zip(held, held[1:]):
            assert a == b or f1 - f0 - 1 >= max_age + 1, (s, f0, f1)
    assert len(last_seen) > slots                                                        # tracks ended and began


def test_any_partition_gives_the_whole_clips_bits():
    k = crowd(21, 23, 4)
    for kw in (dict(), dict(slots=3, max_age=1, gate=0.3), dict(slots=6, max_age=0)):
        state = tr.fresh_state(kw.get("slots", 4))
        want, want_ids = tr.frames(k, state, tr.prepare(**kw))
        for parts in ([1] * 23, [5, 18], [22, 1], [7, 7, 9], [23]):
            stream = tr.Stream(**kw)
            assert stream.state is None and stream.ids is None
            got, got_ids, at = [], [], 0
            for m in parts:
                got.append(stream.push(k[at:at + m]))
                got_ids.append(stream.ids)
                at += m
                assert stream.frames_in == at and got[-1].shape == (m, kw.get("slots", 4), 134, 3) and stream.ids.shape == (m, kw.get("slots", 4))
            assert np.array_equal(bits(np.concatenate(got)), bits(want)) and np.array_equal(np.concatenate(got_ids), want_ids), parts
            assert np.array_equal(stream.state, state), parts
            assert stream.close() is None
            with pytest.raises(ValueError, match="closed"):
                stream.push(k[:1])
    stream = tr.Stream()
    stream.push(k[:2])
    with pytest.raises(ValueError, match="holds 4 people, the piece 3"):
        stream.push(k[2:3, :3])
    one = tr.Stream()
    assert one.push(k[:3, 0]).shape == (3, 1, 134, 3) and one.state.shape == (2, 40)     # [F, 134, 3] is one person


def test_the_id_counter_wraps_into_31_bits():
    k = people(14, 2, (0.3, 0.7))
    state = tr.fresh_state(2)
    state[2, 0] = np.uint32(0x7FFFFFFF).view(np.int32)
    _, ids = tr.frames(k, state, tr.prepare())
    assert ids.tolist() == [[0x7FFFFFFF, 0], [0x7FFFFFFF, 0]] and state[2, 0] == np.uint32(0x80000001).view(np.int32)
    state = tr.fresh_state(2)
    state[2, 0] = -1
    assert tr.frames(k, state, tr.prepare())[1][0].tolist() == [0x7FFFFFFF, 0] and state[2, 0] == 1


# ============================================================================================== prepare
def test_prepare_rejects_each_bad_parameter_by_name():
    for bad in (0, 9, -1, 1.0, "2", True):
        with pytest.raises(ValueError, match="slots"):
            tr.prepare(bad)
        with pytest.raises(ValueError, match="slots"):
            tr.fresh_state(bad)
    for bad in (0, -0.5, np.nan, np.inf, "1", None, True, 1e-30, 1e20):                  # 1e-30 squared is 0 as a float32, 1e20 squared inf
        with pytest.raises(ValueError, match="gate"):
            tr.prepare(gate=bad)
        with pytest.raises(ValueError, match="gate"):
            tr.Stream(gate=bad)
    for name, lo, hi in (("max_age", 0, 65535), ("min_points", 1, 18), ("min_common", 1, 18)):
        for bad in (lo - 1, hi + 1, 1.0, "2", None, True, np.nan):
            with pytest.raises(ValueError, match=name):
                tr.prepare(**{name: bad})
        assert getattr(tr.prepare(**{name: lo}), name) == lo and getattr(tr.prepare(**{name: hi}), name) == hi
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="score_threshold"):
            tr.prepare(score_threshold=bad)
    assert tr.prepare(8, 1e-20).gate2 > 0 and tr.prepare(np.int64(3)).slots == 3
    for bad in (np.zeros((134, 3)), np.zeros((2, 9, 134, 3)), np.zeros((0, 1, 134, 3)), np.zeros((2, 1, 133, 3))):
        with pytest.raises(ValueError, match="keypoints must be"):
            tr.track(bad)
    with pytest.raises(ValueError, match="the state holds 3 slots, the parameters say 2"):
        tr.frames(np.zeros((1, 2, 134, 3), F32), tr.fresh_state(3), tr.prepare(2))
    with pytest.raises(ValueError, match="state must be"):
        tr.frames(np.zeros((1, 2, 134, 3), F32), np.zeros((3, 40), np.int64), tr.prepare())
    assert tr.RULES == ("match", "birth", "lost", "freed", "overflow", "gated")


# ============================================================================================== the C entry points
def test_state_bytes():
    lib = sfa._lib.lib()
    assert lib.sf_abi_version() == 11 == sfa._lib.ABI_VERSION
    for slots in range(1, 9):
        assert lib.sf_pose_track_state_bytes(slots) == (slots + 1) * 160 == tr.state_bytes(slots) == tr.fresh_state(slots).nbytes
        assert sfa.ops.pose_track_state_bytes(slots) == (slots + 1) * 160
    for slots in (0, 9, -1, 1 << 20):
        assert lib.sf_pose_track_state_bytes(slots) == 0 == tr.state_bytes(slots)


def test_c_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    lib, L = sfa._lib.lib(), sfa._lib
    A = L.PoseTrackArgs
    assert C.sizeof(A) == 5 * 8 + 6 * 4 + 2 * 4 == 72 and A.n.offset == 40 and A.max_age.offset == 60 and A.gate2.offset == 64
    assert L.POSE_TRACK_MAX_AGE == tr.MAX_AGE == 65535 and L.POSE_TRACK_STATE_WORDS == tr.STATE_WORDS == 40
    n, people, slots = 10, 2, 3
    ok = dict(src=1 << 20, out=2 << 20, ids=3 << 20, state=4 << 20, assign=5 << 20, n=n, people=people, slots=slots, min_points=4, min_common=3,
              max_age=2, gate2=0.25, score_threshold=0.3)
    size = dict(src=n * people * 134 * 12, out=n * slots * 134 * 12, ids=n * slots * 4, state=(slots + 1) * 160, assign=n * slots * 4)

    def call(**kw):
        return lib.sf_pose_track_frames(C.byref(A(**{**ok, **kw})), None)
    err = lib.sf_last_error
    assert lib.sf_pose_track_frames(None, None) != 0 and b"null args" in err()
    for name in size:
        assert call(**{name: None}) != 0 and b"null buffer" in err(), name
    for name in ("src", "out"):
        assert call(**{name: ok[name] + 2}) != 0 and b"src and out must be 4-byte aligned" in err(), name
    for name in ("ids", "assign"):
        assert call(**{name: ok[name] + 2}) != 0 and b"ids and assign must be 4-byte aligned" in err(), name
    for off in (4, 8, 12):
        assert call(state=ok["state"] + off) != 0 and b"state must be 16-byte aligned" in err()
    for name in ("people", "slots"):
        for bad in (0, 9, -1):
            assert call(**{name: bad}) != 0 and b"%s=%d (1..8)" % (name.encode(), bad) in err()
    for bad in (0, -1, (1 << 20) + 1):
        assert call(n=bad) != 0 and b"n=%d (1..1048576)" % bad in err()
    for name in ("min_points", "min_common"):
        for bad in (0, 19, -1):
            assert call(**{name: bad}) != 0 and b"%s=%d (1..18)" % (name.encode(), bad) in err()
    for bad in (-1, 65536):
        assert call(max_age=bad) != 0 and b"max_age=%d (0..65535)" % bad in err()
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        assert call(gate2=bad) != 0 and b"gate2 must be finite and > 0" in err(), bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(score_threshold=bad) != 0 and b"score_threshold must be finite" in err()
    # every pair of the five ranges: the second placed over the first's last bytes, and the first's start inside the second
    names = list(size)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for at in (ok[a] + (size[a] - 1) // 16 * 16, ok[a] - size[b] // 16 * 16 + 16, ok[a]):     # 16-byte aligned, as state must be
                assert call(**{b: at}) != 0 and b"%s and %s overlap" % (a.encode(), b.encode()) in err(), (a, b, at)


# ============================================================================================== the Python surface
def test_operator_schema_and_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "pose_track_frames" in sfa.torch_ops.OPS
    schema = str(torch.ops.sf_hip.pose_track_frames.default._schema)
    assert "Tensor(a1!) state" in schema and schema.count("!") == 1 and schema.endswith("-> (Tensor, Tensor)")
    with FakeTensorMode():
        k, s = torch.empty(5, 2, 134, 3, device="cuda"), torch.empty(4, 40, dtype=torch.int32, device="cuda")
        o, i = torch.ops.sf_hip.pose_track_frames(k, s, 3, 0.25)
        assert tuple(o.shape) == (5, 3, 134, 3) and o.dtype == torch.float32 and tuple(i.shape) == (5, 3) and i.dtype == torch.int32
        with pytest.raises(Exception, match="state must be"):
            torch.ops.sf_hip.pose_track_frames(k, s, 2, 0.25)
        with pytest.raises(Exception, match="state must be"):
            torch.ops.sf_hip.pose_track_frames(k, s.float(), 3, 0.25)
        with pytest.raises(Exception, match="src must be"):
            torch.ops.sf_hip.pose_track_frames(k[0], s, 3, 0.25)
        with pytest.raises(Exception, match="slots must be"):
            torch.ops.sf_hip.pose_track_frames(k, s, 9, 0.25)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sfa.ops.pose_track_frames(torch.zeros(2, 1, 134, 3), torch.zeros(2, 40, dtype=torch.int32), 1, 0.25)


def test_pose_tracker_checks_that_need_no_device():
    assert sfa.PoseTracker is sfa.pose_track.PoseTracker and sfa.PoseTrackStream is sfa.pose_track.PoseTrackStream
    assert {"PoseTracker", "PoseTrackStream", "pose_track", "pose_track_reference"} <= set(sfa.__all__)
    t = sfa.PoseTracker()
    k = np.zeros((3, 2, 134, 3), F32)
    for kw, match in ((dict(slots=0), "slots"), (dict(slots=9), "slots"), (dict(gate=0), "gate"), (dict(gate=float("nan")), "gate"),
                      (dict(max_age=-1), "max_age"), (dict(max_age=1.5), "max_age"), (dict(min_points=0), "min_points"),
                      (dict(min_common=19), "min_common"), (dict(score_threshold=float("nan")), "score_threshold")):
        with pytest.raises(ValueError, match=match):
            t.track(k, **kw)
        with pytest.raises(ValueError, match=match):
            t.open_stream(**kw)
    for bad in (k[0, 0], np.zeros((2, 9, 134, 3), F32), np.zeros((0, 1, 134, 3), F32), torch.zeros(2, 134, 2)):
        with pytest.raises(ValueError, match="keypoints must be"):
            t.track(bad)
    with pytest.raises(ValueError, match="numbers"):
        t.track(np.zeros((2, 134, 3), object))
    cpu = sfa.PoseTracker(device="cpu")
    for kk in (k, torch.from_numpy(k), k[:, 0].tolist()):
        with pytest.raises(ValueError, match="no CPU fallback"):
            cpu.track(kk)
    s = cpu.open_stream(3, gate=0.4, max_age=5)
    assert isinstance(s, sfa.PoseTrackStream)
    assert (s.params.slots, s.params.gate2, s.params.max_age, s.frames_in, s.state, s.ids) == (3, F32(0.4 * 0.4), 5, 0, None, None)
    with pytest.raises(ValueError, match="no CPU fallback"):
        s.push(k)
    assert s.state is None and s.frames_in == 0 and s.people is None
    s.people = 2                                                                         # a stream that has seen two people
    with pytest.raises(ValueError, match="holds 2 people, the piece 1"):
        s.push(k[:, :1])
    with pytest.raises(ValueError, match="keypoints must be"):
        s.push(k[0, 0])
    assert s.close() is None
    with pytest.raises(ValueError, match="closed"):
        s.push(k)


def test_pose_feed_puts_the_tracker_first_and_refuses_a_smoother_that_bridges_more_than_the_tracker_waits():
    r = sfa.PoseRenderer(device="cpu")
    k = np.zeros((5, 1, 134, 3), F32)
    pulled = []

    def source():
        for i in range(5):
            pulled.append(i)
            yield k[i]
    tracker, smoother = sfa.PoseTracker(device="cpu"), sfa.PoseSmoother(device="cpu")
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, tracker=tracker.open_stream(), smoother=smoother.open_stream(30, max_gap=2))
    assert pulled == []
    with pytest.raises(ValueError, match="PoseTracker: expected a CUDA/ROCm device"):    # the tracker comes first
        next(feed)
    assert pulled == [0, 1]
    pulled.clear()
    live = sfa.PoseRetargeter(device="cpu").open_stream(k[0], (24, 40), source_fps=30)
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, retargeter=live, smoother=smoother.open_stream(30), tracker=tracker.open_stream())
    with pytest.raises(ValueError, match="PoseTracker: expected a CUDA/ROCm device"):
        next(feed)
    assert pulled == [0, 1, 2]
    pulled.clear()
    for max_gap, max_age in ((3, 2), (1, 0), (65535, 65534)):
        feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, tracker=tracker.open_stream(max_age=max_age),
                                         smoother=smoother.open_stream(30, max_gap=max_gap))
        with pytest.raises(ValueError, match="one person towards another") as e:
            next(feed)
        assert f"max_gap = {max_gap}" in str(e.value) and f"max_age + 1 = {max_age + 1}" in str(e.value) and pulled == []
    feed = sfa.pose_render.pose_feed(source(), r, (24, 40), 2, tracker=tracker.open_stream(max_age=3), smoother=smoother.open_stream(30, max_gap=3))
    with pytest.raises(ValueError, match="PoseTracker: expected a CUDA/ROCm device"):    # max_gap == max_age is within the guarantee
        next(feed)


def test_generate_flags(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import generate
    k = np.random.default_rng(0).random((5, 2, 134, 3)).astype(F32)
    np.savez(tmp_path / "clip.npz", keypoints=k)
    np.savez(tmp_path / "ref.npz", keypoints=k[0])
    np.save(tmp_path / "dict.npy", {"dwpose_data": np.zeros((3, 1, 8, 8), np.uint8), "random_ref_dwpose": np.zeros((8, 8, 3), np.uint8)}, allow_pickle=True)
    base = ["generate.py", "--config_path", "c", "--data_path", "d", "--output_folder", "o"]

    def run(*more):
        """the parser's error text: every one of these ends in ap.error, before any file of the config is opened"""
        monkeypatch.setattr(sys, "argv", base + list(more))
        with pytest.raises(SystemExit) as e:
            generate.main()
        assert e.value.code == 2
        return capsys.readouterr().err
    seeded = ("--pose_random_init_seed", "0")
    for flag in (("--pose_track",), ("--pose_track", "3"), ("--pose_track_gate", "0.5"), ("--pose_track_age", "2")):
        assert f"{flag[0]} needs a keypoint --pose_path" in run(*flag), flag
        assert f"{flag[0]} goes with a keypoint --pose_path" in run(*seeded, "--pose_path", str(tmp_path / "dict.npy"), *flag), flag
    keypoints = (*seeded, "--pose_path", str(tmp_path / "clip.npz"), "--ref_pose_path", str(tmp_path / "ref.npz"))
    for flag in (("--pose_track_gate", "0.5"), ("--pose_track_age", "2")):
        assert "go with --pose_track" in run(*keypoints, *flag)
    for bad in ("0", "9", "-1"):
        err = run(*keypoints, f"--pose_track={bad}")
        assert f"--pose_track {bad}" in err and "slots" in err, bad
    assert "SLOTS expected" in run(*keypoints, "--pose_track", "two")
    for bad in ("0", "-1", "nan", "inf"):
        err = run(*keypoints, "--pose_track", f"--pose_track_gate={bad}")
        assert f"--pose_track_gate {float(bad)}" in err and "gate must be" in err, bad
    for bad in ("-1", "65536"):
        err = run(*keypoints, "--pose_track", "2", f"--pose_track_age={bad}")
        assert f"--pose_track_age {bad}" in err and "max_age" in err, bad
    assert "--pose_hold 3 exceeds --pose_track_age 2" in run(*keypoints, "--pose_track", "--pose_hold", "3")
    assert "--pose_hold 2 exceeds --pose_track_age 1" in run(*keypoints, "--pose_track", "--pose_track_age", "1", "--pose_hold", "2")
    # the track flags are no retarget flags: alone they ask for no --pose_fps, and a good set gets past the parser's pose checks
    err = run(*keypoints, "--pose_track", "2", "--pose_track_gate", "0.4", "--pose_track_age", "3", "--pose_hold", "3", "--pose_resize", "stretch")
    assert err.splitlines()[-1].startswith("generate.py: error: --pose_resize")          # the next check behind the pose flags
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--pose_track [SLOTS]", "--pose_track_gate G", "--pose_track_age N"))
