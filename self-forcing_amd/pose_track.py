"""Pose tracker on the GPU path: a detector lists the people of a frame in detection order, which changes whenever two scores
cross, a person leaves or a person enters, while the smoother and the retargeter assume that person q of one frame is
person q of the next.  The tracker puts each detected person into a stable slot on the device (csrc/pose_track.hip behind
sf_pose_track_frames), between the upload and `PoseSmoother`.  The definition of every number is `pose_track_reference.py`
(float32, every operation rounded on its own), which the kernels equal bit for bit.  A slot's row is the matched
detection's floats, copied bit for bit; a slot with no detection comes out as (-1, -1, 0) with id -1."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops
from . import pose_track_reference as tr
from .pose_keypoints import KeypointStage, KeypointStream

Tensor = torch.Tensor


class Tracked(NamedTuple):
    keypoints: Tensor          # float32 [F, S, 134, 3]
    ids: Tensor                # int32 [F, S]


class PoseTrackStream(KeypointStream):
    """`PoseTracker.track` piece by piece, for a live source.  `push(piece)` takes detections [n, P, 134, 3] or [n, 134, 3]
    (numpy, host tensor or device tensor; a device tensor causes no host copy and no synchronisation) and returns them in
    slots, float32 [n, S, 134, 3] on the device; `ids`, int32 [n, S], are the track ids of the last push.  Every push
    returns as many frames as it took, and any partition of a clip gives the bits of `track` on the whole clip.  `state`
    is the packed tracker state, int32 [S + 1, 40] on the device (`pose_track_reference`), allocated zeroed at the first
    push, when S defaults to that piece's P; later pieces must have the same P.  The stream keeps nothing else of the
    caller's."""

    who = "PoseTracker"
    state: Optional[Tensor] = None
    ids: Optional[Tensor] = None

    def _open(self, people: int, k: Tensor) -> None:
        slots = people if self.params.slots is None else self.params.slots
        self.state = torch.zeros((slots + 1, tr.STATE_WORDS), dtype=torch.int32, device=k.device)
        self.people = people

    def _launch(self, k: Tensor) -> Tensor:
        p = self.params
        with torch.cuda.device(k.device):
            out, self.ids = ops.pose_track_frames(k, self.state, self.state.shape[0] - 1, float(p.gate2), float(p.threshold), p.min_points,
                                                  p.min_common, p.max_age)
        return out


class PoseTracker(KeypointStage):
    """`track(keypoints)` -> the named pair (keypoints float32 [F, S, 134, 3], ids int32 [F, S]) on the device, every number
    as `pose_track_reference.track` defines it.

    keypoints: float [F, P, 134, 3] or [F, 134, 3], P <= 8, the detections of each frame in any order: a numpy array, a
    host tensor (uploaded once to the tracker's device) or a device tensor (used where it is).  slots (1..8, default P) is
    the number of people kept at once.  A detection is a person when at least min_points of its 18 body points are valid;
    it continues a track when they share at least min_common valid points whose mean squared distance is at most
    gate^2 of the squared diagonal of the track's body box (gate = 0.5: half a body diagonal between matches); the best
    pairs are taken first.  A track that goes unmatched for more than max_age frames frees its slot, and the slot is not
    given to a newcomer in the frame that frees it, so it is empty for at least max_age + 1 frames between two people.
    Two launches on the current stream, with no synchronisation."""

    def track(self, keypoints, slots: Optional[int] = None, gate: float = 0.5, max_age: int = 2, min_points: int = 4, min_common: int = 3,
              score_threshold: float = 0.3) -> Tracked:
        stream = self.open_stream(slots, gate, max_age, min_points, min_common, score_threshold)
        return Tracked(stream.push(keypoints), stream.ids)

    def open_stream(self, slots: Optional[int] = None, gate: float = 0.5, max_age: int = 2, min_points: int = 4, min_common: int = 3,
                    score_threshold: float = 0.3) -> PoseTrackStream:
        return PoseTrackStream(self.device, tr.prepare(slots, gate, max_age, min_points, min_common, score_threshold))
