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
from . import pose_render_reference as pr
from . import pose_track_reference as tr
from .pose_render import as_tensor

Tensor = torch.Tensor


class Tracked(NamedTuple):
    keypoints: Tensor          # float32 [F, S, 134, 3]
    ids: Tensor                # int32 [F, S]


def _place(keypoints: Tensor, device: torch.device, shape) -> Tensor:
    """float32 [shape] on `device`: a host tensor is uploaded (the only host-to-device copy), a device tensor stays."""
    if device.type != "cuda":
        raise ValueError("PoseTracker: expected a CUDA/ROCm device (the HIP path has no CPU fallback)")
    return keypoints.to(device=device, dtype=torch.float32).reshape(shape).contiguous()


def _launch(p: tr.Params, src: Tensor, state: Tensor) -> Tracked:
    with torch.cuda.device(src.device):
        return Tracked(*ops.pose_track_frames(src, state, state.shape[0] - 1, float(p.gate2), float(p.threshold), p.min_points, p.min_common, p.max_age))


def _fresh_state(slots: int, device: torch.device) -> Tensor:
    return torch.zeros((slots + 1, tr.STATE_WORDS), dtype=torch.int32, device=device)


class PoseTrackStream:
    """`PoseTracker.track` piece by piece, for a live source.  `push(piece)` takes detections [n, P, 134, 3] or [n, 134, 3]
    (numpy, host tensor or device tensor; a device tensor causes no host copy and no synchronisation) and returns them in
    slots, float32 [n, S, 134, 3] on the device; `ids`, int32 [n, S], are the track ids of the last push.  Every push
    returns as many frames as it took, and any partition of a clip gives the bits of `track` on the whole clip.  `state`
    is the packed tracker state, int32 [S + 1, 40] on the device (`pose_track_reference`), allocated zeroed at the first
    push, when S defaults to that piece's P; later pieces must have the same P.  The stream keeps nothing else of the
    caller's."""

    def __init__(self, device: torch.device, params: tr.Params):
        self.params = params
        self.device = device
        self.frames_in = 0
        self.closed = False
        self.people: Optional[int] = None
        self.state: Optional[Tensor] = None
        self.ids: Optional[Tensor] = None

    def push(self, piece) -> Tensor:
        if self.closed:
            raise ValueError("PoseTrackStream: the stream is closed")
        piece = as_tensor(piece, "PoseTracker: keypoints")
        n, people = pr.check_keypoints_shape(piece.shape)
        if self.people is not None and people != self.people:
            raise ValueError(f"PoseTrackStream: the stream holds {self.people} people, the piece {people}")
        if self.state is None and piece.is_cuda:
            self.device = piece.device
        k = _place(piece, self.device, (n, people, pr.KEYPOINTS, 3))
        if self.state is None:
            self.state = _fresh_state(people if self.params.slots is None else self.params.slots, self.device)
        self.people = people
        out, self.ids = _launch(self.params, k, self.state)
        self.frames_in += n
        return out

    def close(self) -> None:
        """Ends the stream.  Nothing further comes out: every frame has been returned by its push."""
        self.closed = True


class PoseTracker:
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

    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def track(self, keypoints, slots: Optional[int] = None, gate: float = 0.5, max_age: int = 2, min_points: int = 4, min_common: int = 3,
              score_threshold: float = 0.3) -> Tracked:
        p = tr.prepare(slots, gate, max_age, min_points, min_common, score_threshold)
        keypoints = as_tensor(keypoints, "PoseTracker: keypoints")
        f, people = pr.check_keypoints_shape(keypoints.shape)
        device = keypoints.device if keypoints.is_cuda else self.device
        k = _place(keypoints, device, (f, people, pr.KEYPOINTS, 3))
        return _launch(p, k, _fresh_state(people if p.slots is None else p.slots, device))

    def open_stream(self, slots: Optional[int] = None, gate: float = 0.5, max_age: int = 2, min_points: int = 4, min_common: int = 3,
                    score_threshold: float = 0.3) -> PoseTrackStream:
        return PoseTrackStream(self.device, tr.prepare(slots, gate, max_age, min_points, min_common, score_threshold))
