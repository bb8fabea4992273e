"""What the keypoint stages on the GPU path share (`PoseTracker`, `PoseSmoother`, `PoseRetargeter`, in front of
`PoseRenderer`): how keypoints become a tensor and reach the device, the scaffold of a stage's stream, and
`KeypointChain`, the one place that knows the order of the stages and the rule between them."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import pose_render_reference as pr
from . import pose_retarget_reference as rr

Tensor = torch.Tensor


def as_tensor(keypoints, who: str, what: str = "keypoints") -> Tensor:
    """A numpy array (or what `np.asarray` takes), a host tensor or a device tensor of numbers -> a tensor, where it is."""
    if not isinstance(keypoints, Tensor):
        keypoints = np.asarray(keypoints)
        if keypoints.dtype.kind not in "fiu":
            raise ValueError(f"{who}: {what} must be numbers, got an array of {keypoints.dtype}")
        return torch.from_numpy(np.ascontiguousarray(keypoints, dtype=np.float32))
    if keypoints.is_complex() or keypoints.dtype == torch.bool:
        raise ValueError(f"{who}: {what} must be numbers, got {keypoints.dtype}")
    return keypoints


def place(keypoints: Tensor, device: torch.device, shape, who: str) -> Tensor:
    """float32 [shape] on `device`: a host tensor is uploaded (the only host-to-device copy), a device tensor stays."""
    if device.type != "cuda":
        raise ValueError(f"{who}: expected a CUDA/ROCm device (the HIP path has no CPU fallback)")
    return keypoints.to(device=device, dtype=torch.float32).reshape(shape).contiguous()


class KeypointStage:
    """A stage of the keypoint path and the device its host input goes to; a device tensor is used where it is."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)


class KeypointStream:
    """The scaffold of a stage's stream: `push(piece)` takes frames [n, P, 134, 3] or [n, 134, 3] (numpy, host tensor or
    device tensor), checks them, puts them on the device and hands them to the stage.  The first piece decides P and, when
    it is a device tensor, the device; a push that fails leaves the stream as it was.  A stage says who it is (`who`, the
    name its errors carry) and how many `people` it holds (None before the first piece), and supplies `_open(people, k)`,
    which allocates what it keeps for them at the first piece, once that is on the device, and `_launch(k)`, which returns
    the output of a placed piece float32 [n, P, 134, 3]."""

    who = ""
    people: Optional[int] = None

    def __init__(self, device: torch.device, params):
        self.params = params
        self.device = device
        self.frames_in = 0
        self.closed = False

    def _admit(self, people: int) -> None:
        """A stage's own check of the first piece's people, before anything reaches the device."""

    def push(self, piece) -> Tensor:
        if self.closed:
            raise ValueError(f"{type(self).__name__}: the stream is closed")
        piece = as_tensor(piece, self.who)
        n, people = pr.check_keypoints_shape(piece.shape)
        held = self.people
        if held is None:
            self._admit(people)
            if piece.is_cuda:
                self.device = piece.device
        elif people != held:
            raise ValueError(f"{type(self).__name__}: the stream holds {held} people, the piece {people}")
        k = place(piece, self.device, (n, people, pr.KEYPOINTS, 3), self.who)
        if held is None:
            self._open(people, k)
        out = self._launch(k)
        self.frames_in += n
        return out

    def close(self) -> None:
        """Ends the stream.  Nothing further comes out: every frame that can be computed has been returned by its push."""
        self.closed = True


class KeypointChain:
    """The stages between a keypoint source and the renderer, each optional, in the one order they run in: a
    `PoseTrackStream`, then a `PoseSmoothStream`, then a `PoseRetargetStream`.  A tracker keeps a slot empty for at least
    max_age + 1 frames between two different people, so a smoother that bridges at most max_age frames never filters one
    person towards another; a smoother whose max_gap exceeds the tracker's max_age is refused."""

    def __init__(self, tracker=None, smoother=None, retargeter=None):
        if tracker is not None and smoother is not None and self.bridges_two_people(smoother.params.max_gap, tracker.params.max_age):
            raise ValueError(f"pose_feed: the smoother bridges gaps of up to max_gap = {smoother.params.max_gap} frames, the tracker keeps a slot empty "
                             f"for only max_age + 1 = {tracker.params.max_age + 1} frames between two different people: with max_gap > max_age the "
                             f"smoother could filter one person towards another")
        self.retargeter = retargeter
        self.stages = [s for s in (tracker, smoother, retargeter) if s is not None]
        self.in_pixels = retargeter is not None        # a retargeter's output is in pixels of the output frames, else in the source's own units

    @staticmethod
    def bridges_two_people(max_gap: int, max_age: int) -> bool:
        """The rule between the stages: could a smoother with `max_gap` reach across the empty frames of a tracker's slot?"""
        return max_gap > max_age

    def planned(self, n: int) -> int:
        """How many output frames `n` more source frames would make final."""
        r = self.retargeter
        return n if r is None else rr.plan(r.frames_in, n, r.params.num, r.params.den)[1]

    def push(self, batch):
        """A batch of source frames through the stages that are present -> the output frames that became final."""
        for stage in self.stages:
            batch = stage.push(batch)
        return batch
