"""Pose smoother on the GPU path: keypoints of a live detector jitter by a pixel or two and lose points for a frame or two;
a One-Euro filter per point and a bounded hold across the gaps steady them on the device (csrc/pose_smooth.hip behind
sf_pose_smooth_frames), between the upload of about 1.6 KB per frame and person and `PoseRetargeter` / `PoseRenderer`.
The definition of every number is `pose_smooth_reference.py` (float32, every operation rounded on its own), which the
kernel equals bit for bit.  The values stay in the caller's units; a missing point comes out as (-1, -1, 0)."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from . import pose_render_reference as pr
from . import pose_smooth_reference as sr
from .pose_keypoints import KeypointStage, KeypointStream

Tensor = torch.Tensor


class PoseSmoothStream(KeypointStream):
    """`PoseSmoother.smooth` piece by piece, for a live source.  `push(piece)` takes frames [n, P, 134, 3] or [n, 134, 3]
    (numpy, host tensor or device tensor; a device tensor causes no host copy and no synchronisation) and returns them
    smoothed, float32 [n, P, 134, 3] on the device: the filter is causal, so every push returns as many frames as it
    took.  Any partition of a clip gives the bits of `smooth` on the whole clip.  `state` is the packed filter state,
    int32 [P, 134, 8] on the device (`pose_smooth_reference`), allocated zeroed at the first push, once P is known; the
    stream keeps nothing else of the caller's."""

    who = "PoseSmoother"
    state: Optional[Tensor] = None

    @property
    def people(self) -> Optional[int]:
        """The state says how many people the stream holds: a caller may hand a stream the state of another."""
        return None if self.state is None else self.state.shape[0]

    def _open(self, people: int, k: Tensor) -> None:
        self.state = torch.zeros((people, pr.KEYPOINTS, sr.STATE_WORDS), dtype=torch.int32, device=k.device)

    def _launch(self, k: Tensor) -> Tensor:
        p = self.params
        with torch.cuda.device(k.device):
            return ops.pose_smooth_frames(k, self.state, float(p.period), float(p.min_cutoff), float(p.beta), float(p.kd), float(p.threshold), p.max_gap)


class PoseSmoother(KeypointStage):
    """`smooth(keypoints, fps)` -> float32 [F, P, 134, 3] on the device, in the keypoints' own units, every number as
    `pose_smooth_reference.smooth` defines it.

    keypoints: float [F, P, 134, 3] or [F, 134, 3], P <= 8: a numpy array, a host tensor (uploaded once to the smoother's
    device) or a device tensor (used where it is).  fps is the rate they were recorded at: int, fractions.Fraction or
    "30000/1001".  min_cutoff (Hz) is the cutoff of a point at rest: lower is steadier and lags more; beta (1 / unit of
    the coordinates) raises the cutoff with the point's speed so that fast motion is followed; d_cutoff (Hz) is the cutoff
    of the speed estimate.  max_gap is the longest run of missing samples that is bridged with the last filtered position
    and the last valid score; 0 bridges none.  One launch on the current stream, with no synchronisation."""

    def smooth(self, keypoints, fps, min_cutoff: float = 1.0, beta: float = 0.0, d_cutoff: float = 1.0, max_gap: int = 0,
               score_threshold: float = 0.3) -> Tensor:
        return self.open_stream(fps, min_cutoff, beta, d_cutoff, max_gap, score_threshold).push(keypoints)

    def open_stream(self, fps, min_cutoff: float = 1.0, beta: float = 0.0, d_cutoff: float = 1.0, max_gap: int = 0,
                    score_threshold: float = 0.3) -> PoseSmoothStream:
        return PoseSmoothStream(self.device, sr.prepare(fps, min_cutoff, beta, d_cutoff, max_gap, score_threshold))
