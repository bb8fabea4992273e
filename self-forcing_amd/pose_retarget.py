"""Pose retargeter on the GPU path: driving keypoints (another person, another video, another frame rate) become keypoints
of the reference person's proportions and position on the generator's 16 frames/s timeline, on the device
(csrc/pose_retarget.hip behind sf_pose_retarget_frames), between the upload of about 1.6 KB per frame and person and
`PoseRenderer`.  The definition of every number is `pose_retarget_reference.py` (float32, every operation rounded on its
own), which the kernel equals bit for bit.  The result is in pixels of the output: draw it with `normalized=False`; a
retargeted point that lands at a negative coordinate is what the renderer already calls missing."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from . import pose_render_reference as pr
from . import pose_retarget_reference as rr
from .pose_keypoints import KeypointStage, KeypointStream, as_tensor, place

Tensor = torch.Tensor


def _launch(p: rr.Params, src: Tensor, src0: int, first: Tensor, ref: Tensor, out0: int, n_out: int) -> Tensor:
    if n_out == 0:
        return torch.empty((0, src.shape[1], pr.KEYPOINTS, 3), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        return ops.pose_retarget_frames(src, first, ref, src0, out0, n_out, p.num, p.den, float(p.src_sx), float(p.src_sy), float(p.ref_sx),
                                        float(p.ref_sy), float(p.threshold), p.align)


class PoseRetargetStream(KeypointStream):
    """`PoseRetargeter.retarget` piece by piece, for a live source.  `push(piece)` takes source frames [n, P, 134, 3] or
    [n, 134, 3] (numpy, host tensor or device tensor; a device tensor causes no host copy and no synchronisation) and
    returns the output frames that became final, float32 [m, P, 134, 3] on the device; m may be 0.  Output frame j is final
    once source frame i1(j) is in, so nothing is held back for `close()`.  Any partition of a clip gives the bits of
    `retarget` on the whole clip.  The stream keeps the clip's frame 0 and the last source frame on the device; its two
    counters are plain integers (a piece's length is known to the host)."""

    who = "PoseRetargeter"

    def __init__(self, device: torch.device, ref_keypoints, params: rr.Params):
        super().__init__(device, params)
        self._ref_in = as_tensor(ref_keypoints, self.who, "ref_keypoints")
        rr.check_reference_shape(self._ref_in.shape)
        self.frames_out = 0
        self._first = self._last = self._ref = None

    def _admit(self, people: int) -> None:
        rr.check_reference_shape(self._ref_in.shape, people)

    def _open(self, people: int, k: Tensor) -> None:
        self._ref = place(self._ref_in, k.device, (-1, pr.KEYPOINTS, 3), self.who)     # [Pr, 134, 3], Pr = P or 1: `_admit` has checked it
        self._first = k[0].clone()
        self.people = people

    def _launch(self, k: Tensor) -> Tensor:
        window, src0 = (k, 0) if self._last is None else (torch.cat([self._last, k]), self.frames_in - 1)
        out0, n_out = rr.plan(self.frames_in, k.shape[0], self.params.num, self.params.den)
        out = _launch(self.params, window, src0, self._first, self._ref, out0, n_out)
        self._last = k[-1:].clone()
        self.frames_out += n_out
        return out


class PoseRetargeter(KeypointStage):
    """`retarget(keypoints, ref_keypoints, size)` -> float32 [F_out, P, 134, 3] on the device, in pixels of the (H, W) output,
    every number as `pose_retarget_reference.retarget` defines it.

    keypoints: float [F, P, 134, 3] or [F, 134, 3], P <= 8; ref_keypoints: [Pr, 134, 3] or [134, 3], Pr = P or 1.  Each a
    numpy array, a host tensor (uploaded once to the retargeter's device) or a device tensor (used where it is).
    normalized applies to both: x, y in [0, 1], else in pixels.  source_size = (hs, ws) is the source video's size where
    it differs from the output's: the source is scaled by the heights, so another aspect is not stretched.  source_fps /
    target_fps: int, fractions.Fraction or "30000/1001"; output frame j sits at source position j * source_fps / target_fps
    and F_out = (F - 1) * den // num + 1.  align=False lifts and resamples only.  Work runs on the current stream, with no
    synchronisation."""

    def retarget(self, keypoints, ref_keypoints, size: Sequence[int], source_fps=16, target_fps=16, align: bool = True, normalized: bool = True,
                 score_threshold: float = 0.3, source_size: Optional[Sequence[float]] = None) -> Tensor:
        p = rr.prepare(size, source_fps, target_fps, align, normalized, score_threshold, source_size)
        keypoints, ref = as_tensor(keypoints, "PoseRetargeter"), as_tensor(ref_keypoints, "PoseRetargeter", "ref_keypoints")
        f, people = pr.check_keypoints_shape(keypoints.shape)
        ref_people = rr.check_reference_shape(ref.shape, people)
        device = keypoints.device if keypoints.is_cuda else (ref.device if ref.is_cuda else self.device)
        k = place(keypoints, device, (f, people, pr.KEYPOINTS, 3), "PoseRetargeter")
        r = place(ref, device, (ref_people, pr.KEYPOINTS, 3), "PoseRetargeter")
        return _launch(p, k, 0, k[0], r, 0, rr.frames_out(f, p.num, p.den))

    def open_stream(self, ref_keypoints, size: Sequence[int], source_fps=16, target_fps=16, align: bool = True, normalized: bool = True,
                    score_threshold: float = 0.3, source_size: Optional[Sequence[float]] = None) -> PoseRetargetStream:
        return PoseRetargetStream(self.device, ref_keypoints, rr.prepare(size, source_fps, target_fps, align, normalized, score_threshold, source_size))
