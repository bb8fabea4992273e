"""Pose renderer on the GPU path: DWPose whole-body keypoints become the skeleton frames the pose branch embeds, drawn on the
device (csrc/pose_render.hip behind sf_pose_render_frames).  A keypoint source hands over about 1.5 KB per frame and person;
that upload is the only host-to-device copy.  The definition of every pixel is `pose_render_reference.py`: this project's
drawing in DWPose's style, in integer arithmetic, which the kernel equals bit for bit."""
from __future__ import annotations

from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import pose_render_reference as pr
from .pose_keypoints import KeypointChain, KeypointStage, as_tensor

Tensor = torch.Tensor
_DTYPES = (torch.uint8, torch.float32, torch.bfloat16)


def check_arguments(size, layout: str, dtype, score_threshold) -> Tuple[int, int]:
    """The checks of `PoseRenderer.render` that need neither keypoints nor a device: (height, width) of the frames."""
    h, w = pr.check_size(size)
    if layout not in _lib.JPEG_LAYOUTS:
        raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
    pr.check_threshold(score_threshold)
    return h, w


class PoseRenderer(KeypointStage):
    """`render(keypoints, size)` -> skeleton frames on the device, every pixel as `pose_render_reference.render` defines it.

    keypoints: float [F, P, 134, 3] or [F, 134, 3] = (x, y, score) in DWPose's whole-body order, P <= 8; a numpy array, a
    host tensor (uploaded to the renderer's device: the only host-to-device copy) or a device tensor (rendered where it
    is).  normalized=True: x, y in [0, 1]; False: in pixels of the output.  A point counts when it is finite, its score is
    at least `score_threshold` and it is not negative.  The frames have layout "hwc" [F, H, W, 3], "pose" [3, F, H, W]
    (what `PoseEmbedder` / `PoseStream` take) or "chw" [F, 3, H, W], as uint8 or as float32 / bfloat16 u8 / 127.5 - 1 (the
    decoder's conversion); H, W <= 4096.  `out`: a contiguous, 16-byte-aligned tensor of that shape to fill, a slice of a
    larger buffer included.  Work runs on the current stream."""

    def render(self, keypoints, size: Sequence[int], layout: str = "pose", dtype=torch.uint8, normalized: bool = True,
               score_threshold: float = 0.3, out: Optional[Tensor] = None) -> Tensor:
        h, w = check_arguments(size, layout, dtype, score_threshold)
        keypoints = as_tensor(keypoints, "PoseRenderer")
        f, p = pr.check_keypoints_shape(keypoints.shape)
        device = keypoints.device if keypoints.is_cuda else self.device
        if device.type != "cuda":
            raise ValueError("PoseRenderer: expected a CUDA/ROCm device (the HIP path has no CPU fallback)")
        shape = {"hwc": (f, h, w, 3), "pose": (3, f, h, w), "chw": (f, 3, h, w)}[layout]
        if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or not out.is_cuda or (keypoints.is_cuda and out.device != device)
                                or not out.is_contiguous() or out.data_ptr() % 16):
            raise ValueError(f"PoseRenderer: out must be a contiguous, 16-byte-aligned {dtype} tensor {shape} on {device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
        if out is not None:
            device = out.device
        keypoints = keypoints.to(device=device, dtype=torch.float32).reshape(f, p, pr.KEYPOINTS, 3).contiguous()
        with torch.cuda.device(device):
            return ops.pose_render_frames(keypoints, h, w, layout, dtype, bool(normalized), float(score_threshold), out)


def pose_feed(keypoints: Iterable, renderer: PoseRenderer, size: Sequence[int], frames_per_piece: int = 12, normalized: bool = True,
              score_threshold: float = 0.3, retargeter=None, smoother=None, tracker=None) -> Iterator[Tensor]:
    """Keypoints as the pieces `CausalInferencePipeline.stream(pose_feed=...)` pulls, the counterpart of `jpeg.pose_feed`:
    uint8 [3, n, H, W], n = `frames_per_piece` (the last piece may be shorter), each rendered when it is asked for.
    `keypoints` yields one frame at a time, [P, 134, 3] or [134, 3] (an array [F, P, 134, 3] does); it may be a live source.
    `retargeter`: a `PoseRetargetStream` (`PoseRetargeter.open_stream`, opened for the same `size`) the source frames go
    through first; pieces are then counted in its OUTPUT frames, and `normalized` is the stream's own (its output is drawn
    as pixels).  `smoother`: a `PoseSmoothStream` (`PoseSmoother.open_stream`) the source frames go through before anything
    else: with a retargeter each gathered batch is smoothed and then pushed to it, without one each piece is smoothed and
    then drawn with `normalized`.  `tracker`: a `PoseTrackStream` (`PoseTracker.open_stream`) in front of the smoother, for a
    source that lists the people of a frame in no stable order: source frames go through the tracker, then the smoother,
    then the retargeter.  A tracker keeps a slot empty for at least max_age + 1 frames between two different people, so a
    smoother that bridges at most max_age frames never filters one person towards another; a smoother whose max_gap
    exceeds the tracker's max_age is refused.  Source frames are gathered until the chain's plan says that a piece of
    output frames is final, pushed through it in one call, and the output is drawn `frames_per_piece` frames at a time."""
    chain = KeypointChain(tracker, smoother, retargeter)
    if frames_per_piece < 1:
        raise ValueError(f"frames_per_piece must be >= 1, got {frames_per_piece}")
    size = check_arguments(size, "pose", torch.uint8, score_threshold)
    if retargeter is not None and (retargeter.params.h, retargeter.params.w) != size:
        raise ValueError(f"pose_feed: the retargeter was opened for {(retargeter.params.h, retargeter.params.w)}, the frames are {size}")
    normalized = normalized and not chain.in_pixels

    def pushed(ready, frames: List):
        """`frames` through the chain as one batch, behind the output frames that wait in `ready`."""
        new = chain.push(torch.stack(frames) if isinstance(frames[0], Tensor) else np.stack([np.asarray(k) for k in frames]))
        return new if ready is None or not ready.shape[0] else torch.cat([ready, new])

    ready = None                           # output frames not yet drawn, fewer than a piece
    gathered: List = []
    for k in keypoints:
        gathered.append(k)
        held = 0 if ready is None else ready.shape[0]
        if held + chain.planned(len(gathered)) < frames_per_piece:
            continue
        ready, gathered = pushed(ready, gathered), []
        while ready.shape[0] >= frames_per_piece:
            piece, ready = ready[:frames_per_piece], ready[frames_per_piece:]
            yield renderer.render(piece, size, "pose", torch.uint8, normalized, score_threshold)
    if gathered:                           # the clip's end, or source frames behind the last output frame, which make nothing final
        ready = pushed(ready, gathered)
    if ready is not None and ready.shape[0]:
        yield renderer.render(ready, size, "pose", torch.uint8, normalized, score_threshold)
