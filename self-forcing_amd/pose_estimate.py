"""The DWPose glue on the GPU path: a frame on the device -> whole-body keypoints [F, P, 134, 3] on the device, around two
networks the caller brings (YOLOX-L for person boxes, RTMPose for SimCC keypoints: their weights and their runtime --
MIGraphX, ONNX Runtime, a torch module -- are not this project's).  Everything DWPose does around them in numpy and OpenCV
on the host, one frame and one person at a time, runs here as HIP kernels (csrc/pose_estimate.hip behind
sf_pose_boxes_decode, sf_pose_crop_people and sf_pose_simcc_decode): the YOLOX head decode and greedy NMS, the padded,
aspect-fixed crop of each person, the SimCC arg-max and the map back to the frame, the synthesised neck and the reorder
into the layout `PoseRenderer` and `PoseTracker` take.  The definition of every number is `pose_estimate_reference.py`
(float32, every operation rounded on its own), which the kernels equal bit for bit.  The defaults are DWPose's published
constants as remembered, not checked against a DWPose checkout; every one is a parameter."""
from __future__ import annotations

from typing import Callable, Iterable, Iterator, NamedTuple, Optional, Tuple

import torch

from . import _lib, ops
from . import pose_estimate_reference as er
from .resize import FrameResizer

Tensor = torch.Tensor
_LAYOUT_DIMS = {"hwc": (0, 1, 2, 3), "pose": (1, 2, 3, 0), "chw": (0, 2, 3, 1)}          # the axes of (N, H, W, 3)
_CROP_DTYPES = (torch.float32, torch.bfloat16)


class Estimated(NamedTuple):
    keypoints: Tensor          # float32 [F, P, 134, 3]
    boxes: Tensor              # float32 [F, P, 5]
    count: Tensor              # int32 [F]


class PoseEstimator:
    """`estimate(frames, max_people)` -> the named triple (keypoints float32 [F, P, 134, 3], boxes float32 [F, P, 5],
    count int32 [F]) on the device, every number as `pose_estimate_reference` defines it given the networks' outputs.

    detector: a callable, float32 [F, 3, in_h, in_w] of values 0..255 on the device (the letterboxed frames, 114 where the
    frame does not reach) -> the YOLOX head float32 [F, A, 5 + C].  pose_net: a callable, crops [F * P, 3, out_h, out_w] in
    `crop_dtype` -> (simcc_x [F * P, 133, Wx], simcc_y [F * P, 133, Wy]), float32 or float16.  Rows of people who are not
    there are zeros going in and ignored coming out: the batch is not compacted, which would need a host read of `count`.

    frames: uint8 on the device in a decoder layout, "hwc" [F, H, W, 3], "pose" [3, F, H, W] or "chw" [F, 3, H, W].  The steps:
    the letterbox (`FrameResizer`, bilinear, stretched to (int(H * r), int(W * r)) with r = min(in_h / H, in_w / W) and
    pasted top-left; these are Pillow's antialiased pixels, not cv2.resize's), detector, `ops.decode_boxes`,
    `ops.crop_people`, pose_net, `ops.decode_simcc`.  This class's own code reads nothing back and never synchronises;
    the launches go on the current stream.  The keypoints are normalised to [0, 1] unless normalized=False."""

    def __init__(self, detector: Callable, pose_net: Callable, device="cuda", layout: str = "hwc", input_size=er.INPUT_SIZE, strides=er.STRIDES,
                 class_index: int = 0, score_threshold: float = er.SCORE_THRESHOLD, iou_threshold: float = er.IOU_THRESHOLD, decoded: bool = False,
                 out_size=er.OUT_SIZE, padding: float = er.PADDING, mean=er.MEAN, std=er.STD, channels: str = "rgb", crop_dtype=torch.float32,
                 split_ratio: float = er.SPLIT_RATIO, normalized: bool = True, neck_threshold: float = er.NECK_THRESHOLD, body_dst=er.BODY_DST,
                 body_src=er.BODY_SRC, letterbox_fill: float = er.LETTERBOX_FILL):
        if not callable(detector) or not callable(pose_net):
            raise ValueError("PoseEstimator: detector and pose_net must be callables")
        if layout not in _lib.JPEG_LAYOUTS:
            raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
        if crop_dtype not in _CROP_DTYPES:
            raise ValueError(f"crop_dtype must be torch.float32 or torch.bfloat16, got {crop_dtype}")
        self.detector, self.pose_net = detector, pose_net
        self.device = torch.device(device)
        self.layout, self.crop_dtype, self.channels = layout, crop_dtype, channels
        self.box = er.box_params(input_size, strides, class_index, score_threshold, iou_threshold, decoded)
        self.crop = er.crop_params(out_size, padding, mean, std, channels)
        self.simcc = er.simcc_params(out_size, padding, split_ratio, normalized, neck_threshold, body_dst, body_src)
        self.letterbox_fill = float(letterbox_fill)
        self._order = torch.from_numpy(self.simcc.order.copy())          # the host table the kernel's launch reads
        self.resizer = FrameResizer(self.device)

    def _geometry(self, frames, layout: str) -> Tuple[int, int, int]:
        if layout not in _lib.JPEG_LAYOUTS:
            raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
        if not isinstance(frames, Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[_LAYOUT_DIMS[layout][3]] != 3 \
                or frames.numel() == 0:
            raise ValueError(f"PoseEstimator: frames must be a uint8 tensor in layout {layout!r}, got {getattr(frames, 'dtype', type(frames))} "
                             f"{tuple(getattr(frames, 'shape', ()))}")
        n, h, w = (int(frames.shape[d]) for d in _LAYOUT_DIMS[layout][:3])
        er.check_frame_size((h, w))
        if not frames.is_cuda:
            raise ValueError("PoseEstimator: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
        return n, h, w

    def check_head(self, head, frames: int) -> Tensor:
        """What the detector returned for `frames` frames, or a ValueError that says what it should have been."""
        if not isinstance(head, Tensor) or head.dim() != 3 or head.shape[0] != frames or head.shape[1] != self.box.anchors \
                or not 5 + self.box.class_index < head.shape[2] <= 5 + er.MAX_CLASSES:
            raise ValueError(f"PoseEstimator: the detector must return a head [{frames}, {self.box.anchors}, 5 + C] with C > {self.box.class_index}, "
                             f"got {tuple(getattr(head, 'shape', ()))}")
        return head

    def check_simcc(self, simcc, rows: int) -> Tuple[Tensor, Tensor]:
        """What the pose network returned for `rows` crops, or a ValueError that says what it should have been."""
        if not isinstance(simcc, (tuple, list)) or len(simcc) != 2 or not all(isinstance(t, Tensor) for t in simcc):
            raise ValueError("PoseEstimator: the pose network must return the pair (simcc_x, simcc_y)")
        for name, t in zip(("simcc_x", "simcc_y"), simcc):
            if t.dim() != 3 or t.shape[0] != rows or t.shape[1] != er.SIMCC_POINTS or not 1 <= t.shape[2] <= er.MAX_BINS:
                raise ValueError(f"PoseEstimator: {name} must be [{rows}, {er.SIMCC_POINTS}, bins], got {tuple(t.shape)}")
        if simcc[0].dtype != simcc[1].dtype or simcc[0].dtype not in (torch.float32, torch.float16):
            raise ValueError(f"PoseEstimator: simcc_x and simcc_y must both be float32 or both float16, got {simcc[0].dtype} and {simcc[1].dtype}")
        return simcc[0], simcc[1]

    def letterbox(self, frames: Tensor, layout: Optional[str] = None) -> Tuple[Tensor, float]:
        """(float32 [F, 3, in_h, in_w] of values 0..255, the frame stretched by r into the top-left corner and
        `letterbox_fill` elsewhere; r as a Python float that holds the fp32 value)."""
        layout = self.layout if layout is None else layout
        n, h, w = self._geometry(frames, layout)
        ratio = er.letterbox_ratio((h, w), (self.box.in_h, self.box.in_w))
        nh, nw = er.letterbox_size((h, w), ratio)
        small = self.resizer.resize(frames, (nh, nw), "bilinear", layout, "chw", torch.uint8)
        x = torch.full((n, 3, self.box.in_h, self.box.in_w), self.letterbox_fill, dtype=torch.float32, device=frames.device)
        x[:, :, :nh, :nw] = small
        return x, float(ratio)

    def estimate(self, frames: Tensor, max_people: int, layout: Optional[str] = None) -> Estimated:
        layout = self.layout if layout is None else layout
        people = er.check_people(max_people)
        n, h, w = self._geometry(frames, layout)
        frames = frames.contiguous()
        with torch.cuda.device(frames.device):
            x, ratio = self.letterbox(frames, layout)
            head = self.check_head(self.detector(x), n)
            b = self.box
            boxes, count = ops.decode_boxes(head.to(dtype=torch.float32).contiguous(), ratio, people, (b.in_h, b.in_w), b.strides, b.class_index,
                                            float(b.score_threshold), float(b.iou_threshold), b.decoded)
            c = self.crop
            crops = ops.crop_people(frames, boxes, count, layout, (c.out_h, c.out_w), float(c.padding), [float(v) for v in c.mean],
                                    [float(v) for v in c.std], self.channels, self.crop_dtype)
            simcc = self.check_simcc(self.pose_net(crops), n * people)
            s = self.simcc
            keypoints = ops.decode_simcc(simcc[0].contiguous(), simcc[1].contiguous(), boxes, count, (h, w), (s.out_h, s.out_w), float(s.padding),
                                         float(s.split_ratio), s.normalized, float(s.neck_threshold), self._order)
        return Estimated(keypoints, boxes, count)


def keypoint_feed(frame_pieces: Iterable[Tensor], estimator: PoseEstimator, max_people: int, layout: Optional[str] = None) -> Iterator[Tensor]:
    """One keypoint tensor float32 [n, P, 134, 3] per piece of frames (uint8 on the device in the estimator's layout, as
    `JpegDecoder` and `FrameResizer` give them), each estimated when it is asked for.  A frame's keypoints depend on that
    frame alone, so any partition of a clip gives the whole clip's bits.  `pose_render.pose_feed` takes its keypoints one
    FRAME at a time: hand it `itertools.chain.from_iterable(keypoint_feed(...))`, which splits a piece into views."""
    for piece in frame_pieces:
        yield estimator.estimate(piece, max_people, layout).keypoints
