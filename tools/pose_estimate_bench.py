"""Time the DWPose glue on the MI355X and write profiles/pose_estimate_bench.json.

Workload: uint8 frames of 480 x 832 on the device (seeded noise), one frame and a 12-frame piece, with one, three and eight
people, at DWPose's sizes: a 640 x 640 detector input, a YOLOX head of 8400 x 85, crops of 384 x 288, SimCC rows of 576 and
768 float32 bins.  The two networks are stubs that return fixed device tensors (a head with exactly `people` person-sized
boxes on the stride-32 level, seeded SimCC logits), so what is timed is the glue alone.  One process, a warm-up of
everything, the kernels' boxes, crops and keypoints compared with `pose_estimate_reference` bit for bit before anything is
timed, then medians of `--iters` windows, each a run of back-to-back calls long enough to fill `--window` seconds, between
device events.  Per configuration:

* each stage on its own: `ops.decode_boxes` (two kernels and the scratch's allocation), `ops.crop_people`,
  `ops.decode_simcc`;
* the whole glue, `PoseEstimator.estimate` with the stubs: the letterbox (`FrameResizer` and a torch fill and copy), the
  three stages, and the stubs' returns;
* wall time of the same with a synchronise at the end, against the host alternative in the same process: the head copied
  to the host, `decode_boxes` of the numpy definition, the frames copied to the host and cropped there, the crops uploaded
  for the pose network, the SimCC logits copied to the host and decoded there, the keypoints uploaded.  The two take turns
  inside every repeat.  The host alternative is this project's numpy definition, not DWPose's OpenCV code.

Not measured here: the time of each kernel from a profiler trace (the device-event figures hold the launch gaps of
back-to-back calls and the allocator), and the two networks.  The tool fails without a GPU.

    python tools/pose_estimate_bench.py [--iters 5] [--window 0.5] [--out profiles/pose_estimate_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import pose_estimate_reference as er  # noqa: E402
from pose_render_bench import device_ms, med, wall_s  # noqa: E402

SIZE, CLASSES, BINS = (480, 832), 80, (576, 768)


def stub_head(frames: int, people: int, p: er.BoxParams) -> np.ndarray:
    """float32 [frames, 8400, 85]: low scores everywhere, `people` person-sized boxes side by side on the last level."""
    rng = np.random.default_rng(people)
    head = rng.normal(0, 1, (frames, p.anchors, 5 + CLASSES)).astype(np.float32)
    head[..., 4:] = rng.uniform(0, 0.5, (frames, p.anchors, 1 + CLASSES))                   # products below 0.25: no candidate
    last = p.anchors - (p.in_h // 32) * (p.in_w // 32)
    for q in range(people):
        a = last + 5 * (p.in_w // 32) + 2 + 2 * q
        head[:, a, :4] = (0.5, 0.5, 0.3, 1.5)
        head[:, a, 4], head[:, a, 5] = 0.95 - 0.05 * q, 1.0
    return head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time one timing window should fill")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_estimate_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_estimate_bench: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    box, crop, simcc = er.box_params(), er.crop_params(), er.simcc_params()
    res = {"what": "pose_estimate_bench", "height": SIZE[0], "width": SIZE[1], "input_size": [box.in_h, box.in_w], "anchors": box.anchors,
           "classes": CLASSES, "crop": [crop.out_h, crop.out_w], "bins": list(BINS), "simcc_dtype": "float32", "crop_dtype": "float32",
           "iters": a.iters, "window_s": a.window, "configs": {}}

    def calls_for(fn):
        return max(10, int(a.window * 1e3 / device_ms(fn, 10)) + 1)

    for frames in (1, 12):
        for people in (1, 3, 8):
            rng = np.random.default_rng(100 * frames + people)
            pix = rng.integers(0, 256, (frames,) + SIZE + (3,), dtype=np.uint8)
            head = stub_head(frames, people, box)
            sx = rng.normal(0, 1, (frames * people, 133, BINS[0])).astype(np.float32)
            sy = rng.normal(0, 1, (frames * people, 133, BINS[1])).astype(np.float32)
            pix_d, head_d, sx_d, sy_d = (torch.from_numpy(v).to(dev) for v in (pix, head, sx, sy))
            est = sfa.PoseEstimator(lambda x: head_d, lambda crops: (sx_d, sy_d), dev)
            got = est.estimate(pix_d, people)
            ratio = er.letterbox_ratio(SIZE, (box.in_h, box.in_w))
            want_b, want_c = er.decode_boxes(head, ratio, people, box)
            assert want_c.tolist() == [people] * frames, "the stub head does not hold the people it should"
            want_crops = er.crop_people(pix, want_b, want_c, "hwc", crop)
            want_k = er.decode_simcc(sx, sy, want_b, want_c, SIZE, simcc)
            same = lambda t, w: np.array_equal(t.cpu().numpy().view(np.int32), w.view(np.int32))                 # noqa: E731
            assert same(got.boxes, want_b) and same(got.count, want_c) and same(got.keypoints, want_k), "the kernels and their definition disagree"
            assert same(sfa.ops.crop_people(pix_d, got.boxes, got.count), want_crops), "the crop kernel and its definition disagree"

            boxes_d, count_d = got.boxes, got.count
            stages = {"decode_boxes": lambda: sfa.ops.decode_boxes(head_d, float(ratio), people),
                      "crop_people": lambda: sfa.ops.crop_people(pix_d, boxes_d, count_d),
                      "decode_simcc": lambda: sfa.ops.decode_simcc(sx_d, sy_d, boxes_d, count_d, SIZE),
                      "letterbox": lambda: est.letterbox(pix_d),
                      "estimate": lambda: est.estimate(pix_d, people)}
            r = {"head_bytes": int(head.nbytes), "crop_bytes": int(want_crops.nbytes), "simcc_bytes": int(sx.nbytes + sy.nbytes),
                 "valid_points": int((want_k[..., 2] > 0).sum())}
            for name, fn in stages.items():
                calls = calls_for(fn)
                t = [device_ms(fn, calls) for _ in range(a.iters)]
                r.update({f"{name}_ms": round(med(t), 5), f"{name}_ms_all": [round(v, 5) for v in t], f"{name}_calls_per_window": calls})

            def gpu_path():
                return est.estimate(pix_d, people).keypoints

            def host_path():
                b, c = er.decode_boxes(head_d.cpu().numpy(), ratio, people, box)
                crops = torch.from_numpy(er.crop_people(pix_d.cpu().numpy(), b, c, "hwc", crop)).to(dev)      # what the pose network would take
                assert crops.shape[0] == frames * people
                return torch.from_numpy(er.decode_simcc(sx_d.cpu().numpy(), sy_d.cpu().numpy(), b, c, SIZE, simcc)).to(dev)
            assert torch.equal(gpu_path(), host_path()), "the two paths give different keypoints"
            walls = {"gpu": [], "host": []}
            for _ in range(a.iters):                                       # the candidates take turns
                walls["gpu"].append(wall_s(gpu_path))
                walls["host"].append(wall_s(host_path))
            r.update({"gpu_path_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "gpu_path_wall_ms_all": [round(v * 1e3, 3) for v in walls["gpu"]],
                      "host_path_wall_ms": round(med(walls["host"]) * 1e3, 2), "host_path_wall_ms_all": [round(v * 1e3, 2) for v in walls["host"]]})
            res["configs"][f"{frames}x{people}"] = r
    res["not_measured"] = ["the time of each kernel from a profiler trace", "the two networks", "float16 SimCC logits and bfloat16 crops"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
