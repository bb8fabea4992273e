"""Time the GPU pose retargeter on the MI355X and write profiles/pose_retarget_bench.json.

Workload: 151 frames of one person's 134 DWPose keypoints recorded at 30 frames/s (the seeded figure of
tools/pose_render_bench.py, float32 on the host, 1.6 KB per frame), retargeted to a reference person of other proportions
and resampled to the generator's 16 frames/s: 81 output frames, drawn at 480 x 832.  One process, a warm-up of everything,
the kernel's output compared with `pose_retarget_reference.retarget` bit for bit before anything is timed, then:

* `PoseRetargeter.retarget` of keypoints that are already on the device: device time from device events around a run of
  back-to-back calls long enough to fill `--window` seconds (a call is one kernel);
* retarget + `PoseRenderer.render` against the render alone (of keypoints already retargeted), the same way;
* wall time from keypoints on the host to pose frames on the device (upload, retarget, render, synchronise) against the
  host alternative in the same process: the numpy definition on the host, an upload of its result, the same render.  The
  two take turns inside every repeat.

Not measured here: the kernel's time from a profiler trace (the device-event figure holds the launch gap of back-to-back
calls), more than one person, a stream of single-frame pushes.

    python tools/pose_retarget_bench.py [--iters 5] [--window 1.0] [--out profiles/pose_retarget_bench.json]
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
from self_forcing_amd import pose_retarget_reference as rr  # noqa: E402
from pose_render_bench import device_ms, figure, med, wall_s  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device time one timing window should fill")
    ap.add_argument("--frames", type=int, default=151, help="source frames at 30 frames/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_retarget_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, size, fps = a.frames, (480, 832), 30
    retargeter, renderer = sfa.PoseRetargeter(device=dev), sfa.PoseRenderer(device=dev)
    k = figure(0, n)
    ref = figure(1, 1)[0]
    ref[..., :2] = (ref[..., :2] - ref[:, 1:2, :2]) * np.float32([0.8, 1.15]) + np.float32([0.45, 0.3])      # another build, another place
    kd, refd = torch.from_numpy(k).to(dev), torch.from_numpy(ref).to(dev)
    retarget = lambda: retargeter.retarget(kd, refd, size, source_fps=fps)                                    # noqa: E731
    moved = retarget()
    want = rr.retarget(k, ref, size, source_fps=fps)
    assert np.array_equal(moved.cpu().numpy().view(np.int32), want.view(np.int32)), "the kernel and its definition disagree"
    n_out = moved.shape[0]
    render = lambda: renderer.render(moved, size, normalized=False)                                           # noqa: E731
    both = lambda: renderer.render(retargeter.retarget(kd, refd, size, source_fps=fps), size, normalized=False)      # noqa: E731
    gpu_path = lambda: renderer.render(retargeter.retarget(k, ref, size, source_fps=fps), size, normalized=False)    # noqa: E731
    host_path = lambda: renderer.render(rr.retarget(k, ref, size, source_fps=fps), size, normalized=False)    # noqa: E731
    frames = gpu_path()
    assert torch.equal(frames, host_path()) and torch.equal(frames, both()) and frames.any(), "the two paths draw different frames"
    res = {"what": "pose_retarget_bench", "source_frames": n, "source_fps": fps, "target_fps": 16, "frames": n_out, "people": 1, "height": size[0],
           "width": size[1], "iters": a.iters, "window_s": a.window, "keypoint_bytes": int(k.nbytes), "bytes_written": int(moved.numel() * 4)}
    for name, fn in (("retarget", retarget), ("render", render), ("retarget_render", both)):
        calls = max(10, int(a.window * 1e3 / device_ms(fn, 10)) + 1)
        t = [device_ms(fn, calls) for _ in range(a.iters)]
        res.update({f"{name}_ms": round(med(t), 5), f"{name}_ms_all": [round(v, 5) for v in t], f"{name}_calls_per_window": calls})
    res["retarget_us_per_frame"] = round(res["retarget_ms"] * 1e3 / n_out, 4)
    walls = {"gpu": [], "host": []}
    for _ in range(a.iters):                                               # the candidates take turns
        walls["gpu"].append(wall_s(gpu_path))
        walls["host"].append(wall_s(host_path))
    res.update({"gpu_path_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "gpu_path_wall_ms_all": [round(v * 1e3, 3) for v in walls["gpu"]],
                "host_path_wall_ms": round(med(walls["host"]) * 1e3, 2), "host_path_wall_ms_all": [round(v * 1e3, 2) for v in walls["host"]],
                "not_measured": ["kernel time from a profiler trace", "more than one person", "single-frame stream pushes"]})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
