"""Time the GPU pose renderer on the MI355X against drawing on the host and write profiles/pose_render_bench.json.

Workload: 81 frames of one person's 134 DWPose keypoints (a seeded figure that drifts and sways; float32 on the host,
1.6 KB per frame), rendered at 480 x 832 in the "pose" layout [3, 81, 480, 832] uint8.  One process, a warm-up of
everything, then:

* `PoseRenderer.render` of keypoints that are already on the device: device time from device events around a run of
  back-to-back calls long enough to fill `--window` seconds (a call is one kernel), and the output bytes written per second;
* the whole GPU path from keypoints on the host to frames on the device (upload, kernel, synchronise): wall time;
* the host path: Pillow `ImageDraw` per frame (a 360-point ellipse polygon per limb, `ellipse` per disc, `line(width=2)`
  per hand edge; one thread), an upload of each frame, then the pose layout: wall time, taking turns with the GPU path
  inside every repeat.  Pillow's pixels are not the renderer's; the share that differs is recorded.

The kernel's frames are compared with `pose_render_reference.render` before anything is timed.

    python tools/pose_render_bench.py [--iters 5] [--window 1.0] [--out profiles/pose_render_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import pose_render_reference as pr  # noqa: E402

# a standing figure in a unit box, OpenPose-18 order: (x, y), y down
BODY = [(0.50, 0.12), (0.50, 0.24), (0.40, 0.24), (0.34, 0.40), (0.30, 0.54), (0.60, 0.24), (0.66, 0.40), (0.70, 0.54), (0.44, 0.55), (0.43, 0.75),
        (0.42, 0.95), (0.56, 0.55), (0.57, 0.75), (0.58, 0.95), (0.48, 0.10), (0.52, 0.10), (0.45, 0.12), (0.55, 0.12)]


def figure(seed: int, frames: int) -> np.ndarray:
    """float32 [frames, 1, 134, 3]: the figure above drifting across the frame, every point swaying a little; the face is
    a ring of 68 points about the nose, a hand five fingers of four points fanning out of each wrist; scores 0.5..1."""
    rng = np.random.default_rng(seed)
    k = np.zeros((frames, 1, 134, 3), np.float32)
    t = np.linspace(0, 1, frames)[:, None]
    body = np.asarray(BODY, np.float32)
    drift = np.stack([0.25 * np.sin(2 * math.pi * t[:, 0]), 0.03 * np.cos(4 * math.pi * t[:, 0])], -1)[:, None]
    sway = 0.01 * np.sin(2 * math.pi * (3 * t[..., None] + rng.random((1, 18, 2))))
    pts = (body[None] - 0.5) * np.float32([0.45, 0.85]) + 0.5 + drift + sway
    k[:, 0, :18, :2] = pts
    k[:, 0, 18:24, :2] = pts[:, [10, 10, 10, 13, 13, 13]]
    a = np.linspace(0, 2 * math.pi, 68, endpoint=False)
    k[:, 0, 24:92, :2] = pts[:, :1] + np.stack([0.035 * np.cos(a), 0.06 * np.sin(a)], -1)[None] * (0.4 + 0.6 * (np.arange(68) % 3 == 0))[None, :, None]
    for base, wrist, side in ((92, 7, 1.0), (113, 4, -1.0)):
        k[:, 0, base, :2] = pts[:, wrist]
        for finger in range(5):
            ang = math.pi / 2 + side * (finger - 2) * 0.35
            for j in range(4):
                k[:, 0, base + 1 + 4 * finger + j, :2] = pts[:, wrist] + (j + 1) * np.float32([0.012 * math.cos(ang), 0.02 * math.sin(ang)])
    k[..., 2] = rng.uniform(0.5, 1.0, (frames, 1, 134))
    return k


def pillow_frame(k: np.ndarray, h: int, w: int) -> np.ndarray:
    """One frame [P, 134, 3] drawn by Pillow in the renderer's order and colours: uint8 [h, w, 3]."""
    im = Image.new("RGB", (w, h))
    d = ImageDraw.Draw(im)
    X, Y, ok = pr.quantize(k, (h, w))
    people = range(k.shape[0])
    for i, (a, b) in enumerate(pr.LIMBS):
        for p in people:
            if ok[p, a] and ok[p, b] and (X[p, a], Y[p, a]) != (X[p, b], Y[p, b]):
                x0, y0, x1, y1 = int(X[p, a]), int(Y[p, a]), int(X[p, b]), int(Y[p, b])
                cx, cy, half, ang = (x0 + x1) / 2, (y0 + y1) / 2, math.hypot(x1 - x0, y1 - y0) / 2, math.atan2(y1 - y0, x1 - x0)
                ca, sa = math.cos(ang), math.sin(ang)
                d.polygon([(cx + half * math.cos(t) * ca - 4 * math.sin(t) * sa, cy + half * math.cos(t) * sa + 4 * math.sin(t) * ca)
                           for t in np.linspace(0, 2 * math.pi, 360, False)], fill=pr.LIMB_COLORS[i])

    def disc(p, j, r, rgb):
        if ok[p, j]:
            d.ellipse([int(X[p, j]) - r, int(Y[p, j]) - r, int(X[p, j]) + r, int(Y[p, j]) + r], fill=rgb)
    for j in range(18):
        for p in people:
            disc(p, j, 4, pr.COLORS[j])
    for p in people:
        for base in pr.HANDS0:
            for e, (a, b) in enumerate(pr.HAND_EDGES):
                if ok[p, base + a] and ok[p, base + b]:
                    d.line([(int(X[p, base + a]), int(Y[p, base + a])), (int(X[p, base + b]), int(Y[p, base + b]))], fill=pr.HAND_EDGE_COLORS[e], width=2)
            for j in range(21):
                disc(p, base + j, 4, pr.HAND_COLOR)
    for p in people:
        for j in range(68):
            disc(p, pr.FACE0 + j, 3, pr.FACE_COLOR)
    return np.asarray(im)


def pillow_path(k, size, dev):
    """Per frame: Pillow drawing on the host, the frame to the device; then the pose layout."""
    out = torch.empty(len(k), size[0], size[1], 3, dtype=torch.uint8, device=dev)
    for f in range(len(k)):
        out[f].copy_(torch.from_numpy(pillow_frame(k[f], *size)))
    return out.permute(3, 0, 1, 2).contiguous()


def device_ms(fn, calls):
    """device milliseconds per call over `calls` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device time one timing window should fill")
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_render_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, size = a.frames, (480, 832)
    renderer = sfa.PoseRenderer(device=dev)
    k = figure(0, n)
    kd = torch.from_numpy(k).to(dev)
    on_device = lambda: renderer.render(kd, size)                                                     # noqa: E731
    from_host = lambda: renderer.render(k, size)                                                      # noqa: E731
    got = from_host()
    want = pr.render(k, size, "pose")
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(on_device(), got), "the kernel and its definition disagree"
    pil = pillow_path(k, size, dev)
    differ = (pil != got).any(0)
    drawn = got.any(0) | pil.any(0)
    calls = max(10, int(a.window * 1e3 / device_ms(on_device, 10)) + 1)
    gpu = [device_ms(on_device, calls) for _ in range(a.iters)]
    walls = {"gpu": [], "pil": []}
    for _ in range(a.iters):                                               # the candidates take turns
        walls["gpu"].append(wall_s(from_host))
        walls["pil"].append(wall_s(lambda: pillow_path(k, size, dev)))
    written = n * 3 * size[0] * size[1]
    res = {"what": "pose_render_bench", "frames": n, "people": 1, "height": size[0], "width": size[1], "layout": "pose", "dtype": "uint8",
           "iters": a.iters, "window_s": a.window, "calls_per_window": calls, "keypoint_bytes": int(k.nbytes), "bytes_written": written,
           "drawn_share_of_pixels": round(float(drawn.float().mean()), 5),
           "gpu_ms": round(med(gpu), 4), "gpu_ms_all": [round(t, 4) for t in gpu], "gpu_us_per_frame": round(med(gpu) * 1e3 / n, 3),
           "gbytes_written_per_s": round(written / (med(gpu) * 1e-3) / 1e9, 1),
           "gpu_path_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "gpu_path_wall_ms_all": [round(v * 1e3, 3) for v in walls["gpu"]],
           "pillow_path_wall_ms": round(med(walls["pil"]) * 1e3, 2), "pillow_path_wall_ms_all": [round(v * 1e3, 2) for v in walls["pil"]],
           "pillow_differs_share_of_pixels": round(float(differ.float().mean()), 5),
           "pillow_differs_share_of_drawn": round(float(differ.sum() / drawn.sum()), 4)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
