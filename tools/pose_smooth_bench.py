"""Time the GPU pose smoother on the MI355X and write profiles/pose_smooth_bench.json.

Workload: 151 frames of one person's 134 DWPose keypoints recorded at 30 frames/s (the seeded figure of
tools/pose_render_bench.py with a seeded jitter of +-0.004 and 5 % of the samples missing, float32 on the host, 1.6 KB per
frame), smoothed with min_cutoff 1, beta 0.7 and a hold of 2 frames, then retargeted to a reference person of other
proportions, resampled to the generator's 16 frames/s (81 frames) and drawn at 480 x 832.  One process, a warm-up of
everything, the kernel's output and state compared with `pose_smooth_reference` bit for bit before anything is timed, then
medians of `--iters` windows, each a run of back-to-back calls long enough to fill `--window` seconds, between device events:

* `PoseSmoother.smooth` of keypoints that are already on the device (a call zeroes a fresh state and launches one kernel),
  and the operator alone on a state that is reused;
* smooth + retarget + render against retarget + render, taking turns inside every repeat;
* a stream of 151 one-frame pushes (a kernel per push on a state that stays on the device);
* wall time from keypoints on the host to pose frames on the device (upload, smooth, retarget, render, synchronise)
  against the host alternative in the same process: the numpy definition on the host, an upload of its result, the same
  retarget and render.  The two take turns inside every repeat.

Not measured here: the kernel's time from a profiler trace (the device-event figures hold the launch gap of back-to-back
calls), more than one person.  The tool fails without a GPU.

    python tools/pose_smooth_bench.py [--iters 5] [--window 0.5] [--out profiles/pose_smooth_bench.json]
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
from self_forcing_amd import pose_smooth_reference as sr  # noqa: E402
from pose_render_bench import device_ms, figure, med, wall_s  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time one timing window should fill")
    ap.add_argument("--frames", type=int, default=151, help="source frames at 30 frames/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_smooth_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_smooth_bench: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, size, fps = a.frames, (480, 832), 30
    kw = dict(min_cutoff=1.0, beta=0.7, max_gap=2)
    smoother, retargeter, renderer = sfa.PoseSmoother(device=dev), sfa.PoseRetargeter(device=dev), sfa.PoseRenderer(device=dev)
    rng = np.random.default_rng(2)
    k = figure(0, n)
    k[..., :2] += rng.uniform(-0.004, 0.004, k[..., :2].shape).astype(np.float32)
    k[rng.random(k.shape[:3]) < 0.05] = (-1, -1, 0)
    ref = figure(1, 1)[0]
    ref[..., :2] = (ref[..., :2] - ref[:, 1:2, :2]) * np.float32([0.8, 1.15]) + np.float32([0.45, 0.3])      # another build, another place
    kd, refd = torch.from_numpy(k).to(dev), torch.from_numpy(ref).to(dev)

    p = sr.prepare(fps, **kw)
    want_state, fired = sr.fresh_state(1), {}
    want = sr.frames(k, want_state, p, fired)
    check = smoother.open_stream(fps, **kw)
    got = check.push(kd)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), "the kernel and its definition disagree"
    assert np.array_equal(check.state.cpu().numpy(), want_state), "the kernel's state and the definition's disagree"
    assert torch.equal(smoother.smooth(kd, fps, **kw), got)

    smooth = lambda: smoother.smooth(kd, fps, **kw)                                                             # noqa: E731
    state = torch.zeros_like(check.state)
    op = lambda: sfa.ops.pose_smooth_frames(kd, state, float(p.period), float(p.min_cutoff), float(p.beta), float(p.kd), float(p.threshold), p.max_gap)  # noqa: E731
    draw = lambda pts: renderer.render(retargeter.retarget(pts, refd, size, source_fps=fps), size, normalized=False)      # noqa: E731
    plain = lambda: draw(kd)                                                                                    # noqa: E731
    smoothed = lambda: draw(smoother.smooth(kd, fps, **kw))                                                     # noqa: E731

    def pushes():
        stream = smoother.open_stream(fps, **kw)
        for i in range(n):
            stream.push(kd[i:i + 1])
    gpu_path = lambda: renderer.render(retargeter.retarget(smoother.smooth(k, fps, **kw), ref, size, source_fps=fps), size, normalized=False)  # noqa: E731
    host_path = lambda: renderer.render(retargeter.retarget(sr.smooth(k, fps, **kw), ref, size, source_fps=fps), size, normalized=False)       # noqa: E731
    frames = gpu_path()
    assert torch.equal(frames, host_path()) and torch.equal(frames, smoothed()) and frames.any(), "the two paths draw different frames"
    assert not torch.equal(frames, plain()), "smoothing changed nothing"
    pushes()
    res = {"what": "pose_smooth_bench", "source_frames": n, "source_fps": fps, "target_fps": 16, "frames": int(frames.shape[1]), "people": 1,
           "height": size[0], "width": size[1], "iters": a.iters, "window_s": a.window, "keypoint_bytes": int(k.nbytes),
           "settings": {key: float(v) for key, v in kw.items()}, "rules_fired": fired}

    def calls_for(fn):
        return max(10, int(a.window * 1e3 / device_ms(fn, 10)) + 1)
    for name, fn in (("smooth", smooth), ("smooth_op", op)):
        calls = calls_for(fn)
        t = [device_ms(fn, calls) for _ in range(a.iters)]
        res.update({f"{name}_ms": round(med(t), 5), f"{name}_ms_all": [round(v, 5) for v in t], f"{name}_calls_per_window": calls})
    res["smooth_us_per_frame"] = round(res["smooth_ms"] * 1e3 / n, 4)
    calls = calls_for(smoothed)
    turns = {"smooth_retarget_render": [], "retarget_render": []}
    for _ in range(a.iters):                                               # the candidates take turns
        turns["smooth_retarget_render"].append(device_ms(smoothed, calls))
        turns["retarget_render"].append(device_ms(plain, calls))
    for name, t in turns.items():
        res.update({f"{name}_ms": round(med(t), 5), f"{name}_ms_all": [round(v, 5) for v in t]})
    res["chain_calls_per_window"] = calls
    calls = max(2, int(a.window * 1e3 / device_ms(pushes, 2)) + 1)
    t = [device_ms(pushes, calls) for _ in range(a.iters)]
    res.update({"stream_151_pushes_ms": round(med(t), 4), "stream_151_pushes_ms_all": [round(v, 4) for v in t],
                "stream_push_us": round(med(t) * 1e3 / n, 3), "stream_runs_per_window": calls})
    walls = {"gpu": [], "host": []}
    for _ in range(a.iters):
        walls["gpu"].append(wall_s(gpu_path))
        walls["host"].append(wall_s(host_path))
    res.update({"gpu_path_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "gpu_path_wall_ms_all": [round(v * 1e3, 3) for v in walls["gpu"]],
                "host_path_wall_ms": round(med(walls["host"]) * 1e3, 2), "host_path_wall_ms_all": [round(v * 1e3, 2) for v in walls["host"]],
                "not_measured": ["kernel time from a profiler trace", "more than one person"]})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
