"""Time the GPU pose tracker on the MI355X and write profiles/pose_track_bench.json.

Workload: 151 frames at 30 frames/s of one, three and eight people's 134 DWPose keypoints (the seeded figure of
tools/pose_render_bench.py, one per person, scaled and placed side by side, with a seeded jitter and 5 % of the samples
missing, float32 on the host, 1.6 KB per frame and person), the people of every frame after the first in a seeded random
order, tracked with the defaults (gate 0.5, max_age 2), then smoothed (min_cutoff 1, beta 0.7, a hold of 2 frames), retargeted to a reference
person of other proportions, resampled to the generator's 16 frames/s (81 frames) and drawn at 480 x 832.  One process, a
warm-up of everything, the kernels' output, ids and state compared with `pose_track_reference` bit for bit before anything
is timed, then medians of `--iters` windows, each a run of back-to-back calls long enough to fill `--window` seconds,
between device events.  Per number of people:

* `PoseTracker.track` of keypoints that are already on the device (a call zeroes a fresh state, allocates the outputs and
  the scratch and launches the two kernels), and the operator alone on a state that is reused;
* track + smooth + retarget + render against smooth + retarget + render, taking turns inside every repeat: the difference
  is what the stage adds;
* a stream of 151 one-frame pushes (two kernels per push on a state that stays on the device);

and for three people, wall time from keypoints on the host to pose frames on the device (upload, track, smooth, retarget,
render, synchronise) against the host alternative in the same process: the numpy definition of the tracker on the host, an
upload of its result, the same smooth, retarget and render.  The two take turns inside every repeat.

Not measured here: the time of either kernel from a profiler trace (the device-event figures hold the launch gaps of
back-to-back calls, and the split between the assignment and the gather kernel is not known from them).  The tool fails
without a GPU.

    python tools/pose_track_bench.py [--iters 5] [--window 0.5] [--out profiles/pose_track_bench.json]
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
from self_forcing_amd import pose_track_reference as tr  # noqa: E402
from pose_render_bench import device_ms, figure, med, wall_s  # noqa: E402


def crowd(people: int, frames: int):
    """(the clip in a stable order, the same clip with the people of every later frame shuffled): float32 [frames, people, 134, 3]"""
    rng = np.random.default_rng(2 + people)
    k = np.concatenate([figure(q, frames) for q in range(people)], axis=1)
    scale = np.float32([0.9 / people, 0.8])
    for q in range(people):
        k[:, q, :, :2] = (k[:, q, :, :2] - 0.5) * scale + np.float32([(q + 0.5) / people, 0.5])
    k[..., :2] += (rng.uniform(-0.004, 0.004, k[..., :2].shape) * scale).astype(np.float32)
    k[rng.random(k.shape[:3]) < 0.05] = (-1, -1, 0)
    mixed = k.copy()
    for f in range(1, frames):                                              # frame 0 sets the slots: its order is the stable one
        mixed[f] = k[f, rng.permutation(people)]
    return k, mixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time one timing window should fill")
    ap.add_argument("--frames", type=int, default=151, help="source frames at 30 frames/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_track_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_track_bench: no GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, size, fps = a.frames, (480, 832), 30
    kw = dict(min_cutoff=1.0, beta=0.7, max_gap=2)
    tracker, smoother = sfa.PoseTracker(device=dev), sfa.PoseSmoother(device=dev)
    retargeter, renderer = sfa.PoseRetargeter(device=dev), sfa.PoseRenderer(device=dev)
    ref = figure(1, 1)[0]
    ref[..., :2] = (ref[..., :2] - ref[:, 1:2, :2]) * np.float32([0.8, 1.15]) + np.float32([0.45, 0.3])      # another build, another place
    refd = torch.from_numpy(ref).to(dev)
    p = tr.prepare()
    res = {"what": "pose_track_bench", "source_frames": n, "source_fps": fps, "target_fps": 16, "height": size[0], "width": size[1],
           "iters": a.iters, "window_s": a.window, "tracker": {"gate": 0.5, "max_age": p.max_age, "min_points": p.min_points, "min_common": p.min_common},
           "smoother": {key: float(v) for key, v in kw.items()}, "people": {}}

    def calls_for(fn):
        return max(10, int(a.window * 1e3 / device_ms(fn, 10)) + 1)

    for people in (1, 3, 8):
        steady, k = crowd(people, n)
        kd = torch.from_numpy(k).to(dev)
        want_state, fired = tr.fresh_state(people), {}
        want, want_ids = tr.frames(k, want_state, p, fired)
        check = tracker.open_stream()
        got = check.push(kd)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), "the kernels and their definition disagree"
        assert np.array_equal(check.ids.cpu().numpy(), want_ids), "the kernels' ids and the definition's disagree"
        assert np.array_equal(check.state.cpu().numpy(), want_state), "the kernels' state and the definition's disagree"
        assert torch.equal(tracker.track(kd).keypoints, got)
        in_order = bool(np.array_equal(want.view(np.int32), steady.view(np.int32)))       # the tracker undid the shuffle

        track = lambda: tracker.track(kd)                                                                       # noqa: E731
        state = torch.zeros_like(check.state)
        op = lambda: sfa.ops.pose_track_frames(kd, state, people, float(p.gate2), float(p.threshold), p.min_points, p.min_common, p.max_age)    # noqa: E731
        draw = lambda pts: renderer.render(retargeter.retarget(smoother.smooth(pts, fps, **kw), refd, size, source_fps=fps), size, normalized=False)  # noqa: E731
        plain = lambda: draw(kd)                                                                                # noqa: E731
        tracked = lambda: draw(tracker.track(kd).keypoints)                                                     # noqa: E731

        def pushes():
            stream = tracker.open_stream()
            for i in range(n):
                stream.push(kd[i:i + 1])
        frames = tracked()
        assert frames.any() and (people == 1 or not torch.equal(frames, plain())), "tracking changed nothing"
        pushes()
        r = {"keypoint_bytes": int(k.nbytes), "rules_fired": fired, "ids_used": int(want_ids.max()) + 1, "shuffle_undone": in_order,
             "frames": int(frames.shape[1])}
        for name, fn in (("track", track), ("track_op", op)):
            calls = calls_for(fn)
            t = [device_ms(fn, calls) for _ in range(a.iters)]
            r.update({f"{name}_ms": round(med(t), 5), f"{name}_ms_all": [round(v, 5) for v in t], f"{name}_calls_per_window": calls})
        r["track_us_per_frame"] = round(r["track_ms"] * 1e3 / n, 4)
        calls = calls_for(tracked)
        turns = {"track_smooth_retarget_render": [], "smooth_retarget_render": []}
        for _ in range(a.iters):                                           # the candidates take turns
            turns["track_smooth_retarget_render"].append(device_ms(tracked, calls))
            turns["smooth_retarget_render"].append(device_ms(plain, calls))
        for name, t in turns.items():
            r.update({f"{name}_ms": round(med(t), 5), f"{name}_ms_all": [round(v, 5) for v in t]})
        r["track_adds_ms"] = round(r["track_smooth_retarget_render_ms"] - r["smooth_retarget_render_ms"], 5)   # inferred from the two, not traced
        r["chain_calls_per_window"] = calls
        calls = max(2, int(a.window * 1e3 / device_ms(pushes, 2)) + 1)
        t = [device_ms(pushes, calls) for _ in range(a.iters)]
        r.update({"stream_151_pushes_ms": round(med(t), 4), "stream_151_pushes_ms_all": [round(v, 4) for v in t],
                  "stream_push_us": round(med(t) * 1e3 / n, 3), "stream_runs_per_window": calls})
        if people == 3:
            gpu_path = lambda: draw(tracker.track(k).keypoints)                                                 # noqa: E731
            host_path = lambda: draw(tr.track(k)[0])                                                            # noqa: E731
            assert torch.equal(gpu_path(), host_path()) and torch.equal(gpu_path(), frames), "the two paths draw different frames"
            walls = {"gpu": [], "host": []}
            for _ in range(a.iters):
                walls["gpu"].append(wall_s(gpu_path))
                walls["host"].append(wall_s(host_path))
            r.update({"gpu_path_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "gpu_path_wall_ms_all": [round(v * 1e3, 3) for v in walls["gpu"]],
                      "host_path_wall_ms": round(med(walls["host"]) * 1e3, 2), "host_path_wall_ms_all": [round(v * 1e3, 2) for v in walls["host"]]})
        res["people"][str(people)] = r
    res["not_measured"] = ["the time of either kernel from a profiler trace", "the split between the assignment and the gather kernel"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
