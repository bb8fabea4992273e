"""Time the GPU frame resizer on the MI355X against the host path and write profiles/resize_bench.json.

Workload: 81 skeleton pose frames (`pose_weights.synth_pose_clip`) of 720 x 1280 and of 1080 x 1920, uint8 [N, H, W, 3] on
the device, resized to 480 x 832 in the "pose" layout [3, N, 480, 832] uint8, bilinear and bicubic.  One process, a warm-up
of everything, then per case:

* `FrameResizer.resize`: device time from device events around a run of back-to-back calls long enough to fill
  `--window` seconds (the tables are cached, so a call is one kernel), and the bytes it moves per second, counting the input
  frames read once and the output written once;
* the host path, the only one there was: per frame a PIL resize (one thread) and an upload of the result, then the pose
  layout; wall time, alternating with the GPU path's wall time (host call to synchronise) inside every repeat;
* for 720 x 1280, where `JpegEncoder` can write the clip (1080 is no multiple of its 16-pixel MCU): `JpegDecoder.decode(files,
  layout="pose", size=(480, 832))` against the plain `decode(files, layout="pose")` of the same files, wall and device time.

    python tools/resize_bench.py [--iters 5] [--window 1.0] [--out profiles/resize_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import pose_weights as pw  # noqa: E402

PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


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


def pil_path(frames_host, size, filter, dev):
    """Per frame: PIL resize on the host, the result to the device; then the pose layout."""
    out = torch.empty(len(frames_host), size[0], size[1], 3, dtype=torch.uint8, device=dev)
    for k, f in enumerate(frames_host):
        out[k].copy_(torch.from_numpy(np.asarray(Image.fromarray(f).resize((size[1], size[0]), PIL_FILTERS[filter]))))
    return out.permute(3, 0, 1, 2).contiguous()


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device time one timing window should fill")
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, size = a.frames, (480, 832)
    rs = sfa.FrameResizer(device=dev)
    dec = sfa.JpegDecoder(device=dev)
    res = {"what": "resize_bench", "frames": n, "out_height": size[0], "out_width": size[1], "out_layout": "pose", "iters": a.iters, "window_s": a.window,
           "cases": {}}
    for h, w in ((720, 1280), (1080, 1920)):
        host = pw.synth_pose_clip(0, n, h, w, "skeleton").permute(1, 2, 3, 0).contiguous()
        x = host.to(dev)
        frames_host = host.numpy()
        moved = n * 3 * (h * w + size[0] * size[1])
        for filter in ("bilinear", "bicubic"):
            run = lambda: rs.resize(x, size, filter, out_layout="pose")                                   # noqa: E731
            got = run()
            assert torch.equal(got, pil_path(frames_host, size, filter, dev)), "the kernel and Pillow disagree"
            calls = max(10, int(a.window * 1e3 / device_ms(run, 10)) + 1)
            gpu = [device_ms(run, calls) for _ in range(a.iters)]
            walls = {"gpu": [], "pil": []}
            for _ in range(a.iters):                                       # the candidates take turns
                walls["gpu"].append(wall_s(run))
                walls["pil"].append(wall_s(lambda: pil_path(frames_host, size, filter, dev)))
            res["cases"][f"{h}x{w}_{filter}"] = {
                "in_height": h, "in_width": w, "filter": filter, "calls_per_window": calls, "bytes_moved": moved,
                "gpu_ms": round(med(gpu), 4), "gpu_ms_all": [round(t, 4) for t in gpu], "gpu_us_per_frame": round(med(gpu) * 1e3 / n, 3),
                "gbytes_per_s": round(moved / (med(gpu) * 1e-3) / 1e9, 1),
                "gpu_path_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "pil_path_wall_ms": round(med(walls["pil"]) * 1e3, 2),
                "pil_path_wall_ms_all": [round(v * 1e3, 2) for v in walls["pil"]],
                "wall_speedup_over_pil_path": round(med(walls["pil"]) / med(walls["gpu"]), 1)}
        if h % 16 == 0 and w % 16 == 0:
            files = sfa.JpegEncoder(90, "420", device=dev).encode(x)
            plain = lambda: dec.decode(files, layout="pose")                                              # noqa: E731
            sized = lambda: dec.decode(files, layout="pose", size=size)                                   # noqa: E731
            assert torch.equal(sized(), rs.resize(dec.decode(files), size, out_layout="pose"))
            plain()
            t = {"plain_wall": [], "sized_wall": [], "plain_gpu": [], "sized_gpu": []}
            for _ in range(a.iters):
                t["plain_wall"].append(wall_s(plain) * 1e3), t["sized_wall"].append(wall_s(sized) * 1e3)
                t["plain_gpu"].append(device_ms(plain, 1)), t["sized_gpu"].append(device_ms(sized, 1))
            res["decode"] = {"in_height": h, "in_width": w, "jpeg_bytes_per_frame": round(sum(len(f) for f in files) / n),
                             **{k + "_ms": round(med(v), 3) for k, v in t.items()}, **{k + "_ms_all": [round(s, 3) for s in v] for k, v in t.items()}}
        del x, host, frames_host
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
