"""Time the GPU JPEG decoder on the MI355X against a host decode and write profiles/jpeg_decode_bench.json.

Workload: 81 frames of 480 x 832 written by `JpegEncoder` at quality 90, "420", the default restart interval (156 intervals
per frame), for two contents: a skeleton pose clip (`pose_weights.synth_pose_clip`, what the decoder is for) and the frames
a seeded TAEHV decode gives (dense pictures, five times the bytes).  One process, a warm-up of everything, then the
candidates take turns inside every repeat (medians and all samples):

* `JpegDecoder.decode(files, layout="pose")`: wall time per clip from the files' bytes on the host to the uint8 clip on the
  device, upload and header parsing included, and the host CPU seconds of it;
* the two halves of it on the device alone (device events): restart search + entropy decoding, IDCT + colour;
* the host path: per frame a PIL decode, one thread, and an upload of the raw pixels;
* one frame as a single restart interval (what a file without DRI is): one lane decodes it;
* the skeleton clip written with 1 .. 52 MCUs per restart interval: device time of the whole call, and the file size.

`--kernel-stats FILE` folds in the per-kernel times of a separate `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/jpeg_decode_bench.py [--iters 5] [--out profiles/jpeg_decode_bench.json]
"""
import argparse
import csv
import io
import json
import os
import re
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import ops  # noqa: E402
from self_forcing_amd import pose_weights as pw  # noqa: E402
from self_forcing_amd import taehv_weights as tw  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_clock(fn):
    """(result, wall seconds, host CPU seconds of this process) of one call"""
    torch.cuda.synchronize()
    w0, c0 = time.perf_counter(), time.process_time()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - w0, time.process_time() - c0


def pil_path(files, dev):
    """Per frame: PIL decode on the host, the raw pixels to the device; then the pose layout."""
    h, w = Image.open(io.BytesIO(files[0])).size[::-1]
    out = torch.empty(len(files), h, w, 3, dtype=torch.uint8, device=dev)
    for k, f in enumerate(files):
        im = Image.open(io.BytesIO(f))
        im.load()
        out[k].copy_(torch.from_numpy(np.asarray(im)))
    return out.permute(3, 0, 1, 2).contiguous()


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, h, w = a.frames, 480, 832
    lat = torch.randn(1, (n + 3) // 4, 16, h // 8, w // 8, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(dev)
    tae = sfa.TAEHVWrapper(tw.synth_taehv_state_dict(0), device=dev)
    clips = {"skeleton": pw.synth_pose_clip(0, n, h, w, "skeleton").permute(1, 2, 3, 0).contiguous().to(dev),
             "taehv": tae.decode_to_pixel(lat)[0][:n].contiguous()}
    del tae
    enc = sfa.JpegEncoder(90, "420", device=dev)
    dec = sfa.JpegDecoder(device=dev)
    res = {"what": "jpeg_decode_bench", "frames": n, "height": h, "width": w, "iters": a.iters, "quality": 90, "subsampling": "420",
           "restart_interval": enc.restart_interval, "raw_bytes_per_frame": 3 * h * w, "contents": {}}
    for name, clip in clips.items():
        files = enc.encode(clip)
        whole = dec.decode(files, layout="pose")
        # the two halves on the device, from the upload the last decode left behind
        _, infos = dec._parse(files)
        up, nbytes, info, max_iv = dec._upload(files, infos)
        ws = dec._workspace(n, info, max_iv)
        coef = torch.empty(n, info.blocks, 64, dtype=torch.int16, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.empty(3, n, h, w, dtype=torch.uint8, device=dev)
        stages = {"marks_entropy": lambda: ops.jpeg_decode_entropy(up, nbytes, n, h, w, info.sampling, max_iv, ws, coef, status),
                  "idct_colour": lambda: ops.jpeg_decode_pixels(coef, up, nbytes, n, h, w, info.sampling, ws, out, "pose"),
                  "decode_frames": lambda: ops.jpeg_decode_frames(up, nbytes, n, h, w, info.sampling, max_iv, ws, out, "pose", status)}
        for _ in range(a.warmup):
            for fn in stages.values():
                fn()
            dec.decode(files, layout="pose"), pil_path(files, dev)
        torch.cuda.synchronize()
        gpu = {k: [] for k in stages}
        walls = {"gpu": [], "pil": []}
        cpus = {"gpu": [], "pil": []}
        for _ in range(a.iters):                                       # the candidates take turns
            for k, fn in stages.items():
                gpu[k].append(timed(fn))
            _, wall, cpu = host_clock(lambda: dec.decode(files, layout="pose"))
            walls["gpu"].append(wall), cpus["gpu"].append(cpu)
            _, wall, cpu = host_clock(lambda: pil_path(files, dev))
            walls["pil"].append(wall), cpus["pil"].append(cpu)
        assert torch.equal(out, whole)
        res["contents"][name] = {
            "jpeg_bytes_per_frame": round(sum(len(f) for f in files) / n), "upload_bytes": int(nbytes),
            "gpu_ms": {k: round(med(v), 4) for k, v in gpu.items()}, "gpu_ms_all": {k: [round(t, 4) for t in v] for k, v in gpu.items()},
            "gpu_ms_per_frame": round(med(gpu["decode_frames"]) / n, 4),
            "gpu_path": {"wall_ms_per_clip": round(med(walls["gpu"]) * 1e3, 2), "wall_ms_per_frame": round(med(walls["gpu"]) * 1e3 / n, 4),
                         "host_cpu_s_per_clip": round(med(cpus["gpu"]), 4), "wall_s_all": [round(v, 4) for v in walls["gpu"]]},
            "pil_path": {"wall_ms_per_clip": round(med(walls["pil"]) * 1e3, 2), "wall_ms_per_frame": round(med(walls["pil"]) * 1e3 / n, 4),
                         "host_cpu_s_per_clip": round(med(cpus["pil"]), 4), "wall_s_all": [round(v, 4) for v in walls["pil"]]},
            "wall_speedup_over_pil_path": round(med(walls["pil"]) / med(walls["gpu"]), 2), "workspace_bytes": int(ws.numel())}
        # one frame as a single interval: one lane decodes all of it
        single = sfa.JpegEncoder(90, "420", restart_interval=60000, device=dev).encode(clip[:1])
        dec.decode(single)
        ts = [timed(lambda: dec.decode(single)) for _ in range(a.iters)]
        both = [timed(lambda: dec.decode(files[:1])) for _ in range(a.iters)]
        res["contents"][name]["one_frame_ms"] = {"single_interval": round(med(ts), 4), "default_interval": round(med(both), 4),
                                                 "single_interval_all": [round(t, 4) for t in ts]}
    # the restart interval is the decoder's grain: one lane walks one interval.  The skeleton clip written with other intervals
    sweep = {}
    clip = clips["skeleton"]
    for ri in (1, 2, 5, 10, 26, 52):
        files = sfa.JpegEncoder(90, "420", restart_interval=ri, device=dev).encode(clip)
        _, infos = dec._parse(files)
        up, nbytes, info, max_iv = dec._upload(files, infos)
        ws = dec._workspace(n, info, max_iv)
        out = torch.empty(3, n, h, w, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        run = lambda: ops.jpeg_decode_frames(up, nbytes, n, h, w, info.sampling, max_iv, ws, out, "pose", status)      # noqa: E731
        run()
        ts = [timed(run) for _ in range(a.iters)]
        assert int(status.abs().sum()) == 0
        sweep[ri] = {"decode_frames_ms": round(med(ts), 4), "all": [round(t, 4) for t in ts], "jpeg_bytes_per_frame": round(sum(len(f) for f in files) / n),
                     "intervals_per_frame": max_iv}
    res["restart_interval_sweep_skeleton"] = sweep
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "jpeg_decode" in r["Name"]]
        # (the calls mix the 81-frame clips, the one-frame calls and the single-interval frame: min and max say which is which)
        res["kernel_stats"] = {re.search(r"jpeg_decode_\w+", r["Name"]).group(0): {
            "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3), "min_ms": round(float(r["MinNs"]) / 1e6, 4),
            "max_ms": round(float(r["MaxNs"]) / 1e6, 4)} for r in rows}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
