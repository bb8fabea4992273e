"""Time the GPU JPEG encoder on the MI355X against the demo's host path and write profiles/jpeg_bench.json.

Workload: the 81 frames of 480 x 832 a seeded TAEHV decode gives, encoded at (quality, subsampling) = (100, "420") -- the
demo's setting --, (100, "444") and (90, "420").  One process, a warm-up of everything, then the candidates take turns
inside every repeat (device events around each; median and all samples):

* GPU time of the transform kernel, of the entropy + pack kernels, and of the whole `sf_jpeg_encode_frames` call;
* `JpegEncoder.encode`: wall time per clip including the read-back, host CPU seconds, bytes that cross to the host;
* the demo's host path on this box (demo.py:162-187): per frame an fp32 device-to-host copy, the truncation and a PIL save,
  one thread: wall time, host CPU seconds, bytes that cross;
* the restart interval: GPU time and file size over 1 .. 260 MCUs per interval at (100, "420");
* one streaming run of the 1.3B generator with `TAEHVWrapper`, with and without `frame_encoder`: frames/s, host core share.

`--kernel-stats FILE` folds in the per-kernel times of a separate `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/jpeg_bench.py [--iters 5] [--host-iters 2] [--skip-stream] [--out profiles/jpeg_bench.json]
"""
import argparse
import csv
import io
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import taehv_weights as tw  # noqa: E402

CONFIGS = [(100, "420"), (100, "444"), (90, "420")]
PIL_SUB = {"420": 2, "444": 0}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, iters, warmup):
    """{name: fn} -> {name: (median ms, all ms)}, the candidates taking turns inside every repeat."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return {k: (sorted(v)[len(v) // 2], [round(t, 4) for t in v]) for k, v in ts.items()}


def host_clock(fn):
    """(result, wall seconds, host CPU seconds of this process) of one call"""
    torch.cuda.synchronize()
    w0, c0 = time.perf_counter(), time.process_time()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - w0, time.process_time() - c0


def demo_host_path(clip, quality, subsampling):
    """demo.py:162-187 frame by frame: fp32 to the host, clamp * 127.5 + 127.5, uint8, PIL save."""
    sizes = []
    for frame in clip:
        x = frame.cpu()
        u8 = (x.clamp(-1, 1) * 127.5 + 127.5).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, "JPEG", quality=quality, subsampling=PIL_SUB[subsampling])
        sizes.append(buf.tell())
    return sizes


def stream_run(dev, encoder, frames):
    shape = sfa.WAN_1_3B
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=3, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0), timestep_shift=5.0, is_causal=True, device=dev)
    vae = sfa.TAEHVWrapper(tw.synth_taehv_state_dict(0), device=dev)
    pipe = sfa.CausalInferencePipeline(args, dev, generator=gen, text_encoder=sfa.SyntheticTextEncoder(shape.text_len, shape.text_dim, device=dev), vae=vae)
    noise = torch.randn(1, frames, 16, 60, 104, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    out = {}
    runs = {"without_encoder": None, "with_encoder": encoder}
    for _ in range(2):                                    # the first round is the warm-up; the second is kept
        for name, enc in runs.items():
            def go():
                n, nbytes = 0, 0
                for chunk in pipe.stream(noise, ["a prompt"], overlap_decode=True, frame_encoder=enc):
                    n += chunk[2].shape[1]
                    nbytes += sum(len(f) for f in chunk[3]) if enc is not None else 0
                return n, nbytes
            (n, nbytes), wall, cpu = host_clock(go)
            out[name] = {"pixel_frames": n, "wall_s": round(wall, 4), "frames_per_s": round(n / wall, 2), "host_cpu_s": round(cpu, 4),
                         "host_core_share": round(cpu / wall, 3), "jpeg_bytes": nbytes}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=21, help="latent frames of the clip (21 -> 81 pixel frames)")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)                              # the demo's sender is one thread
    lat = torch.randn(1, a.frames, 16, 60, 104, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(dev)
    tae = sfa.TAEHVWrapper(tw.synth_taehv_state_dict(0), device=dev)
    clip = tae.decode_to_pixel(lat)[0].contiguous()       # [81, 3, 480, 832] fp32 in [-1, 1]
    del tae
    n, _, h, w = clip.shape
    res = {"what": "jpeg_bench", "frames": n, "height": h, "width": w, "iters": a.iters, "host_iters": a.host_iters,
           "fp32_bytes_per_frame": 3 * h * w * 4, "configs": []}
    for quality, sub in CONFIGS:
        enc = sfa.JpegEncoder(quality, sub, device=dev)
        coef = enc.coefficients(clip)
        fns = {"transform": lambda: enc.coefficients(clip), "entropy_pack": lambda: enc.entropy(coef, h, w), "encode_frames": lambda: enc._encode(clip)}
        gpu = alternate(fns, a.iters, a.warmup)
        gpu_walls, gpu_cpus, host_walls, host_cpus = [], [], [], []
        for _ in range(a.host_iters):                     # the two paths take turns
            files, wall, cpu = host_clock(lambda: enc.encode(clip))
            gpu_walls.append(wall), gpu_cpus.append(cpu)
            sizes, wall, cpu = host_clock(lambda: demo_host_path(clip, quality, sub))
            host_walls.append(wall), host_cpus.append(cpu)
        med = lambda v: sorted(v)[len(v) // 2]            # noqa: E731
        jpeg_bytes = sum(len(f) for f in files)
        res["configs"].append({
            "quality": quality, "subsampling": sub, "restart_interval": enc.restart_interval,
            "gpu_ms": {k: round(v[0], 4) for k, v in gpu.items()}, "gpu_ms_all": {k: v[1] for k, v in gpu.items()},
            "gpu_ms_per_frame": round(gpu["encode_frames"][0] / n, 4),
            "gpu_path": {"wall_ms_per_clip": round(med(gpu_walls) * 1e3, 2), "wall_ms_per_frame": round(med(gpu_walls) * 1e3 / n, 4),
                         "host_cpu_s_per_clip": round(med(gpu_cpus), 4), "bytes_to_host": jpeg_bytes + 8 * (n + 2),
                         "jpeg_bytes_per_frame": round(jpeg_bytes / n), "wall_s_all": [round(v, 4) for v in gpu_walls]},
            "host_path": {"wall_ms_per_clip": round(med(host_walls) * 1e3, 2), "wall_ms_per_frame": round(med(host_walls) * 1e3 / n, 4),
                          "host_cpu_s_per_clip": round(med(host_cpus), 4), "bytes_to_host": n * 3 * h * w * 4,
                          "jpeg_bytes_per_frame": round(sum(sizes) / n), "wall_s_all": [round(v, 4) for v in host_walls]},
            "wall_speedup_over_host_path": round(med(host_walls) / med(gpu_walls), 2),
            "workspace_bytes": int(enc._ws.numel())})
    # ---- the restart interval at the demo's setting
    sweep = {}
    encs = {ri: sfa.JpegEncoder(100, "420", restart_interval=ri, device=dev) for ri in (1, 5, 10, 26, 52, 260)}
    times = alternate({ri: (lambda e=e: e._encode(clip)) for ri, e in encs.items()}, a.iters, a.warmup)
    for ri, e in encs.items():
        files = e.encode(clip)
        sweep[ri] = {"gpu_ms": round(times[ri][0], 4), "gpu_ms_all": times[ri][1], "jpeg_bytes_per_frame": round(sum(len(f) for f in files) / n),
                     "workspace_bytes": int(e._ws.numel())}
    res["restart_interval_sweep_q100_420"] = sweep
    del encs
    torch.cuda.empty_cache()
    res["stream"] = "not measured" if a.skip_stream else stream_run(dev, sfa.JpegEncoder(90, "420", device=dev), a.frames)
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "jpeg_" in r["Name"]]
        res["kernel_stats"] = {r["Name"][:60]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)} for r in rows}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
