"""Time the raw YUV kernels on the MI355X against a device copy and the host path, and write profiles/yuv_bench.json.

Workload: 81 frames of 480 x 832 (`pose_weights.synth_pose_clip`, encoded by the definition's constants on the device, so the
bytes are what a camera or a decoder would deliver).  One process, a warm-up of everything, then per case:

* decode: nv12 and yuyv to uint8 "pose", i420 to float32 "chw", each with the triangle and the nearest chroma filter;
  encode: the float32 "chw" frames to i420 and to nv12.  Device time from device events around a run of back-to-back calls
  long enough to fill `--window` seconds, and the bytes per second over `frame_bytes + output bytes` (each read or written
  once);
* the ceiling a memory-bound kernel is held against: a device-to-device `copy_` of the same number of bytes (half read, half
  written), timed in the same process in the same way;
* wall time from bytes on the host to frames on the device (decode) or from frames on the device to bytes on the host
  (encode), alternating with the host path inside every repeat: `PIL.Image.frombuffer(..., "YCbCr").convert("RGB")` of
  nearest-upsampled planes plus one upload (decode; Pillow's matrix is BT.601 full range, so its pixels are not this
  decoder's), `Image.convert("YCbCr")` of downloaded uint8 frames (encode);
* 720 x 1280 nv12 to 480 x 832 through `size=` against the plain decode of the same frames.

    python tools/yuv_bench.py [--iters 5] [--window 1.0] [--out profiles/yuv_bench.json]
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
from self_forcing_amd import yuv_reference as yr  # noqa: E402


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


def windows(fn, window, iters):
    fn()
    calls = max(10, int(window * 1e3 / device_ms(fn, 10)) + 1)
    return calls, [device_ms(fn, calls) for _ in range(iters)]


def copy_ms(nbytes, dev, window, iters):
    """A device-to-device copy that moves `nbytes` in all (reads half, writes half)."""
    src = torch.randint(0, 256, (nbytes // 2,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return med(windows(lambda: dst.copy_(src), window, iters)[1])


def pil_decode(frames, fmt, h, w, dev):
    """Per frame: planes, nearest up-sampling in numpy, Pillow's YCbCr -> RGB; then one upload and the pose layout."""
    out = np.empty((len(frames), h, w, 3), np.uint8)
    for k, f in enumerate(frames):
        y, u, v = yr.planes(f, fmt, h, w)
        sx, sy = w // u.shape[1], h // u.shape[0]
        ycc = np.stack([y, np.repeat(np.repeat(u, sy, 0), sx, 1), np.repeat(np.repeat(v, sy, 0), sx, 1)], -1)
        out[k] = np.asarray(Image.frombytes("YCbCr", (w, h), ycc.tobytes()).convert("RGB"))
    return torch.from_numpy(out).to(dev).permute(3, 0, 1, 2).contiguous()


def pil_encode(x):
    """Frames float32 [n, 3, h, w] on the device -> uint8 on the host -> Pillow's YCbCr and a 2 x 2 box average per frame."""
    u8 = (x.clamp(-1, 1) * 127.5 + 127.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    out = []
    for f in u8:
        ycc = np.asarray(Image.fromarray(f).convert("YCbCr")).astype(np.uint16)
        c = (ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:] + 2) >> 2
        out.append(ycc[..., 0].astype(np.uint8).tobytes() + c[..., 0].astype(np.uint8).tobytes() + c[..., 1].astype(np.uint8).tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device time one timing window should fill")
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    n, h, w = a.frames, 480, 832
    dec = sfa.YuvDecoder(dev)
    res = {"what": "yuv_bench", "frames": n, "height": h, "width": w, "iters": a.iters, "window_s": a.window, "decode": {}, "encode": {}}

    clip = pw.synth_pose_clip(0, n, h, w, "skeleton").permute(1, 2, 3, 0).contiguous().to(dev)            # uint8 [n, h, w, 3]
    raws = {"i420": sfa.YuvEncoder("i420", device=dev).encode_to_device(clip), "nv12": sfa.YuvEncoder("nv12", device=dev).encode_to_device(clip)}
    i422 = sfa.YuvEncoder("i422", device=dev).encode_to_device(clip)
    y, u, v = i422[:, :h * w].view(n, h, w), i422[:, h * w:h * w + h * w // 2].view(n, h, w // 2), i422[:, h * w + h * w // 2:].view(n, h, w // 2)
    raws["yuyv"] = torch.stack([y[:, :, 0::2], u, y[:, :, 1::2], v], -1).reshape(n, -1).contiguous()
    assert torch.equal(dec.decode(raws["yuyv"], "yuyv", (h, w)), dec.decode(i422, "i422", (h, w)))

    copies = {}
    for fmt, layout, dtype in (("nv12", "pose", torch.uint8), ("yuyv", "pose", torch.uint8), ("i420", "chw", torch.float32)):
        raw = raws[fmt]
        host_frames = [bytes(f) for f in raw.cpu().numpy()]
        moved = n * (yr.frame_bytes(fmt, h, w) + 3 * h * w * (1 if dtype == torch.uint8 else 4))
        if moved not in copies:
            copies[moved] = copy_ms(moved, dev, a.window, a.iters)
        for chroma in ("triangle", "nearest"):
            run = lambda: dec.decode(raw, fmt, (h, w), layout, dtype, chroma=chroma)                      # noqa: E731
            calls, gpu = windows(run, a.window, a.iters)
            from_host = lambda: dec.decode(host_frames, fmt, (h, w), layout, dtype, chroma=chroma)        # noqa: E731
            walls = {"gpu": [], "pil": []}
            for _ in range(a.iters):                                       # the candidates take turns
                walls["gpu"].append(wall_s(from_host))
                walls["pil"].append(wall_s(lambda: pil_decode(host_frames, fmt, h, w, dev)))
            gbs, copy_gbs = moved / (med(gpu) * 1e-3) / 1e9, moved / (copies[moved] * 1e-3) / 1e9
            res["decode"][f"{fmt}_{layout}_{str(dtype).replace('torch.', '')}_{chroma}"] = {
                "format": fmt, "layout": layout, "dtype": str(dtype).replace("torch.", ""), "chroma": chroma, "calls_per_window": calls, "bytes_moved": moved,
                "gpu_ms": round(med(gpu), 4), "gpu_ms_all": [round(t, 4) for t in gpu], "gpu_us_per_frame": round(med(gpu) * 1e3 / n, 3),
                "gbytes_per_s": round(gbs, 1), "copy_ms": round(copies[moved], 4), "copy_gbytes_per_s": round(copy_gbs, 1),
                "fraction_of_copy": round(gbs / copy_gbs, 3),
                "host_to_device_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "pil_path_wall_ms": round(med(walls["pil"]) * 1e3, 2),
                "wall_speedup_over_pil_path": round(med(walls["pil"]) / med(walls["gpu"]), 1)}

    x = dec.decode(raws["i420"], "i420", (h, w), "chw", torch.float32)
    for fmt in ("i420", "nv12"):
        enc = sfa.YuvEncoder(fmt, device=dev)
        moved = n * (yr.frame_bytes(fmt, h, w) + 3 * h * w * 4)
        if moved not in copies:
            copies[moved] = copy_ms(moved, dev, a.window, a.iters)
        calls, gpu = windows(lambda: enc.encode_to_device(x), a.window, a.iters)
        walls = {"gpu": [], "pil": []}
        for _ in range(a.iters):
            walls["gpu"].append(wall_s(lambda: enc.encode(x)))
            walls["pil"].append(wall_s(lambda: pil_encode(x)))
        gbs, copy_gbs = moved / (med(gpu) * 1e-3) / 1e9, moved / (copies[moved] * 1e-3) / 1e9
        res["encode"][f"float32_{fmt}"] = {
            "format": fmt, "calls_per_window": calls, "bytes_moved": moved, "gpu_ms": round(med(gpu), 4), "gpu_ms_all": [round(t, 4) for t in gpu],
            "gpu_us_per_frame": round(med(gpu) * 1e3 / n, 3), "gbytes_per_s": round(gbs, 1), "copy_ms": round(copies[moved], 4),
            "copy_gbytes_per_s": round(copy_gbs, 1), "fraction_of_copy": round(gbs / copy_gbs, 3),
            "device_to_host_wall_ms": round(med(walls["gpu"]) * 1e3, 3), "pil_path_wall_ms": round(med(walls["pil"]) * 1e3, 2),
            "wall_speedup_over_pil_path": round(med(walls["pil"]) / med(walls["gpu"]), 1)}
    del x, clip, raws

    bh, bw = 720, 1280
    big = sfa.YuvEncoder("nv12", device=dev).encode_to_device(pw.synth_pose_clip(0, n, bh, bw, "skeleton").permute(1, 2, 3, 0).contiguous().to(dev))
    plain = lambda: dec.decode(big, "nv12", (bh, bw), "pose")                                             # noqa: E731
    sized = lambda: dec.decode(big, "nv12", (bh, bw), "pose", size=(h, w))                                # noqa: E731
    assert torch.equal(sized(), sfa.FrameResizer(dev).resize(dec.decode(big, "nv12", (bh, bw)), (h, w), out_layout="pose"))
    t = {"plain_gpu": windows(plain, a.window, a.iters)[1], "sized_gpu": windows(sized, a.window, a.iters)[1]}
    res["resized"] = {"in_height": bh, "in_width": bw, "format": "nv12", **{k + "_ms": round(med(v), 4) for k, v in t.items()},
                      **{k + "_ms_all": [round(s, 4) for s in v] for k, v in t.items()}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
