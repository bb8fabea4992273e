"""Time the VAE encoder on the MI355X and print one JSON line: one 480 x 832 image (the image-to-video call) and one
81-frame clip, ms and TFLOP/s (vae_weights.vae_encode_flops), state / scratch bytes.  Weights are the seeded stand-in
(same shapes as Wan2.1_VAE.pth).  `--kernel-stats FILE`: fold in the per-kernel shares of a separate
`rocprofv3 --kernel-trace --stats` run (its *_kernel_stats.csv).

    python tools/vae_encode_bench.py [--iters 5] [--warmup 2] [--kernel-stats out/kernel_stats.csv]
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import vae_weights as vw  # noqa: E402


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    vae = sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.WAN_VAE, seed=0, encoder=True), device=dev)
    g = torch.Generator().manual_seed(0)
    H, W = a.height, a.width
    res = {"what": "vae_encode", "height": H, "width": W}
    for name, T in (("image", 1), ("clip", a.frames)):
        x = (torch.rand(1, 3, T, H, W, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        ms, all_ms = time_ms(lambda: vae.encode_to_latent(x), a.iters, a.warmup)
        fl = vw.vae_encode_flops(vw.WAN_VAE, H, W, T)
        res[name] = {"frames": T, "latent_frames": vw.encode_chunks(T), "ms": round(ms, 3), "ms_all": [round(t, 3) for t in all_ms],
                     "tflop": round(fl / 1e12, 3), "tflops_per_s": round(fl / 1e12 / (ms / 1e3), 1)}
    enc = vae.encoder
    res["state_bytes"] = {f"{k[0]}x{k[1]}_window{k[2]}": int(v.numel()) for k, v in enc._state.items()}
    res["scratch_bytes"] = {f"{k[0]}x{k[1]}_window{k[2]}": int(v.numel()) for k, v in enc._scratch.items()}
    res["frames_per_call"] = enc.frames_per_call
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = list(csv.DictReader(f))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        res["kernel_shares"] = {r["Name"][:80]: round(float(r["TotalDurationNs"]) / tot, 4) for r in rows
                                if float(r["TotalDurationNs"]) / tot >= 0.005}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
