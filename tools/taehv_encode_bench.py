"""Time the TAEHV tiny encoder on the MI355X against the Wan VAE encoder and write one JSON line.

Both encoders take turns in one process after a warm-up of every shape, device events around each repeat, median and
all samples:

* the single image [1, 3, 1, H, W] and the 81-frame clip [1, 3, 81, H, W] through `TAEHVWrapper.encode_to_latent` and
  through `WanVAEWrapper.encode_to_latent`: ms, TFLOP/s against `taehv_encode_flops` (the reference's work; the image is
  one group of four copies), state and scratch bytes, and whether the TAEHV clip encode is the faster one;
* the stem alone on one call's frames: its bytes (pixels read once + the 64-channel volume written) over its time.

`--kernel-stats FILE` folds in the per-kernel shares of a separate `rocprofv3 --kernel-trace --stats` run of
`--only-taehv --iters 3`.

    python tools/taehv_encode_bench.py [--iters 7] [--warmup 2] [--out profiles/taehv_encode_bench.json] [--kernel-stats stats.csv]
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
from self_forcing_amd import ops, taehv_weights as tw, vae_weights as vw  # noqa: E402

PEAK_BYTES = 6.3e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=81, help="pixel frames of the clip (1 + 4k)")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--frames-per-call", type=int, default=3)
    ap.add_argument("--only-taehv", action="store_true", help="skip the Wan VAE encoder (the kernel-trace run)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taehv_encode_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(0)
    H, W, T = a.height, a.width, a.frames
    res = {"what": "taehv_encode_bench", "height": H, "width": W, "clip_frames": T, "iters": a.iters, "warmup": a.warmup}
    clip = (torch.rand(1, 3, T, H, W, generator=g) * 2 - 1).to(dev)
    image = clip[:, :, :1].contiguous()
    tae = sfa.TAEHVWrapper({**tw.synth_taehv_state_dict(0), **tw.synth_taehv_encoder_state_dict(0)}, device=dev, frames_per_call=a.frames_per_call)
    wan = None if a.only_taehv else sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.WAN_VAE, seed=0, encoder=True), device=dev)
    for name, x in (("image", image), ("clip", clip)):
        fns = {"taehv": lambda x=x: tae.encode_to_latent(x)}
        if wan is not None:
            fns["wan_vae"] = lambda x=x: wan.encode_to_latent(x)
        latent_frames = 1 + (x.shape[2] - 1) // 4
        flops = tw.taehv_encode_flops(H, W, latent_frames)
        r = alternate(fns, a.iters, a.warmup)
        res[name] = {k: {"ms": round(ms, 3), "ms_all": all_ms} for k, (ms, all_ms) in r.items()}
        res[name]["latent_frames"] = latent_frames
        res[name]["taehv"].update(tflop=round(flops / 1e12, 3), tflops_per_s=round(flops / 1e12 / (r["taehv"][0] / 1e3), 1))
        if wan is not None:
            res[name]["taehv_speedup_over_wan_vae"] = round(r["wan_vae"][0] / r["taehv"][0], 2)
    enc = tae.encoder
    res["taehv"] = {"state_bytes": enc.state_bytes(H, W), "scratch_bytes": enc.scratch_bytes(H, W), "frames_per_call": enc.frames_per_call,
                    "param_bytes": enc.param_bytes()}
    if wan is not None:
        res["wan_vae"] = {"state_bytes": sum(int(v.numel()) for v in wan.encoder._state.values()) if hasattr(wan.encoder, "_state") else None,
                          "scratch_bytes": sum(int(v.numel()) for v in wan.encoder._scratch.values())}
        faster = res["clip"]["taehv"]["ms"] < res["clip"]["wan_vae"]["ms"]
        res["taehv_clip_faster_than_wan_vae"] = faster
        print(f"TAEHV clip encode {res['clip']['taehv']['ms']} ms vs Wan VAE {res['clip']['wan_vae']['ms']} ms: "
              + ("faster, as the FLOP counts let expect" if faster else "NOT faster -- a finding to explain"), file=sys.stderr)
    # ---- the stem alone, on one call's frames
    n = 4 * a.frames_per_call
    px = clip[0, :, :n].contiguous()
    w = tw.repack_stem(torch.randn(64, 3, 3, 3, generator=g) * 27 ** -0.5).to(torch.bfloat16).to(dev)
    b = (torch.randn(64, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    ms, all_ms = alternate({"stem": lambda: ops.taehv_encode_stem(px, w, b)}, a.iters, a.warmup)["stem"]
    by = px.numel() * 4 + n * H * W * 64 * 2
    res["stem"] = {"frames": n, "ms": round(ms, 4), "ms_all": all_ms, "mbytes": round(by / 1e6, 1), "tbytes_per_s": round(by / 1e12 / (ms / 1e3), 2),
                   "share_of_peak_bytes": round(by / PEAK_BYTES / (ms / 1e3), 3),
                   "write_and_reread_mbytes_per_frame": round(2 * H * W * 64 * 2 / 1e6, 1)}
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = list(csv.DictReader(f))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        res["kernel_shares"] = {r["Name"][:80]: round(float(r["TotalDurationNs"]) / tot, 4) for r in rows if float(r["TotalDurationNs"]) / tot >= 0.005}
    else:
        res["kernel_shares"] = "not measured"
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
