"""Time the TAEHV tiny decoder on the MI355X against the Wan VAE decode and print one JSON line.

Everything is alternated in one process after a warm-up of every shape, device events around each repeat, median and
all samples:

* the 21 x 60 x 104 clip through `WanVAEWrapper.decode_to_pixel` and through `TAEHVWrapper.decode_to_pixel`: ms,
  TFLOP/s (by `vae_decode_flops` / `taehv_decode_flops`), state and scratch bytes;
* per production convolution shape: `sf_taehv_conv` against the only way the Wan VAE kernels can compute it --
  `ops.conv_igemm` (kt = 3 with a zero tap for the MemBlock's first convolution, kt = 1 otherwise; the folded exit
  convolutions with its interleave where tgrow = 2) plus torch's bias-free / ReLU / residual elementwise passes -- with the
  least time the hardware could take (FLOPs over 2.5 PFLOP/s, bytes over 6.3 TB/s, whichever is larger).

`--kernel-stats FILE` folds in the per-kernel shares of a separate `rocprofv3 --kernel-trace --stats` run.

    python tools/taehv_bench.py [--iters 10] [--warmup 2] [--kernel-stats out/kernel_stats.csv]
"""
import argparse
import csv
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import ops, taehv_weights as tw, vae_weights as vw  # noqa: E402
from self_forcing_amd.vae import repack_conv  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 2.5e15, 6.3e12


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


def conv_case(c, dev, g):
    kt, cin, cout, H, W, up, tg, epi, T = c["kt"], c["cin"], c["cout"], c["H"], c["W"], c["up"], c["tgrow"], c["epi"], c["T"]
    hin, win = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(T + kt - 1, hin, win, cin, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(cout, cin, kt, 3, 3, generator=g) * (cin * kt * 9) ** -0.5).to(torch.bfloat16)
    b = (torch.randn(cout, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    has_bias = epi in ("bias_relu", "bias_resid_relu", "head_f32")
    resid = torch.randn(T, H, W, cout, generator=g).to(torch.bfloat16).to(dev) if epi == "bias_resid_relu" else None
    wn = tw.repack_taehv_conv(w).to(dev)
    new = lambda: ops.taehv_conv(x, wn, b if has_bias else None, kt, T, epilogue=epi, upsample=bool(up), resid=resid, tgrow=tg, clamp=True)  # noqa: E731
    # the parent's composition: conv_igemm always adds a bias (zero where the layer has none) and has no ReLU
    zb = b if has_bias else torch.zeros_like(b)
    if kt == 2:
        w = torch.cat([torch.zeros(cout, cin, 1, 3, 3, dtype=torch.bfloat16), w], 2)
        xo = torch.cat([x[:1], x])
    else:
        xo = x
    wo = repack_conv(w).to(dev)
    kern = (3 if kt == 2 else 1, 3, 3)

    def old():
        if epi == "head_f32":       # conv_igemm's float head clamps y itself: take the bf16 result and finish in torch
            y = ops.conv_igemm(xo, wo, zb, kern, T, upsample=bool(up), clamp_f32=True)
            return (2 * y - 1).clamp_(-1, 1)
        y = ops.conv_igemm(xo, wo, zb, kern, T, upsample=bool(up), resid=resid, interleave=tg == 2)
        return y if epi == "plain" else F.relu_(y)

    flops = 2.0 * kt * 9 * cin * cout * T * H * W
    out_bytes = T * H * W * cout * (4 if epi == "head_f32" else 2)
    bytes_ = x.numel() * 2 + wn.numel() * 2 + out_bytes + (resid.numel() * 2 if resid is not None else 0)
    return new, old, flops, bytes_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=21, help="latent frames of the clip")
    ap.add_argument("--lat_h", type=int, default=60)
    ap.add_argument("--lat_w", type=int, default=104)
    ap.add_argument("--skip-wan", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(0)
    h, w, Fr = a.lat_h, a.lat_w, a.frames
    res = {"what": "taehv_bench", "lat_h": h, "lat_w": w, "latent_frames": Fr, "pixel_frames": 1 + 4 * (Fr - 1), "iters": a.iters}
    lat = torch.randn(1, Fr, 16, h, w, generator=g).to(torch.bfloat16).to(dev)
    tae = sfa.TAEHVWrapper(tw.synth_taehv_state_dict(0), device=dev)
    fns = {"taehv": lambda: tae.decode_to_pixel(lat)}
    flops = {"taehv": tw.taehv_decode_flops(h, w, Fr)}
    if not a.skip_wan:
        wan = sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.WAN_VAE, seed=0), device=dev)
        fns["wan_vae"] = lambda: wan.decode_to_pixel(lat)
        flops["wan_vae"] = vw.vae_decode_flops(vw.WAN_VAE, h, w, Fr)
    for k, (ms, all_ms) in alternate(fns, a.iters, a.warmup).items():
        res[k] = {"ms": round(ms, 3), "ms_all": all_ms, "tflop": round(flops[k] / 1e12, 3), "tflops_per_s": round(flops[k] / 1e12 / (ms / 1e3), 1),
                  "pixel_frames_per_s": round((1 + 4 * (Fr - 1)) / (ms / 1e3), 1)}
    res["taehv"].update(state_bytes=tae.decoder.state_bytes(h, w), scratch_bytes=tae.decoder.scratch_bytes(h, w),
                        frames_per_call=tae.decoder.frames_per_call, param_bytes=tae.decoder.param_bytes())
    if not a.skip_wan:
        res["wan_vae"].update(state_bytes=sum(int(v.numel()) for v in wan.model._state.values()),
                              scratch_bytes=sum(int(v.numel()) for v in wan.model._scratch.values()), frames_per_call=wan.model.frames_per_call)
        res["taehv_speedup_over_wan_vae"] = round(res["wan_vae"]["ms"] / res["taehv"]["ms"], 2)
        del wan
    del tae
    torch.cuda.empty_cache()
    # ---- per production convolution shape (frames_per_call = 3 latent frames, as the wrapper issues them)
    seen, convs = set(), []
    for c in tw.decoder_convs(h, w, 3):
        key = (c["kt"], c["cin"], c["cout"], c["H"], c["W"], c["up"], c["tgrow"], c["epi"])
        if key not in seen:
            seen.add(key)
            convs.append(c)
    res["convs"] = []
    for c in convs:
        new, old, fl, by = conv_case(c, dev, g)
        r = alternate({"new": new, "parent": old}, a.iters, a.warmup)
        bound_ms = max(fl / PEAK_FLOPS, by / PEAK_BYTES) * 1e3
        spread = (max(r["new"][1]) - min(r["new"][1]))
        res["convs"].append({"name": c["name"], "kt": c["kt"], "cin": c["cin"], "cout": c["cout"], "T": c["T"], "H": c["H"], "W": c["W"], "up": c["up"],
                             "tgrow": c["tgrow"], "epi": c["epi"], "new_ms": round(r["new"][0], 4), "parent_ms": round(r["parent"][0], 4),
                             "new_ms_all": r["new"][1], "parent_ms_all": r["parent"][1], "new_spread_ms": round(spread, 4),
                             "gflop": round(fl / 1e9, 2), "mbytes": round(by / 1e6, 2), "bound": "flops" if fl / PEAK_FLOPS >= by / PEAK_BYTES else "bytes",
                             "bound_ms": round(bound_ms, 4), "share_of_bound": round(bound_ms / r["new"][0], 3),
                             "tflops_per_s": round(fl / 1e12 / (r["new"][0] / 1e3), 1)})
        torch.cuda.empty_cache()
    res["stream_s1"] = "not measured"
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = list(csv.DictReader(f))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        res["kernel_shares"] = {r["Name"][:80]: round(float(r["TotalDurationNs"]) / tot, 4) for r in rows if float(r["TotalDurationNs"]) / tot >= 0.005}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
