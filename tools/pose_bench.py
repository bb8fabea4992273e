"""Time the pose front end on the MI355X and print one JSON line.

81 pose frames of 480 x 832 (the S1 clip), device events, a warm-up, the median of `--iters` repeats, the candidates
alternated inside every repeat of one process:

* `new`: `PoseEmbedder.embed` (sf_pose_embed: prepare, six sf_pose_conv, gather + sf_gemm_bf16), uint8 frames on the
  device -> tokens;
* `torch_bf16` / `torch_fp32`: what a user had to write before -- the same seven layers as `torch.nn.Conv3d` modules of
  PyTorch-ROCm on the same GPU in channels-last-3d bf16, and in float32 as the reference runs them -- input transform,
  stack and the 'b c f h w -> b (f h w) c' copy included.  `--skip-torch` leaves them out ("not measured").

Then every launch of the new path alone, with FLOPs and bytes from `pose_weights.pose_embed_layers`, the bound (the
larger of FLOPs / 2.5 PFLOP/s and bytes / 6.3 TB/s, DESIGN.md section 12's constants) and new / bound.

It fails rather than falling back when it finds no GPU.

    python tools/pose_bench.py [--iters 10] [--warmup 2] [--skip-torch]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import ops, pose_weights as pw  # noqa: E402

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


def torch_stack(sd, dtype, dev):
    layers = []
    for idx, cin, cout, k, stride, pad, act in pw.DWPOSE_LAYERS:
        conv = torch.nn.Conv3d(cin, cout, k, stride=stride, padding=pad)
        conv.weight.data.copy_(sd[f"{pw.DWPOSE_PREFIX}{idx}.weight"])
        conv.bias.data.copy_(sd[f"{pw.DWPOSE_PREFIX}{idx}.bias"])
        layers += [conv] + ([torch.nn.SiLU()] if act else [])
    m = torch.nn.Sequential(*layers).to(device=dev, dtype=dtype).eval().requires_grad_(False)
    return m.to(memory_format=torch.channels_last_3d) if dtype == torch.bfloat16 else m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_bench: no GPU found (this tool measures the HIP path; there is nothing to fall back to)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    Fr, H, W = a.frames, a.height, a.width
    sd = pw.synth_pose_state_dict(0)
    clip = pw.synth_pose_clip(1, Fr, H, W, "skeleton").to(dev)
    emb = sfa.PoseEmbedder(sd, device=dev)
    layers = pw.pose_embed_layers(Fr, H, W)
    flops, bytes_ = sum(l["flops"] for l in layers), sum(l["bytes"] for l in layers)
    res = {"what": "pose_bench", "frames": Fr, "height": H, "width": W, "tokens": list(pw.pose_plan(Fr, H, W)), "iters": a.iters,
           "tflop": round(flops / 1e12, 3), "gbytes": round(bytes_ / 1e9, 3), "scratch_bytes": emb.scratch_bytes(Fr, H, W)}
    fns = {"new": lambda: emb.embed(clip)}
    if not a.skip_torch:
        def user(m, dtype):
            def run():
                x = pw.pose_input_torch(clip).to(dtype)
                if dtype == torch.bfloat16:
                    x = x.contiguous(memory_format=torch.channels_last_3d)
                y = m(x).to(torch.bfloat16)
                return y.permute(0, 2, 3, 4, 1).flatten(1, 3).contiguous()
            return run
        fns["torch_bf16"] = user(torch_stack(sd, torch.bfloat16, dev), torch.bfloat16)
        fns["torch_fp32"] = user(torch_stack(sd, torch.float32, dev), torch.float32)
    r = alternate(fns, a.iters, a.warmup)
    bound_ms = max(flops / PEAK_FLOPS, bytes_ / PEAK_BYTES) * 1e3
    for k, (ms, all_ms) in r.items():
        res[k] = {"ms": round(ms, 3), "ms_all": all_ms, "spread_ms": round(max(all_ms) - min(all_ms), 3)}
    res["new"].update(bound_ms=round(bound_ms, 3), new_over_bound=round(r["new"][0] / bound_ms, 2))
    if a.skip_torch:
        res["torch_bf16"] = res["torch_fp32"] = "not measured"
    else:
        res["speedup_over_torch_bf16"] = round(r["torch_bf16"][0] / r["new"][0], 2)
        res["speedup_over_torch_fp32"] = round(r["torch_fp32"][0] / r["new"][0], 2)
        fns.pop("torch_bf16"), fns.pop("torch_fp32")
        torch.cuda.empty_cache()

    # ---- every launch of the new path alone, on inputs of its own shape
    g = torch.Generator().manual_seed(0)
    vols = pw.pose_layer_volumes(Fr, H, W)
    res["layers"] = []
    prep = lambda: ops.pose_prepare(clip, lead=3)  # noqa: E731
    cases = [(layers[0], prep)]
    for i, (idx, cin, cout, k, stride, pad, act) in enumerate(pw.DWPOSE_LAYERS):
        T, h, w = vols[i]
        cs = 8 if cin == 3 else 16
        x = torch.zeros(T, h, w, cs, dtype=torch.bfloat16, device=dev)
        x[..., :cin] = torch.rand(T, h, w, cin, generator=g).to(torch.bfloat16).to(dev)
        wt, b = sd[f"{pw.DWPOSE_PREFIX}{idx}.weight"], sd[f"{pw.DWPOSE_PREFIX}{idx}.bias"]
        if idx == 12:
            wp, bp = pw.repack_pose_embed(wt).to(torch.bfloat16).to(dev), b.to(torch.bfloat16).to(dev)
            cases.append((layers[i + 1], lambda x=x, wp=wp, bp=bp: ops.pose_patch_embed(x, wp, bp)))
        else:
            wp, bp = pw.repack_pose_conv(wt, cs).to(torch.bfloat16).to(dev), pw.pad_pose_bias(b).to(dev)
            cases.append((layers[i + 1], lambda x=x, wp=wp, bp=bp, cout=cout, stride=stride, act=act:
                          ops.pose_conv(x, wp, bp, cout, kt=3, stride_t=stride[0], stride_s=stride[1], silu=act)))
    for l, fn in cases:
        ms, all_ms = alternate({"new": fn}, a.iters, a.warmup)["new"]
        b_ms = max(l["flops"] / PEAK_FLOPS, l["bytes"] / PEAK_BYTES) * 1e3
        res["layers"].append({"name": l["name"], "gflop": round(l["flops"] / 1e9, 2), "mbytes": round(l["bytes"] / 1e6, 1),
                              "bound": "flops" if l["flops"] / PEAK_FLOPS >= l["bytes"] / PEAK_BYTES else "bytes", "bound_ms": round(b_ms, 4),
                              "new_ms": round(ms, 4), "new_ms_all": all_ms, "new_over_bound": round(ms / b_ms, 2)})
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
