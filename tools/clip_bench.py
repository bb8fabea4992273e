"""Time the CLIP image encoder on the MI355X and write one JSON line (profiles/clip_bench.json).

For n = 1 and n = 8 frames of 480 x 832, full ViT-H/14 (31 of 32 blocks run) with synthetic weights, in one process after a
warm-up, device events around each repeat, median and all samples:

* ms per `CLIPModel.visual` call (`sf_clip_encode`: one C call);
* the per-kernel split: each kernel of the pass timed alone on the pass's shapes (same events), times its launches per
  pass; the matrix products also under the automatic tiling, which the sequencer does not use (a frame must come out the
  same alone and in a batch, so it pins the 128 x 128 tiles);
* the same model as plain torch on the GPU in the same process: `clip_reference`-style modules under bf16 autocast with
  SDPA, taking turns with the HIP path;
* the weight-read bound: uploaded parameter bytes over the `sf_probe_copy` rate measured here.  At n = 1 the pass is
  weight-bandwidth-bound (1.2 GB of bf16 weights; 257 rows fill two of three 128-row tiles).

Nothing gates on these numbers.

    python tools/clip_bench.py [--iters 7] [--warmup 2] [--layers 32] [--out profiles/clip_bench.json]
"""
import argparse
import dataclasses
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import clip_weights as cw, ops  # noqa: E402


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


class TorchTower(torch.nn.Module):
    """The vision tower as plain torch modules (fp32 parameters, run under bf16 autocast): the comparison, not the product."""

    def __init__(self, s, sd):
        super().__init__()
        self.s = s
        self.sd = {k[len(cw.PREFIX):]: v for k, v in sd.items() if not cw.never_run(k, s)}

    def to_device(self, dev):
        self.sd = {k: v.float().to(dev) for k, v in self.sd.items()}
        self.mean = torch.tensor(cw.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
        self.std = torch.tensor(cw.CLIP_STD, device=dev).view(1, 3, 1, 1)
        return self

    def forward(self, frames):
        s, sd = self.s, self.sd
        x = F.interpolate(frames, size=(s.image_size, s.image_size), mode="bicubic", align_corners=False)
        x = (x * 0.5 + 0.5 - self.mean) / self.std
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x = F.conv2d(x, sd["patch_embedding.weight"], stride=s.patch_size).flatten(2).transpose(1, 2)
            n = x.shape[0]
            x = torch.cat([sd["cls_embedding"].expand(n, -1, -1), x.float()], 1) + sd["pos_embedding"]
            x = F.layer_norm(x, (s.dim,), sd["pre_norm.weight"], sd["pre_norm.bias"], s.eps)
            for i in range(s.layers_built):
                p = f"transformer.{i}."
                h = F.layer_norm(x, (s.dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], s.eps)
                q, k, v = F.linear(h, sd[p + "attn.to_qkv.weight"], sd[p + "attn.to_qkv.bias"]).view(n, s.seq_len, 3, s.num_heads, s.head_dim).unbind(2)
                a = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).reshape(n, s.seq_len, s.dim)
                x = x + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
                h = F.layer_norm(x, (s.dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], s.eps)
                h = F.gelu(F.linear(h, sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"]))
                x = x + F.linear(h, sd[p + "mlp.2.weight"], sd[p + "mlp.2.bias"])
        return x.float()


def kernel_split(s, n, dev, iters, warmup):
    """Each kernel of one pass alone on the pass's shapes: {name: {ms, launches, ms_per_pass}}."""
    g = torch.Generator().manual_seed(1)
    M, D, Fd, L, P, nl = n * s.seq_len, s.dim, s.mlp_dim, s.seq_len, s.num_patches, s.layers_built
    bf = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).bfloat16().to(dev)  # noqa: E731
    f32 = lambda *shape: torch.randn(*shape, generator=g).to(dev)  # noqa: E731
    frames = (torch.rand(n, 3, 480, 832, generator=g) * 2 - 1).to(dev)
    rows, xn, qkv, h = bf(n * P, s.patch_kp), bf(M, D), bf(n, L, 3, s.num_heads, 80), bf(M, Fd)
    wp, wq, wo, w1, w2 = bf(D, s.patch_kp), bf(3 * D, D), bf(D, D), bf(Fd, D), bf(D, Fd)
    bq, bo, b1 = bf(3 * D), bf(D), bf(Fd)
    x32, lw, lb, cls, pos = f32(M, D), f32(D), f32(D), f32(D), f32(L, D)
    patch = bf(n, P, D)
    fns = {
        "preprocess": (1, lambda: ops.clip_preprocess(frames)),
        "embed_norm": (1, lambda: ops.clip_embed_norm(patch, cls, pos, lw, lb, lw, lb)),
        "attention": (nl, lambda: ops.clip_attention(qkv)),
        "add_layernorm": (2 * nl, lambda: ops.clip_add_layernorm(x32, xn, lw, lb, xn=xn)),
        "gelu": (nl, lambda: ops.clip_gelu(h)),
    }
    for name, a, w, b, count in (("gemm_patch", rows, wp, None, 1), ("gemm_qkv", xn, wq, bq, nl), ("gemm_proj", xn, wo, bo, nl),
                                 ("gemm_fc1", xn, w1, b1, nl), ("gemm_fc2", h, w2, bo, nl)):
        fns[name] = (count, lambda a=a, w=w, b=b: ops.gemm(a, w, b, structure="t128"))
        fns[name + "_auto_tiling"] = (0, lambda a=a, w=w, b=b: ops.gemm(a, w, b))
    r = alternate({k: fn for k, (_, fn) in fns.items()}, iters, warmup)
    out = {k: {"ms": round(r[k][0], 4), "launches": c, "ms_per_pass": round(r[k][0] * c, 3)} for k, (c, _) in fns.items()}
    out["sum_ms_per_pass"] = round(sum(v["ms_per_pass"] for v in out.values()), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=32, help="transformer blocks of the tower (all but the last run)")
    ap.add_argument("--no-torch", action="store_true", help="skip the plain-torch comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    s = dataclasses.replace(cw.CLIP_VIT_H_14, num_layers=a.layers)
    sd = cw.synth_clip_state_dict(s, 0, dtype=torch.bfloat16)
    model = sfa.CLIPModel(state_dict=sd, shape=s, device=dev)
    tower = None if a.no_torch else TorchTower(s, sd).to_device(dev)
    del sd
    res = {"what": "clip_bench", "height": 480, "width": 832, "layers_run": s.layers_built, "dim": s.dim, "iters": a.iters, "warmup": a.warmup,
           "param_bytes": model.model.param_bytes()}
    # the copy rate of this box: 1 GiB through sf_probe_copy
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = alternate({"copy": lambda: ops.probe_copy(src, dst)}, a.iters, a.warmup)["copy"][0]
    del src, dst
    res["probe_copy_read_tbytes_per_s"] = round((1 << 30) / 1e12 / (copy_ms / 1e3), 3)
    res["weight_read_bound_ms"] = round(res["param_bytes"] / ((1 << 30) / (copy_ms / 1e3)) * 1e3, 3)
    g = torch.Generator().manual_seed(0)
    flops_frame = 2.0 * s.seq_len * s.layers_built * (4 * s.dim * s.dim + 2 * s.dim * s.mlp_dim) + 4.0 * s.layers_built * s.seq_len ** 2 * s.dim
    for n in (1, 8):
        video = (torch.rand(3, n, 480, 832, generator=g) * 2 - 1).to(dev)
        fns = {"hip": lambda: model.visual([video])}
        if tower is not None:
            fns["torch_autocast_sdpa"] = lambda: tower(video.transpose(0, 1))
        r = alternate(fns, a.iters, a.warmup)
        entry = {k: {"ms": round(ms, 3), "ms_all": all_ms} for k, (ms, all_ms) in r.items()}
        entry["hip"]["tflops_per_s"] = round(n * flops_frame / 1e12 / (r["hip"][0] / 1e3), 1)
        entry["hip"]["times_the_weight_read_bound"] = round(r["hip"][0] / res["weight_read_bound_ms"], 2)
        if tower is not None:
            entry["hip_speedup_over_torch"] = round(r["torch_autocast_sdpa"][0] / r["hip"][0], 2)
            a_, b_ = model.visual([video]).double(), tower(video.transpose(0, 1)).double()
            entry["rel_diff_hip_vs_torch"] = float((a_ - b_).norm() / b_.norm())
        entry["kernels"] = kernel_split(s, n, dev, a.iters, a.warmup)
        entry["workspace_bytes"] = model.model.workspace_bytes(n)
        res[f"n{n}"] = entry
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
