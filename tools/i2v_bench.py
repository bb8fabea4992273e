"""Time the generator's i2v model type on the MI355X against the t2v forward of the same commit and write one JSON line.

One process, a warm-up of every candidate, then the candidates taking turns inside every repeat (device events around
each call; median and all samples):

* one 3-frame pass (4680 tokens of 60 x 104 latents) of an i2v-typed model at the 1.3B dims against the t2v model with
  the same seed, attending 4680 keys (the first chunk) and 32760 keys (the last chunk of a 21-frame cache);
* the same pass with `init_cross` (the once-per-prompt work: text K / V for both, plus img_emb and k_img / v_img for i2v);
  the image context's cost is the difference of the two differences;
* `ops.attention_accum` over 257 keys against `ops.attention` at the same shape (4680 queries, 12 heads).

    python tools/i2v_bench.py [--iters 7] [--warmup 2] [--out profiles/i2v_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import ops  # noqa: E402
from self_forcing_amd.kvcache import new_crossattn_cache, new_kv_cache  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, iters, warmup):
    """{name: fn} -> {name: {"ms": median, "all_ms": [...]}}, the candidates taking turns inside every repeat."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return {k: {"ms": round(sorted(v)[len(v) // 2], 4), "all_ms": [round(t, 4) for t in v]} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i2v_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    F, H, W, frames_total = 3, 60, 104, 21
    fs = (H // 2) * (W // 2)
    t2v_shape = sfa.WAN_1_3B
    i2v_shape = t2v_shape.replace(model_type="i2v", in_dim=36)
    res = {"what": "i2v_bench", "dims": "1.3B", "frames": F, "lat_h": H, "lat_w": W, "tokens": F * fs, "iters": a.iters, "warmup": a.warmup}
    g = torch.Generator().manual_seed(0)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)  # noqa: E731
    x, pe, clip, y = bf(1, F, 16, H, W), bf(1, 512, 4096), bf(1, 257, 1280), bf(1, 20, F, H, W)
    pe[:, 77:] = 0
    ts = torch.full((1, F), 500.0, device=dev)
    gens = {"t2v": sfa.WanDiffusionWrapper(shape=t2v_shape, random_init_seed=0, is_causal=True, device=dev),
            "i2v": sfa.WanDiffusionWrapper(shape=i2v_shape, random_init_seed=0, is_causal=True, device=dev)}
    for gen in gens.values():
        gen.max_inflight_forwards = 0
    caches = {k: (new_kv_cache(gen.model.shape, 30, 1, frames_total * fs, torch.bfloat16, dev),
                  new_crossattn_cache(gen.model.shape, 30, 1, torch.bfloat16, dev)) for k, gen in gens.items()}
    extra = {"t2v": {}, "i2v": {"clip_feature": clip, "y": y}}

    def call(name, start_frame, init):
        gen, (kv, cc) = gens[name], caches[name]
        if init:
            for c in cc:
                c["is_init"] = False
        gen.forward(x, {"prompt_embeds": pe}, ts, kv, cc, start_frame * fs, **extra[name])

    for name in gens:       # fill the cross caches once
        call(name, 0, True)
    for label, start in (("lk4680", 0), ("lk32760", frames_total - F)):
        for name, gen in gens.items():      # the cache holds `start` frames in front of the chunk; repeats rewrite the chunk in place
            gen._write_indices(caches[name][0], start * fs, start * fs)
        res["forward_" + label] = alternate({n: (lambda n=n, start=start: call(n, start, False)) for n in gens}, a.iters, a.warmup)
        r = res["forward_" + label]
        r["i2v_over_t2v"] = round(r["i2v"]["ms"] / r["t2v"]["ms"], 4)
    for name, gen in gens.items():
        gen._write_indices(caches[name][0], 0, 0)
    res["forward_init_cross"] = alternate({n: (lambda n=n: call(n, 0, True)) for n in gens}, a.iters, a.warmup)
    plain, init = res["forward_lk4680"], res["forward_init_cross"]
    res["image_context_ms"] = round((init["i2v"]["ms"] - plain["i2v"]["ms"]) - (init["t2v"]["ms"] - plain["t2v"]["ms"]), 4)

    q, k, v = bf(1, F * fs, 12, 128), bf(1, 257, 12, 128), bf(1, 257, 12, 128)
    out = ops.attention(q, k, v)
    res["attention_lk257"] = alternate({"attention": lambda: ops.attention(q, k, v), "attention_accum": lambda: ops.attention_accum(q, k, v, out)},
                                       a.iters, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items()}))


if __name__ == "__main__":
    main()
