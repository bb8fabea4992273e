"""FP8 linear layers against bf16 on the MI355X, one JSON line.  In one process, interleaved, on
the same seeded Wan-1.3B weights:
  * the four GEMMs of a block (qkv, o, ffn.0, ffn.2) at M = 4680 and 9360 rows: us and TFLOP/s, bf16 vs fp8 (the fp8
    GEMM on operands quantised beforehand), and the quantiser's own time for the GEMM's input;
  * the S1 rollout (21 latent frames of 60 x 104, 3 frames per chunk, 4 steps) in decoded frames/s at --batch 1 and 2;
  * the fp8 and bf16 latents of the first two S1 chunks against the fp32 golden (tests/golden/s1_2chunks_1p3b.npz).
`--kernel-stats FILE`: fold in the per-kernel shares of a separate `rocprofv3 --kernel-trace --stats` run of
`--profile-run` (an fp8 rollout only) and report the quantiser's share.

    python tools/fp8_bench.py [--iters 3] [--gemm-iters 20] [--kernel-stats out/kernel_stats.csv]
    rocprofv3 --kernel-trace --stats -d out -o run -- python tools/fp8_bench.py --profile-run
"""
import argparse
import csv
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
SHAPE = sfa.WAN_1_3B
LAT_H, LAT_W, FRAMES, NFPB = 60, 104, 21, 3


def gemm_ms(fn, n):
    """Mean device time of n back-to-back launches (ms)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def gemm_leg(iters, rounds=3):
    C, Fd = SHAPE.dim, SHAPE.ffn_dim
    g = torch.Generator().manual_seed(0)
    out = {}
    for M in (4680, 9360):
        for name, N, K in (("qkv", 3 * C, C), ("o", C, C), ("ffn0", Fd, C), ("ffn2", C, Fd)):
            a = (torch.randn(M, K, generator=g)).to(torch.bfloat16).to(DEV)
            w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
            bias = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
            aq, sa = ops.quantize_fp8(a)
            wq, sw = ops.quantize_fp8(w)
            sw = sw.expand(N).contiguous()
            runs = {"bf16": lambda: ops.gemm(a, w, bias), "fp8": lambda: ops.gemm_fp8(aq, sa, wq, sw, bias),
                    "quantize": lambda: ops.quantize_fp8(a)}
            for fn in runs.values():
                fn()
            ts = {k: [] for k in runs}
            for _ in range(rounds):                      # interleaved: the board's power state is shared by all three
                for k, fn in runs.items():
                    ts[k].append(gemm_ms(fn, iters))
            flop = 2.0 * M * N * K
            rec = {}
            for k in runs:
                ms = sorted(ts[k])[len(ts[k]) // 2]
                rec[k + "_us"] = round(1e3 * ms, 1)
                if k != "quantize":
                    rec[k + "_tflops"] = round(flop / (ms * 1e-3) / 1e12, 1)
            rec["fp8_speedup"] = round(rec["bf16_us"] / rec["fp8_us"], 3)
            rec["fp8_plus_quantize_speedup"] = round(rec["bf16_us"] / (rec["fp8_us"] + rec["quantize_us"]), 3)
            out[f"{name}_M{M}"] = rec
    return out


def make_pipe(gen):
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=NFPB, context_noise=0)
    enc = sfa.SyntheticTextEncoder(SHAPE.text_len, SHAPE.text_dim, device=DEV)
    return sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=enc, vae=sfa.IdentityVAE())


def rollout_s(pipe, batch, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pipe.noise_source = lambda t: torch.randn(t.shape, generator=g, device=t.device, dtype=t.dtype)
    noise = torch.randn([batch, FRAMES, 16, LAT_H, LAT_W], generator=g, device=DEV, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe.inference(noise, [f"prompt {i}" for i in range(batch)], return_latents=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def rollout_leg(gens, iters):
    decoded = 1 + 4 * (FRAMES - 1)
    out = {}
    for batch in (1, 2):
        pipes = {k: make_pipe(g) for k, g in gens.items()}
        for k, p in pipes.items():
            rollout_s(p, batch, 0)                       # warm-up: caches, workspaces
        ts = {k: [] for k in pipes}
        for i in range(iters):
            for k, p in pipes.items():                   # interleaved
                ts[k].append(rollout_s(p, batch, 1 + i))
        rec = {}
        for k in pipes:
            s = sorted(ts[k])[len(ts[k]) // 2]
            rec[k] = {"seconds": round(s, 3), "frames_per_s": round(batch * decoded / s, 2), "all_s": [round(t, 3) for t in ts[k]]}
        rec["fp8_speedup"] = round(rec["fp8"]["frames_per_s"] / rec["bf16"]["frames_per_s"], 3)
        out[f"batch{batch}"] = rec
        del pipes
        torch.cuda.empty_cache()
    return out


def latent_error_leg(gens):
    """First two S1 chunks on the golden's inputs (as tests/test_gpu_fullsize.py draws them) against its fp32 latents."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "s1_2chunks_1p3b.npz"))
    g = torch.Generator().manual_seed(int(G["input_seed"]))
    bf = lambda shape: torch.randn(shape, generator=g).to(torch.bfloat16)  # noqa: E731
    noise = bf((1, 6, 16, 60, 104))
    pe = bf((1, 512, SHAPE.text_dim))
    pe[:, 141:] = 0
    eps = [bf((3, 16, 60, 104)) for _ in range(6)]
    want = torch.from_numpy(G["lat_f32_frames"]).double()
    frames = [int(f) for f in G["frames"]]
    out = {"reference_bf16_vs_f32": float(G["ref_bf16_vs_f32"])}
    for k, gen in gens.items():
        args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                               num_frame_per_block=3, context_noise=0)
        pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe.to(DEV)), vae=sfa.IdentityVAE())
        q = list(eps)
        pipe.noise_source = lambda t: q.pop(0).to(DEV).reshape(t.shape)
        lat = pipe.inference(noise.to(DEV), ["p"], return_latents=True)[1][:, frames].double().cpu()
        out[f"{k}_vs_f32"] = round(((lat - want).norm() / want.norm()).item(), 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="timed rollouts per configuration")
    ap.add_argument("--gemm-iters", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--profile-run", action="store_true", help="only two fp8 rollouts at batch 1 (for a rocprofv3 run)")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    sd = sfa.synth_state_dict(SHAPE, seed=0)
    kw = dict(shape=SHAPE, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV)
    if a.profile_run:
        pipe = make_pipe(sfa.WanDiffusionWrapper(**kw, fp8=True))
        for i in range(2):
            rollout_s(pipe, 1, i)
        return
    gens = {"bf16": sfa.WanDiffusionWrapper(**kw), "fp8": sfa.WanDiffusionWrapper(**kw, fp8=True)}
    del sd
    res = {"what": "fp8_linear_layers", "model": "Wan2.1-T2V-1.3B (seeded weights)",
           "param_bytes": {k: g.model.param_bytes() for k, g in gens.items()}}
    res["gemm"] = gemm_leg(a.gemm_iters)
    res["rollout_s1"] = {"latent": [FRAMES, LAT_H, LAT_W], "frames_per_chunk": NFPB, "steps": 4, **rollout_leg(gens, a.iters)}
    res["latent_error_s1_2chunks"] = latent_error_leg(gens)
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            rows = list(csv.DictReader(f))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        share = lambda pred: round(sum(float(r["TotalDurationNs"]) for r in rows if pred(r["Name"])) / tot, 4)  # noqa: E731
        res["fp8_rollout_kernel_shares"] = {
            "quantize (fp8_amax_kernel + fp8_quantize_kernel)": share(lambda n: "fp8_amax_kernel" in n or "fp8_quantize_kernel" in n),
            "gemm (all structures)": share(lambda n: "gemm_" in n),
            "small_linear_fp8_kernel": share(lambda n: "small_linear_fp8_kernel" in n),
            "attention": share(lambda n: "attention" in n),
            "top": {r["Name"][:80]: round(float(r["TotalDurationNs"]) / tot, 4) for r in rows if float(r["TotalDurationNs"]) / tot >= 0.01}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
