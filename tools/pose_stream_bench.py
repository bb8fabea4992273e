"""Time the pose front end in pieces on the MI355X and write profiles/pose_stream_bench.json (and print it as one line).

Seeded weights, 480 x 832 unless said otherwise, device events or a host clock around a device synchronise, a warm-up, the
median of `--iters` repeats, the candidates alternated inside every repeat of one process.  There is no earlier build to
compare with: the whole-clip path of this same build is the yardstick everywhere.

* `push12`: one `PoseStream.push` of 12 frames in the middle of a clip (3 latent frames become final) against
  `PoseEmbedder.embed` of 81 frames divided by 7 (its 21 latent frames, three at a time); the timed window holds seven
  pushes back to back, so both candidates do the same work in it.  Same FLOPs per latent frame; the push adds the
  two-frame history copies and runs its kernels on a seventh of the bricks.
* `first_chunk`: the time from calling `CausalInferencePipeline.stream` to its first yielded chunk (3 latent frames of a
  21-frame rollout, reduced generator: the generator's work is the same on both sides) with `pose_feed` delivering
  1-frame pieces (13 pushes before chunk 0) against the same 81 frames passed as `dwpose_data` (embedded whole first).
* `embed_long_720p`: `embed_long` on 200 frames of 720 x 1280, which `embed` refuses (4 GiB volumes), with its peak
  device memory; and the check that `embed_long` gives `embed`'s bits on the 81-frame clip.

It fails rather than falling back when it finds no GPU.

    python tools/pose_stream_bench.py [--iters 10] [--warmup 2] [--out profiles/pose_stream_bench.json]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import pose_weights as pw  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns, iters, warmup, clock=timed):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ts[k].append(clock(fn))
    return {k: {"ms": round(sorted(v)[len(v) // 2], 3), "ms_all": [round(t, 3) for t in v], "spread_ms": round(max(v) - min(v), 3)} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--long-frames", type=int, default=200)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_stream_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_stream_bench: no GPU found (this tool measures the HIP path; there is nothing to fall back to)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    H, W = a.height, a.width
    emb = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=dev)
    clip = pw.synth_pose_clip(1, 81, H, W, "skeleton").to(dev)
    res = {"what": "pose_stream_bench", "height": H, "width": W, "iters": a.iters,
           "yardstick": "the whole-clip path of the same build, alternated in the same process (there is no earlier build with a counterpart)"}

    # ---- 1. one push of 12 frames against a seventh of the whole clip
    stream = emb.open_stream(H, W, 12)
    stream.push(clip[:, :13])
    piece = clip[:, 13:25].contiguous()
    out = torch.empty(1, 3 * stream.h * stream.w, 5120, dtype=torch.bfloat16, device=dev)

    def seven_pushes():      # 84 frames, 21 latent frames: the whole clip's work in one timed window
        for _ in range(7):
            stream.push(piece, out=out)

    r = alternate({"push12_x7": seven_pushes, "embed81": lambda: emb.embed(clip)}, a.iters, a.warmup)
    r["push12_ms"] = round(r["push12_x7"]["ms"] / 7, 3)
    r["embed81_over_7_ms"] = round(r["embed81"]["ms"] / 7, 3)
    r["push12_over_embed81_seventh"] = round(r["push12_x7"]["ms"] / r["embed81"]["ms"], 3)
    r["stream_bytes"] = {"state": stream._state.numel(), "scratch": stream._scratch.numel()}
    r["embed81_scratch_bytes"] = emb.scratch_bytes(81, H, W)
    whole = emb.embed(clip)[0].clone()
    r["embed_long_equals_embed"] = bool(torch.equal(emb.embed_long(clip, 12)[0], whole))
    res["push12"] = r
    del stream, out, whole
    torch.cuda.empty_cache()

    # ---- 2. the first chunk of stream(): a feed of 1-frame pieces against the whole clip
    shape = sfa.WAN_REDUCED
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0, pose=True), timestep_shift=5.0, is_causal=True, device=dev)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(1, 21, 16, H // 8, W // 8, generator=g).to(torch.bfloat16).to(dev)
    pe = torch.randn(1, 512, shape.text_dim, generator=g).to(torch.bfloat16).to(dev)
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False, num_frame_per_block=3,
                           context_noise=0)
    pipe = sfa.CausalInferencePipeline(args, dev, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=sfa.IdentityVAE(), pose_embedder=emb)
    image = pw.synth_pose_image(2, H, W, "skeleton")
    pieces = list(clip.split(1, dim=1))

    def first(**kw):
        it = pipe.stream(noise, ["p"], **kw)
        next(it)
        it.close()

    r = alternate({"pose_feed_1_frame_pieces": lambda: first(pose_feed=iter(pieces)),
                   "dwpose_data_whole_clip": lambda: first(dwpose_data=clip, random_ref_dwpose=image)}, a.iters, a.warmup, clock=wall)
    r["generator"] = "WAN_REDUCED (seeded), 3 latent frames per chunk, 4 steps"
    res["first_chunk"] = r
    del pipe, gen, noise
    emb._scratch.clear()
    torch.cuda.empty_cache()

    # ---- 3. a clip `embed` refuses
    if a.skip_long:
        res["embed_long_720p"] = "not measured"
    else:
        F = a.long_frames
        torch.manual_seed(4)
        long_clip = torch.randint(0, 256, (3, F, 720, 1280), dtype=torch.uint8, device=dev)
        refused = None
        try:
            emb.scratch_bytes(F, 720, 1280)
        except sfa._lib.SfHipError as e:
            refused = str(e)[:320]
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        emb.embed_long(long_clip[:, :25], 12)          # warm-up: the same kernels on the same frame size
        ms = [wall(lambda: emb.embed_long(long_clip, 12)) for _ in range(3)]
        res["embed_long_720p"] = {"frames": F, "tokens": list(pw.pose_plan(F, 720, 1280)), "frames_per_push": 12, "ms": round(sorted(ms)[1], 2),
                                  "ms_all": [round(t, 2) for t in ms], "embed_refuses": refused,
                                  "peak_bytes_beyond_the_clip": int(torch.cuda.max_memory_allocated(dev) - base),
                                  "tokens_bytes": int(pw.pose_plan(F, 720, 1280)[0] * 45 * 80 * 5120 * 2)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
