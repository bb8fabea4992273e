"""Time the few-step rollout's image and pose conditioning on the MI355X and write one JSON line.

One process, the 1.3B dims (a t2v generator with `pose_proj`, and its i2v-typed stand-in), 480 x 832 (60 x 104 latents), 21
latent frames in chunks of 3, seeded weights everywhere:

* `y_chunk`: `I2VConditioner.frames(3)` -- VAE encode of 12 pixel frames + `sf_i2v_assemble_y` -- per chunk of one clip
  (chunk 0 holds the image's own frame), and the assemble kernel alone;
* `first_chunk`: wall time from calling `stream()` to its first chunk (latents + decoded pixels), with and without an image;
* `rollout`: decoded frames per second of `inference()` (decode excluded: the VAE's decode is replaced by the identity)
  plain, with a pose clip, with an image, with both -- the candidates taking turns inside every repeat -- and plain / pose
  with `pair_context_with_next` off.

    python tools/fewstep_cond_bench.py [--iters 5] [--warmup 1] [--out profiles/fewstep_cond_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import pose_weights as pw  # noqa: E402

F, CHUNK, H, W = 21, 3, 60, 104


class EncodeOnlyVAE:
    """The real VAE's encoder, decode = identity: the rollout legs time the generator and the conditioning alone."""

    def __init__(self, vae):
        self.encoder = vae.encoder

    def decode_to_pixel(self, latents, use_cache=False):
        return latents


def median(v):
    return round(sorted(v)[len(v) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fewstep_cond_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    res = {"what": "fewstep_cond_bench", "dims": "1.3B", "frames": F, "frames_per_chunk": CHUNK, "lat_h": H, "lat_w": W, "iters": a.iters,
           "warmup": a.warmup}
    t2v_shape = sfa.WAN_1_3B
    i2v_shape = t2v_shape.replace(model_type="i2v", in_dim=36)
    gens = {"t2v": sfa.WanDiffusionWrapper(shape=t2v_shape, state_dict=sfa.synth_state_dict(t2v_shape, seed=0, pose=True), timestep_shift=5.0,
                                           is_causal=True, device=dev),
            "i2v": sfa.WanDiffusionWrapper(shape=i2v_shape, state_dict=sfa.synth_state_dict(i2v_shape, seed=0, pose=True), timestep_shift=5.0,
                                           is_causal=True, device=dev)}
    vae = sfa.WanVAEWrapper(sfa.synth_vae_state_dict(sfa.WAN_VAE, seed=0, encoder=True), device=dev)
    clip = sfa.CLIPModel(state_dict=sfa.synth_clip_state_dict(sfa.CLIP_VIT_H_14, 0), shape=sfa.CLIP_VIT_H_14, device=dev)
    embedder = sfa.PoseEmbedder(sfa.synth_pose_state_dict(seed=0), device=dev)
    enc = sfa.SyntheticTextEncoder(t2v_shape.text_len, t2v_shape.text_dim, device=dev)
    args = argparse.Namespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                              num_frame_per_block=CHUNK, context_noise=0)
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(1, F, 16, H, W, generator=g).to(torch.bfloat16).to(dev)
    image = torch.rand(3, 8 * H, 8 * W, generator=g) * 2 - 1
    pose_clip = pw.synth_pose_clip(1, 4 * (F - 1) + 1, 8 * H, 8 * W, "skeleton")
    pose_ref = pw.synth_pose_image(2, 8 * H, 8 * W, "skeleton")
    assert pw.pose_plan(*pose_clip.shape[1:]) == (F, H // 2, W // 2)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    # ---- y per chunk
    cond = sfa.I2VConditioner(vae, clip, pose_embedder=embedder, device=dev)
    per_chunk = [[] for _ in range(F // CHUNK)]
    for it in range(a.warmup + a.iters):
        cond.begin(image, 8 * H, 8 * W)
        for k in range(F // CHUNK):
            s, e = ev(), ev()
            s.record()
            y = cond.frames(CHUNK)
            e.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                per_chunk[k].append(s.elapsed_time(e))
    latent = torch.randn(CHUNK, 16, H, W, device=dev)
    asm = []
    for it in range(a.warmup + a.iters):
        s, e = ev(), ev()
        s.record()
        torch.ops.sf_hip.i2v_assemble_y(latent, y[0], False, None)
        e.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            asm.append(s.elapsed_time(e))
    res["y_chunk"] = {"encode_plus_assemble_ms_by_chunk": [median(v) for v in per_chunk], "assemble_ms": median(asm),
                      "all_ms_by_chunk": [[round(t, 4) for t in v] for v in per_chunk]}

    # ---- the pipelines
    def pipeline(kind, vae_):
        p = sfa.CausalInferencePipeline(args, dev, generator=gens[kind], text_encoder=enc, vae=vae_, image_encoder=clip, pose_embedder=embedder)
        return p
    kw = {"plain": ("t2v", {}), "pose": ("t2v", dict(dwpose_data=pose_clip, random_ref_dwpose=pose_ref)),
          "image": ("i2v", dict(input_image=image)), "image_pose": ("i2v", dict(input_image=image, dwpose_data=pose_clip, random_ref_dwpose=pose_ref))}

    # first chunk of stream(): latents and decoded pixels of chunk 0 on the host's clock
    first = {}
    for name in ("plain", "image"):
        kind, extra = kw[name]
        pipe = pipeline(kind, vae)
        ts = []
        for it in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stream = pipe.stream(noise, ["a prompt"], **extra)
            next(stream)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            for _ in stream:
                pass
        first[name] = {"ms": median(ts[a.warmup:]), "all_ms": [round(t, 3) for t in ts[a.warmup:]]}
    res["first_chunk"] = first

    # rollout frames/s, the candidates taking turns
    pipes = {name: pipeline(kind, EncodeOnlyVAE(vae)) for name, (kind, _) in kw.items()}
    for name in ("plain", "pose"):
        pipes[name + "_unpaired"] = pipeline("t2v", EncodeOnlyVAE(vae))
        pipes[name + "_unpaired"].pair_context_with_next = False
        kw[name + "_unpaired"] = kw[name]
    secs = {name: [] for name in pipes}
    for it in range(a.warmup + a.iters):
        for name, pipe in pipes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.inference(noise, ["a prompt"], **kw[name][1])
            torch.cuda.synchronize()
            if it >= a.warmup:
                secs[name].append(time.perf_counter() - t0)
    decoded = 4 * (F - 1) + 1
    res["rollout"] = {name: {"decoded_frames_per_s": round(decoded / sorted(v)[len(v) // 2], 3), "all_s": [round(t, 4) for t in v]}
                      for name, v in secs.items()}

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
