"""Generate the pose front end's golden fixtures by running the REFERENCE's own modules on CPU (build container only).

TEST INFRASTRUCTURE, like tools/make_golden_taehv.py (nothing under oracle/ is touched): `oracle/ref_shim.load_sampler()`
imports `pipeline/causal_diffusion_inference.py`; `_get_dwpose_embedding` / `_get_randomref_embedding_pose` (:87-122,
they do not use `self`) build the two `nn.Sequential`s, which are loaded with `synth_pose_state_dict(SEED)` and run on
the reference's input transform (:337-343) in float32 (the truth) and with module and input cast to bfloat16 (the
floor the GPU tolerances are taken from).  Weights are never stored: both sides regenerate them from the seed.  Inputs
are `pose_weights.synth_pose_clip / synth_pose_image` of two kinds, "dense" and "skeleton".  No file exceeds 1 MiB.

    tests/golden/pose_small_{a,b}_{dense,skeleton}.npz      9 frames of 64 x 96 (a: below one tile at the late layers) and of
                                 120 x 208 (b: ragged, 7 x 13 tokens): the clip and the reference image (uint8), the
                                 reference-pose map of the fp32 run (float16), the bf16 run's rel-Frobenius error per
                                 latent frame (dwpose) and overall (map); a_dense also holds the reference's state_dict
                                 names and shapes
    tests/golden/pose_small_{a,b}_{kind}_f{0,1,2}.npz       tokens [h*w, 5120] of latent frame f, fp32 run, as float16
    tests/golden/pose_480p_{dense,skeleton}.npz             81 frames of 480 x 832 (regenerated from the seed by the test;
                                 the file holds its CRC-32): the bf16 run's rel error per latent frame on both
                                 subsamples; skeleton also: the bf16 run's deviation per latent frame of the
                                 per-channel mean and rms
    tests/golden/pose_480p_{kind}_subA{0,1}.npz             every 32nd channel of every 8th token, fp32 run, float16
    tests/golden/pose_480p_skeleton_subB{0,1,2}.npz         all channels of every 195th token
    tests/golden/pose_480p_skeleton_{sum,sumsq}.npz         per (latent frame, channel) sum and sum of squares, float64

Usage: python tools/make_golden_pose.py [--small-only]
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from self_forcing_amd import pose_weights as pw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 5
SMALL = (("a", (9, 64, 96)), ("b", (9, 120, 208)))
BIG = (81, 480, 832)
KINDS = ("dense", "skeleton")
SUB_A_TOKENS, SUB_A_CHANNELS, SUB_B_TOKENS = 8, 32, 195
SUB_A_FILES = ((0, 11), (11, 21))
SUB_B_FILES = ((0, 7), (7, 14), (14, 21))


def input_seed(tag: str, kind: str) -> int:
    return 7000 + 100 * SEED + 10 * ("a", "b", "big").index(tag) + KINDS.index(kind)


def reference(dtype):
    sys.dont_write_bytecode = True
    from oracle import ref_shim
    cls = ref_shim.load_sampler().CausalDiffusionInferencePipeline
    dw, rr = cls._get_dwpose_embedding(None), cls._get_randomref_embedding_pose(None)
    sd = pw.synth_pose_state_dict(SEED)
    dw.load_state_dict({k[len(pw.DWPOSE_PREFIX):]: v for k, v in sd.items() if k.startswith(pw.DWPOSE_PREFIX)}, strict=True)
    rr.load_state_dict({k[len(pw.RANDOMREF_PREFIX):]: v for k, v in sd.items() if k.startswith(pw.RANDOMREF_PREFIX)}, strict=True)
    names = [(pw.DWPOSE_PREFIX + k, tuple(v.shape)) for k, v in dw.state_dict().items()]
    names += [(pw.RANDOMREF_PREFIX + k, tuple(v.shape)) for k, v in rr.state_dict().items()]
    return dw.eval().requires_grad_(False).to(dtype), rr.eval().requires_grad_(False).to(dtype), names


def run_dwpose(m, clip, dtype) -> np.ndarray:
    """The reference's call (:337-340) -> tokens [F', h*w, 5120] float32."""
    with torch.no_grad():
        d = clip.unsqueeze(0)
        y = m((torch.cat([d[:, :, :1].repeat(1, 1, 3, 1, 1), d], dim=2) / 255.0).to(dtype))
    return y[0].float().permute(1, 2, 3, 0).flatten(1, 2).numpy()


def run_ref(m, image, dtype) -> np.ndarray:
    with torch.no_grad():
        y = m((image.unsqueeze(0) / 255.0).permute(0, 3, 1, 2).to(dtype))
    return y[0].float().numpy()          # [20, h, w]


def rel(a, b) -> float:
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rel_frames(a, b):
    return np.array([rel(a[f], b[f]) for f in range(b.shape[0])])


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{name}: {size} bytes"
    return size


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dw32, rr32, names = reference(torch.float32)
    dw16, rr16, _ = reference(torch.bfloat16)
    assert names == list(pw.pose_param_shapes().items())
    total = 0
    for tag, (F, H, W) in SMALL:
        for kind in KINDS:
            seed = input_seed(tag, kind)
            clip, image = pw.synth_pose_clip(seed, F, H, W, kind), pw.synth_pose_image(seed + 50, H, W, kind)
            t32, t16 = run_dwpose(dw32, clip, torch.float32), run_dwpose(dw16, clip, torch.bfloat16)
            r32, r16 = run_ref(rr32, image, torch.float32), run_ref(rr16, image, torch.bfloat16)
            assert t32.shape[0] * t32.shape[1] == int(np.prod(pw.pose_plan(F, H, W))) and r32.shape[1:] == pw.ref_plan(H, W)
            extra = {}
            if tag == "a" and kind == "dense":
                extra = dict(state_keys=np.array([k for k, _ in names]), state_shapes=np.array([",".join(map(str, s)) for _, s in names]))
            total += save(f"pose_small_{tag}_{kind}.npz", seed=np.int64(SEED), clip_u8=clip.numpy(), image_u8=image.numpy(),
                          plan=np.array(pw.pose_plan(F, H, W), dtype=np.int64), ref_map_f32=r32.astype(np.float16),
                          ref_bf16_rel_err_frame=rel_frames(t16, t32), ref_bf16_rel_err_map=np.float64(rel(r16, r32)), **extra)
            for f in range(t32.shape[0]):
                total += save(f"pose_small_{tag}_{kind}_f{f}.npz", tokens_f32=t32[f].astype(np.float16))
            e = rel_frames(t16, t32)
            print(f"pose_small_{tag}_{kind}: tokens {t32.shape} rms {np.sqrt((t32 ** 2).mean()):.3f}, lit {float((clip > 0).any(0).float().mean()):.3f}; "
                  f"reference bf16 per frame {e.min():.2e}..{e.max():.2e}, map {rel(r16, r32):.2e}", flush=True)
    if "--small-only" not in sys.argv:
        F, H, W = BIG
        for kind in KINDS:
            clip = pw.synth_pose_clip(input_seed("big", kind), F, H, W, kind)
            t32, t16 = run_dwpose(dw32, clip, torch.float32), run_dwpose(dw16, clip, torch.bfloat16)
            assert t32.shape == (21, 1560, 5120)
            a32, a16 = t32[:, ::SUB_A_TOKENS, ::SUB_A_CHANNELS], t16[:, ::SUB_A_TOKENS, ::SUB_A_CHANNELS]
            b32, b16 = t32[:, ::SUB_B_TOKENS], t16[:, ::SUB_B_TOKENS]
            main_arrays = dict(seed=np.int64(SEED), input_seed=np.int64(input_seed("big", kind)), clip_crc32=np.int64(zlib.crc32(clip.numpy().tobytes())),
                               ref_bf16_rel_err_frame=rel_frames(t16, t32), ref_bf16_subA_rel_err_frame=rel_frames(a16, a32),
                               ref_bf16_subB_rel_err_frame=rel_frames(b16, b32))
            for i, (lo, hi) in enumerate(SUB_A_FILES):
                total += save(f"pose_480p_{kind}_subA{i}.npz", first_frame=np.int64(lo), tokens_f32=a32[lo:hi].astype(np.float16))
            if kind == "skeleton":
                for i, (lo, hi) in enumerate(SUB_B_FILES):
                    total += save(f"pose_480p_{kind}_subB{i}.npz", first_frame=np.int64(lo), tokens_f32=b32[lo:hi].astype(np.float16))
                s32, q32 = t32.astype(np.float64).sum(1), (t32.astype(np.float64) ** 2).sum(1)
                s16, q16 = t16.astype(np.float64).sum(1), (t16.astype(np.float64) ** 2).sum(1)
                n = t32.shape[1]
                main_arrays.update(ref_bf16_mean_dev_frame=rel_frames(s16 / n, s32 / n), ref_bf16_rms_dev_frame=rel_frames(np.sqrt(q16 / n), np.sqrt(q32 / n)))
                total += save(f"pose_480p_{kind}_sum.npz", sum_f32=s32)
                total += save(f"pose_480p_{kind}_sumsq.npz", sumsq_f32=q32)
            total += save(f"pose_480p_{kind}.npz", **main_arrays)
            e = main_arrays["ref_bf16_rel_err_frame"]
            print(f"pose_480p_{kind}: tokens {t32.shape} rms {np.sqrt((t32 ** 2).mean()):.3f}, lit {float((clip > 0).any(0).float().mean()):.3f}; "
                  f"reference bf16 per frame {e.min():.2e}..{e.max():.2e}", flush=True)
            if kind == "skeleton":
                print(f"  mean dev {main_arrays['ref_bf16_mean_dev_frame'].max():.2e}, rms dev {main_arrays['ref_bf16_rms_dev_frame'].max():.2e}")
    print(f"total {total / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
