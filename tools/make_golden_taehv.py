"""Generate the TAEHV decode golden fixtures by running the REFERENCE on CPU (build container only).

TEST INFRASTRUCTURE, like tools/make_golden_vae_decode_480p.py (nothing under oracle/ is touched): imports
`demo_utils/taehv.py` from the reference checkout, builds `TAEHV(checkpoint_path=None)`, loads
`synth_taehv_state_dict(SEED)` into its decoder (the encoder keeps its own init and is never run) and decodes seeded
latents with `decode_video(parallel=True)` in float32 and in bfloat16 (the bf16 run's distance from the fp32 one is the
noise floor the GPU tolerances are taken from, stored per pixel frame).  Weights are never stored: both sides regenerate
them from the seed.  `y` below is `decode_video`'s output (~[0, 1]); the GPU path returns `2 y - 1`.

    tests/golden/taehv_small_{a,b}.npz   5 latent frames of 6 x 8 and 2 of 13 x 21 (every stage has ragged tiles; 6 x 8 is
                                         below one tile): latent as bf16 bit patterns, y of the fp32 run as float16,
                                         the bf16 run's rel-Frobenius error per pixel frame; (a) also holds the
                                         reference's decoder state_dict names and shapes
    tests/golden/taehv_480p.npz          3 latent frames of 60 x 104 -> 12 frames of 480 x 832: latent bits; per
                                         (pixel frame, channel) sum and sum of squares of y in fp64, fp32 and bf16 run;
                                         32 x 32 crops of the fp32 run at the four corners and across the centre tile seams
                                         (float16), the bf16 run's max-abs error on every crop; its rel error per frame
    tests/golden/taehv_480p_sub{0,1,2}.npz   y of the fp32 run at stride 4 as float16, 4 pixel frames per file, and the
                                         bf16 run's rel error on that subsample per frame

Usage: python tools/make_golden_taehv.py [--small-only]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from self_forcing_amd import taehv_weights as tw  # noqa: E402

REFERENCE_ROOT = os.environ.get("SF_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
SEED = 3
SMALL = (("a", (5, 16, 6, 8)), ("b", (2, 16, 13, 21)))
BIG = (3, 16, 60, 104)
STRIDE, CROP, H, W = 4, 32, 480, 832
CROPS = ((0, 0), (0, W - CROP), (H - CROP, 0), (H - CROP, W - CROP), (H // 2 - CROP // 2, W // 2 - CROP // 2))
SUB_FILES = ((0, 4), (4, 8), (8, 12))


def reference(dtype):
    sys.dont_write_bytecode = True
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    from demo_utils.taehv import TAEHV
    m = TAEHV(checkpoint_path=None)
    sd = tw.synth_taehv_state_dict(SEED)
    missing, unexpected = m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing), (missing, unexpected)
    names = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if k.startswith("decoder.")]
    return m.eval().requires_grad_(False).to(dtype), names


def decode(m, latent, dtype) -> np.ndarray:
    with torch.no_grad():
        y = m.decode_video(latent[None].to(dtype), parallel=True, show_progress_bar=False)
    return y[0].float().numpy()          # [4F, 3, 8h, 8w]


def rel_frames(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.array([np.linalg.norm(a[t] - b[t]) / np.linalg.norm(b[t]) for t in range(b.shape[0])])


def bits(latent):
    return latent.view(torch.int16).numpy().view(np.uint16)


def crops(x):
    return np.stack([x[:, :, r:r + CROP, c:c + CROP] for r, c in CROPS])


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    m32, names = reference(torch.float32)
    m16, _ = reference(torch.bfloat16)
    assert names == list(tw.taehv_param_shapes().items())
    for i, (tag, shape) in enumerate(SMALL):
        latent = torch.randn(shape, generator=torch.Generator().manual_seed(2000 + SEED + i)).to(torch.bfloat16)
        f32, b16 = decode(m32, latent, torch.float32), decode(m16, latent, torch.bfloat16)
        extra = {}
        if tag == "a":
            extra = dict(decoder_keys=np.array([k for k, _ in names]), decoder_shapes=np.array([",".join(map(str, s)) for _, s in names]))
        np.savez_compressed(os.path.join(OUT, f"taehv_small_{tag}.npz"), seed=np.int64(SEED), latent_bf16_bits=bits(latent),
                            y_f32=f32.astype(np.float16), ref_bf16_rel_err_frame=rel_frames(b16, f32), **extra)
        print(f"taehv_small_{tag}: y {f32.shape} mean {f32.mean():.3f} std {f32.std():.3f}; reference bf16 per frame "
              f"{rel_frames(b16, f32).min():.2e}..{rel_frames(b16, f32).max():.2e}", flush=True)
    if "--small-only" in sys.argv:
        return
    latent = torch.randn(BIG, generator=torch.Generator().manual_seed(1000 + SEED)).to(torch.bfloat16)
    f32, b16 = decode(m32, latent, torch.float32), decode(m16, latent, torch.bfloat16)
    assert f32.shape == (12, 3, H, W)

    def moments(x):
        x = x.astype(np.float64)
        return x.sum(axis=(2, 3)), (x * x).sum(axis=(2, 3))

    s1, s2 = moments(f32)
    b1, b2 = moments(b16)
    per_frame = rel_frames(b16, f32)
    np.savez_compressed(
        os.path.join(OUT, "taehv_480p.npz"), seed=np.int64(SEED), latent_bf16_bits=bits(latent),
        sum_f32=s1, sumsq_f32=s2, sum_bf16=b1, sumsq_bf16=b2, crop_origins=np.array(CROPS, dtype=np.int64),
        crops_f32=crops(f32).astype(np.float16),
        crops_ref_bf16_max_abs=np.abs(crops(b16).astype(np.float64) - crops(f32)).max(axis=(3, 4)),
        ref_bf16_rel_err_frame=per_frame, ref_bf16_max_abs_2y=np.float64(2 * np.abs(b16 - f32).max()))
    sub = f32[:, :, ::STRIDE, ::STRIDE]
    sub_err = rel_frames(b16[:, :, ::STRIDE, ::STRIDE], sub)
    for i, (a, b) in enumerate(SUB_FILES):
        np.savez_compressed(os.path.join(OUT, f"taehv_480p_sub{i}.npz"), stride=np.int64(STRIDE), first_frame=np.int64(a),
                            y_f32_sub=sub[a:b].astype(np.float16), ref_bf16_sub_rel_err_frame=sub_err[a:b])
    print(f"taehv_480p: y {f32.shape} mean {f32.mean():.3f} std {f32.std():.3f}; reference bf16 vs fp32 per frame "
          f"{per_frame.min():.2e}..{per_frame.max():.2e}, max-abs on 2y-1 {2 * np.abs(b16 - f32).max():.2e}")


if __name__ == "__main__":
    main()
