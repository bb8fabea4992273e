"""Generate the 480 x 832 VAE-decode golden fixture by running the REFERENCE on CPU (build container only).

TEST INFRASTRUCTURE, like tools/make_golden_vae_encode.py (oracle/make_golden_vae.py and the existing fixtures are left
untouched): imports `wan/modules/vae.py` from the reference checkout through `oracle/ref_shim.py`, builds `WanVAE_` with
the real widths (`WAN_VAE`, dim 96), loads `synth_vae_state_dict(WAN_VAE, SEED)` (the encoder keeps its own init and is
never run) and decodes one seeded latent of 3 frames at 60 x 104 -> 9 pixel frames of 480 x 832, in float32 and in
bfloat16 (the bf16 run's distance from the fp32 one is the noise floor the GPU tolerances are compared with).

A whole 480 x 832 clip does not fit a committed file (1 MiB at most), so the fixture keeps what the tests need, in
three files:

    tests/golden/vae_decode_480p.npz        latent [1,3,16,60,104] as bf16 bit patterns (uint16); per (pixel frame,
                                            channel) sum, sum of squares and clamped count (|x| == 1) of the full fp32
                                            output in fp64 (and of the bf16 run); full-resolution 32 x 32 crops of both
                                            runs at the four corners and across the centre patch seams, as float16
                                            (abs error <= 2.5e-4), with the bf16 run's max-abs error on every crop taken
                                            before that rounding; the reference bf16 run's rel-Frobenius error vs fp32,
                                            overall and per pixel frame
    tests/golden/vae_decode_480p_sub{0,1}.npz   the fp32 pixels at stride 4 (16 samples in every 16 x 16 output patch)
                                            as float16, pixel frames 0-4 and 5-8 ([5|4, 3, 120, 208]), and the bf16
                                            run's error on that subsample per frame

Usage: python tools/make_golden_vae_decode_480p.py      (about 2.5 min on 8 CPUs)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402
from self_forcing_amd import vae_weights as vw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 2
LATENT_SHAPE = (1, 3, 16, 60, 104)          # [B, F, C, h, w]
STRIDE = 4
CROP = 32
H, W = 480, 832
# top-left corners of the stored crops: the four corners, then the window across the centre patch seams (240 = 15 * 16,
# 416 = 26 * 16: two patch rows and two patch columns of the 480 x 832 stage meet in it)
CROPS = ((0, 0), (0, W - CROP), (H - CROP, 0), (H - CROP, W - CROP), (H // 2 - CROP // 2, W // 2 - CROP // 2))
SUB_FILES = ((0, 5), (5, 9))                # pixel frames per subsample file (each stays under 1 MiB)


def build_reference(sd, dtype):
    ref_shim.load()
    import wan.modules.vae as rv
    s = vw.WAN_VAE
    m = rv.WanVAE_(dim=s.dim, z_dim=s.z_dim, dim_mult=list(s.dim_mult), num_res_blocks=s.num_res_blocks, attn_scales=[],
                   temperal_downsample=list(s.temperal_upsample[::-1]), dropout=0.0)
    missing, unexpected = m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("encoder.") or k.startswith("conv1.") for k in missing), missing
    return m.eval().requires_grad_(False).to(dtype)


def decode(sd, latent, dtype) -> np.ndarray:
    m = build_reference(sd, dtype)
    mean, std = torch.tensor(vw.LATENT_MEAN), torch.tensor(vw.LATENT_STD)
    with torch.no_grad():
        y = m.decode(latent.to(dtype).permute(0, 2, 1, 3, 4), [mean.to(dtype), 1.0 / std.to(dtype)]).float().clamp_(-1, 1)
    return y[0].permute(1, 0, 2, 3).contiguous().numpy()          # [T, 3, H, W]


def moments(x: np.ndarray):
    x = x.astype(np.float64)
    return x.sum(axis=(2, 3)), (x * x).sum(axis=(2, 3)), (np.abs(x) >= 1.0).sum(axis=(2, 3)).astype(np.int64)


def crops(x: np.ndarray) -> np.ndarray:
    return np.stack([x[:, :, r:r + CROP, c:c + CROP] for r, c in CROPS])      # [5, T, 3, 32, 32]


def rel_frames(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.array([np.linalg.norm(a[t] - b[t]) / np.linalg.norm(b[t]) for t in range(b.shape[0])])


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = vw.synth_vae_state_dict(vw.WAN_VAE, seed=SEED)
    latent = torch.randn(LATENT_SHAPE, generator=torch.Generator().manual_seed(1000 + SEED)).to(torch.bfloat16)
    f32 = decode(sd, latent, torch.float32)
    b16 = decode(sd, latent, torch.bfloat16)
    assert f32.shape == (9, 3, H, W), f32.shape
    s1, s2, nc = moments(f32)
    b1, b2, bc = moments(b16)
    overall = float(np.linalg.norm((b16 - f32).astype(np.float64)) / np.linalg.norm(f32.astype(np.float64)))
    per_frame = rel_frames(b16, f32)
    sub = f32[:, :, ::STRIDE, ::STRIDE]
    sub16 = sub.astype(np.float16)
    assert np.abs(sub16.astype(np.float32) - sub).max() <= 5e-4
    assert np.abs(crops(f32).astype(np.float16).astype(np.float32) - crops(f32)).max() <= 2.5e-4
    np.savez_compressed(
        os.path.join(OUT, "vae_decode_480p.npz"),
        seed=np.int64(SEED), shape_dim=np.int64(vw.WAN_VAE.dim),
        latent_bf16_bits=latent.view(torch.int16).numpy().view(np.uint16),
        sum_f32=s1, sumsq_f32=s2, clamped_f32=nc, sum_bf16=b1, sumsq_bf16=b2, clamped_bf16=bc,
        crop_origins=np.array(CROPS, dtype=np.int64), crops_f32=crops(f32).astype(np.float16), crops_bf16=crops(b16).astype(np.float16),
        crops_ref_bf16_max_abs=np.abs(crops(b16).astype(np.float64) - crops(f32)).max(axis=(3, 4)),
        ref_bf16_rel_err=np.float64(overall), ref_bf16_rel_err_frame=per_frame)
    sub_err = rel_frames(b16[:, :, ::STRIDE, ::STRIDE], sub)
    for i, (a, b) in enumerate(SUB_FILES):
        np.savez_compressed(os.path.join(OUT, f"vae_decode_480p_sub{i}.npz"), stride=np.int64(STRIDE), first_frame=np.int64(a),
                            pixels_f32_sub=sub16[a:b], ref_bf16_sub_rel_err_frame=sub_err[a:b])
    print(f"vae_decode_480p: pixels {f32.shape}, rms {f32.std():.3f}, clamped {np.mean(np.abs(f32) >= 1):.3f}, reference bf16 "
          f"vs fp32 rel err {overall:.4f} (per frame {per_frame.min():.4f}..{per_frame.max():.4f})")


if __name__ == "__main__":
    main()
