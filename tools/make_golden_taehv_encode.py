"""Generate the TAEHV encode golden fixtures by running the REFERENCE on CPU (build container only).

TEST INFRASTRUCTURE, like tools/make_golden_taehv.py (nothing under oracle/ is touched): imports `demo_utils/taehv.py`
from the reference checkout, builds `TAEHV(checkpoint_path=None)`, loads `synth_taehv_encoder_state_dict(SEED)` into its
encoder (the decoder keeps its own init and is never run) and encodes seeded pixels with `encode_video(parallel=True)`
in float32 (the truth) and in bfloat16 (its distance from the fp32 run is the noise floor the GPU tolerance is taken
from, stored per latent frame).  Weights are never stored: both sides regenerate them from the seed.  Pixels are seeded
uint8 values u, handed to the GPU path as x = u / 127.5 - 1 and to the reference as 0.5 x + 0.5, of two kinds: noise,
and structured (gradients that move from frame to frame, plus hard edges).

    tests/golden/taehv_enc_{a,b,c}.npz   8 frames of 16 x 24 (noise; every stage below one 128-row tile), 12 of 104 x 168
                                         (noise; ragged tiles at every stage, three latent frames), 8 of 40 x 72
                                         (structured): the uint8 pixels, latents of the fp32 run as float16, the bf16
                                         run's rel-Frobenius error per latent frame; (a) also holds the reference's
                                         encoder state_dict names and shapes
    tests/golden/taehv_enc_480p.npz      8 frames of 480 x 832 (noise): the same, with the CRC-32 of the uint8 pixels
                                         in place of the pixels (the test regenerates them from the seed)

Usage: python tools/make_golden_taehv_encode.py [--small-only]
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from self_forcing_amd import taehv_weights as tw  # noqa: E402

REFERENCE_ROOT = os.environ.get("SF_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
SEED = 3
CASES = (("a", "noise", (8, 16, 24)), ("b", "noise", (12, 104, 168)), ("c", "structured", (8, 40, 72)), ("480p", "noise", (8, 480, 832)))


def pixels_u8(kind: str, seed: int, T: int, H: int, W: int) -> torch.Tensor:
    """[T, 3, H, W] uint8.  noise: uniform bytes.  structured: per channel a gradient whose direction and phase move with
    the frame, a bright rectangle that travels, and a one-pixel checkerboard corner (hard edges at every stride)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = torch.empty(T, 3, H, W)
    for t in range(T):
        for c in range(3):
            a = 0.7 * c + 0.35 * t
            ramp = (np.cos(a) * x / W + np.sin(a) * y / H + 0.11 * t) % 1.0
            out[t, c] = 255 * ramp
        r0, c0 = (3 * t) % max(H - 10, 1), (5 * t) % max(W - 14, 1)
        out[t, :, r0:r0 + 10, c0:c0 + 14] = torch.tensor([250.0, 20.0, 128.0])[:, None, None]
        out[t, :, H - 12:, W - 12:] = 255 * ((y[H - 12:, W - 12:] + x[H - 12:, W - 12:] + t) % 2)
    return out.round().clamp(0, 255).to(torch.uint8)


def to_pm1(u8: torch.Tensor) -> torch.Tensor:
    return u8.float() / 127.5 - 1.0


def reference(dtype):
    sys.dont_write_bytecode = True
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    from demo_utils.taehv import TAEHV
    m = TAEHV(checkpoint_path=None)
    sd = tw.synth_taehv_encoder_state_dict(SEED)
    missing, unexpected = m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("decoder.") for k in missing), (missing, unexpected)
    names = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if k.startswith("encoder.")]
    return m.eval().requires_grad_(False).to(dtype), names


def encode(m, x_pm1, dtype) -> np.ndarray:
    with torch.no_grad():
        z = m.encode_video((0.5 * x_pm1 + 0.5)[None].to(dtype), parallel=True, show_progress_bar=False)
    return z[0].float().numpy()          # [T/4, 16, H/8, W/8]


def rel_frames(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.array([np.linalg.norm(a[t] - b[t]) / np.linalg.norm(b[t]) for t in range(b.shape[0])])


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    m32, names = reference(torch.float32)
    m16, _ = reference(torch.bfloat16)
    assert names == list(tw.taehv_encoder_param_shapes().items())
    for i, (tag, kind, (T, H, W)) in enumerate(CASES):
        if tag == "480p" and "--small-only" in sys.argv:
            continue
        pix_seed = 3000 + SEED + i
        u8 = pixels_u8(kind, pix_seed, T, H, W)
        x = to_pm1(u8)
        f32, b16 = encode(m32, x, torch.float32), encode(m16, x, torch.bfloat16)
        assert f32.shape == (T // 4, 16, H // 8, W // 8)
        floor = rel_frames(b16, f32)
        extra = {}
        if tag == "a":
            extra = dict(encoder_keys=np.array([k for k, _ in names]), encoder_shapes=np.array([",".join(map(str, s)) for _, s in names]))
        if tag == "480p":
            extra = dict(pixels_crc32=np.int64(zlib.crc32(u8.numpy().tobytes())))
        else:
            extra["pixels_u8"] = u8.numpy()
        np.savez_compressed(os.path.join(OUT, f"taehv_enc_{tag}.npz"), seed=np.int64(SEED), kind=np.array(kind), pixel_seed=np.int64(pix_seed),
                            shape=np.array([T, H, W], dtype=np.int64), latent_f32=f32.astype(np.float16), ref_bf16_rel_err_frame=floor, **extra)
        print(f"taehv_enc_{tag} ({kind} {T}x{H}x{W}): latent {f32.shape} mean {f32.mean():.3f} std {f32.std():.3f}; reference bf16 per latent frame "
              + " ".join(f"{e:.2e}" for e in floor), flush=True)


if __name__ == "__main__":
    main()
