"""Generate the CLIP image-encoder golden fixtures by running the REFERENCE on the CPU (build container only).

TEST INFRASTRUCTURE, like tools/make_golden_taehv.py (nothing under oracle/ is touched): imports `wan/modules/clip.py`
from the reference checkout through `oracle.ref_shim` (torchvision and the tokenizer module are not installed here and are
replaced by empty stand-ins; the only thing used from torchvision, `T.Normalize`, is `(x - mean) / std`), builds its
`VisionTransformer(pool_type='token', pre_norm=True, activation='gelu')`, loads `synth_clip_state_dict(shape, SEED)` with
`strict=True`, and runs `CLIPModel.visual` (preprocessing + tower, `use_31_block=True`) on seeded frames in float32 and
again under `torch.autocast('cpu', dtype=torch.bfloat16)`.  The autocast run's distance from the fp32 run is the noise
floor the GPU tolerances are taken from.  Weights and frames are never stored: both sides regenerate them from seeds.

    tests/golden/clip_reduced_17.npz    CLIP_REDUCED at image_size 56 (17 tokens), 2 frames of 40 x 72; out float32
    tests/golden/clip_reduced_257.npz   CLIP_REDUCED at image_size 224 (257 tokens), a 40 x 72 and a 480 x 832 frame; float32
    tests/golden/clip_w1280_l16.npz     dim 1280, 16 heads, 16 layers (15 run), 257 tokens, 1 frame of 96 x 160; float16
    tests/golden/clip_pipeline_mask.npz the first-frame mask of `encode_image` (causal_diffusion_inference.py:160-164) for
                                        5 frames of 128 x 128 (see mask_fixture: those lines do not run as written)

Each tower fixture holds: the shape's fields, the weight seed, one row (seed, T, H, W) per video, the reference's
state-dict names and shapes, `out`, and the autocast run's relative Frobenius error, whole and per frame.

Usage: python tools/make_golden_clip.py [--mask-only]
"""
from __future__ import annotations

import dataclasses
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from self_forcing_amd import clip_weights as cw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 0
CASES = (
    ("clip_reduced_17", dataclasses.replace(cw.CLIP_REDUCED, image_size=56), ((101, 2, 40, 72),), np.float32),
    ("clip_reduced_257", cw.CLIP_REDUCED, ((102, 1, 40, 72), (103, 1, 480, 832)), np.float32),
    ("clip_w1280_l16", dataclasses.replace(cw.CLIP_VIT_H_14, num_layers=16), ((104, 1, 96, 160),), np.float16),
)


def reference_modules():
    from oracle import ref_shim
    ns = ref_shim.load()
    for name in ("torchvision", "torchvision.transforms", "wan.modules.tokenizers"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["wan.modules.tokenizers"].HuggingfaceTokenizer = object
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    import wan.modules.clip as rc
    # flash_attention asserts a CUDA device; the reference's own CPU fallback in the dtype of its inputs
    rc.flash_attention = lambda q, k, v, **kw: ns.attention_mod.attention(q, k, v, dtype=q.dtype)
    return rc


def reference_clip(rc, s: cw.ClipVisionShape, sd):
    vit = rc.VisionTransformer(image_size=s.image_size, patch_size=s.patch_size, dim=s.dim, mlp_ratio=s.mlp_ratio, out_dim=s.out_dim,
                               num_heads=s.num_heads, num_layers=s.num_layers, pool_type="token", pre_norm=True, post_norm=False,
                               activation="gelu", norm_eps=s.eps)
    vit.load_state_dict({k[len(cw.PREFIX):]: v.float() for k, v in sd.items()}, strict=True)
    vit = vit.eval().requires_grad_(False)
    names = [(k, tuple(v.shape)) for k, v in vit.state_dict().items()]
    m = rc.CLIPModel.__new__(rc.CLIPModel)
    m.dtype = torch.float32
    m.model = types.SimpleNamespace(image_size=s.image_size, visual=vit)
    mean, std = torch.tensor(cw.CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(cw.CLIP_STD).view(1, 3, 1, 1)
    m.transforms = types.SimpleNamespace(transforms=[lambda x: (x - mean) / std])
    return m, names


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def mask_fixture():
    """The first-frame mask of `encode_image` for 5 frames of 128 x 128.  The reference's own lines cannot produce it: :163
    views the [1, F + 3, h, w] mask as [1, (F + 3) / 4, 4, 4, h, w], one factor of 4 too many, and raises for every input
    (checked here), as does the `visual([image])` call of :159 on a [1, 3, H, W] tensor.  So this is the computation those
    lines state once the stray factor is dropped, written out per element: pixel frame 0 is known (1), every later one is
    not (0); frame 0 is repeated 4 times so that the F + 3 entries fold into (F + 3) / 4 latent frames of 4 channels, channel
    c of latent frame t being entry 4 t + c."""
    frames, height, width = 5, 128, 128
    entries = [1.0] * 4 + [0.0] * (frames - 1)
    lat_t = len(entries) // 4
    mask = np.zeros((4, lat_t, height // 8, width // 8), dtype=np.float32)
    for t in range(lat_t):
        for c in range(4):
            mask[c, t] = entries[4 * t + c]
    np.savez_compressed(os.path.join(OUT, "clip_pipeline_mask.npz"), num_frames=np.int64(frames), height=np.int64(height), width=np.int64(width),
                        mask=mask)
    print("clip_pipeline_mask:", mask.shape, "mask sum", float(mask.sum()))


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--mask-only" in sys.argv:
        return mask_fixture()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rc = reference_modules()
    for tag, s, videos, store in CASES:
        sd = cw.synth_clip_state_dict(s, SEED)
        m, names = reference_clip(rc, s, sd)
        assert names == [(k[len(cw.PREFIX):], v) for k, v in cw.clip_param_shapes(s).items()], "clip_param_shapes is out of step with the reference"
        del sd
        clips = [cw.synth_frames(*v) for v in videos]
        with torch.no_grad():
            f32 = m.visual([c.clone() for c in clips]).float()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                b16 = m.visual([c.clone() for c in clips]).float()
        assert f32.shape == (sum(v[1] for v in videos), s.seq_len, s.dim)
        np.savez_compressed(
            os.path.join(OUT, tag + ".npz"), seed=np.int64(SEED), videos=np.array(videos, dtype=np.int64),
            shape_fields=np.array(list(s.as_dict().keys())), shape_values=np.array([float(v) for v in s.as_dict().values()]),
            state_keys=np.array([k for k, _ in names]), state_shapes=np.array([",".join(map(str, shp)) for _, shp in names]),
            out=f32.numpy().astype(store), floor=np.float64(rel(b16, f32)),
            floor_frame=np.array([rel(b16[i], f32[i]) for i in range(f32.shape[0])]))
        print(f"{tag}: out {tuple(f32.shape)} std {f32.std():.3f} absmax {f32.abs().max():.2f}; reference autocast-bf16 vs fp32 {rel(b16, f32):.3e}", flush=True)
        del m
    mask_fixture()


if __name__ == "__main__":
    main()
