"""GPU tests of the CLIP image encoder (csrc/clip_encoder.hip): every new kernel against a CPU computation of the same
inputs, the encoder against the reference's recorded outputs, and `encode_image` of the pipeline.  Run with `-m gpu`."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import clip_reference as cr
from self_forcing_amd import clip_weights as cw
from self_forcing_amd import ops
from self_forcing_amd import vae_weights as vw

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
BF16_EPS = 2.0 ** -8
_cache = {}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def fixture(tag):
    """(npz, shape, device model, videos, recorded output): built once per tag, shared by the tests and left unchanged."""
    if tag not in _cache:
        g = np.load(os.path.join(GOLD, tag + ".npz"))
        s = cw.ClipVisionShape(**{str(k): (float(v) if k == "eps" else int(v)) for k, v in zip(g["shape_fields"], g["shape_values"])})
        model = sfa.CLIPModel(state_dict=cw.synth_clip_state_dict(s, int(g["seed"])), shape=s, device=DEV)
        videos = [cw.synth_frames(*(int(x) for x in v)) for v in g["videos"]]
        _cache[tag] = (g, s, model, videos, torch.from_numpy(g["out"].astype(np.float32)))
    return _cache[tag]


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("n,H,L", [(1, 1, 1), (2, 4, 17), (1, 4, 64), (1, 4, 65), (1, 16, 257)])
def test_attention_against_fp64(n, H, L):
    """Non-causal D = 80 attention of bf16 inputs against fp64 softmax attention of the same inputs.  Tolerance: twice the
    error torch's own bf16 SDPA makes on the CPU on these inputs against that fp64 result (another order of sums, P in bf16).
    qkv lies inside a NaN-filled allocation, the output between sentinel rows."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * H + L)
    qkv = torch.randn(n, L, 3, H, 80, generator=gen).bfloat16()
    pad = 4096
    big = torch.full((qkv.numel() + 2 * pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    big[pad:pad + qkv.numel()] = qkv.flatten().to(DEV)
    inner = big[pad:pad + qkv.numel()].view(n, L, 3, H, 80)
    guard = torch.full((n * L + 2, H * 80), 777.0, dtype=torch.bfloat16, device=DEV)
    out = ops.clip_attention(inner, out=guard[1:-1].view(n, L, H * 80))
    torch.cuda.synchronize()
    assert out.shape == (n, L, H * 80) and out.dtype == torch.bfloat16
    assert (guard[0] == 777.0).all() and (guard[-1] == 777.0).all()
    assert torch.isfinite(out.float()).all()
    q, k, v = (t.transpose(1, 2) for t in qkv.unbind(2))                         # [n, H, L, 80]
    ref = (torch.softmax(q.double() @ k.double().transpose(-1, -2) / math.sqrt(80.0), -1) @ v.double()).transpose(1, 2).reshape(n, L, H * 80)
    if L == 1:
        assert torch.equal(out.cpu(), qkv[:, :, 2].reshape(n, 1, H * 80))         # one key: the output is V, bit for bit
        return
    sdpa = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(n, L, H * 80)
    tol, err = 2.0 * rel(sdpa, ref), rel(out, ref)
    print(f"attention n={n} H={H} L={L}: gpu {err:.3e}, torch bf16 SDPA {tol / 2:.3e} (ratio {2 * err / tol:.3f})")
    assert err <= tol
    for b in range(n):                                                            # every (image, head) on its own
        for h in range(H):
            sl = (b, slice(None), slice(80 * h, 80 * h + 80))
            assert rel(out[sl], ref[sl]) <= 2.0 * rel(sdpa[sl], ref[sl])


def test_attention_rejects_what_does_not_fit():
    qkv = torch.zeros(1, 481, 3, 1, 80, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(sfa._lib.SfHipError, match="L=481"):
        ops.clip_attention(qkv)


# ------------------------------------------------------------------------------------------ add + LayerNorm
@pytest.mark.parametrize("dim", [320, 1280])
@pytest.mark.parametrize("M", [1, 257, 514])
def test_add_layernorm(M, dim):
    gen = torch.Generator().manual_seed(M + dim)
    x = torch.randn(M, dim, generator=gen) * 3.0 + 0.5
    x[0, 0] = 40.0                                                                # an outlier channel in the stream
    y = torch.randn(M, dim, generator=gen).bfloat16()
    w, b = 1.0 + 0.1 * torch.randn(dim, generator=gen), 0.1 * torch.randn(dim, generator=gen)
    want_x = x + y.float()
    want_n = F.layer_norm(want_x, (dim,), w, b, 1e-5).bfloat16()
    xd = x.to(DEV)
    xn = ops.clip_add_layernorm(xd, y.to(DEV), w.to(DEV), b.to(DEV))
    assert torch.equal(xd.cpu(), want_x)                                          # the fp32 add, bit for bit
    assert xn.dtype == torch.bfloat16 and xn.shape == (M, dim)
    err = rel(xn.float(), want_n.float())
    print(f"add+LN M={M} dim={dim}: xn rel {err:.3e}")
    assert err <= BF16_EPS
    assert max(rel(xn[r].float(), want_n[r].float()) for r in {0, M // 2, M - 1}) <= BF16_EPS
    # add only: the stream moves on, xn is not touched
    keep = torch.full((M, dim), 5.0, dtype=torch.bfloat16, device=DEV)
    assert ops.clip_add_layernorm(xd, y.to(DEV), None, None, xn=keep) is None
    assert torch.equal(xd.cpu(), want_x + y.float()) and (keep == 5.0).all()


def test_embed_norm():
    """cls / patch rows + position, pre_norm into the fp32 stream, norm1 into the bf16 copy."""
    n, P, dim = 2, 16, 320
    gen = torch.Generator().manual_seed(7)
    patch = torch.randn(n, P, dim, generator=gen).bfloat16()
    cls, pos = torch.randn(dim, generator=gen), torch.randn(P + 1, dim, generator=gen)
    w0, b0, w1, b1 = (f(torch.randn(dim, generator=gen)) for f in (lambda t: 1 + 0.1 * t, lambda t: 0.1 * t) * 2)
    x = torch.cat([cls.expand(n, 1, dim), patch.float()], 1) + pos
    want_x = F.layer_norm(x, (dim,), w0, b0, 1e-5)
    want_n = F.layer_norm(want_x, (dim,), w1, b1, 1e-5).bfloat16()
    x32, xn = ops.clip_embed_norm(patch.to(DEV), cls.to(DEV), pos.to(DEV), w0.to(DEV), b0.to(DEV), w1.to(DEV), b1.to(DEV))
    assert x32.dtype == torch.float32 and tuple(x32.shape) == (n, P + 1, dim)
    assert rel(x32, want_x) < 1e-6 and rel(xn.float(), want_n.float()) <= BF16_EPS
    x32b, none = ops.clip_embed_norm(patch.to(DEV), cls.to(DEV), pos.to(DEV), w0.to(DEV), b0.to(DEV), None, None)
    assert none is None and torch.equal(x32b, x32)


# ------------------------------------------------------------------------------------------ GELU
def test_gelu_is_the_erf_form_on_every_bf16_value():
    """Every bf16 value with |x| <= 4 (33 026 of them): within one bf16 ulp (of the exact result) + 2e-5 of the erf GELU
    in fp64.  The tanh form misses this at 119 values.  Further out fp32 `1 + erf` cancels, so the range stops at 4."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16)
    x = x[torch.isfinite(x.float()) & (x.float().abs() <= 4.0)]
    assert x.numel() == 33026
    padded = torch.zeros((x.numel() + 7) // 8 * 8, dtype=torch.bfloat16)
    padded[:x.numel()] = x
    out = ops.clip_gelu(padded.to(DEV)).cpu()[:x.numel()].double()
    xd = x.double()
    want = 0.5 * xd * torch.special.erfc(-xd / math.sqrt(2.0))
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want.abs().clamp_min(1e-300))[1] - 8)
    excess = (out - want).abs() - (ulp + 2e-5)
    print(f"gelu: worst excess over the bound {excess.max().item():.3e} at x = {xd[excess.argmax()].item()}")
    assert int((excess > 0).sum()) == 0
    tanh = F.gelu(x.float(), approximate="tanh").bfloat16().double()              # the check does tell the two forms apart
    assert int(((tanh - want).abs() > ulp + 2e-5).sum()) == 119


# ------------------------------------------------------------------------------------------ preprocessing
def _normalise(frames):
    mean, std = torch.tensor(cw.CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(cw.CLIP_STD).view(1, 3, 1, 1)
    return (frames * 0.5 + 0.5 - mean) / std


def test_preprocess_identity_size_is_normalisation_alone():
    frames = cw.synth_frames(11, 2, 224, 224).transpose(0, 1).contiguous()
    rows = ops.clip_preprocess(frames.to(DEV)).cpu()
    assert rows.shape == (2 * 256, 640) and rows.dtype == torch.bfloat16
    assert torch.equal(rows, cr.patch_rows(_normalise(frames), 14, 640).bfloat16())
    assert (rows[:, 588:] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(40, 72), (480, 832)])
def test_preprocess_resize_matches_interpolate(H, W, dtype):
    frames = cw.synth_frames(12 + H, 2, H, W).transpose(0, 1).contiguous().to(dtype)
    want = cr.patch_rows(_normalise(F.interpolate(frames.float(), size=(224, 224), mode="bicubic", align_corners=False)), 14, 640).bfloat16()
    rows = ops.clip_preprocess(frames.to(DEV)).cpu()
    err = rel(rows.float(), want.float())
    print(f"preprocess {H}x{W} {dtype}: rel {err:.3e}")
    assert err < BF16_EPS and (rows[:, 588:] == 0).all()
    assert rel(rows[256:].float(), want[256:].float()) < BF16_EPS                # the second frame on its own
    small = ops.clip_preprocess(frames[:1].to(DEV), image_size=56).cpu()          # another grid: 16 patches
    want56 = cr.patch_rows(_normalise(F.interpolate(frames[:1].float(), size=(56, 56), mode="bicubic", align_corners=False)), 14, 640).bfloat16()
    assert small.shape == (16, 640) and rel(small.float(), want56.float()) < BF16_EPS


# ------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("tag,factor", [("clip_reduced_17", 2.0), ("clip_reduced_257", 2.0), ("clip_w1280_l16", 1.5)])
def test_encoder_matches_the_reference(tag, factor):
    """Against the reference's recorded fp32 run, within `factor` x its own bf16-autocast error (the floor).  At width
    1280 and 15 blocks a bf16 residual stream lands at 1.7 x the floor and the reference's rounding points at 1.00 x, so
    1.5 x tells them apart."""
    g, s, model, videos, gold = fixture(tag)
    floor = float(g["floor"])
    out = model.visual(videos)
    assert tuple(out.shape) == tuple(gold.shape) == (sum(int(v[1]) for v in g["videos"]), s.seq_len, s.dim) and out.dtype == torch.float32
    err = rel(out, gold)
    print(f"{tag}: gpu vs reference fp32 {err:.3e} = {err / floor:.3f} x floor {floor:.3e}")
    assert err < factor * floor
    for i in range(gold.shape[0]):                                                # each frame on its own
        assert rel(out[i], gold[i]) < factor * floor
    # against the restatement under the reference's rounding points: the same arithmetic up to the order of sums
    if s.dim == 320:
        twin = cr.clip_visual_reference(cw.synth_clip_state_dict(s, int(g["seed"])), s, videos, "autocast_bf16")
        assert rel(out, twin) < factor * floor


def test_encoder_is_deterministic_and_batch_invariant():
    g, s, model, videos, _ = fixture("clip_reduced_17")
    clip = videos[0]                                                              # [3, 2, 40, 72]
    a, b = clip[:, :1].contiguous(), clip[:, 1:].contiguous()
    both = model.visual([clip])
    assert torch.equal(both, model.visual([clip]))                                # two calls
    assert torch.equal(both, model.visual([a, b]))                                # a list of videos = their frames in order
    assert torch.equal(both, torch.cat([model.visual([a]), model.visual([b])]))   # a frame alone = the frame in a batch
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = model.visual([clip])
    side.synchronize()
    assert torch.equal(both, other)
    g2, _, model2, videos2, _ = fixture("clip_reduced_257")
    assert torch.equal(model2.visual(videos2), torch.cat([model2.visual([v]) for v in videos2]))
    assert torch.equal(model2.visual([videos2[0].bfloat16()]), model2.visual([videos2[0].bfloat16().float()]))   # bf16 frames are read as they are


# ------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_encode_image():
    g = np.load(os.path.join(GOLD, "clip_pipeline_mask.npz"))
    frames, height, width = int(g["num_frames"]), int(g["height"]), int(g["width"])
    _, s, clip, _, _ = fixture("clip_reduced_17")
    vae = sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.VAE_REDUCED, seed=0, encoder=True), device=DEV, shape=vw.VAE_REDUCED)
    shape = sfa.WAN_REDUCED
    args = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, num_frame_per_block=1,
                           negative_prompt="NEG", guidance_scale=3.0)
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0), timestep_shift=5.0, is_causal=True, device=DEV)
    pipe = sfa.CausalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.SyntheticTextEncoder(text_len=shape.text_len, text_dim=shape.text_dim, device=DEV), vae=vae,
                                                image_encoder=clip)
    image = cw.synth_frames(21, 1, height, width)[:, 0]                           # [3, 128, 128]
    cond = pipe.encode_image(image.unsqueeze(0), frames, height, width)
    feat, y = cond["clip_feature"], cond["y"]
    assert tuple(feat.shape) == (1, s.seq_len, 320) and feat.dtype == torch.bfloat16
    assert torch.equal(feat, clip.visual([image.unsqueeze(1)]).bfloat16())
    assert tuple(y.shape) == (1, 20, 2, 16, 16) and y.dtype == torch.bfloat16
    assert torch.equal(y[0, :4].float().cpu(), torch.from_numpy(g["mask"]))
    video = torch.zeros(1, 3, frames, height, width, dtype=torch.bfloat16, device=DEV)
    video[0, :, 0] = image.to(DEV).bfloat16()
    latent = vae.encode_to_latent(video)                                          # [1, 2, 16, 16, 16]
    assert torch.equal(y[0, 4:], latent[0].transpose(0, 1).bfloat16())
    assert torch.equal(pipe.encode_image(image, frames, height, width)["y"], y)   # [3, H, W] is accepted too
    from PIL import Image
    pil = Image.fromarray(((image.permute(1, 2, 0) * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8).numpy())
    as_tensor = torch.from_numpy(np.array(pil, dtype=np.float32) * (2 / 255) - 1).permute(2, 0, 1)       # the 8-bit picture, scaled as :148
    from_pil, from_tensor = pipe.encode_image(pil, frames, height, width), pipe.encode_image(as_tensor, frames, height, width)
    assert torch.equal(from_pil["clip_feature"], from_tensor["clip_feature"]) and torch.equal(from_pil["y"], from_tensor["y"])
    small = pipe.encode_image(pil.resize((64, 64)), frames, height, width)       # a PIL image of another size is resized first
    assert tuple(small["y"].shape) == (1, 20, 2, 16, 16)
    noise = torch.zeros(1, 3, 16, 16, 16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(NotImplementedError, match="i2v branch"):
        pipe.inference(noise, ["p"], input_image=image, dwpose_data=None, random_ref_dwpose=None)
