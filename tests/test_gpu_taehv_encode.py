"""GPU parity of the TAEHV tiny encoder against the reference's `TAEHV.encode_video` recorded by
`tools/make_golden_taehv_encode.py` (seeded weights, fp32 run = the truth, bf16 run = the noise floor per latent frame):

- whole encode of 8 x 16 x 24 (every stage below one 128-row tile), 12 x 104 x 168 (ragged tiles at every stage, the
  histories cross twice), 8 x 40 x 72 (structured pixels) and 8 x 480 x 832 (production geometry), every latent value,
  tolerance 1.5 x the reference's own bf16 figure on the same latent frame;
- carried state: every frames_per_call, uneven pieces and a reset are bit-identical to the one-shot encode, two frame
  sizes and two HIP streams stay independent;
- the wrapper contract (T = 1 + 4k, the first frame fills the first group) and a reduced pipeline run that starts from
  an encoded image;
- the stem, the three strided convolutions and the head at production geometry, per kernel against fp32 torch on the
  same bf16 operands, overall and per 16 x 16 patch.

Run with `-m gpu` (`-s` shows the measured figures).

Measured on one MI355X: no GPU run of this file is on record yet.  The reference's own bf16 run, which sets the bounds: per
latent frame 7.2e-3..8.8e-3 at all four sizes (8.4e-3, 8.8e-3 at 480 x 832)."""
import os
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import ops, taehv_weights as tw

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
FLOOR_MARGIN = 1.5  # x the reference bf16 run's own error on the same latent frame (test_gpu_taehv.py)
CONV_TOL = 4e-3     # per-kernel contract of the convolutions (test_gpu_vae.py, test_gpu_taehv.py)
PATCH_TOL = 1e-2    # ... and of every 16 x 16 output patch of them


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def block_rel(out, ref, bh=16, bw=16):
    """[T, H, W, C] volumes -> rel-Frobenius error of every bh x bw patch of every frame."""
    d = (out.double() - ref.double()).pow(2).sum(-1)
    r = ref.double().pow(2).sum(-1)
    T, H, W = d.shape
    ph, pw = -(-H // bh), -(-W // bw)

    def fold(t):
        return F.pad(t, (0, pw * bw - W, 0, ph * bh - H)).reshape(T, ph, bh, pw, bw).sum((2, 4))

    return (fold(d) / fold(r).clamp_min(1e-30)).sqrt()


def check_kernel(name, out, ref):
    overall = rel(out, ref)
    patches = block_rel(out, ref)
    worst = patches.max().item()
    print(f"\n{name}: rel {overall:.2e}, worst of {patches.numel()} 16x16 patches {worst:.2e}", end="")
    assert overall < CONV_TOL
    bad = (patches > PATCH_TOL).nonzero().tolist()
    assert not bad, f"{len(bad)} patches (t, row, col) above {PATCH_TOL}, e.g. {bad[:4]}; worst {worst:.3e}"


# ======================================================================================= whole encode vs the goldens
def golden_pixels(g):
    """The fixture's uint8 pixels [T, 3, H, W] (the 480 x 832 case: regenerated from its seed, CRC-checked) as x in [-1, 1]."""
    T, H, W = (int(v) for v in g["shape"])
    if "pixels_u8" in g:
        u8 = torch.from_numpy(g["pixels_u8"])
    else:
        assert str(g["kind"]) == "noise"
        u8 = torch.randint(0, 256, (T, 3, H, W), generator=torch.Generator().manual_seed(int(g["pixel_seed"])), dtype=torch.uint8)
        assert zlib.crc32(u8.numpy().tobytes()) == int(g["pixels_crc32"])
    assert tuple(u8.shape) == (T, 3, H, W)
    return u8.float() / 127.5 - 1.0


@pytest.mark.parametrize("tag,shape", [("a", (8, 16, 24)), ("b", (12, 104, 168)), ("c", (8, 40, 72)), ("480p", (8, 480, 832))],
                         ids=["8x16x24", "12x104x168", "8x40x72-structured", "8x480x832"])
def test_encode_against_the_reference(tag, shape):
    """Per latent frame the rel-Frobenius error vs the fp32 reference within 1.5 x the reference bf16 run's on that frame."""
    g = np.load(os.path.join(GOLD, f"taehv_enc_{tag}.npz"))
    x = golden_pixels(g)
    T, H, W = shape
    assert tuple(x.shape) == (T, 3, H, W)
    enc = sfa.TAEHVEncoder(tw.synth_taehv_encoder_state_dict(int(g["seed"])), device=DEV, frames_per_call=2)
    out = enc.encode(x.to(DEV))
    assert out.shape == (T // 4, 16, H // 8, W // 8) and out.dtype == torch.float32
    gold = torch.from_numpy(g["latent_f32"].astype(np.float32))
    errs = [rel(out[t].cpu(), gold[t]) for t in range(out.shape[0])]
    floor = g["ref_bf16_rel_err_frame"]
    assert len(floor) == len(errs) == T // 4                                # no frame is skipped
    print(f"\nTAEHV encode {shape}: HIP per latent frame " + " ".join(f"{e:.2e}" for e in errs) + "\n  reference bf16: " + " ".join(f"{e:.2e}" for e in floor))
    for t, e in enumerate(errs):
        assert e <= FLOOR_MARGIN * floor[t], f"latent frame {t}: rel err {e:.4f}, reference bf16 run {floor[t]:.4f}"


# ================================================================================================= carried state
@pytest.fixture(scope="module")
def small():
    sd = tw.synth_taehv_encoder_state_dict(5)
    x = (torch.rand(16, 3, 24, 40, generator=torch.Generator().manual_seed(78)) * 2 - 1).to(DEV)
    enc = sfa.TAEHVEncoder(sd, device=DEV, frames_per_call=4)
    return sd, x, enc, enc.encode(x)


@pytest.mark.parametrize("fpc", [1, 2, 3])
def test_frames_per_call_is_bit_identical(small, fpc):
    sd, x, _, ref = small
    assert ref.shape == (4, 16, 3, 5)
    assert torch.equal(sfa.TAEHVEncoder(sd, device=DEV, frames_per_call=fpc).encode(x), ref)


def test_uneven_pieces_and_reset(small):
    sd, x, enc, ref = small
    enc.clear_cache()
    pieces = torch.cat([enc.cached_encode(x[a:b]) for a, b in ((0, 4), (4, 12), (12, 16))])
    assert torch.equal(pieces, ref)
    warm = enc.cached_encode(x[4:12])                          # memory NOT cleared: frames 4..11 after frame 15 differ
    assert not torch.equal(warm, ref[1:3])
    enc.clear_cache()
    cold = enc.cached_encode(x[4:12])                          # the memory matters: a fresh one gives other latents
    assert not torch.equal(cold, ref[1:3]) and not torch.equal(cold, warm)
    assert torch.equal(enc.encode(x), ref) and torch.equal(enc.encode(x), ref)        # reset really resets; run-to-run
    # both pixel layouts and dtypes' plumbing: [3, T, H, W] with a channel stride, and bf16 pixels
    cf = torch.zeros(3, 20, 24, 40, device=DEV)
    cf[:, 2:18] = x.transpose(0, 1)
    assert torch.equal(enc.encode(cf[:, 2:18], channels_first=True), ref)
    xb = x.to(torch.bfloat16)
    assert torch.equal(enc.encode(xb), enc.encode(xb.float()))
    with pytest.raises(ValueError):
        enc.cached_encode(x[:6])
    with pytest.raises(ValueError):
        enc.cached_encode(x[:4, :, :20])


def test_two_frame_sizes_stream_independently(small):
    sd, x, _, ref = small
    enc = sfa.TAEHVEncoder(sd, device=DEV)
    other = (torch.rand(8, 3, 16, 48, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV)
    ref_o = sfa.TAEHVEncoder(sd, device=DEV).encode(other)
    a0 = enc.cached_encode(x[:8])
    o0 = enc.cached_encode(other[:4])
    a1 = enc.cached_encode(x[8:])
    o1 = enc.cached_encode(other[4:])
    assert torch.equal(torch.cat([a0, a1]), ref) and torch.equal(torch.cat([o0, o1]), ref_o)


def test_second_stream_beside_another_encoder(small):
    sd, x, enc, ref = small
    other = sfa.TAEHVEncoder(sd, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = other.encode(x)
    a = enc.encode(x)
    torch.cuda.synchronize()
    assert torch.equal(a, ref) and torch.equal(b, ref)


# ========================================================================================== wrapper and pipeline
@pytest.fixture(scope="module")
def full_sd():
    return {**tw.synth_taehv_state_dict(5), **tw.synth_taehv_encoder_state_dict(5)}


def test_wrapper_encode_contract(full_sd):
    vae = sfa.TAEHVWrapper(full_sd, device=DEV)
    x = (torch.rand(2, 3, 5, 48, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(DEV)
    z = vae.encode_to_latent(x)
    assert z.shape == (2, 2, 16, 6, 8) and z.dtype == torch.float32
    enc = sfa.TAEHVEncoder(full_sd, device=DEV)
    for b in range(2):                                                      # the first frame fills the first group of four
        padded = torch.cat([x[b, :, :1]] * 3 + [x[b]], dim=1)
        assert torch.equal(z[b], enc.encode(padded, channels_first=True))
    assert torch.equal(vae.encode_to_latent(x[1:])[0], z[1])                # per-sample independent
    assert not torch.equal(z[0], z[1])
    with pytest.raises(ValueError, match="1 \\+ 4k"):
        vae.encode_to_latent(x.new_zeros(1, 3, 6, 48, 64))
    with pytest.raises(ValueError):
        vae.encode_to_latent(x.new_zeros(1, 3, 5, 44, 64))
    pix = vae.decode_to_pixel(vae.encode_to_latent(x))
    assert pix.shape == (2, 5, 3, 48, 64)                                   # x's frame count and size
    # .model.clear_cache() clears both halves: a cached encode after it equals the one-shot encode
    vae.encoder.cached_encode(x[0, :, 1:], channels_first=True)
    vae.model.clear_cache()
    assert torch.equal(vae.encoder.cached_encode(torch.cat([x[0, :, :1]] * 3 + [x[0]], dim=1), channels_first=True), z[0])
    vae.model.clear_cache()
    # decoder-only state dicts keep raising, and say what is missing
    with pytest.raises(NotImplementedError, match="encoder.0.weight"):
        sfa.TAEHVWrapper(tw.synth_taehv_state_dict(5), device=DEV).encode_to_latent(x)


def test_pipeline_starts_from_an_encoded_image(full_sd):
    H, W = 8, 12
    g = torch.Generator().manual_seed(43)
    noise = torch.randn(1, 4, 16, H, W, generator=g).to(torch.bfloat16).to(DEV)
    pe = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    img = (torch.rand(1, 3, 1, 8 * H, 8 * W, generator=g) * 2 - 1).to(DEV)
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=True,
                           num_frame_per_block=2, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0), timestep_shift=5.0,
                                  is_causal=True, device=DEV)
    vae = sfa.TAEHVWrapper(full_sd, device=DEV)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=vae)
    initial = vae.encode_to_latent(img).to(torch.bfloat16)
    assert initial.shape == (1, 1, 16, H, W)
    video, lat = pipe.inference(noise, ["p"], initial_latent=initial, return_latents=True)
    assert lat.shape == (1, 5, 16, H, W) and torch.equal(lat[:, :1], initial)      # causal_inference.py:142
    assert video.shape == (1, 17, 3, 8 * H, 8 * W) and bool(torch.isfinite(video).all())


# ======================================================================================= per kernel, 480 x 832 geometry
@pytest.fixture(scope="module")
def stem_case():
    """2 frames of 480 x 832 in [-1, 1] (values on the bf16 grid, so that both pixel dtypes carry the same numbers) and
    the fp32 torch statement on the operands the kernel multiplies: u = bf16(0.5 x + 0.5), bf16 weights."""
    g = torch.Generator().manual_seed(480)
    x = (torch.rand(3, 2, 480, 832, generator=g) * 2 - 1).to(torch.bfloat16)
    w = bf((64, 3, 3, 3), g, 27 ** -0.5)
    b = bf((64,), g, 0.1)
    u = (0.5 * x.float() + 0.5).to(torch.bfloat16).float()
    pre = F.conv2d(u.transpose(0, 1), w.float(), b.float(), padding=1)                      # [2, 64, H, W]
    zeros = float((pre <= 0).float().mean())
    assert 0.2 <= zeros <= 0.8, zeros                                                       # the ReLU is exercised
    return x, w, b, F.relu(pre).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype,lead", [(torch.float32, 0), (torch.float32, 3), (torch.bfloat16, 0), (torch.bfloat16, 3)],
                         ids=["f32", "f32-lead3", "bf16", "bf16-lead3"])
def test_stem_at_production_geometry(stem_case, dtype, lead):
    x, w, b, ref = stem_case
    out = ops.taehv_encode_stem(x.to(dtype).to(DEV), tw.repack_stem(w).to(DEV), b.to(DEV), lead=lead)
    assert out.shape == (lead + 2, 480, 832, 64) and out.dtype == torch.bfloat16
    check_kernel(f"stem {str(dtype)[6:]} lead {lead}", out, ref[[max(t - lead, 0) for t in range(lead + 2)]].to(DEV))


@pytest.mark.parametrize("hin,win,kt", [(480, 832, 2), (240, 416, 2), (120, 208, 1)], ids=["480x832-kt2", "240x416-kt2", "120x208-kt1"])
def test_strided_conv_at_production_geometry(hin, win, kt):
    """One output frame; the weights are the FOLDED ones (TPool into the 3x3, fp32, rounded once to bf16), which both
    sides multiply."""
    g = torch.Generator().manual_seed(hin + kt)
    x = bf((kt, hin, win, 64), g)
    tpool = bf((64, 64 * kt, 1, 1), g, (64 * kt) ** -0.5)
    conv = bf((64, 64, 3, 3), g, 576 ** -0.5)
    taps = tw.tpool_taps(tw.fold_tpool(tpool, conv), kt).to(torch.bfloat16)                 # [64, 64, kt, 3, 3]
    ref = F.conv3d(F.pad(x.float().permute(3, 0, 1, 2)[None], (1, 1, 1, 1, 0, 0)), taps.float(), stride=(kt, 2, 2))[0].permute(1, 2, 3, 0).contiguous()
    out = ops.taehv_down_conv(x.to(DEV), tw.repack_taehv_conv(taps).to(DEV), kt)
    assert out.shape == ref.shape == (1, hin // 2, win // 2, 64)
    check_kernel(f"strided conv {hin}x{win} kt {kt}", out, ref.to(DEV))


def test_head_at_production_geometry():
    g = torch.Generator().manual_seed(17)
    x = bf((1, 60, 104, 64), g)
    w = bf((16, 64, 1, 3, 3), g, 576 ** -0.5)
    b = bf((16,), g, 0.1)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float()[:, :, 0], b.float(), padding=1)   # [1, 16, 60, 104]
    out = ops.taehv_conv(x.to(DEV), tw.repack_taehv_conv(w).to(DEV), b.to(DEV), 1, 1, epilogue="latent_f32")
    assert out.shape == ref.shape and out.dtype == torch.float32
    check_kernel("head 60x104", out.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1).to(DEV))
