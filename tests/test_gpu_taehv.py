"""GPU parity of the TAEHV tiny decoder against the reference's `TAEHV.decode_video` recorded by
`tools/make_golden_taehv.py` (seeded weights, fp32 run = the truth, bf16 run = the noise floor per pixel frame):

- whole decode at small ragged sizes (full resolution) and at 60 x 104 latents = 480 x 832 pixels (stride-4 subsample,
  per-(frame, channel) moments, full-resolution crops), tolerance 1.5 x the reference's own bf16 figure per frame;
- carried state: chunks, uneven pieces and every frames_per_call are bit-identical to the one-shot decode;
- the wrapper contract and a reduced pipeline run with `TAEHVWrapper` injected;
- every convolution the sequencer issues at 60 x 104, per kernel against fp32 torch, overall and per 16 x 16 patch;
- the MemBlock's first convolution against the Wan VAE's implicit-GEMM kernel (kt = 3, zero oldest tap).
- kt = 1 against the Wan VAE's implicit-GEMM kernel, bit for bit: the property that lets both kernels share one core.

All comparisons of the whole decode are on y = (out + 1) / 2, the decoder's own output (the `- 1` offset would
flatter a relative error).  Run with `-m gpu` (`-s` shows the measured figures).

Measured on one MI355X: 480 x 832 per pixel frame 6.7e-3..1.40e-2 (the reference's bf16 run on the same samples
7.7e-3..1.56e-2: under the floor on every frame), small sizes 6.7e-3..1.32e-2 (7.6e-3..1.40e-2); moments: mean within 8.3e-3,
rms within 4.9e-3 of the reference rms; crops max-abs 1.5..1.8e-2 (1.7..2.1e-2), worst error / bound 0.47; every kernel
rel 1.66e-3, worst 16 x 16 patch 1.71e-3, head max-abs 4.7e-6; kt = 2 vs conv_igemm(kt = 3, zero tap): bit-identical."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import ops, taehv_weights as tw
from self_forcing_amd.vae import repack_conv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
FLOOR_MARGIN = 1.5  # x the reference bf16 run's own error on the same frame (the Wan decode contract's margin: 2e-2 vs 1.14-1.62e-2)
CONV_TOL = 4e-3     # per-kernel contract of the convolutions (test_gpu_vae.py)
PATCH_TOL = 1e-2    # ... and of every 16 x 16 output patch of them
HEAD_TOL = 2e-2     # max-abs of the 3-channel float head
CROSS_TOL = 1e-3    # new kernel vs conv_igemm on the same sums (one bf16 step on a small share of elements)
LAT_H, LAT_W = 60, 104


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def block_rel(out, ref, bh=16, bw=16):
    d = (out.double() - ref.double()).pow(2).sum(-1)
    r = ref.double().pow(2).sum(-1)
    T, H, W = d.shape
    ph, pw = -(-H // bh), -(-W // bw)

    def fold(t):
        return F.pad(t, (0, pw * bw - W, 0, ph * bh - H)).reshape(T, ph, bh, pw, bw).sum((2, 4))

    return (fold(d) / fold(r).clamp_min(1e-30)).sqrt()


def latent_of(g):
    return torch.from_numpy(g["latent_bf16_bits"].view(np.int16)).view(torch.bfloat16)


# ==================================================================================== whole decode, small ragged sizes
@pytest.mark.parametrize("tag,shape", [("a", (5, 16, 6, 8)), ("b", (2, 16, 13, 21))], ids=["5x6x8", "2x13x21"])
def test_decode_small_sizes_full_resolution(tag, shape):
    """5 latent frames of 6 x 8 (below one 128-row tile at the first stage) and 2 of 13 x 21 (ragged tiles at every
    stage), every pixel: per pixel frame the rel-Frobenius error of y vs the fp32 reference within 1.5 x the reference
    bf16 run's on that frame."""
    g = np.load(os.path.join(GOLD, f"taehv_small_{tag}.npz"))
    lat = latent_of(g)
    assert tuple(lat.shape) == shape
    dec = sfa.TAEHVDecoder(tw.synth_taehv_state_dict(int(g["seed"])), device=DEV)
    out = dec.decode(lat.to(DEV))
    assert out.shape == (4 * shape[0], 3, 8 * shape[2], 8 * shape[3]) and out.dtype == torch.float32
    y = ((out + 1) / 2).cpu()
    gold = torch.from_numpy(g["y_f32"].astype(np.float32))
    errs = [rel(y[t], gold[t]) for t in range(y.shape[0])]
    floor = g["ref_bf16_rel_err_frame"]
    print(f"\nTAEHV {shape}: HIP per frame " + " ".join(f"{e:.2e}" for e in errs) + "\n  reference bf16: " + " ".join(f"{e:.2e}" for e in floor))
    for t, e in enumerate(errs):
        assert e <= FLOOR_MARGIN * floor[t], f"pixel frame {t}: rel err {e:.4f}, reference bf16 run {floor[t]:.4f}"


# ======================================================================================== whole decode at 480 x 832
@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(GOLD, "taehv_480p.npz")))
    subs = [np.load(os.path.join(GOLD, f"taehv_480p_sub{i}.npz")) for i in range(3)]
    assert [int(s["first_frame"]) for s in subs] == [0, 4, 8]
    g["sub"] = np.concatenate([s["y_f32_sub"] for s in subs])
    g["ref_bf16_sub_rel_err_frame"] = np.concatenate([s["ref_bf16_sub_rel_err_frame"] for s in subs])
    g["stride"] = int(subs[0]["stride"])
    return g


@pytest.fixture(scope="module")
def decoded(golden):
    lat = latent_of(golden).to(DEV)
    assert lat.shape == (3, 16, LAT_H, LAT_W)
    dec = sfa.TAEHVDecoder(tw.synth_taehv_state_dict(int(golden["seed"])), device=DEV)
    out = dec.decode(lat)
    torch.cuda.synchronize()
    assert out.shape == (12, 3, 8 * LAT_H, 8 * LAT_W)
    return dec, lat, out


def test_decode_480p_subsample_per_frame(golden, decoded):
    _, _, out = decoded
    s = golden["stride"]
    y = ((out[:, :, ::s, ::s].double() + 1) / 2).cpu()
    gold = torch.from_numpy(golden["sub"].astype(np.float64))
    assert y.shape == gold.shape == (12, 3, 120, 208)
    errs = [rel(y[t], gold[t]) for t in range(12)]
    floor = golden["ref_bf16_sub_rel_err_frame"]
    print(f"\nTAEHV 480x832 vs fp32 reference, stride-{s} subsample, per pixel frame: HIP " + " ".join(f"{e:.2e}" for e in errs)
          + "\n  reference bf16 run on the same samples: " + " ".join(f"{e:.2e}" for e in floor))
    for t, e in enumerate(errs):
        assert e <= FLOOR_MARGIN * floor[t], f"pixel frame {t}: rel err {e:.4f}, reference bf16 run {floor[t]:.4f}"


def test_decode_480p_moments_per_frame_and_channel(golden, decoded):
    """Mean and rms of every (pixel frame, channel) plane of y over all 399360 pixels (fp64 sums) against the fp32
    reference's, as a share of the reference rms, within that frame's bound (1.5 x the reference bf16 run's error)."""
    _, _, out = decoded
    n = 8 * LAT_H * 8 * LAT_W
    y = (out.double() + 1) / 2
    s1, s2 = y.sum((2, 3)).cpu().numpy(), y.pow(2).sum((2, 3)).cpu().numpy()
    rms_r = np.sqrt(golden["sumsq_f32"] / n)
    mean_err = np.abs(s1 - golden["sum_f32"]) / n / rms_r
    rms_err = np.abs(np.sqrt(s2 / n) - rms_r) / rms_r
    bound = FLOOR_MARGIN * golden["ref_bf16_rel_err_frame"][:, None]
    ref_mean = np.abs(golden["sum_bf16"] - golden["sum_f32"]) / n / rms_r
    ref_rms = np.abs(np.sqrt(golden["sumsq_bf16"] / n) - rms_r) / rms_r
    print(f"\nTAEHV 480x832 moments, worst (frame, channel): mean {mean_err.max():.2e} rms {rms_err.max():.2e} of the rms "
          f"(reference bf16 run: mean {ref_mean.max():.2e} rms {ref_rms.max():.2e})")
    assert (mean_err <= bound).all(), mean_err
    assert (rms_err <= bound).all(), rms_err


def test_decode_480p_full_resolution_crops(golden, decoded):
    """32 x 32 crops of every frame and channel at the four corners and across the centre tile seams: max-abs error of
    y vs fp32 <= 2 x the reference bf16 run's on the same crop + 1e-2."""
    _, _, out = decoded
    y = ((out.double() + 1) / 2).cpu()
    crops_f32 = golden["crops_f32"].astype(np.float64)
    ref_max = golden["crops_ref_bf16_max_abs"]
    worst = 0.0
    for k, (r, c) in enumerate(golden["crop_origins"]):
        err = (y[:, :, r:r + 32, c:c + 32] - torch.from_numpy(crops_f32[k])).abs().amax((2, 3)).numpy()
        bound = 2 * ref_max[k] + 1e-2
        worst = max(worst, float((err / bound).max()))
        print(f"\nTAEHV 480x832 crop at ({r:3d},{c:3d}): HIP max-abs {err.max():.2e} (reference bf16 run {ref_max[k].max():.2e})", end="")
        assert (err <= bound).all(), f"crop {k} at ({r}, {c}): max-abs {err.max():.4f}"
    print(f"\n  worst error / bound {worst:.2f}")


def test_decode_480p_chunks_equal_one_shot(decoded):
    dec, lat, out = decoded
    dec.clear_cache()
    a = dec.cached_decode(lat[:1])
    b = dec.cached_decode(lat[1:])
    dec.clear_cache()
    assert torch.equal(torch.cat([a, b]), out)


# ================================================================================================= carried state
@pytest.fixture(scope="module")
def small():
    sd = tw.synth_taehv_state_dict(5)
    g = torch.Generator().manual_seed(77)
    lat = torch.randn(7, 16, 6, 8, generator=g).to(torch.bfloat16).to(DEV)
    dec = sfa.TAEHVDecoder(sd, device=DEV, frames_per_call=7)
    return sd, lat, dec, dec.decode(lat)


@pytest.mark.parametrize("fpc", [1, 2, 3, 7])
def test_frames_per_call_is_bit_identical(small, fpc):
    sd, lat, _, ref = small
    assert torch.equal(sfa.TAEHVDecoder(sd, device=DEV, frames_per_call=fpc).decode(lat), ref)


def test_uneven_pieces_chunks_and_reset(small):
    sd, lat, dec, ref = small
    dec.clear_cache()
    pieces = torch.cat([dec.cached_decode(lat[a:b]) for a, b in ((0, 1), (1, 3), (3, 7))])
    assert torch.equal(pieces, ref)
    fresh = dec.cached_decode(lat[1:3])                        # memory NOT cleared: frames 1..2 after frame 6 differ
    assert not torch.equal(fresh, ref[4:12])
    dec.clear_cache()
    cold = dec.cached_decode(lat[1:3])                         # the memory matters: a fresh one gives other pixels
    assert rel(cold, ref[4:12]) > 0.05
    assert torch.equal(dec.decode(lat), ref) and torch.equal(dec.decode(lat), ref)        # reset really resets; run-to-run
    vae = sfa.TAEHVWrapper(sd, device=DEV)
    chunks = [vae.decode_chunk(lat[None, i:i + 3], i // 3) for i in (0, 3)]
    assert chunks[0].shape[1] == 9 and chunks[1].shape[1] == 12
    assert torch.equal(torch.cat(chunks, 1)[0], ref[3:24].clamp(-1, 1))


def test_two_latent_sizes_stream_independently(small):
    sd, lat, _, ref = small
    dec = sfa.TAEHVDecoder(sd, device=DEV)
    other = torch.randn(3, 16, 10, 6, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(DEV)
    ref_o = sfa.TAEHVDecoder(sd, device=DEV).decode(other)
    a0 = dec.cached_decode(lat[:2])
    o0 = dec.cached_decode(other[:1])
    a1 = dec.cached_decode(lat[2:])
    o1 = dec.cached_decode(other[1:])
    assert torch.equal(torch.cat([a0, a1]), ref) and torch.equal(torch.cat([o0, o1]), ref_o)


def test_second_stream_beside_another_decoder(small):
    sd, lat, dec, ref = small
    other = sfa.TAEHVDecoder(sd, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = other.decode(lat)
    a = dec.decode(lat)
    torch.cuda.synchronize()
    assert torch.equal(a, ref) and torch.equal(b, ref)


# ============================================================================================== wrapper contract
def test_wrapper_contract(small):
    sd, lat, _, ref = small
    vae = sfa.TAEHVWrapper(sd, device=DEV)
    out = vae.decode_to_pixel(lat[None, :3])
    assert out.shape == (1, 9, 3, 48, 64) and out.dtype == torch.float32
    assert float(out.abs().max()) <= 1.0 and float((ref[3:12].abs() > 1).float().mean()) > 0      # the clamp acts
    assert torch.equal(out[0], ref[3:12].clamp(-1, 1))                                             # first 3 frames dropped
    two = torch.stack([lat[:3], lat[2:5]])
    both = vae.decode_to_pixel(two)
    assert torch.equal(both[0], out[0]) and torch.equal(both[1], vae.decode_to_pixel(two[1:])[0])
    with pytest.raises(AssertionError):
        vae.decode_to_pixel(two, use_cache=True)
    with pytest.raises(NotImplementedError):
        vae.encode_to_latent(torch.zeros(1, 3, 1, 48, 64))
    vae.model.clear_cache()


def test_pipeline_stream_equals_inference_with_taehv():
    H, W = 8, 12
    g = torch.Generator().manual_seed(41)
    noise = torch.randn(1, 6, 16, H, W, generator=g).to(torch.bfloat16).to(DEV)
    pe = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    eps = [torch.randn(2, 16, H, W, generator=g).to(torch.bfloat16) for _ in range(9)]
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=2, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0), timestep_shift=5.0,
                                  is_causal=True, device=DEV)
    vae = sfa.TAEHVWrapper(tw.synth_taehv_state_dict(0), device=DEV)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=vae)
    q = list(eps)
    pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
    video, lat = pipe.inference(noise, ["p"], return_latents=True)
    video = video.clone()
    assert video.shape == (1, 21, 3, 8 * H, 8 * W)
    q.extend(eps)
    serial = [(i, x.clone(), p.clone()) for i, x, p in pipe.stream(noise, ["p"])]
    q.extend(eps)
    over = [(i, x.clone(), p.clone()) for i, x, p in pipe.stream(noise, ["p"], overlap_decode=True)]
    assert [c[2].shape[1] for c in serial] == [5, 8, 8]
    for chunks in (serial, over):
        assert torch.equal(torch.cat([c[1] for c in chunks], 1), lat)
        assert torch.equal(torch.cat([c[2] for c in chunks], 1), video)


# ===================================================================== every convolution at 60 x 104, per kernel
def production_convs(h=LAT_H, w=LAT_W):
    """The launches of `sf_taehv_decode_frames` at an h x w latent (`taehv_weights.decoder_convs` mirrors the sequencer),
    de-duplicated by (kt, cin, cout, H, W, up, tgrow, epilogue): {key: first layer name}."""
    out = {}
    for c in tw.decoder_convs(h, w, 1):
        out.setdefault((c["kt"], c["cin"], c["cout"], c["H"], c["W"], c["up"], c["tgrow"], c["epi"]), c["name"])
    return out


CONVS = production_convs()


def _conv_id(key):
    kt, cin, cout, H, W, up, tg, epi = key
    return f"{CONVS[key]}-kt{kt}-{cin}to{cout}-{H}x{W}" + ("-up" if up else "") + (f"-tgrow{tg}" if tg > 1 else "") + f"-{epi}"


def test_conv_list_covers_the_production_shapes():
    assert list(CONVS) == [
        (1, 32, 256, 60, 104, 0, 1, "bias_relu"),
        (2, 256, 256, 60, 104, 0, 1, "bias_relu"), (1, 256, 256, 60, 104, 0, 1, "bias_relu"), (1, 256, 256, 60, 104, 0, 1, "bias_resid_relu"),
        (1, 256, 128, 120, 208, 1, 1, "plain"),
        (2, 128, 128, 120, 208, 0, 1, "bias_relu"), (1, 128, 128, 120, 208, 0, 1, "bias_relu"), (1, 128, 128, 120, 208, 0, 1, "bias_resid_relu"),
        (1, 128, 128, 240, 416, 1, 2, "plain"),
        (2, 64, 64, 240, 416, 0, 1, "bias_relu"), (1, 64, 64, 240, 416, 0, 1, "bias_relu"), (1, 64, 64, 240, 416, 0, 1, "bias_resid_relu"),
        (1, 64, 128, 480, 832, 1, 2, "relu"),
        (1, 64, 3, 480, 832, 0, 1, "head_f32")]


def _reference(x, w, b, kt, up, tgrow, epi, resid):
    """fp32 torch statement in the kernel's output layout: x [T + kt - 1, Hin, Win, Cin] -> [tgrow T, H, W, Cout / tgrow]
    (head: [T, 3, H, W] = clamp(2 y - 1))."""
    xf = x.float().permute(3, 0, 1, 2)[None]
    if up:
        xf = F.interpolate(xf, scale_factor=(1.0, 2.0, 2.0), mode="nearest")
    y = F.conv3d(F.pad(xf, (1, 1, 1, 1, 0, 0)), w.float(), b.float() if b is not None else None)[0]      # [Cout, T, H, W]
    if epi == "head_f32":
        return (2 * y - 1).clamp(-1, 1).permute(1, 0, 2, 3).contiguous(), None
    c, T = y.shape[0] // tgrow, y.shape[1]
    y = y.reshape(tgrow, c, T, *y.shape[2:]).permute(2, 0, 3, 4, 1).reshape(T * tgrow, *y.shape[2:], c)
    if resid is not None:
        y = y + resid.float()
    pre = y
    return (F.relu(y) if epi != "plain" else y).contiguous(), pre


@pytest.mark.parametrize("key", list(CONVS), ids=_conv_id)
def test_conv_at_production_geometry_per_patch(key):
    kt, cin, cout, H, W, up, tg, epi = key
    T = 3 if H * W <= 120 * 208 else 1
    g = torch.Generator().manual_seed(cin * 7 + cout + H + kt)
    hin, win = (H // 2, W // 2) if up else (H, W)
    real_cin = 16 if cin == 32 else cin                                    # decoder.1: 16 latent channels padded to 32
    x = torch.zeros(T + kt - 1, hin, win, cin, dtype=torch.bfloat16)
    x[..., :real_cin] = bf((T + kt - 1, hin, win, real_cin), g)
    w = bf((cout, real_cin, kt, 3, 3), g, (3.0 if epi == "head_f32" else 1.0) * (real_cin * kt * 9) ** -0.5)
    b = bf((cout,), g, 0.1) if epi in ("bias_relu", "bias_resid_relu", "head_f32") else None
    resid = bf((T, H, W, cout), g) if epi == "bias_resid_relu" else None
    ref, pre = _reference(x[..., :real_cin], w, b, kt, up, tg, epi, resid)
    ref = ref.to(DEV)
    wd = tw.repack_taehv_conv(w, cin_pad=cin).to(DEV)
    out = ops.taehv_conv(x.to(DEV), wd, b.to(DEV) if b is not None else None, kt, T, epilogue=epi, upsample=bool(up),
                         resid=resid.to(DEV) if resid is not None else None, tgrow=tg, clamp=True)
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    if epi == "head_f32":
        assert float((ref.abs() >= 1).float().mean()) > 0.02                 # the clamp is exercised
        err = (out - ref).abs().max().item()
        print(f"\n{_conv_id(key)}: max-abs {err:.2e}", end="")
        assert err < HEAD_TOL
        return
    if epi != "plain":
        zeros = float((pre <= 0).float().mean())
        assert 0.2 <= zeros <= 0.8, zeros                                  # the ReLU is exercised
    overall = rel(out, ref)
    patches = block_rel(out, ref)
    worst = patches.max().item()
    print(f"\n{_conv_id(key)}: rel {overall:.2e}, worst of {patches.numel()} 16x16 patches {worst:.2e}", end="")
    assert overall < CONV_TOL
    bad = (patches > PATCH_TOL).nonzero().tolist()
    assert not bad, f"{len(bad)} patches (t, row, col) above {PATCH_TOL}, e.g. {bad[:4]}; worst {worst:.3e}"


@pytest.mark.parametrize("c,H,W", [(256, 60, 104), (128, 120, 208), (64, 240, 416)], ids=["256-60x104", "128-120x208", "64-240x416"])
def test_memblock_conv0_against_the_wan_vae_kernel(c, H, W):
    """An independent path for the kt = 2 convolution: the existing implicit GEMM with kt = 3 and a zero oldest tap (one
    more, unread, history frame in front), ReLU in torch.  Both round the same fp32 sums to bf16 and differ in k-order."""
    T = 2
    g = torch.Generator().manual_seed(c + H)
    x = bf((T + 1, H, W, c), g)
    w = bf((c, c, 2, 3, 3), g, (c * 18) ** -0.5)
    b = bf((c,), g, 0.1)
    new = ops.taehv_conv(x.to(DEV), tw.repack_taehv_conv(w).to(DEV), b.to(DEV), 2, T, epilogue="bias_relu")
    w3 = torch.cat([torch.zeros(c, c, 1, 3, 3, dtype=torch.bfloat16), w], 2)
    x3 = torch.cat([bf((1, H, W, c), g), x])
    old = F.relu(ops.conv_igemm(x3.to(DEV), repack_conv(w3).to(DEV), b.to(DEV), (3, 3, 3), T, structure="igemm"))
    d = rel(new, old)
    print(f"\nMemBlock conv.0 {c} ch {H}x{W}: new kernel vs conv_igemm(kt=3, zero tap) + relu: rel {d:.2e}", end="")
    assert d <= CROSS_TOL


@pytest.mark.parametrize("cin,cout,T,hin,win,up", [(64, 64, 2, 9, 14, False), (32, 128, 1, 5, 7, True)], ids=["plain-252rows", "upsample-9slices"])
def test_kt1_is_bit_identical_to_the_wan_vae_kernel(cin, cout, T, hin, win, up):
    """What lets the two kernels share one implicit-GEMM core: with kt = 1 both walk k in the same order into fp32
    accumulators, add the bias in fp32 and round once, and ReLU commutes with the rounding to bf16.  The plain case has two
    row tiles, the second partial (M = 252); the upsampled one both parities on both axes and an odd slice count (9: the
    padding slice).  The equality follows from the code; no GPU run of it is on record yet, neither with the kernels'
    own copies of the core nor with the shared one."""
    g = torch.Generator().manual_seed(cin + cout + hin)
    x = bf((T, hin, win, cin), g)
    w = bf((cout, cin, 1, 3, 3), g, (9 * cin) ** -0.5)
    b = bf((cout,), g, 0.1)
    new = ops.taehv_conv(x.to(DEV), tw.repack_taehv_conv(w).to(DEV), b.to(DEV), 1, T, epilogue="bias_relu", upsample=up)
    pre = ops.conv_igemm(x.to(DEV), repack_conv(w).to(DEV), b.to(DEV), (1, 3, 3), T, upsample=up, structure="igemm")
    zeros = float((pre <= 0).float().mean())
    print(f"\nkt = 1 {cin}->{cout} {tuple(pre.shape)}: {int((new != F.relu(pre)).sum())} differing elements, {zeros:.2f} non-positive", end="")
    assert 0.2 <= zeros <= 0.8, zeros                                      # the ReLU is exercised
    assert new.shape == pre.shape == (T, hin * (2 if up else 1), win * (2 if up else 1), cout)
    assert torch.equal(new, F.relu(pre))
