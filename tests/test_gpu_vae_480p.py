"""GPU parity of the VAE at the production size, 60 x 104 latents = 480 x 832 pixels (the other VAE tests stop at 40 x 48):

- the whole decode against the reference's `WanVAE_.decode` recorded at 480 x 832 (`tools/make_golden_vae_decode_480p.py`),
  per pixel frame: a stride-4 subsample (16 samples in every 16 x 16 output patch), per-(frame, channel) moments, and
  full-resolution crops at the corners and across the centre patch seams; and the pipeline's streaming hook at that size;
- every convolution the decoder issues at a 60 x 104 latent, walked from `decoder_layout`, per kernel structure against
  fp32 torch, overall and per 16 x 16 output patch (one wrong patch among thousands barely moves the overall figure);
- the middle attention's row softmax and its two GEMMs at 60 x 104 = 6240 tokens (and 90 x 160 = 14400, the 720p
  latent), with the decoder's own strides;
- the encoder's strided convolutions at 480 x 832 input, walked from `encoder_layout`.

Run with `-m gpu` (`-s` shows the measured figures)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import ops, vae_weights as vw
from self_forcing_amd.vae import repack_conv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
TOL = 2e-2          # decode contract (test_gpu_vae.py): the reference's own bf16 run is 1.14-1.62e-2 per pixel frame here
CONV_TOL = 4e-3     # per-kernel contract of the convolutions (test_gpu_vae.py)
PATCH_TOL = 1e-2    # ... and of every 16 x 16 output patch of them
HEAD_TOL = 2e-2     # max-abs of the 3-channel float head (test_gpu_vae.py)
LAT_H, LAT_W = 60, 104
PIX_H, PIX_W = 8 * LAT_H, 8 * LAT_W


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def block_rel(out, ref, bh, bw):
    """rel-Frobenius error of every bh x bw block of positions: out, ref [T, H, W, C] (all channels of a position count
    in its block) -> [T, ceil(H / bh), ceil(W / bw)]; ragged edge blocks keep their true extent."""
    d = (out.double() - ref.double()).pow(2).sum(-1)
    r = ref.double().pow(2).sum(-1)
    T, H, W = d.shape
    ph, pw = -(-H // bh), -(-W // bw)

    def fold(t):
        return F.pad(t, (0, pw * bw - W, 0, ph * bh - H)).reshape(T, ph, bh, pw, bw).sum((2, 4))

    return (fold(d) / fold(r).clamp_min(1e-30)).sqrt()


# ============================================================================================ whole decode at 480 x 832
@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(GOLD, "vae_decode_480p.npz")))
    subs = [np.load(os.path.join(GOLD, f"vae_decode_480p_sub{i}.npz")) for i in (0, 1)]
    assert [int(s["first_frame"]) for s in subs] == [0, 5]
    g["sub"] = np.concatenate([s["pixels_f32_sub"] for s in subs])
    g["ref_bf16_sub_rel_err_frame"] = np.concatenate([s["ref_bf16_sub_rel_err_frame"] for s in subs])
    g["stride"] = int(subs[0]["stride"])
    return g


@pytest.fixture(scope="module")
def decoded(golden):
    sd = vw.synth_vae_state_dict(vw.WAN_VAE, seed=int(golden["seed"]))
    lat = torch.from_numpy(golden["latent_bf16_bits"].view(np.int16)).view(torch.bfloat16).to(DEV)
    assert lat.shape == (1, 3, 16, LAT_H, LAT_W)
    vae = sfa.WanVAEWrapper(sd, device=DEV)
    out = vae.decode_to_pixel(lat, use_cache=False)
    torch.cuda.synchronize()
    return vae, lat, out


def test_decode_480p_subsample_per_frame(golden, decoded):
    """Every 4th pixel of every row and column of all 9 pixel frames (the first latent frame alone, then one grouped
    call of two: both temporal upsamplers and the causal histories) against the reference's fp32 decode."""
    _, _, out = decoded
    assert out.shape == (1, 9, 3, PIX_H, PIX_W) and out.dtype == torch.float32
    assert float(out.abs().max()) <= 1.0
    s = golden["stride"]
    sub = out[0, :, :, ::s, ::s].double().cpu()
    gold = torch.from_numpy(golden["sub"].astype(np.float64))
    assert sub.shape == gold.shape == (9, 3, PIX_H // s, PIX_W // s)
    errs = [rel(sub[t], gold[t]) for t in range(9)]
    ref = golden["ref_bf16_sub_rel_err_frame"]
    print(f"\n480x832 decode vs fp32 reference, stride-{s} subsample, per pixel frame: HIP "
          + " ".join(f"{e:.2e}" for e in errs) + f"; overall {rel(sub, gold):.2e}\n  reference bf16 run on the same samples: "
          + " ".join(f"{e:.2e}" for e in ref))
    for t, e in enumerate(errs):
        assert e < TOL, f"pixel frame {t}: rel err {e:.4f} (reference bf16 run: {ref[t]:.4f})"
    assert rel(sub, gold) < TOL


def test_decode_480p_moments_per_frame_and_channel(golden, decoded):
    """Mean, rms and clamped count of every (pixel frame, channel) plane of the full 480 x 832 output against the fp32
    reference's (fp64 sums over all 399360 pixels): mean and rms within TOL of the reference rms; the clamped count
    within TOL of itself plus twice the reference bf16 run's own deviation (its values move across +-1 too)."""
    _, _, out = decoded
    n = PIX_H * PIX_W
    x = out[0].double()
    s1, s2 = x.sum((2, 3)).cpu().numpy(), x.pow(2).sum((2, 3)).cpu().numpy()
    nc = (x.abs() >= 1.0).sum((2, 3)).cpu().numpy()
    rms_r = np.sqrt(golden["sumsq_f32"] / n)
    mean_err = np.abs(s1 - golden["sum_f32"]) / n / rms_r
    rms_err = np.abs(np.sqrt(s2 / n) - rms_r) / rms_r
    clamp_err = np.abs(nc - golden["clamped_f32"])
    clamp_ref = np.abs(golden["clamped_bf16"] - golden["clamped_f32"])
    ref_mean = np.abs(golden["sum_bf16"] - golden["sum_f32"]) / n / rms_r
    ref_rms = np.abs(np.sqrt(golden["sumsq_bf16"] / n) - rms_r) / rms_r
    print(f"\n480x832 moments, worst (frame, channel): mean {mean_err.max():.2e} rms {rms_err.max():.2e} of the rms, clamped count "
          f"{clamp_err.max()} of {golden['clamped_f32'].min()}..{golden['clamped_f32'].max()} (reference bf16 run: mean {ref_mean.max():.2e} "
          f"rms {ref_rms.max():.2e} clamped {clamp_ref.max()})")
    assert (mean_err <= TOL).all(), mean_err
    assert (rms_err <= TOL).all(), rms_err
    assert (clamp_err <= TOL * golden["clamped_f32"] + 2 * clamp_ref).all(), (clamp_err, golden["clamped_f32"])


def test_decode_480p_full_resolution_crops(golden, decoded):
    """Full-resolution 32 x 32 crops of every pixel frame and channel: the four corners (the first and last 16 x 16 patch
    of the top stage, inside the ragged last patch of every latent-rate stage) and a window across the centre patch
    seams.  Max-abs error vs fp32 <= 2 x the reference bf16 run's on the same crop + 1e-2 (the fp32 crops are stored as
    float16: <= 2.5e-4 of that slack)."""
    _, _, out = decoded
    x = out[0].cpu().double()
    crops_f32 = golden["crops_f32"].astype(np.float64)
    ref_max = golden["crops_ref_bf16_max_abs"]
    worst = 0.0
    for k, (r, c) in enumerate(golden["crop_origins"]):
        err = (x[:, :, r:r + 32, c:c + 32] - torch.from_numpy(crops_f32[k])).abs().amax((2, 3)).numpy()     # [T, 3]
        bound = 2 * ref_max[k] + 1e-2
        worst = max(worst, float((err / bound).max()))
        print(f"\n480x832 crop at ({r:3d},{c:3d}): HIP max-abs {err.max():.2e} (reference bf16 run {ref_max[k].max():.2e})", end="")
        assert (err <= bound).all(), f"crop {k} at ({r}, {c}): max-abs {err.max():.4f}, bound {bound[err > bound]}"
    print(f"\n  worst error / bound {worst:.2f}")


def test_decode_480p_streaming_hook_equals_one_shot(decoded):
    """CausalInferencePipeline's streaming hook at full size: the first latent frame, then the rest, continue the same
    histories -- bit-identical to the one-shot decode."""
    vae, lat, out = decoded
    c0 = vae.decode_chunk(lat[:, :1], 0)
    c1 = vae.decode_chunk(lat[:, 1:], 1)
    assert c0.shape[1] == 1 and c1.shape[1] == 8
    assert torch.equal(torch.cat([c0, c1], 1), out)


# ========================================================================= every decoder convolution at 60 x 104, per kernel
def decoder_convs(shape: vw.VaeShape = vw.WAN_VAE, h: int = LAT_H, w: int = LAT_W):
    """The convolutions sf_vae_decode_frames issues at an h x w latent, walked from `decoder_layout` and de-duplicated by
    (taps, Cin, Cout, output H x W, upsample, epilogue): {key: first module name}."""
    out = {}

    def add(name, kernel, cin, cout, H, W, upsample=False, epi="bias"):
        out.setdefault((kernel, cin, cout, H, W, upsample, epi), name)

    def res(spec, H, W):
        add(spec.prefix + "residual.2", (3, 3, 3), spec.in_dim, spec.out_dim, H, W)
        add(spec.prefix + "residual.6", (3, 3, 3), spec.out_dim, spec.out_dim, H, W, epi="resid")
        if spec.in_dim != spec.out_dim:
            add(spec.prefix + "shortcut", (1, 1, 1), spec.in_dim, spec.out_dim, H, W)

    middle, ups = vw.decoder_layout(shape)
    add("decoder.conv1", (3, 3, 3), shape.z_dim, shape.dims[0], h, w)
    res(middle[0], h, w)
    res(middle[2], h, w)
    H, W = h, w
    for spec in ups:
        if isinstance(spec, vw.ResBlockSpec):
            res(spec, H, W)
            continue
        if spec.mode == "upsample3d":
            add(spec.prefix + "time_conv", (3, 1, 1), spec.dim, 2 * spec.dim, H, W, epi="interleave")
        H, W = 2 * H, 2 * W
        add(spec.prefix + "resample.1", (1, 3, 3), spec.dim, spec.dim // 2, H, W, upsample=True)
    add("decoder.head.2", (3, 3, 3), shape.dims[-1], 3, H, W, epi="clamp")
    return out


DECODER_CONVS = decoder_convs()


def halo_takes(kernel, cout, H, W, epi):
    """conv_halo.hip's domain (sf_conv_halo_launch) for these unstrided convolutions: 3 x 3 spatial taps, H, W >= 16, no
    interleave; Cout % 96 == 0 with a bf16 bias (+ residual) epilogue, or the <= 4-channel clamped float head."""
    if kernel[1:] != (3, 3) or epi == "interleave" or H < 16 or W < 16:
        return False
    return cout <= 4 if epi == "clamp" else cout % 96 == 0


def _conv_id(key):
    (kt, kh, kw), cin, cout, H, W, up, epi = key
    return f"{DECODER_CONVS[key]}-{kt}{kh}{kw}-{cin}to{cout}-{H}x{W}" + ("-up" if up else "") + ("" if epi == "bias" else f"-{epi}")


def test_decoder_conv_list_covers_the_production_shapes():
    """The walk reaches every stage the decoder runs at 60 x 104 (a layout change updates the sweep; this pins what it
    must at least hold)."""
    keys = set(DECODER_CONVS)
    assert ((3, 3, 3), 16, 384, 60, 104, False, "bias") in keys                      # decoder.conv1
    assert ((3, 3, 3), 384, 384, 60, 104, False, "resid") in keys
    assert ((3, 1, 1), 384, 768, 60, 104, False, "interleave") in keys               # upsample3d time_conv
    assert ((1, 3, 3), 384, 192, 120, 208, True, "bias") in keys
    assert ((1, 3, 3), 384, 192, 240, 416, True, "bias") in keys
    assert ((1, 1, 1), 192, 384, 120, 208, False, "bias") in keys                    # the 192 -> 384 block's shortcut
    assert ((3, 3, 3), 192, 384, 120, 208, False, "bias") in keys
    assert ((3, 3, 3), 192, 192, 240, 416, False, "resid") in keys
    assert ((1, 3, 3), 192, 96, 480, 832, True, "bias") in keys                      # upsample2d
    assert ((3, 3, 3), 96, 96, 480, 832, False, "resid") in keys
    assert ((3, 3, 3), 96, 3, 480, 832, False, "clamp") in keys                      # the head
    assert len(keys) == 17


def _reference(x, w, b, kernel, upsample, epi, resid):
    """fp32 torch statement of the convolution in the kernel's output layout: x [Tin, Hin, Win, Cin] channels-last (the
    causal history frames in front) -> [Tout, H, W, Cout] ([2 Tout, H, W, Cout / 2] interleaved, [Tout, 3, H, W] head)."""
    kt, kh, _ = kernel
    xf = x.float().permute(3, 0, 1, 2)[None]                                # [1, Cin, Tin, Hin, Win]
    if upsample:
        xf = F.interpolate(xf, scale_factor=(1.0, 2.0, 2.0), mode="nearest")
    pad = (1, 1, 1, 1, 0, 0) if kh == 3 else (0,) * 6
    y = F.conv3d(F.pad(xf, pad), w.float(), b.float())[0]                  # [Cout, Tout, H, W]
    del xf
    if epi == "clamp":
        return y.clamp(-1, 1).permute(1, 0, 2, 3).contiguous()
    if epi == "interleave":
        c, T = y.shape[0] // 2, y.shape[1]
        return y.reshape(2, c, T, *y.shape[2:]).permute(1, 2, 0, 3, 4).reshape(c, 2 * T, *y.shape[2:]).permute(1, 2, 3, 0).contiguous()
    y = y.permute(1, 2, 3, 0).contiguous()
    return y + resid.float() if resid is not None else y


@pytest.mark.parametrize("key", list(DECODER_CONVS), ids=_conv_id)
def test_decoder_conv_at_480p_per_patch(key):
    """One decoder convolution at its production geometry -- T = 4 output frames at the 60 x 104 and 120 x 208 stages
    (a grouped call), T = 2 at 240 x 416 and 480 x 832 (the fp32 CPU reference's cost) -- through the halo kernel (where
    it takes the shape), the implicit GEMM and AUTO: rel-Frobenius <= 4e-3 overall and <= 1e-2 in every 16 x 16 output
    patch (ragged edge patches included: 60 = 3 * 16 + 12, 104 = 6 * 16 + 8); the head: max-abs <= 2e-2; AUTO is
    bit-identical to the structure it selects."""
    kernel, cin, cout, H, W, up, epi = key
    kt = kernel[0]
    T = 4 if H * W <= 120 * 208 else 2
    g = torch.Generator().manual_seed(cin * 7 + cout + H + kt)
    hin, win = (H // 2, W // 2) if up else (H, W)
    cp = -(-cin // 32) * 32                                                # decoder.conv1: 16 latent channels padded to 32
    x = torch.zeros(T + kt - 1, hin, win, cp, dtype=torch.bfloat16)
    x[..., :cin] = bf((T + kt - 1, hin, win, cin), g)
    fan = cin * kt * kernel[1] * kernel[2]
    w = bf((cout, cin) + kernel, g, (3.0 if epi == "clamp" else 1.0) * fan ** -0.5)
    b = bf((cout,), g, 0.1)
    resid = bf((T, H, W, cout), g) if epi == "resid" else None
    ref = _reference(x[..., :cin], w, b, kernel, up, epi, resid).to(DEV)
    xd, wd, bd = x.to(DEV), repack_conv(w, cin_pad=cp).to(DEV), b.to(DEV)
    rd = resid.to(DEV) if resid is not None else None
    del x

    def run(structure):
        return ops.conv_igemm(xd, wd, bd, kernel, T, upsample=up, resid=rd, interleave=epi == "interleave",
                              clamp_f32=epi == "clamp", structure=structure)

    structures = (["halo"] if halo_takes(kernel, cout, H, W, epi) else []) + ["igemm"]
    outs = {}
    for st in structures:
        out = run(st)
        assert out.shape == ref.shape, (st, tuple(out.shape), tuple(ref.shape))
        if epi == "clamp":
            assert float((ref.abs() >= 1).float().mean()) > 0.02                 # the clamp is exercised
            err = (out - ref).abs().max().item()
            print(f"\n{_conv_id(key)} {st}: max-abs {err:.2e}", end="")
            assert err < HEAD_TOL, (st, err)
        else:
            overall = rel(out, ref)
            patches = block_rel(out, ref, 16, 16)
            worst = patches.max().item()
            print(f"\n{_conv_id(key)} {st}: rel {overall:.2e}, worst of {patches.numel()} 16x16 patches {worst:.2e}", end="")
            assert overall < CONV_TOL, (st, overall)
            bad = (patches > PATCH_TOL).nonzero().tolist()
            assert not bad, f"{st}: {len(bad)} patches (t, row, col) above {PATCH_TOL}, e.g. {bad[:4]}; worst {worst:.3e}"
        outs[st] = out
    assert torch.equal(run("auto"), outs[structures[0]])


# ====================================================================== the middle attention's kernels at 6240 / 14400 tokens
def _padded(n):
    return (n + 63) & ~63            # att_npad of vae_decode.hip


@pytest.mark.parametrize("h,w", [(60, 104), (90, 160)], ids=["480p-6240", "720p-14400"])
def test_softmax_rows_decoder_attention_size(h, w):
    """sf_softmax_rows as attention_block issues it: n = h*w score columns of a row of stride n padded to a multiple of
    64 (6272 for 6240; the padding the score GEMM leaves unwritten holds garbage; 14400 needs none), scale 1/sqrt(384),
    256 threads striding the row -- 25 (57) passes, the last one partial.  Rows with their maximum in the first pass, in
    the last partial pass, and one row with a single dominant score in the final column; against fp64 softmax
    elementwise (round-to-nearest bf16: <= 2^-8 relative; the fp32 arithmetic adds ~1e-6 of it), padded columns exactly
    0, rows summing to 1 within the same 2^-8."""
    n, C = h * w, 384
    npd = _padded(n)
    scale = 1.0 / math.sqrt(C)
    g = torch.Generator().manual_seed(n)
    s = torch.randn(n, npd, generator=g) * 30
    s[:, n:] = 1.0e4                                           # would dominate every row if the kernel read it
    rows = torch.arange(n)
    last = (n // 256) * 256                                    # first column of the last (partial) pass
    assert last < n
    a, bq = rows[rows % 4 == 0], rows[rows % 4 == 1]
    s[a, a % 256] += 200.0                                     # maximum in the first pass
    s[bq, last + bq % (n - last)] += 200.0                     # maximum in the last, partial pass
    s[n - 1, n - 1] = s[n - 1, :n].max() + 2000.0              # a single dominant score in the final column
    sd = s.to(DEV)
    out = ops.softmax_rows(sd[:, :n], scale, cols_padded=npd)
    assert out.shape == (n, npd) and out.dtype == torch.bfloat16
    if npd > n:
        assert float(out[:, n:].abs().max()) == 0.0
    assert float(out[n - 1, n - 1]) == 1.0
    o = out.cpu()
    del sd, out
    worst_rel, worst_sum = 0.0, 0.0
    for r0 in range(0, n, 2048):
        ref = torch.softmax(s[r0:r0 + 2048, :n].double() * scale, dim=-1)
        got = o[r0:r0 + 2048, :n].double()
        err = (got - ref).abs()
        ok = err <= 2.0 ** -8 * ref + 1e-30
        assert ok.all(), f"rows {r0}+: {int((~ok).sum())} entries off, e.g. row {int((~ok).nonzero()[0, 0]) + r0}: max-abs {err.max():.3e}"
        worst_rel = max(worst_rel, float((err / ref.clamp_min(1e-30)).max()))
        worst_sum = max(worst_sum, float((got.sum(-1) - 1).abs().max()))
    print(f"\nsoftmax_rows {n} columns: worst relative entry error {worst_rel:.2e}, worst |row sum - 1| {worst_sum:.2e}")
    assert worst_sum <= 2.0 ** -8


@pytest.mark.parametrize("h,w", [(60, 104), (90, 160)], ids=["480p-6240", "720p-14400"])
def test_score_gemm_decoder_attention_size(h, w):
    """The f32-epilogue score GEMM S = Q K^T of attention_block at (n, n, 384) with the decoder's strides: q and k are
    the two halves of the stacked [n, 2C] projection (lda = ldw = 2C = 768), S is written with ldo = n padded to 64.
    rel <= 1e-5 vs fp64, overall and in every 256 x 256 block; the padding columns are left alone."""
    n, C = h * w, 384
    npd = _padded(n)
    g = torch.Generator().manual_seed(n + 1)
    qk = bf((n, 2 * C), g)
    qkd = qk.to(DEV)
    sbuf = torch.full((n, npd), -7.0, dtype=torch.float32, device=DEV)
    ops.gemm(qkd[:, :C], qkd[:, C:], None, "f32", out=sbuf[:, :n])
    assert float((sbuf[:, n:] != -7.0).sum()) == 0                        # nothing written past the n score columns
    got = sbuf[:, :n].cpu()
    del sbuf, qkd
    q, k = qk[:, :C].double(), qk[:, C:].double()
    num = den = 0.0
    worst = 0.0
    for r0 in range(0, n, 2048):
        ref = q[r0:r0 + 2048] @ k.t()
        d = got[r0:r0 + 2048].double() - ref
        num, den = num + float(d.pow(2).sum()), den + float(ref.pow(2).sum())
        worst = max(worst, block_rel(got[r0:r0 + 2048].double()[None, ..., None], ref[None, ..., None], 256, 256).max().item())
    overall = math.sqrt(num / den)
    print(f"\nscore GEMM ({n}, {n}, {C}): rel {overall:.2e}, worst 256x256 block {worst:.2e}")
    assert overall < 1e-5 and worst < 1e-5


@pytest.mark.parametrize("h,w", [(60, 104), (90, 160)], ids=["480p-6240", "720p-14400"])
def test_pv_gemm_decoder_attention_size(h, w):
    """O = P V + b_v of attention_block at (n, 384, n padded to 64): P the bf16 softmax rows [n, npad] (zero past n), V^T
    [384, npad] with zero padding columns, the v bias in the epilogue.  rel <= 4e-3 vs fp64, overall and in every
    block of 128 rows."""
    n, C = h * w, 384
    npd = _padded(n)
    g = torch.Generator().manual_seed(n + 2)
    p = torch.zeros(n, npd, dtype=torch.bfloat16)
    for r0 in range(0, n, 2048):
        p[r0:r0 + 2048, :n] = torch.softmax(torch.randn(min(2048, n - r0), n, generator=g) * 3.0, dim=-1).to(torch.bfloat16)
    vt = torch.zeros(C, npd, dtype=torch.bfloat16)
    vt[:, :n] = bf((C, n), g)
    b = bf((C,), g, 0.02)
    out = ops.gemm(p.to(DEV), vt.to(DEV), b.to(DEV)).cpu()
    assert out.shape == (n, C) and out.dtype == torch.bfloat16
    vtd = vt[:, :n].double()
    num = den = 0.0
    worst = 0.0
    for r0 in range(0, n, 2048):
        ref = p[r0:r0 + 2048, :n].double() @ vtd.t() + b.double()
        d = out[r0:r0 + 2048].double() - ref
        num, den = num + float(d.pow(2).sum()), den + float(ref.pow(2).sum())
        worst = max(worst, block_rel(out[r0:r0 + 2048].double()[None, :, None], ref[None, :, None], 128, 1).max().item())
    overall = math.sqrt(num / den)
    print(f"\nP.V GEMM ({n}, {C}, {npd}): rel {overall:.2e}, worst 128-row block {worst:.2e}")
    assert overall < 4e-3 and worst < 4e-3


# =================================================================== the encoder's strided convolutions at 480 x 832 input
def encoder_strided_convs(shape: vw.VaeShape = vw.WAN_VAE, H0: int = PIX_H, W0: int = PIX_W):
    """The strided convolutions sf_vae_encode_frames issues on H0 x W0 pixels, walked from `encoder_layout`:
    [(name, 'spatial' | 'temporal', channels, output H, output W)]."""
    stages, _ = vw.encoder_layout(shape)
    H, W, out = H0, W0, []
    for st in stages:
        for spec in st:
            if isinstance(spec, vw.ResampleSpec):
                H, W = H // 2, W // 2
                out.append((spec.prefix + "resample.1", "spatial", spec.dim, H, W))
                if spec.mode == "downsample3d":
                    out.append((spec.prefix + "time_conv", "temporal", spec.dim, H, W))
    return out


ENCODER_CONVS = encoder_strided_convs()


def test_encoder_strided_conv_list():
    assert [(k, c, H, W) for _, k, c, H, W in ENCODER_CONVS] == [
        ("spatial", 96, 240, 416), ("spatial", 192, 120, 208), ("temporal", 192, 120, 208),
        ("spatial", 384, 60, 104), ("temporal", 384, 60, 104)]


@pytest.mark.parametrize("case", ENCODER_CONVS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}x{c[4]}")
def test_encoder_strided_conv_at_480p_per_patch(case):
    """A stride-2 convolution of the encoder at its production geometry: ZeroPad2d((0,1,0,1)) + 3 x 3 stride 2 per frame
    (2 frames at 480 x 832 input, 4 below), or the (3,1,1) time convolution with temporal stride 2 (4 output frames of a
    grouped call, input offset 1).  Implicit GEMM and AUTO (the halo kernel declines strided shapes, so they are the same
    bits): rel-Frobenius <= 4e-3 overall and <= 1e-2 in every 16 x 16 output patch."""
    _, kind, c, H, W = case
    g = torch.Generator().manual_seed(c + H)
    b = bf((c,), g, 0.1)
    if kind == "spatial":
        T = 2 if H * W > 120 * 208 else 4
        x = bf((T, 2 * H, 2 * W, c), g)
        w = bf((c, c, 3, 3), g, (9 * c) ** -0.5)
        ref = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.float(), b.float(), stride=2)
        kernel, stride, off = (1, 3, 3), (1, 2), 0
    else:
        T, off = 4, 1
        x = bf((off + 2 * (T - 1) + 3, H, W, c), g)
        w = bf((c, c, 3, 1, 1), g, (3 * c) ** -0.5)
        ref = F.conv3d(x.float().permute(3, 0, 1, 2)[None, :, off:], w.float(), b.float(), stride=(2, 1, 1))[0].permute(1, 0, 2, 3)
        kernel, stride = (3, 1, 1), (2, 1)
    ref = ref.permute(0, 2, 3, 1).contiguous().to(DEV)                       # [T, H, W, C]
    xd, wd, bd = x.to(DEV), repack_conv(w).to(DEV), b.to(DEV)
    out = ops.conv_igemm(xd, wd, bd, kernel, T, t_in_offset=off, structure="igemm", stride=stride)
    assert out.shape == ref.shape == (T, H, W, c)
    overall = rel(out, ref)
    patches = block_rel(out, ref, 16, 16)
    worst = patches.max().item()
    print(f"\n{case[0]} ({kind}, {c} ch, -> {H}x{W}): rel {overall:.2e}, worst of {patches.numel()} 16x16 patches {worst:.2e}")
    assert overall < CONV_TOL
    bad = (patches > PATCH_TOL).nonzero().tolist()
    assert not bad, f"{len(bad)} patches (t, row, col) above {PATCH_TOL}, e.g. {bad[:4]}; worst {worst:.3e}"
    assert torch.equal(ops.conv_igemm(xd, wd, bd, kernel, T, t_in_offset=off, stride=stride), out)
