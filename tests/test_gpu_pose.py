"""GPU parity of the pose front end against the reference's own `dwpose_embedding` / `randomref_embedding_pose` modules
recorded by `tools/make_golden_pose.py` (seeded weights; fp32 run = the truth, bf16 run = the noise floor):

- both stacks at 9 frames of 64 x 96 and of 120 x 208 (ragged), every element, dense and skeleton input: per latent
  frame the rel-Frobenius error within 1.5 x the reference bf16 run's own on that frame (FLOOR_MARGIN, the contract
  of test_gpu_taehv.py);
- the 81-frame 480 x 832 clip (regenerated from its seed, CRC-checked): the same bound on two subsamples per latent
  frame; per latent frame the per-channel mean and rms vectors against the fp32 moments, bound 1.5 x the bf16 run's own
  deviation on the same statistic.  (The statistic is the rel-Frobenius distance of the 5120-vector of a frame: one
  channel's own deviation can be arbitrarily close to zero by chance and cannot serve as a bound.);
- every layer the sequencer issues, at the production size of both stacks, per kernel against fp32 torch on the same
  bf16 inputs: CONV_TOL overall, PATCH_TOL per 16 x 16 output patch, and the first / last output frame and the four
  image borders as slices of their own;
- the prepare kernel bit for bit; two runs bit-identical (the sequencer does not split the clip);
- the reduced pipeline: `dwpose_data` + `random_ref_dwpose` == `dwpose_data_emb=encode_pose(...)[0]` bit for bit, the
  pose changes the result, batch 2 shares one clip, weights load from `args.pose_weights_path`.

Run with `-m gpu` (`-s` shows the measured figures).

Measured on one MI355X: not yet -- no GPU was available when this file was written, so no figure is quoted.  The
reference's own bf16 floor (the bound is 1.5 x it): 7.9-8.7e-3 per latent frame on dense input, 4.2-5.2e-3 on skeleton
input, 5.5-5.8e-3 on the reference-pose map."""
import os
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import ops, pose_weights as pw

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
FLOOR_MARGIN = 1.5  # x the reference bf16 run's own error on the same frame (test_gpu_taehv.py's contract)
CONV_TOL = 4e-3     # per-kernel contract of the convolutions (test_gpu_vae.py, test_gpu_taehv.py)
PATCH_TOL = 1e-2    # ... and of every 16 x 16 output patch of them
KINDS = ("dense", "skeleton")
LAT_H, LAT_W = 8, 12


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def block_rel(out, ref, bh=16, bw=16):
    d = (out.double() - ref.double()).pow(2).sum(-1)
    r = ref.double().pow(2).sum(-1)
    T, H, W = d.shape
    ph, pw_ = -(-H // bh), -(-W // bw)

    def fold(t):
        return F.pad(t, (0, pw_ * bw - W, 0, ph * bh - H)).reshape(T, ph, bh, pw_, bw).sum((2, 4))

    return (fold(d) / fold(r).clamp_min(1e-30)).sqrt()


def fmt(v):
    return " ".join(f"{e:.2e}" for e in v)


@pytest.fixture(scope="module")
def embedder():
    g = np.load(os.path.join(GOLD, "pose_small_a_dense.npz"))
    return sfa.PoseEmbedder(pw.synth_pose_state_dict(int(g["seed"])), device=DEV)


# =========================================================================================== whole stacks, small sizes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag,shape", [("a", (9, 64, 96)), ("b", (9, 120, 208))], ids=["9x64x96", "9x120x208"])
def test_stacks_small_sizes_every_element(embedder, tag, shape, kind):
    g = np.load(os.path.join(GOLD, f"pose_small_{tag}_{kind}.npz"))
    clip, image = torch.from_numpy(g["clip_u8"]), torch.from_numpy(g["image_u8"])
    assert tuple(clip.shape) == (3,) + shape
    f, h, w = (int(v) for v in g["plan"])
    gold = torch.from_numpy(np.stack([np.load(os.path.join(GOLD, f"pose_small_{tag}_{kind}_f{i}.npz"))["tokens_f32"] for i in range(f)]).astype(np.float32))
    tokens, fhw = embedder.embed(clip.to(DEV))
    assert fhw == (f, h, w) and tokens.shape == (1, f * h * w, 5120) and tokens.dtype == torch.bfloat16
    t = tokens[0].view(f, h * w, 5120)
    errs, floor = [rel(t[i], gold[i]) for i in range(f)], g["ref_bf16_rel_err_frame"]
    ref_map = embedder.embed_ref(image.to(DEV))
    gold_map = torch.from_numpy(g["ref_map_f32"].astype(np.float32))
    assert ref_map.shape == (1, 20, 1) + tuple(gold_map.shape[1:]) and ref_map.dtype == torch.bfloat16
    e_map, floor_map = rel(ref_map[0, :, 0], gold_map), float(g["ref_bf16_rel_err_map"])
    print(f"\npose {shape} {kind}: HIP per latent frame {fmt(errs)}; reference bf16 {fmt(floor)}; reference-pose map {e_map:.2e} (reference bf16 {floor_map:.2e})")
    for i, e in enumerate(errs):
        assert e <= FLOOR_MARGIN * floor[i], f"latent frame {i}: rel err {e:.4f}, reference bf16 run {floor[i]:.4f}"
    assert e_map <= FLOOR_MARGIN * floor_map
    emb, ref2 = embedder.encode_pose(clip.to(DEV), image.to(DEV))          # the reference's layouts, as views
    assert emb.shape == (1, 5120, f, h, w) and emb.data_ptr() != tokens.data_ptr() and torch.equal(ref2, ref_map)
    assert torch.equal(emb[0].permute(1, 2, 3, 0).reshape(f * h * w, 5120), tokens[0])


# ================================================================================================== the 480 x 832 clip
_EMBEDDED = {}


def embedded_480p(kind, embedder):
    """(fixture arrays, tokens [21, 1560, 5120]) of the recorded 81-frame clip of `kind`, embedded once per module."""
    if kind not in _EMBEDDED:
        g = dict(np.load(os.path.join(GOLD, f"pose_480p_{kind}.npz")))
        clip = pw.synth_pose_clip(int(g["input_seed"]), 81, 480, 832, kind)
        assert zlib.crc32(clip.numpy().tobytes()) == int(g["clip_crc32"]), "the regenerated clip is not the recorded one"
        tokens, fhw = embedder.embed(clip.to(DEV))
        torch.cuda.synchronize()
        assert fhw == (21, 30, 52)
        _EMBEDDED[kind] = (g, tokens[0].view(21, 1560, 5120))
    return _EMBEDDED[kind]


def load_sub(kind, name, first_frames):
    parts = [np.load(os.path.join(GOLD, f"pose_480p_{kind}_{name}{i}.npz")) for i in range(len(first_frames))]
    assert [int(p["first_frame"]) for p in parts] == list(first_frames)
    return torch.from_numpy(np.concatenate([p["tokens_f32"] for p in parts]).astype(np.float32))


def check_sub(kind, name, g, ours, gold):
    assert ours.shape == gold.shape
    errs, floor = [rel(ours[i], gold[i]) for i in range(21)], g[f"ref_bf16_{name}_rel_err_frame"]
    print(f"\npose 81x480x832 {kind} {name}: HIP per latent frame {fmt(errs)}\n  reference bf16 on the same samples: {fmt(floor)}")
    for i, e in enumerate(errs):
        assert e <= FLOOR_MARGIN * floor[i], f"{name} latent frame {i}: rel err {e:.4f}, reference bf16 run {floor[i]:.4f}"


@pytest.mark.parametrize("kind", KINDS)
def test_480p_every_32nd_channel_of_every_8th_token(embedder, kind):
    g, t = embedded_480p(kind, embedder)
    check_sub(kind, "subA", g, t[:, ::8, ::32], load_sub(kind, "subA", (0, 11)))


def test_480p_all_channels_of_every_195th_token(embedder):
    g, t = embedded_480p("skeleton", embedder)
    check_sub("skeleton", "subB", g, t[:, ::195], load_sub("skeleton", "subB", (0, 7, 14)))


def test_480p_moments_per_latent_frame(embedder):
    """Recorded for the skeleton clip, the realistic input."""
    g, t = embedded_480p("skeleton", embedder)
    s32 = torch.from_numpy(np.load(os.path.join(GOLD, "pose_480p_skeleton_sum.npz"))["sum_f32"])
    q32 = torch.from_numpy(np.load(os.path.join(GOLD, "pose_480p_skeleton_sumsq.npz"))["sumsq_f32"])
    n = t.shape[1]
    s, q = t.double().sum(1).cpu(), t.double().pow(2).sum(1).cpu()
    mean_dev = [rel(s[i] / n, s32[i] / n) for i in range(21)]
    rms_dev = [rel((q[i] / n).sqrt(), (q32[i] / n).sqrt()) for i in range(21)]
    print(f"\npose 81x480x832 skeleton moments: mean {fmt(mean_dev)}\n  reference bf16: {fmt(g['ref_bf16_mean_dev_frame'])}\n  rms {fmt(rms_dev)}\n"
          f"  reference bf16: {fmt(g['ref_bf16_rms_dev_frame'])}")
    for i in range(21):
        assert mean_dev[i] <= FLOOR_MARGIN * g["ref_bf16_mean_dev_frame"][i], f"latent frame {i}: mean"
        assert rms_dev[i] <= FLOOR_MARGIN * g["ref_bf16_rms_dev_frame"][i], f"latent frame {i}: rms"


def test_two_runs_are_bit_identical(embedder):
    clip = pw.synth_pose_clip(77, 13, 120, 208, "skeleton").to(DEV)
    image = pw.synth_pose_image(78, 120, 208, "skeleton").to(DEV)
    a, b = embedder.embed(clip)[0].clone(), embedder.embed(clip)[0]
    assert torch.equal(a, b) and torch.equal(embedder.embed_ref(image).clone(), embedder.embed_ref(image))
    assert torch.equal(embedder.embed(clip.float())[0], a) and torch.equal(embedder.embed(clip[None])[0], a)


# ======================================================================================================== per kernel
def layer_cases():
    cases = []
    vols = pw.pose_layer_volumes(81, 480, 832)
    for i, (idx, cin, cout, k, stride, pad, act) in enumerate(pw.DWPOSE_LAYERS[:-1]):
        _, H, W = vols[i]
        cases.append((f"dwpose_embedding.{idx}", pw.DWPOSE_PREFIX, idx, cin, cout, 5 if stride[0] == 1 else 7, H, W, stride, pad, act))
    h, w = 480, 832
    for idx, cin, cout, k, stride, pad, act in pw.RANDOMREF_LAYERS:
        cases.append((f"randomref_embedding_pose.{idx}", pw.RANDOMREF_PREFIX, idx, cin, cout, 1, h, w, (1,) + stride, (0,) + pad, act))
        h, w = (h - 1) // stride[0] + 1, (w - 1) // stride[1] + 1
    return cases


@pytest.mark.parametrize("case", layer_cases(), ids=lambda c: c[0])
def test_every_layer_at_production_size(case):
    """One launch of sf_pose_conv as the sequencer issues it at 480 x 832 (a few frames for the 3-D layers; an odd
    frame count, so the last output frame of the temporally strided ones reads the zero padding behind the clip too) against
    fp32 torch on the same bf16 inputs and weights."""
    name, prefix, idx, cin, cout, T, H, W, stride, pad, act = case
    sd = pw.synth_pose_state_dict(11)
    w, b = sd[f"{prefix}{idx}.weight"], sd[f"{prefix}{idx}.bias"]
    w5 = w if w.dim() == 5 else w.unsqueeze(2)
    kt = w5.shape[2]
    g = torch.Generator().manual_seed(idx + (100 if kt == 1 else 0))
    cs = 8 if cin == 3 else 16
    x = torch.zeros(T, H, W, cs, dtype=torch.bfloat16)
    # layer inputs as they occur: 0..1 pose values (many exactly zero) in front, SiLU outputs behind
    x[..., :cin] = (torch.rand(T, H, W, cin, generator=g) * (torch.rand(T, H, W, 1, generator=g) < 0.3)).to(torch.bfloat16) if cin == 3 \
        else F.silu(torch.randn(T, H, W, cin, generator=g)).to(torch.bfloat16)
    wb = w5.to(torch.bfloat16)
    out = ops.pose_conv(x.to(DEV), pw.repack_pose_conv(wb.float(), cs).to(torch.bfloat16).to(DEV), pw.pad_pose_bias(b).to(DEV), cout, kt=kt,
                        stride_t=stride[0], stride_s=stride[1], silu=act)
    torch.cuda.synchronize()
    ref = pw.pose_layer_torch(x[..., :cin].float().permute(3, 0, 1, 2)[None], wb.float(), b, stride, pad, act)[0].permute(1, 2, 3, 0)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    o = out.float().cpu()
    slices = {"all": (o, ref), "first frame": (o[:1], ref[:1]), "last frame": (o[-1:], ref[-1:]), "top row": (o[:, :1], ref[:, :1]),
              "bottom row": (o[:, -1:], ref[:, -1:]), "left column": (o[:, :, :1], ref[:, :, :1]), "right column": (o[:, :, -1:], ref[:, :, -1:])}
    errs = {k: rel(a, r) for k, (a, r) in slices.items()}
    worst = block_rel(o, ref).max().item()
    print(f"\n{name} {tuple(x.shape)} -> {tuple(out.shape)}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f", worst 16x16 patch {worst:.2e}")
    for k, e in errs.items():
        assert e <= CONV_TOL, f"{name}: {k} rel err {e:.2e}"
    assert worst <= PATCH_TOL


def test_token_embedding_layer_at_production_size():
    """dwpose_embedding.12 (gather + sf_gemm_bf16) on 3 frames of 60 x 104 and on a ragged 15 x 27 (the odd last row and
    column are dropped, as the unpadded stride-2 convolution does)."""
    sd = pw.synth_pose_state_dict(11)
    w, b = sd["dwpose_embedding.12.weight"].to(torch.bfloat16), sd["dwpose_embedding.12.bias"].to(torch.bfloat16)
    for T, H, W in ((3, 60, 104), (2, 15, 27)):
        x = F.silu(torch.randn(T, H, W, 16, generator=torch.Generator().manual_seed(H))).to(torch.bfloat16)
        out = ops.pose_patch_embed(x.to(DEV), pw.repack_pose_embed(w.float()).to(torch.bfloat16).to(DEV), b.to(DEV))
        ref = pw.pose_layer_torch(x.float().permute(3, 0, 1, 2)[None], w.float(), b.float(), (1, 2, 2), 0, False)[0].permute(1, 2, 3, 0)
        assert out.shape == (T * (H // 2) * (W // 2), 5120)
        o = out.float().cpu().view(ref.shape)
        e, worst = rel(o, ref), max(rel(o[t, i], ref[t, i]) for t in range(T) for i in range(H // 2))
        print(f"\ndwpose_embedding.12 {(T, H, W)}: rel {e:.2e}, worst token row {worst:.2e}")
        assert e <= CONV_TOL and worst <= PATCH_TOL


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.bfloat16])
def test_prepare_is_bit_exact(dtype):
    clip = pw.synth_pose_clip(5, 6, 33, 50, "dense")
    image = pw.synth_pose_image(6, 33, 50, "dense")
    if dtype != torch.uint8:
        clip, image = clip.to(dtype), image.to(dtype)
    out = ops.pose_prepare(clip.to(DEV), lead=3).cpu()
    want = (torch.cat([clip[:, :1].repeat(1, 3, 1, 1), clip], dim=1) / 255.0).to(torch.bfloat16).permute(1, 2, 3, 0)
    assert out.shape == (9, 33, 50, 8) and torch.equal(out[..., :3], want) and out[..., 3:].abs().sum() == 0
    out = ops.pose_prepare(image.to(DEV), lead=0, hwc=True).cpu()
    assert out.shape == (1, 33, 50, 8) and torch.equal(out[0, ..., :3], (image / 255.0).to(torch.bfloat16)) and out[..., 3:].abs().sum() == 0


# ============================================================================================================ pipeline
class TwoPromptEncoder:
    def __init__(self, pe, ne):
        self.pe, self.ne = pe, ne

    def __call__(self, text_prompts):
        return {"prompt_embeds": (self.ne if text_prompts[0] == "NEG" else self.pe).expand(len(text_prompts), -1, -1).contiguous()}


def test_pipeline_takes_pose_frames(embedder, tmp_path, caplog):
    shape = sfa.WAN_REDUCED
    sd = sfa.synth_state_dict(shape, seed=0, pose=True)
    g = torch.Generator().manual_seed(91)
    pe = torch.randn(1, 512, shape.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    ne = torch.randn(1, 512, shape.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    noise = torch.randn(2, 2, 16, LAT_H, LAT_W, generator=g).to(torch.bfloat16).to(DEV)
    clip = pw.synth_pose_clip(92, 5, 8 * LAT_H, 8 * LAT_W, "skeleton")             # 5 pose frames -> 2 latent frames of 4 x 6 tokens
    image = pw.synth_pose_image(93, 8 * LAT_H, 8 * LAT_W, "skeleton")
    assert pw.pose_plan(*clip.shape[1:]) == (2, LAT_H // 2, LAT_W // 2)
    args = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, num_frame_per_block=1, negative_prompt="NEG",
                           guidance_scale=4.0)
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV)

    def pipeline(a=args, **kw):
        p = sfa.CausalDiffusionInferencePipeline(a, DEV, generator=gen, text_encoder=TwoPromptEncoder(pe, ne), vae=sfa.IdentityVAE(), **kw)
        p.sampling_steps = 6
        return p

    pipe = pipeline(pose_embedder=embedder)
    one = noise[:1]
    lat = pipe.inference(one, ["p"], None, clip, image, return_latents=True)[1]
    emb = embedder.encode_pose(clip, image)[0]
    lat_emb = pipe.inference(one, ["p"], None, None, None, return_latents=True, dwpose_data_emb=emb)[1]
    lat_plain = pipe.inference(one, ["p"], None, None, None, return_latents=True)[1]
    assert torch.equal(lat, lat_emb)
    d = rel(lat, lat_plain)
    print(f"\npipeline: pose vs no pose {d:.3f}")
    assert d > 2e-2
    # only one of the two inputs: the pose branch is not taken (a warning, as the reference silently does)
    with caplog.at_level("WARNING"):
        assert torch.equal(pipe.inference(one, ["p"], None, clip, None, return_latents=True)[1], lat_plain)
    assert "pose branch" in caplog.text
    # batch 2 shares the one clip: each sample equals its own run
    both = pipe.inference(noise, ["p", "p"], None, clip, image, return_latents=True)[1]
    assert torch.equal(both[:1], lat) or rel(both[:1], lat) < 1e-6
    assert rel(both[1:], pipe.inference(noise[1:], ["p"], None, clip, image, return_latents=True)[1]) < 1e-6
    # weights from args.pose_weights_path, loaded on the first pose inference only
    path = str(tmp_path / "pose.pt")
    torch.save(pw.synth_pose_state_dict(int(np.load(os.path.join(GOLD, "pose_small_a_dense.npz"))["seed"])), path)
    lazy = pipeline(SimpleNamespace(**vars(args), pose_weights_path=path))
    assert lazy.pose_embedder is None and not lazy.pose_weights_loaded
    assert torch.equal(lazy.inference(one, ["p"], None, clip, image, return_latents=True)[1], lat) and lazy.pose_weights_loaded
    first = lazy.pose_embedder
    lazy.inference(one, ["p"], None, clip, image)
    assert lazy.pose_embedder is first
    with pytest.raises(AssertionError, match="output timeline"):
        pipe.inference(one, ["p"], None, pw.synth_pose_clip(1, 9, 8 * LAT_H, 8 * LAT_W), image)
    with pytest.raises(NotImplementedError):
        pipe.inference(one, ["p"], object(), clip, image)
