"""GPU tests of the few-step pipeline's image and pose conditioning: the kernel that writes a chunk
of `y`, the incremental `y` against the whole-clip one of `encode_image`, and `CausalInferencePipeline.inference` / `stream`
with an image, with a pose clip, and with both, against loops written here.

Every comparison is `torch.equal`: the incremental path makes the whole-clip path's VAE calls in the same order and the
kernel reproduces its roundings, and a rollout is compared with the same generator calls made by hand.  The one bound, for
"another image moves the latents", is twice the reference's own bf16-vs-fp32 distance recorded in i2v_reduced.npz: a
change of that size is not rounding."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import clip_weights as cw
from self_forcing_amd import pose_weights as pw
from self_forcing_amd import vae_weights as vw
from self_forcing_amd import weights as wt
from self_forcing_amd.kvcache import new_crossattn_cache, new_kv_cache

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
S = wt.WAN_I2V_REDUCED
STEPS = [1000, 750, 500, 250]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


# ------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("with_map", [False, True], ids=["plain", "map"])
@pytest.mark.parametrize("first", [True, False], ids=["frame0", "later"])
@pytest.mark.parametrize("h,w", [(16, 16), (6, 10)], ids=["16x16", "6x10"])
@pytest.mark.parametrize("f", [1, 3])
def test_assemble_y_equals_the_torch_expression(f, h, w, first, with_map):
    """`cat([mask, latent]).to(bf16)` (+ map, a second rounding) written into frames 1..f of a longer buffer whose other
    frames must survive; a plane of 60 elements has no 16-byte multiple and starts off a 16-byte boundary."""
    g = torch.Generator().manual_seed(1000 * f + 10 * h + int(first))
    latent = (3 * torch.randn(f, 16, h, w, generator=g)).to(DEV)
    ref_map = bf(g, h, w, 20) if with_map else None
    msk = torch.zeros(4, f, h, w, device=DEV)
    if first:
        msk[:, 0] = 1
    want = torch.cat([msk, latent.transpose(0, 1).float()]).unsqueeze(0).to(torch.bfloat16)       # diffusion_pipeline.py encode_image
    if with_map:
        want = want + ref_map.permute(2, 0, 1)[None, :, None].to(want.dtype)                        # ... and inference's y + embed_ref
    buf = torch.full((20, f + 2, h, w), 7.0, dtype=torch.bfloat16, device=DEV)
    torch.ops.sf_hip.i2v_assemble_y(latent, buf[:, 1:1 + f], first, ref_map)
    assert torch.equal(buf[:, 1:1 + f], want[0])
    assert bool((buf[:, 0] == 7).all()) and bool((buf[:, -1] == 7).all())
    own = torch.empty(20, f, h, w, dtype=torch.bfloat16, device=DEV)                               # a buffer of its own
    torch.ops.sf_hip.i2v_assemble_y(latent, own, first, ref_map)
    assert torch.equal(own, want[0])


def test_assemble_y_op_checks():
    latent = torch.zeros(2, 16, 6, 10, device=DEV)
    y = torch.zeros(20, 2, 6, 10, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="contiguous h x w planes"):
        torch.ops.sf_hip.i2v_assemble_y(latent, y[:, :1], True, None)
    with pytest.raises(ValueError, match="overlap"):
        torch.ops.sf_hip.i2v_assemble_y(latent, torch.as_strided(y, (20, 2, 6, 10), (60, 60, 10, 1)), True, None)
    with pytest.raises(ValueError, match="channels-last"):
        torch.ops.sf_hip.i2v_assemble_y(latent, y, True, torch.zeros(20, 6, 10, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        torch.ops.sf_hip.i2v_assemble_y(latent.to(torch.bfloat16), y, True, None)


# ------------------------------------------------------------------------------------------ shared models
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "i2v_reduced.npz"))


@pytest.fixture(scope="module")
def clip_model():
    g = np.load(os.path.join(GOLD, "clip_reduced_257.npz"))
    cs = cw.ClipVisionShape(**{str(k): (float(v) if k == "eps" else int(v)) for k, v in zip(g["shape_fields"], g["shape_values"])})
    return sfa.CLIPModel(state_dict=cw.synth_clip_state_dict(cs, int(g["seed"])), shape=cs, device=DEV)


@pytest.fixture(scope="module")
def vae():
    return sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.VAE_REDUCED, seed=0, encoder=True), device=DEV, shape=vw.VAE_REDUCED)


@pytest.fixture(scope="module")
def embedder():
    g = np.load(os.path.join(GOLD, "pose_small_a_dense.npz"))
    return sfa.PoseEmbedder(pw.synth_pose_state_dict(int(g["seed"])), device=DEV)


@pytest.fixture(scope="module")
def gen(gold):
    """An i2v generator that also takes pose tokens (tests 3 and 5)."""
    sd = wt.synth_state_dict(S, seed=int(gold["seed"]), pose=True)
    return sfa.WanDiffusionWrapper(shape=S, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV)


@pytest.fixture(scope="module")
def images():
    return cw.synth_frames(21, 1, 128, 128)[:, 0], cw.synth_frames(22, 1, 128, 128)[:, 0]


@pytest.fixture(scope="module")
def ref_pose():
    return pw.synth_pose_image(93, 128, 128, "skeleton")


@pytest.fixture(scope="module")
def whole(gen, clip_model, vae, embedder, images, ref_pose):
    """The whole-clip conditioning of the multi-step pipeline for 5 latent frames of 128 x 128: computed once, never changed."""
    args = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, num_frame_per_block=1,
                           negative_prompt="NEG", guidance_scale=3.0)
    pipe = sfa.CausalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=object(), vae=vae, image_encoder=clip_model,
                                                pose_embedder=embedder)
    cond = pipe.encode_image(images[0], 17, 128, 128)
    y = cond["y"]
    return SimpleNamespace(y=y, clip=cond["clip_feature"], y_pose=y + embedder.embed_ref(ref_pose).to(y.dtype))


# ------------------------------------------------------------------------------------------ 2. incremental = whole
@pytest.mark.parametrize("steps", [[1, 1, 1, 1, 1], [1, 2, 2], [3, 2]], ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("with_map", [False, True], ids=["plain", "map"])
def test_incremental_y_equals_encode_image(whole, clip_model, vae, embedder, images, ref_pose, steps, with_map):
    cond = sfa.I2VConditioner(vae, clip_model, pose_embedder=embedder, device=DEV)
    clip_feature = cond.begin(images[0], 128, 128, ref_pose if with_map else None)
    assert torch.equal(clip_feature, whole.clip) and tuple(clip_feature.shape) == (1, 257, 320)
    parts = [cond.frames(n) for n in steps]
    assert [tuple(p.shape) for p in parts] == [(1, 20, n, 16, 16) for n in steps] and cond.position == 5
    assert tuple(whole.y.shape) == (1, 20, 5, 16, 16)
    assert torch.equal(torch.cat(parts, dim=2), whole.y_pose if with_map else whole.y)
    zeros = vae.encoder._zeros
    assert list(zeros) == [(128, 128)] and zeros[(128, 128)].shape[1] == 4 * vae.encoder.frames_per_call      # never the clip
    # the whole-clip encode still gives what it gave, after (and in between) the resumable calls
    again = cond.begin(images[0], 128, 128)
    first = cond.frames(2)
    px = torch.zeros(1, 3, 17, 128, 128, device=DEV, dtype=torch.bfloat16)
    px[0, :, 0] = images[0].to(DEV).to(torch.bfloat16)
    lat = vae.encode_to_latent(px)[0].transpose(0, 1)
    assert torch.equal(lat.to(torch.bfloat16), whole.y[0, 4:]) and torch.equal(first, whole.y[:, :, :2]) and torch.equal(again, whole.clip)
    with pytest.raises(RuntimeError, match="no clip in progress"):
        cond.frames(1)                                         # encode() took the histories: the clip has ended


# ------------------------------------------------------------------------------------------ the hand-written rollout
def make_pipeline(generator, vae, **kw):
    args = SimpleNamespace(denoising_step_list=STEPS, warp_denoising_step=True, independent_first_frame=False, num_frame_per_block=1,
                           context_noise=0)
    return sfa.CausalInferencePipeline(args, DEV, generator=generator, text_encoder=sfa.FixedTextEncoder(kw.pop("pe")), vae=vae, **kw)


def fix_noise(pipe, eps):
    q = list(eps)
    pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
    return q


def hand_rollout(generator, pipe, noise, pe, eps, y=None, clip_feature=None, tokens=None):
    """The rollout as causal_inference.py:176-244 writes it, one frame per chunk: per chunk i the 4 denoising passes with
    `y[:, :, i:i+1]` / the chunk's pose tokens, `scheduler.add_noise` with the given eps in between, then the context pass."""
    shape = generator.model.shape
    B, F, _, H, W = noise.shape
    fs = (H // 2) * (W // 2)
    kv = new_kv_cache(shape, shape.num_layers, B, 21 * fs, torch.bfloat16, DEV)
    cc = new_crossattn_cache(shape, shape.num_layers, B, torch.bfloat16, DEV)
    steps = pipe.denoising_step_list.to(DEV)
    ones = torch.ones([B, 1], device=DEV, dtype=torch.int64)
    eps = list(eps)
    out = torch.zeros_like(noise)
    for i in range(F):
        d = {"prompt_embeds": pe}
        if y is not None:
            d.update(clip_feature=clip_feature, y=y[:, :, i:i + 1])
        if tokens is not None:
            d["add_condition"] = tokens[:, i * fs:(i + 1) * fs].expand(B, -1, -1).contiguous()
        x = noise[:, i:i + 1]
        for k in range(len(STEPS)):
            _, x0 = generator.forward(x, d, ones * steps[k], kv, cc, i * fs)
            if k < len(STEPS) - 1:
                flat = x0.flatten(0, 1)
                x = pipe.scheduler.add_noise(flat, eps.pop(0).reshape(flat.shape), (ones * steps[k + 1]).flatten()).unflatten(0, x0.shape[:2])
        out[:, i:i + 1] = x0
        generator.forward(x0, d, torch.zeros_like(ones * steps[0]), kv, cc, i * fs, cache_only=True)
    return out


# ------------------------------------------------------------------------------------------ 3. few-step i2v rollout
def test_fewstep_rollout_with_an_input_image(gen, clip_model, vae, whole, images, gold):
    g = torch.Generator().manual_seed(31)
    noise, pe = bf(g, 2, 3, 16, 16, 16), bf(g, 2, 512, S.text_dim)
    eps = [bf(g, 1, 16, 16, 16) for _ in range(9)]
    one, pe1 = noise[:1], pe[:1]
    pipe = make_pipeline(gen, vae, pe=pe1, image_encoder=clip_model)
    fix_noise(pipe, eps)
    video, lat = pipe.inference(one, ["p"], input_image=images[0], return_latents=True)
    assert tuple(lat.shape) == (1, 3, 16, 16, 16) and tuple(video.shape) == (1, 9, 3, 128, 128)
    mine = hand_rollout(gen, pipe, one, pe1, eps, y=whole.y, clip_feature=whole.clip)
    assert torch.equal(lat, mine)
    # the same pipeline again: the caches are reset, not rebuilt
    fix_noise(pipe, eps)
    assert torch.equal(pipe.inference(one, ["p"], input_image=images[0], return_latents=True)[1], lat)
    # chunk by chunk
    fix_noise(pipe, eps)
    chunks = list(pipe.stream(one, ["p"], input_image=images[0]))
    assert [c[0] for c in chunks] == [0, 1, 2] and torch.equal(torch.cat([c[1] for c in chunks], dim=1), lat)
    assert tuple(chunks[0][2].shape) == (1, 1, 3, 128, 128) and tuple(chunks[1][2].shape) == (1, 4, 3, 128, 128)
    # batch 2 with one image: each sample is the bits of that sample alone
    eps2 = [bf(g, 2, 16, 16, 16) for _ in range(9)]
    pipe2 = make_pipeline(gen, vae, pe=pe, image_encoder=clip_model)
    fix_noise(pipe2, eps2)
    both = pipe2.inference(noise, ["p", "p"], input_image=images[0], return_latents=True)[1]
    for b in range(2):
        alone = make_pipeline(gen, vae, pe=pe[b:b + 1], image_encoder=clip_model)
        fix_noise(alone, [e[b:b + 1] for e in eps2])
        assert torch.equal(alone.inference(noise[b:b + 1], ["p"], input_image=images[0], return_latents=True)[1], both[b:b + 1]), b
    # another image: the branch is live, and the change is not rounding
    fix_noise(pipe, eps)
    lat2 = pipe.inference(one, ["p"], input_image=images[1], return_latents=True)[1]
    d, floor = rel(lat2, lat), float(gold["bf16_vs_fp32"])
    print(f"few-step rollout: another image moves the latents by {d:.3e} (bf16 vs fp32 of the reference: {floor:.3e})")
    assert d > 2 * floor
    # with an initial latent the warm-up pass takes frame 0 of y and the rollout goes on from frame 1
    fix_noise(pipe, eps)
    lat3 = pipe.inference(one[:, 1:], ["p"], initial_latent=lat[:, :1], input_image=images[0], return_latents=True)[1]
    assert torch.equal(lat3[:, :1], lat[:, :1]) and tuple(lat3.shape) == (1, 3, 16, 16, 16)


# ------------------------------------------------------------------------------------------ 4. pose
def test_fewstep_rollout_with_a_pose_clip(embedder):
    shape = sfa.WAN_REDUCED
    t2v = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0, pose=True), timestep_shift=5.0, is_causal=True,
                                  device=DEV)
    g = torch.Generator().manual_seed(91)
    noise, pe = bf(g, 1, 3, 16, 8, 12), bf(g, 1, 512, shape.text_dim)
    eps = [bf(g, 1, 16, 8, 12) for _ in range(9)]
    clip = pw.synth_pose_clip(92, 9, 64, 96, "skeleton")             # 9 pose frames -> 3 latent frames of 4 x 6 tokens: 3 chunks
    image = pw.synth_pose_image(93, 64, 96, "skeleton")
    assert pw.pose_plan(*clip.shape[1:]) == (3, 4, 6)
    pipe = make_pipeline(t2v, sfa.IdentityVAE(), pe=pe, pose_embedder=embedder)
    pairs = []
    fwd_pair = t2v.forward_pair
    t2v.forward_pair = lambda *a, **k: (pairs.append(k.get("add_conditions")), fwd_pair(*a, **k))[1]
    try:
        fix_noise(pipe, eps)
        lat = pipe.inference(noise, ["p"], dwpose_data=clip, random_ref_dwpose=image, return_latents=True)[1]
        assert len(pairs) == 2 and all(p is not None and p[0].data_ptr() != p[1].data_ptr() for p in pairs)     # pairs ran, with two chunks' tokens
        pipe.pair_context_with_next = False
        fix_noise(pipe, eps)
        unpaired = pipe.inference(noise, ["p"], dwpose_data=clip, random_ref_dwpose=image, return_latents=True)[1]
        assert len(pairs) == 2 and torch.equal(unpaired, lat)
        pipe.pair_context_with_next = True
    finally:
        del t2v.forward_pair
    tokens = embedder.embed(clip)[0]
    mine = hand_rollout(t2v, pipe, noise, pe, eps, tokens=tokens)
    assert torch.equal(lat, mine)
    fix_noise(pipe, eps)
    chunks = list(pipe.stream(noise, ["p"], skip_last_context=False, dwpose_data=clip, random_ref_dwpose=image))
    assert torch.equal(torch.cat([c[1] for c in chunks], dim=1), lat)
    # already-embedded tokens: the bits of the frames they were embedded from
    fix_noise(pipe, eps)
    emb = embedder.encode_pose(clip, image)[0]
    assert torch.equal(pipe.inference(noise, ["p"], dwpose_data_emb=emb, return_latents=True)[1], lat)
    # the tokens are live: zeroed pose frames give other latents, and no pose at all yet others
    fix_noise(pipe, eps)
    dark = pipe.inference(noise, ["p"], dwpose_data=torch.zeros_like(clip), random_ref_dwpose=image, return_latents=True)[1]
    fix_noise(pipe, eps)
    plain = pipe.inference(noise, ["p"], return_latents=True)[1]
    print(f"few-step rollout: zeroed pose frames move the latents by {rel(dark, lat):.3e}, no pose by {rel(plain, lat):.3e}")
    assert not torch.equal(dark, lat) and not torch.equal(plain, lat) and not torch.equal(plain, dark)
    assert torch.equal(plain, hand_rollout(t2v, pipe, noise, pe, eps))


def test_tokens_in_the_callers_dict_reach_every_pass(embedder):
    """`add_condition` handed through the condition dict (the reference's convention; no pose keywords): every pass of every
    chunk takes it, one call per pass, and `forward_pair` refuses such a dict rather than drop the tokens."""
    shape = sfa.WAN_REDUCED
    t2v = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0, pose=True), timestep_shift=5.0, is_causal=True,
                                  device=DEV)
    g = torch.Generator().manual_seed(17)
    noise, pe = bf(g, 1, 3, 16, 8, 12), bf(g, 1, 512, shape.text_dim)
    eps = [bf(g, 1, 16, 8, 12) for _ in range(9)]
    one = embedder.embed(pw.synth_pose_clip(92, 9, 64, 96, "skeleton"))[0][:, :24]       # one frame's tokens, for every chunk
    args = SimpleNamespace(denoising_step_list=STEPS, warp_denoising_step=True, independent_first_frame=False, num_frame_per_block=1,
                           context_noise=0)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=t2v, text_encoder=lambda text_prompts: {"prompt_embeds": pe, "add_condition": one},
                                       vae=sfa.IdentityVAE())
    pairs = []
    fwd_pair = t2v.forward_pair
    t2v.forward_pair = lambda *a, **k: (pairs.append(1), fwd_pair(*a, **k))[1]
    try:
        fix_noise(pipe, eps)
        lat = pipe.inference(noise, ["p"], return_latents=True)[1]
    finally:
        del t2v.forward_pair
    assert pairs == [] and torch.equal(lat, hand_rollout(t2v, pipe, noise, pe, eps, tokens=one.repeat(1, 3, 1)))
    assert not torch.equal(lat, hand_rollout(t2v, pipe, noise, pe, eps))
    with pytest.raises(ValueError, match="add_conditions="):
        t2v.forward_pair(noise[:, :1], torch.zeros(1, 1, device=DEV), noise[:, 1:2], torch.zeros(1, 1, device=DEV),
                         {"prompt_embeds": pe, "add_condition": one}, pipe.kv_cache1, pipe.crossattn_cache, 0, 24)


# ------------------------------------------------------------------------------------------ 5. image + pose
def test_fewstep_rollout_with_image_and_pose(gen, clip_model, vae, embedder, whole, images, ref_pose):
    g = torch.Generator().manual_seed(57)
    noise, pe = bf(g, 1, 3, 16, 16, 16), bf(g, 1, 512, S.text_dim)
    eps = [bf(g, 1, 16, 16, 16) for _ in range(9)]
    clip = pw.synth_pose_clip(94, 9, 128, 128, "skeleton")
    assert pw.pose_plan(*clip.shape[1:]) == (3, 8, 8)
    pipe = make_pipeline(gen, vae, pe=pe, image_encoder=clip_model, pose_embedder=embedder)
    seen = []
    fwd = gen.forward
    gen.forward = lambda *a, **k: (seen.append(k["conditional_dict"]["y"]), fwd(*a, **k))[1]
    try:
        fix_noise(pipe, eps)
        lat = pipe.inference(noise, ["p"], input_image=images[0], dwpose_data=clip, random_ref_dwpose=ref_pose, return_latents=True)[1]
    finally:
        del gen.forward
    assert len(seen) == 15
    for k, y in enumerate(seen):                               # the y the generator receives includes the reference-pose map
        assert torch.equal(y, whole.y_pose[:, :, k // 5:k // 5 + 1]) and not torch.equal(y, whole.y[:, :, k // 5:k // 5 + 1])
    mine = hand_rollout(gen, pipe, noise, pe, eps, y=whole.y_pose, clip_feature=whole.clip, tokens=embedder.embed(clip)[0])
    assert torch.equal(lat, mine)
    image_only = hand_rollout(gen, pipe, noise, pe, eps, y=whole.y, clip_feature=whole.clip)
    assert not torch.equal(image_only, lat)


# ------------------------------------------------------------------------------------------ 6. the CLI
def test_generate_cli_fewstep_image_and_pose(tmp_path):
    from PIL import Image
    rgb = ((cw.synth_frames(5, 1, 50, 70)[:, 0].float() * 0.5 + 0.5) * 255).round().clamp(0, 255).byte()
    Image.fromarray(rgb.permute(1, 2, 0).numpy()).save(tmp_path / "a.png")
    torch.save({"dwpose_data": pw.synth_pose_clip(92, 9, 64, 96, "skeleton"), "random_ref_dwpose": pw.synth_pose_image(93, 64, 96, "skeleton")},
               tmp_path / "pose.pt")
    (tmp_path / "prompts.txt").write_text("a red fox\n")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\n"
                   "independent_first_frame: false\nmodel_kwargs:\n  model_name: reduced-i2v\n  timestep_shift: 5.0\n")
    out = tmp_path / "out"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", str(cfg), "--data_path",
           str(tmp_path / "prompts.txt"), "--output_folder", str(out), "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height", "8",
           "--latent_width", "12", "--seed", "5", "--vae_random_init_seed", "0", "--input_image", str(tmp_path / "a.png"),
           "--clip_random_init_seed", "0", "--pose_path", str(tmp_path / "pose.pt"), "--pose_random_init_seed", "0"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stderr[-2000:]
    lat, vid = torch.load(out / "0-0.pt"), torch.load(out / "0-0.video.pt")
    assert lat.shape == (3, 16, 8, 12) and bool(lat.float().abs().sum() > 0) and bool(torch.isfinite(lat.float()).all())
    assert vid.shape == (9, 64, 96, 3) and vid.dtype == torch.uint8
