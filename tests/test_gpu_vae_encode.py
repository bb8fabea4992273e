"""GPU tests of the VAE encode path (pixels -> latents, image-to-video): the strided convolution gathers and the
pixel / latent conversions against plain fp32 torch, the whole encode against the golden vectors recorded from the
reference (`tools/make_golden_vae_encode.py`), its causality and chunking invariants, and I2V end to end.
Run with `-m gpu`."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import _lib, ops, vae_weights as vw
from self_forcing_amd.vae import repack_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_vae_encode import pixels  # noqa: E402  (the fixtures' seeded pixel recipe)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
TOL = 2e-2   # relative Frobenius error of the latents against the fp32 reference (the reference's own bf16 run is
             # 0.6-0.8e-2 away from it, see *_ref_bf16_rel_err in the fixtures)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def cl(x):     # [C, T, H, W] -> channels-last [T, H, W, C]
    return x.permute(1, 2, 3, 0).contiguous()


# ------------------------------------------------------------------------------------- strided convolutions
@pytest.mark.parametrize("structure", ["auto", "igemm"])
@pytest.mark.parametrize("cin,T,H,W", [(32, 1, 16, 24), (96, 3, 34, 40), (192, 2, 20, 18), (384, 1, 12, 26), (96, 5, 9, 13)])
def test_conv2d_stride2_right_bottom_padding(cin, T, H, W, structure):
    """Resample downsample: ZeroPad2d((0,1,0,1)) + Conv2d 3x3 stride 2 (vae.py:87-97), per frame."""
    g = torch.Generator().manual_seed(cin + T + H)
    x, w, b = bf((cin, T, H, W), g), bf((cin, cin, 3, 3), g, (9 * cin) ** -0.5), bf((cin,), g, 0.1)
    ref = F.conv2d(F.pad(x.float().permute(1, 0, 2, 3), (0, 1, 0, 1)), w.float(), b.float(), stride=2)   # [T, C, H/2, W/2]
    out = ops.conv_igemm(cl(x).to(DEV), repack_conv(w).to(DEV), b.to(DEV), (1, 3, 3), T, structure=structure, stride=(1, 2))
    assert out.shape == (T, H // 2, W // 2, cin)
    assert rel(out.permute(0, 3, 1, 2), ref) < 4e-3


@pytest.mark.parametrize("structure", ["auto", "igemm"])
@pytest.mark.parametrize("cin,Tin,H,W,off", [(192, 5, 8, 12, 0), (384, 3, 4, 6, 0), (96, 7, 6, 10, 1), (192, 9, 16, 16, 0)])
def test_time_conv_stride2(cin, Tin, H, W, off, structure):
    """downsample3d's time_conv: (3,1,1), temporal stride 2, no padding (vae.py:94-96), odd frame counts."""
    g = torch.Generator().manual_seed(cin + Tin)
    x, w, b = bf((cin, Tin, H, W), g), bf((cin, cin, 3, 1, 1), g, (3 * cin) ** -0.5), bf((cin,), g, 0.1)
    ref = F.conv3d(x.float()[None, :, off:], w.float(), b.float(), stride=(2, 1, 1))[0]                  # [C, Tout, H, W]
    tout = ref.shape[1]
    out = ops.conv_igemm(cl(x).to(DEV), repack_conv(w).to(DEV), b.to(DEV), (3, 1, 1), tout, t_in_offset=off, structure=structure,
                         stride=(2, 1))
    assert out.shape == (tout, H, W, cin)
    assert rel(out.permute(3, 0, 1, 2), ref) < 4e-3


def test_strided_conv_leaves_the_unstrided_result_alone():
    """stride (1, 1) is the existing convolution, bit for bit."""
    g = torch.Generator().manual_seed(3)
    x, w, b = bf((96, 3, 18, 20), g), bf((96, 96, 3, 3, 3), g, (27 * 96) ** -0.5), bf((96,), g, 0.1)
    xd, wd, bd = cl(x).to(DEV), repack_conv(w).to(DEV), b.to(DEV)
    assert torch.equal(ops.conv_igemm(xd, wd, bd, (3, 3, 3), 1), ops.conv_igemm(xd, wd, bd, (3, 3, 3), 1, stride=(1, 1)))


# ------------------------------------------------------------------------------------- conversions
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_prepare_pixels(dtype):
    g = torch.Generator().manual_seed(7)
    px = torch.rand(3, 5, 16, 24, generator=g).mul(2).sub(1).to(dtype).to(DEV)
    sub = px[:, 1:4]                                    # a chunk's frames: channel stride 5 * 16 * 24
    out = torch.full((3, 16, 24, 32), 7.0, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.lib().sf_vae_prepare_pixels(sub.data_ptr(), int(dtype == torch.float32), px.stride(0), out.data_ptr(), 3, 16, 24, 32,
                                                ops.stream_handle()), "sf_vae_prepare_pixels")
    torch.cuda.synchronize()
    ref = torch.zeros(3, 16, 24, 32)
    ref[..., :3] = sub.float().cpu().permute(1, 2, 3, 0)
    assert torch.equal(out.float().cpu(), ref.bfloat16().float())


def test_finish_latent():
    g = torch.Generator().manual_seed(8)
    T, h, w, z = 3, 6, 8, 16
    x, wt, b = bf((T, h, w, 32), g), bf((z, 32), g, 0.2), bf((z,), g, 0.1)
    mean, std = torch.tensor(vw.LATENT_MEAN), torch.tensor(vw.LATENT_STD)
    out = torch.empty(T, z, h, w, dtype=torch.float32, device=DEV)
    md, sd = mean.to(DEV), std.to(DEV)
    xd, wd, bd = x.to(DEV), wt.to(DEV), b.to(DEV)
    _lib.check(_lib.lib().sf_vae_finish_latent(xd.data_ptr(), 32, 32, wd.data_ptr(), 32, bd.data_ptr(), md.data_ptr(), sd.data_ptr(),
                                               out.data_ptr(), T, z, h, w, ops.stream_handle()), "sf_vae_finish_latent")
    torch.cuda.synchronize()
    mu = torch.einsum("thwc,kc->tkhw", x.float(), wt.float()) + b.float().view(1, z, 1, 1)
    ref = (mu - mean.view(1, z, 1, 1)) / std.view(1, z, 1, 1)
    assert rel(out, ref) < 1e-5


# ------------------------------------------------------------------------------------- whole encode
_VAES = {}


def wrapper(name, frames_per_call=4):
    key = (name, frames_per_call)
    if key not in _VAES:
        g = np.load(os.path.join(GOLD, f"vae_encode_{name}.npz"))
        shape = vw.VAE_REDUCED if int(g["shape_dim"]) == vw.VAE_REDUCED.dim else vw.WAN_VAE
        sd = vw.synth_vae_state_dict(shape, seed=int(g["seed"]), encoder=True)
        _VAES[key] = (sfa.WanVAEWrapper(sd, device=DEV, shape=shape, frames_per_call=frames_per_call), g)
    return _VAES[key]


@pytest.mark.parametrize("name", ["reduced", "full"])
@pytest.mark.parametrize("which", ["clip", "image"])
def test_encode_vs_reference_golden(name, which):
    vae, g = wrapper(name)
    x = pixels(tuple(int(d) for d in g[f"{which}_shape"]), int(g["seed"]) + (which == "image"))
    ref = torch.from_numpy(g[f"{which}_f32"]).permute(0, 2, 1, 3, 4)            # [B, F, 16, h, w]
    out = vae.encode_to_latent(x.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == ref.shape
    err = rel(out, ref)
    print(f"{name} {which}: rel err {err:.4f} (reference bf16 {float(g[f'{which}_ref_bf16_rel_err']):.4f})")
    assert err < TOL


def test_encode_is_causal_and_drops_trailing_frames():
    vae, g = wrapper("reduced")
    x = pixels((1, 3, 9, 48, 64), 0).to(DEV)
    full = vae.encode_to_latent(x)
    assert full.shape[1] == 3
    for k in range(3):
        assert torch.equal(vae.encode_to_latent(x[:, :, :1 + 4 * k]), full[:, :1 + k])
    assert torch.equal(vae.encode_to_latent(x[:, :, :6]), vae.encode_to_latent(x[:, :, :5]))
    assert torch.equal(vae.encode_to_latent(x[:, :, :8]), full[:, :2])


@pytest.mark.parametrize("fpc", [1, 2])
def test_chunks_per_call_are_bit_identical(fpc):
    """G = 4 chunks per C call vs fewer (which also restarts the sliding windows)."""
    x = pixels((1, 3, 17, 48, 64), 3).to(DEV)
    a = wrapper("reduced", 4)[0].encode_to_latent(x)
    b = wrapper("reduced", fpc)[0].encode_to_latent(x)
    assert a.shape == (1, 5, 16, 6, 8)
    assert torch.equal(a, b)


def test_batch_and_repeat_are_bit_identical():
    vae, _ = wrapper("reduced")
    x = torch.cat([pixels((1, 3, 5, 48, 64), 4), pixels((1, 3, 5, 48, 64), 5)]).to(DEV)
    both = vae.encode_to_latent(x)
    assert torch.equal(both[:1], vae.encode_to_latent(x[:1]))
    assert torch.equal(both[1:], vae.encode_to_latent(x[1:]))
    assert torch.equal(both, vae.encode_to_latent(x))               # caches are cleared between encodes
    assert torch.equal(vae.encode_to_latent(x.float()), both)       # float32 pixels of bf16 values: same input
    with pytest.raises(ValueError, match="multiples of 8"):
        vae.encode_to_latent(x[..., :60])


def test_decoder_only_state_dict_still_raises_naming_the_tensors():
    vae = sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.VAE_REDUCED, seed=0), device=DEV, shape=vw.VAE_REDUCED)
    with pytest.raises(NotImplementedError, match="encoder.conv1.weight"):
        vae.encode_to_latent(torch.zeros(1, 3, 1, 32, 32, device=DEV))


# ------------------------------------------------------------------------------------- image-to-video
def test_i2v_rollout_reduced():
    shape = vw.VAE_REDUCED
    vae = sfa.WanVAEWrapper(vw.synth_vae_state_dict(shape, seed=0, encoder=True), device=DEV, shape=shape)
    image = pixels((1, 3, 1, 64, 96), 9).to(DEV)
    init = vae.encode_to_latent(image).to(torch.bfloat16)
    assert init.shape == (1, 1, 16, 8, 12)
    sd = sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0)
    g = torch.Generator().manual_seed(4)
    pe = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    noise = torch.randn(1, 4, 16, 8, 12, generator=g).to(torch.bfloat16).to(DEV)
    eps = [torch.randn(1, 2, 16, 8, 12, generator=g).to(torch.bfloat16) for _ in range(6)]

    def run(initial):
        args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=True,
                               num_frame_per_block=2, context_noise=0)
        gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV)
        pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=sfa.IdentityVAE())
        q = list(eps)
        pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
        return pipe.inference(noise, ["p"], initial_latent=initial, return_latents=True)[1]

    lat = run(init)
    assert lat.shape == (1, 5, 16, 8, 12)
    assert torch.equal(lat[:, :1], init)
    assert torch.equal(run(init.clone()), lat)
    assert rel(lat, run(torch.zeros_like(init))) > 1e-3           # the image conditions the rollout
    video = vae.decode_to_pixel(lat)
    assert video.shape == (1, 17, 3, 64, 96) and torch.isfinite(video).all()


def test_generate_cli_i2v(tmp_path):
    from PIL import Image
    data = tmp_path / "data"
    (data / "16-9").mkdir(parents=True)
    rgb = ((pixels((1, 3, 1, 50, 70), 11)[0, :, 0].float() * 0.5 + 0.5) * 255).round().clamp(0, 255).byte()
    Image.fromarray(rgb.permute(1, 2, 0).numpy()).save(data / "16-9" / "a.png")
    (data / "target_crop_info_16-9.json").write_text(json.dumps([{"file_name": "a.png", "caption": "a red fox"}]))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\n"
                   "independent_first_frame: true\nmodel_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n")
    out = tmp_path / "out"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", str(cfg), "--data_path",
           str(data), "--i2v", "--output_folder", str(out), "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height",
           "8", "--latent_width", "12", "--seed", "5", "--vae_random_init_seed", "0", "--num_samples", "2"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=700)
    assert res.returncode == 0, res.stderr[-2000:]
    init = torch.load(out / "0.initial_latent.pt")
    a, b = torch.load(out / "0-0.pt"), torch.load(out / "0-1.pt")
    assert init.shape == (1, 16, 8, 12) and a.shape == b.shape == (3, 16, 8, 12)
    assert torch.equal(a[:1], init) and torch.equal(b[:1], init) and not torch.equal(a, b)
    vid = torch.load(out / "0-0.video.pt")
    assert vid.shape == (9, 64, 96, 3) and vid.dtype == torch.uint8
    # the same image encoded in process, through the same resize / normalisation
    sys.path.insert(0, ROOT)
    import generate
    img = generate.load_image(str(data / "16-9" / "a.png"), 64, 96)[None, :, None].to(DEV, torch.bfloat16)
    vae = sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.WAN_VAE, seed=0, encoder=True), device=DEV)
    assert torch.equal(vae.encode_to_latent(img).to(torch.bfloat16)[0].cpu(), init)
