"""GPU tests of the JPEG encoder (csrc/jpeg.hip behind `JpegEncoder`) against the float64 host reference
`jpeg_reference` and against PIL.  Run with `-m gpu` (`-s` shows the measured figures).

- coefficients: the transform kernel against the reference (float64) of the same definition: at most 1e-4 of the
  coefficients may differ, each by exactly 1 (a quotient within rounding of a tie); none on a constant frame whose
  quotients are not ties (a grey frame with an odd level-shifted value sits exactly on one at quality 50, 8 y / 16, so
  the grey frame here has an even one; the coloured one is generic);
- entropy coding: for the GPU's own coefficient buffer the reference's coder must give byte-identical files, on inputs
  built to reach 0xFF stuffing, ZRL, a non-zero 63rd coefficient, the largest DC and AC categories, all-zero blocks,
  intervals that straddle MCU rows, a short last interval, more than 8 intervals, and intervals of more than 64 blocks;
- whole files: PIL decodes them, not more than 0.1 dB below and not more than 1 % larger than PIL's own encode;
- input forms, batching, a second stream beside a rollout, and `CausalInferencePipeline.stream(frame_encoder=...)`."""
import io
import os
import subprocess
import sys
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import self_forcing_amd as sfa
from self_forcing_amd import jpeg_reference as jr
from self_forcing_amd import taehv_weights as tw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PIL_SUB = {"420": 2, "444": 0}
COEF_CAP = 1e-4       # share of coefficients that may differ (by 1) between the kernel and the float64 reference
PSNR_SLACK = 0.1      # dB below PIL's own encode
SIZE_SLACK = 1.01     # x PIL's own size


def frames_pm1(kind, n, h, w, seed=0):
    """float32 [n, 3, h, w] in about [-1.1, 1.1]: smooth, smooth plus noise, or uniform random"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    phase = torch.arange(n, dtype=torch.float32).reshape(n, 1, 1)
    smooth = torch.stack([0.8 * torch.sin(xx / 17 + yy / 9 + phase), 0.8 * torch.cos(xx / 11 - phase), 0.7 * torch.sin(yy / 7 + 2 * phase)], 1)
    if kind == "smooth":
        return smooth
    if kind == "noise":
        return smooth + 0.1 * torch.randn(n, 3, h, w, generator=g)
    return torch.rand(n, 3, h, w, generator=g) * 2.2 - 1.1


def truncate(x, value_range=(-1, 1)):
    """the torch expression of the definition, on whatever device x is: uint8 [n, h, w, 3]"""
    x = x.float()
    y = x.clamp(-1, 1) * 127.5 + 127.5 if value_range == (-1, 1) else 255.0 * x.clamp(0, 1)
    return y.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def pil_encode(u8, quality, subsampling, restart_interval):
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, "JPEG", quality=quality, subsampling=PIL_SUB[subsampling], restart_marker_blocks=restart_interval)
    return buf.getvalue()


def reference_files(enc, coef, h, w):
    return [jr.encode_coefficients(c, h, w, enc.quality, enc.subsampling, enc.restart_interval) for c in coef.cpu().numpy()]


# ============================================================================================== coefficients
@pytest.mark.parametrize("subsampling", ["420", "444"])
@pytest.mark.parametrize("h,w,kinds", [(480, 832, ("noise", "random")), (16, 16, ("noise",)), (48, 80, ("noise",)), (64, 1008, ("noise",))])
def test_coefficients_against_the_float64_reference(h, w, kinds, subsampling):
    for kind in kinds:
        x = frames_pm1(kind, 2, h, w, seed=h + w)
        u8 = jr.to_uint8(x.numpy())
        for quality in (100, 90, 50):
            enc = sfa.JpegEncoder(quality, subsampling, device=DEV)
            got = enc.coefficients(x.to(DEV)).cpu().numpy().astype(np.int64)
            ref = jr.coefficients(u8, quality, subsampling).astype(np.int64)
            assert got.shape == ref.shape
            diff = np.abs(got - ref)
            share = np.count_nonzero(diff) / diff.size
            print(f"{h}x{w} {kind} q{quality} {subsampling}: {np.count_nonzero(diff)} of {diff.size} coefficients differ ({share:.2e}), max {diff.max()}")
            assert diff.max() <= 1
            assert share <= COEF_CAP


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_constant_frames_have_no_differing_coefficient(subsampling):
    grey = torch.full((1, 3, 32, 48), 200, dtype=torch.uint8)                       # y = 72: 8 y / Q is no tie for Q = 1, 3, 16
    colour = torch.tensor([37, 190, 111], dtype=torch.uint8).reshape(1, 3, 1, 1).expand(1, 3, 32, 48)
    for frame in (grey, colour):
        u8 = frame.permute(0, 2, 3, 1).contiguous()
        for quality in (100, 90, 50):
            enc = sfa.JpegEncoder(quality, subsampling, device=DEV)
            got = enc.coefficients(u8.to(DEV)).cpu().numpy()
            assert np.array_equal(got, jr.coefficients(u8.numpy(), quality, subsampling))
            assert not got[:, :, 1:].any()


# ============================================================================================== entropy coding
def idct_frame(blocks):
    """[by, bx, 64] zigzagged luminance coefficients (quantiser 1) -> grey uint8 frame [1, 8 by, 8 bx, 3]"""
    by, bx, _ = blocks.shape
    nat = np.zeros((by, bx, 64))
    nat[..., jr.ZIGZAG] = blocks
    pix = jr.DCT.T @ nat.reshape(by, bx, 8, 8) @ jr.DCT + 128
    img = np.clip(np.rint(pix.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)), 0, 255).astype(np.uint8)
    return np.repeat(img[None, :, :, None], 3, axis=3)


def crafted_inputs():
    """name -> (uint8 frames [n, h, w, 3], quality, restart_interval or None, predicate on the coefficient buffer).  The two
    frames built from single coefficients use quality 90: its quantisers (3 and more) swallow the +-0.5 of rounding the pixels
    to 8 bit, so the zero runs stay zero."""
    rng = np.random.default_rng(7)
    out = {}
    out["stuffing"] = (rng.integers(0, 256, (1, 64, 96, 3), dtype=np.uint8), 100, None, None)
    zrl = np.zeros((4, 6, 64))
    zrl[..., 0] = rng.integers(-300, 300, (4, 6))
    zrl[..., 40] = 60                                         # one high-frequency coefficient behind 39 zeros: two ZRL, then EOB
    out["zrl"] = (idct_frame(zrl), 90, 3, lambda c: bool(((c[..., 1:40] == 0).all(-1) & (c[..., 40] != 0)).any()))
    last = np.zeros((4, 6, 64))
    last[..., 63] = 70                                        # a non-zero 63rd coefficient: three ZRL and no EOB
    last[::2, :, 5] = -9
    out["no_eob"] = (idct_frame(last), 90, 4, lambda c: bool((c[..., 63] != 0).any()))
    sat = np.zeros((1, 64, 96, 3), np.uint8)
    yy, xx = np.mgrid[0:64, 0:96]
    sat[0, :32][((yy[:32] // 8 + xx[:32] // 8) % 2 == 0)] = 255       # block checkerboard: DC differences of +-2040, category 11
    sat[0, 32:][((yy[32:] + xx[32:]) % 2 == 0)] = 255                 # pixel checkerboard: the largest AC coefficients, category 10
    out["saturated"] = (sat, 100, 5, lambda c: c[..., 0].max() >= 1016 and c[..., 0].min() <= -1024 and int(np.abs(c[..., 1:].astype(int)).max()) >= 512)
    zero = np.full((1, 48, 80, 3), 128, np.uint8)             # y = 0 everywhere: nothing but all-zero blocks
    zero[0, 16:32, 16:48] = rng.integers(0, 256, (16, 32, 3), dtype=np.uint8)
    out["zero_blocks"] = (zero, 90, 4, lambda c: bool((c == 0).all(-1).any()))
    return out


@pytest.mark.parametrize("subsampling", ["420", "444"])
@pytest.mark.parametrize("name", ["stuffing", "zrl", "no_eob", "saturated", "zero_blocks"])
def test_entropy_coding_is_exact_on_crafted_inputs(name, subsampling):
    u8, quality, ri, predicate = crafted_inputs()[name]
    enc = sfa.JpegEncoder(quality, subsampling, restart_interval=ri, device=DEV)
    dev = torch.from_numpy(u8).to(DEV)
    coef = enc.coefficients(dev)
    files = enc.encode(dev)
    h, w = u8.shape[1:3]
    assert files == reference_files(enc, coef, h, w)
    assert files == enc.encode_coefficients(coef, h, w)                       # the entropy entry point alone
    if predicate is not None:
        assert predicate(coef.cpu().numpy())
    if name == "stuffing":
        assert all(b"\xff\x00" in f for f in files)
    for f, src in zip(files, u8):
        assert decode(f).shape == src.shape


@pytest.mark.parametrize("subsampling,h,w,ri", [
    ("420", 48, 80, 3),        # 5 MCUs per row: intervals straddle MCU rows; 15 MCUs = 5 intervals
    ("420", 48, 80, 4),        # a short last interval (3 MCUs)
    ("444", 48, 80, 4),        # 60 MCUs = 15 intervals: RST7 wraps to RST0
    ("420", 64, 1008, 26),     # 156 blocks per interval: three chunks of 64 lanes, bits carried between them
    ("444", 64, 1008, 63),     # 189 blocks per interval
    ("420", 48, 80, 1000),     # one interval for the whole frame, no RST marker
    ("420", 480, 832, None),   # the default at the production size: 156 intervals
    ("444", 480, 832, None),
])
def test_entropy_coding_is_exact_across_interval_shapes(subsampling, h, w, ri):
    x = frames_pm1("random" if h < 480 else "noise", 2, h, w, seed=ri or 1).to(DEV)
    for quality in (100, 50):
        enc = sfa.JpegEncoder(quality, subsampling, restart_interval=ri, device=DEV)
        coef = enc.coefficients(x)
        files = enc.encode(x)
        assert files == reference_files(enc, coef, h, w)
        mcus = (h // jr.mcu_size(subsampling)) * (w // jr.mcu_size(subsampling))
        n_rst = sum(1 for i in range(len(files[0]) - 1) if files[0][i] == 0xFF and 0xD0 <= files[0][i + 1] <= 0xD7)
        assert n_rst == -(-mcus // enc.restart_interval) - 1


def test_out_of_range_coefficients_are_reported():
    enc = sfa.JpegEncoder(100, "420", device=DEV)
    coef = torch.zeros(1, 6, 64, dtype=torch.int16, device=DEV)
    coef[0, 1, 0] = 3000                                                      # a DC difference of category 12
    with pytest.raises(sfa._lib.SfHipError, match="baseline range"):
        enc.encode_coefficients(coef, 16, 16)
    coef[0, 1, 0] = 0
    assert decode(enc.encode_coefficients(coef, 16, 16)[0]).shape == (16, 16, 3)


# ============================================================================================== whole files
@pytest.mark.parametrize("quality,subsampling", [(100, "420"), (100, "444"), (90, "420"), (50, "444")])
def test_whole_files_against_pil(quality, subsampling):
    enc = sfa.JpegEncoder(quality, subsampling, device=DEV)
    for kind in ("smooth", "noise", "random"):
        x = frames_pm1(kind, 2, 480, 832, seed=3)
        u8 = jr.to_uint8(x.numpy())
        files = enc.encode(x.to(DEV))
        assert len(files) == 2
        for f, src in zip(files, u8):
            pil = pil_encode(src, quality, subsampling, enc.restart_interval)
            p_gpu, p_pil = psnr(decode(f), src), psnr(decode(pil), src)
            print(f"{kind} q{quality} {subsampling}: PSNR {p_gpu:.3f} dB (PIL {p_pil:.3f}), {len(f)} bytes (PIL {len(pil)})")
            assert p_gpu >= p_pil - PSNR_SLACK
            assert len(f) <= SIZE_SLACK * len(pil)


# ============================================================================================== input forms
@pytest.mark.parametrize("subsampling", ["420", "444"])
@pytest.mark.parametrize("value_range", [(-1, 1), (0, 1)])
def test_float_inputs_equal_pretruncated_uint8(value_range, subsampling):
    g = torch.Generator().manual_seed(11)
    lo, hi = value_range
    x = torch.rand(2, 3, 32, 64, generator=g) * (hi - lo) * 1.2 + lo - 0.1 * (hi - lo)      # 10 % beyond either end
    x[0, :, 0, :8] = torch.tensor([lo, hi, lo - 0.5, hi + 0.5, float(lo) + 1e-7, float(hi) - 1e-7, 0.0, 0.5])
    x[1, 0, 1] = torch.linspace(lo, hi, 64)
    enc = sfa.JpegEncoder(90, subsampling, value_range=value_range, device=DEV)
    for frames in (x.to(DEV), x.to(torch.bfloat16).to(DEV)):
        u8 = truncate(frames, value_range)                                    # bf16 is widened to fp32 first
        assert torch.equal(enc.coefficients(frames), enc.coefficients(u8))
        assert enc.encode(frames) == enc.encode(u8)
    five = x.to(DEV).reshape(1, 2, 3, 32, 64)
    assert enc.encode(five) == enc.encode(x.to(DEV))                          # [B, T, 3, H, W]
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(1, 3, 28, 64, device=DEV))                     # off the MCU grid of either subsampling
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(1, 3, 32, 64, device=DEV, dtype=torch.float16))


@pytest.mark.parametrize("value_range", [(-1, 1), (0, 1)])
def test_truncation_on_a_large_sample(value_range):
    """2.4 M values per range: a fused multiply-add in `clamp * 127.5 + 127.5` moves about 4e-6 of them across an integer,
    too few for the small frames above to meet one."""
    lo, hi = value_range
    x = torch.rand(2, 3, 480, 832, generator=torch.Generator().manual_seed(13)) * (hi - lo) * 1.1 + lo - 0.05 * (hi - lo)
    u8 = truncate(x.to(DEV), value_range)
    assert np.array_equal(u8.cpu().numpy(), jr.to_uint8(x.numpy(), value_range))         # torch on the GPU = the host definition
    enc = sfa.JpegEncoder(100, "444", value_range=value_range, device=DEV)
    assert torch.equal(enc.coefficients(x.to(DEV)), enc.coefficients(u8))
    xb = x.to(torch.bfloat16).to(DEV)
    assert torch.equal(enc.coefficients(xb), enc.coefficients(truncate(xb, value_range)))


# ============================================================================================== batching and streams
def test_batch_equals_single_frame_calls():
    x = frames_pm1("noise", 5, 48, 80, seed=5).to(DEV)
    for subsampling in ("420", "444"):
        enc = sfa.JpegEncoder(90, subsampling, restart_interval=4, device=DEV)
        together = enc.encode(x)
        assert together == [enc.encode(x[i:i + 1])[0] for i in range(5)]
        data, offsets = enc.encode_to_device(x)
        torch.cuda.synchronize()
        offsets = offsets.cpu().tolist()
        assert int(enc.status.cpu()) == 0 and len(offsets) == 6 and offsets[0] == 0
        host = data[:offsets[-1]].cpu().numpy().tobytes()
        assert [host[a:b] for a, b in zip(offsets, offsets[1:])] == together


def test_side_stream_beside_a_rollout_is_bit_identical():
    H, W = 8, 12
    g = torch.Generator().manual_seed(41)
    noise = torch.randn(1, 6, 16, H, W, generator=g).to(torch.bfloat16).to(DEV)
    pe = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=2, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0), timestep_shift=5.0,
                                  is_causal=True, device=DEV)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=sfa.IdentityVAE())
    x = frames_pm1("noise", 4, 480, 832, seed=9).to(DEV)
    enc = sfa.JpegEncoder(100, "420", device=DEV)
    alone = enc.encode(x)
    torch.cuda.synchronize()

    def rollout():
        torch.cuda.set_device(0)
        with torch.no_grad():
            pipe.inference(noise, ["p"])
        torch.cuda.synchronize()

    side = torch.cuda.Stream(device=DEV)
    worker = threading.Thread(target=rollout)
    worker.start()
    beside = []
    with torch.cuda.stream(side):
        for _ in range(2):
            beside.append(enc.encode(x))
    worker.join()
    torch.cuda.synchronize()
    assert beside[0] == alone and beside[1] == alone


# ============================================================================================== pipeline
def test_pipeline_stream_with_a_frame_encoder():
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
    plain = []
    for chunk in pipe.stream(noise, ["p"]):
        assert len(chunk) == 3                                                # without an encoder: the 3-tuples of before
        plain.append((chunk[0], chunk[1].clone(), chunk[2].clone()))
    assert [c[2].shape[1] for c in plain] == [5, 8, 8]

    enc01 = sfa.JpegEncoder(90, "420", value_range=(0, 1), device=DEV)
    for overlap in (False, True):
        q.extend(eps)
        chunks = [(i, x.clone(), p.clone(), f) for i, x, p, f in pipe.stream(noise, ["p"], overlap_decode=overlap, frame_encoder=enc01)]
        assert len(chunks) == 3
        for (i, x, p, files), (i0, x0, p0) in zip(chunks, plain):
            assert i == i0 and torch.equal(x, x0) and torch.equal(p, p0)          # the other three entries are what they were
            assert len(files) == p.shape[0] * p.shape[1]
            assert files == enc01.encode(p)
            u8 = truncate(p[0], (0, 1)).cpu().numpy()
            for f, src in zip(files, u8):
                pil = pil_encode(src, 90, "420", enc01.restart_interval)
                assert psnr(decode(f), src) >= psnr(decode(pil), src) - PSNR_SLACK
    # the demo's form: an encoder for [-1, 1] is fed the decoder's output, not the rescaled pixels
    q.extend(eps)
    enc = sfa.JpegEncoder(90, "420", device=DEV)
    for (i, x, p, files), (i0, x0, p0) in zip(pipe.stream(noise, ["p"], frame_encoder=enc), plain):
        assert torch.equal(p, p0) and len(files) == p.shape[1]
        u8 = truncate(p[0], (0, 1)).cpu().numpy()
        for f, src in zip(files, u8):
            pil = pil_encode(src, 90, "420", enc.restart_interval)
            assert psnr(decode(f), src) >= psnr(decode(pil), src) - PSNR_SLACK


def test_generate_writes_an_mjpeg_file_that_plays(tmp_path):
    """generate.py --video_format mjpeg: <idx>-<sample>.avi with every frame a JPEG PIL reads, the same seed's default run
    (the uint8 .video.pt, which is unchanged) as the picture it shows."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\n"
                   "model_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n")
    prompts = tmp_path / "p.txt"
    prompts.write_text("a red fox\n")
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", str(cfg), "--data_path", str(prompts),
            "--random_init_seed", "0", "--num_output_frames", "2", "--latent_height", "8", "--latent_width", "12", "--seed", "5",
            "--taehv_random_init_seed", "0"]
    for folder, extra in (("pt", []), ("avi", ["--video_format", "mjpeg", "--jpeg_quality", "95", "--jpeg_subsampling", "444"])):
        res = subprocess.run(base + ["--output_folder", str(tmp_path / folder)] + extra, capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, res.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "pt")) == ["0-0.pt", "0-0.video.pt"]                  # the default files are what they were
    assert sorted(os.listdir(tmp_path / "avi")) == ["0-0.avi", "0-0.pt"]
    video = torch.load(tmp_path / "pt" / "0-0.video.pt").numpy()                              # [T, H, W, 3] uint8
    frames = sfa.mjpeg.read_avi(str(tmp_path / "avi" / "0-0.avi"))
    assert len(frames) == video.shape[0] == 5 and video.shape[1:] == (64, 96, 3)
    data = open(tmp_path / "avi" / "0-0.avi", "rb").read()
    assert data[8:12] == b"AVI " and b"MJPG" in data[:256] and int.from_bytes(data[4:8], "little") == len(data) - 8
    for f, src in zip(frames, video):
        pil = pil_encode(src, 95, "444", 21)
        assert psnr(decode(f), src) >= psnr(decode(pil), src) - PSNR_SLACK
