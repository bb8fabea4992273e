"""Host-side tests of the TAEHV tiny decoder (no GPU): the weight layout against the reference's state_dict, the seeded
weights, the kt = 2 repack of a MemBlock's first convolution, the TGrow fold, the FLOP count, the frame bookkeeping,
TGrow row patching, the upscale switches, and the argument checks of the new C entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import taehv_weights as tw

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_param_shapes_match_the_reference_state_dict():
    g = np.load(os.path.join(GOLD, "taehv_small_a.npz"))
    ref = [(str(k), tuple(int(d) for d in str(s).split(","))) for k, s in zip(g["decoder_keys"], g["decoder_shapes"])]
    ps = tw.taehv_param_shapes()
    assert list(ps.items()) == ref
    assert len(ps) == 64 and sum(math.prod(s) for s in ps.values()) == 9_844_611
    assert next(iter(ps)) == "decoder.1.weight" and list(ps)[-1] == "decoder.22.bias"


def test_seeded_weights_are_reproducible():
    a, b, c = tw.synth_taehv_state_dict(3), tw.synth_taehv_state_dict(3), tw.synth_taehv_state_dict(4)
    assert list(a) == list(tw.taehv_param_shapes()) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["decoder.3.conv.0.weight"], c["decoder.3.conv.0.weight"])
    assert all(v.dtype == torch.bfloat16 and tuple(v.shape) == tw.taehv_param_shapes()[k] for k, v in a.items())
    w = a["decoder.3.conv.0.weight"].float()
    assert abs(float(w.abs().max()) - math.sqrt(3.0 / (512 * 9))) < 1e-3      # U(-a, a), a = sqrt(3 / fan_in)


def test_memblock_conv0_repack_is_a_two_tap_causal_convolution():
    """conv2d(cat[x_t, x_{t-1}]) == conv3d with the (2,3,3) kernel over [x_{t-1}, x_t], zero history for frame 0."""
    g = torch.Generator().manual_seed(0)
    C, T, H, W = 8, 3, 5, 7
    x = torch.randn(T, C, H, W, generator=g)
    w = torch.randn(C, 2 * C, 3, 3, generator=g) * 0.1
    b = torch.randn(C, generator=g)
    past = torch.cat([torch.zeros(1, C, H, W), x[:-1]])
    ref = F.conv2d(torch.cat([x, past], 1), w, b, padding=1)                               # [T, C, H, W]
    vol = torch.cat([torch.zeros(1, C, H, W), x]).permute(1, 0, 2, 3)[None]                # [1, C, T+1, H, W]
    got = F.conv3d(F.pad(vol, (1, 1, 1, 1, 0, 0)), tw.repack_memblock_conv0(w), b)[0].permute(1, 0, 2, 3)
    assert torch.allclose(got, ref, atol=1e-4)
    # and the flat layout the kernel reads: k = ((dt*3 + dh)*3 + dw)*Cin_pad + ci
    rp = tw.repack_taehv_conv(tw.repack_memblock_conv0(w))
    assert rp.shape == (C, 576 + 0) and rp.shape[1] % 64 == 0                             # 2*9*32 = 576
    assert torch.equal(rp[:, (1 * 9 + 4) * 32:(1 * 9 + 4) * 32 + C], w[:, :C, 1, 1])       # tap dt=1 (frame t), centre
    assert torch.equal(rp[:, (0 * 9 + 4) * 32:(0 * 9 + 4) * 32 + C], w[:, C:, 1, 1])       # tap dt=0 (frame t-1)
    assert float(rp[:, C:32].abs().sum()) == 0.0
    with pytest.raises(ValueError):
        tw.repack_memblock_conv0(torch.zeros(8, 8, 3, 3))


@pytest.mark.parametrize("stride", [1, 2])
def test_tgrow_fold_equals_upsample_tgrow_conv(stride):
    """Upsample -> TGrow (1x1, channels re-read as frames) -> bias-free 3x3, as the reference places them, equals the
    folded 3x3 on the upsampled input with its output channels re-read as frames."""
    g = torch.Generator().manual_seed(stride)
    C, Cn, T, H, W = 8, 4, 3, 4, 6
    x = torch.randn(T, C, H, W, generator=g)
    wg = torch.randn(stride * C, C, 1, 1, generator=g) * 0.3
    wc = torch.randn(Cn, C, 3, 3, generator=g) * 0.2
    up = F.interpolate(x, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(F.conv2d(up, wg).reshape(-1, C, 2 * H, 2 * W), wc, padding=1)           # [stride T, Cn, 2H, 2W]
    folded = tw.fold_tgrow(wg, wc)
    assert folded.shape == (stride * Cn, C, 3, 3)
    got = F.conv2d(up, folded, padding=1).reshape(T * stride, Cn, 2 * H, 2 * W)
    assert torch.allclose(got, ref, atol=1e-5)
    with pytest.raises(ValueError):
        tw.fold_tgrow(wg, torch.zeros(Cn, C + 1, 3, 3))


def test_decode_flops_against_a_hand_count():
    hw = 60 * 104
    mem = lambda c: 2 * 9 * (2 * c) * c + 2 * 2 * 9 * c * c            # noqa: E731  one MemBlock per position
    hand = (2 * 9 * 16 * 256 + 3 * mem(256)) * hw                      # decoder.1, stage 0
    hand += (2 * 256 * 256 + 2 * 9 * 256 * 128 + 3 * mem(128)) * 4 * hw          # TGrow(256,1) + exit conv at 120x208, stage 1
    hand += (2 * 128 * 256) * 16 * hw + (2 * 9 * 128 * 64 + 3 * mem(64)) * 16 * hw * 2      # TGrow(128,2) on 1 frame; 2 frames after
    hand += (2 * 64 * 128) * 64 * hw * 2 + (2 * 9 * 64 * 64 + 2 * 9 * 64 * 3) * 64 * hw * 4    # TGrow(64,2) on 2 frames; 4 after
    assert tw.taehv_decode_flops(60, 104, 1) == pytest.approx(hand, rel=1e-12)
    assert 0.53e12 < hand < 0.56e12
    assert tw.taehv_decode_flops(60, 104, 21) == pytest.approx(21 * hand)
    assert sfa.taehv_decode_flops(30, 52, 1) == pytest.approx(hand / 4)


def test_frame_bookkeeping_and_launch_list():
    assert [tw.frames_out(f, True) for f in (1, 3, 21)] == [1, 9, 81]             # 1 + 4 (F - 1), as the Wan VAE
    assert [tw.frames_out(f, False) for f in (1, 3)] == [4, 12]
    convs = tw.decoder_convs(60, 104, 3)
    assert len(convs) == 1 + 3 * 9 + 3 + 1
    assert [c["T"] for c in convs if c["name"].endswith("conv.0")] == [3] * 6 + [6] * 3
    assert convs[-1] == dict(name="decoder.22", kt=1, cin=64, cout=3, T=12, H=480, W=832, up=0, tgrow=1, epi="head_f32")
    assert convs[-2]["cout"] == 128 and convs[-2]["tgrow"] == 2 and convs[-2]["epi"] == "relu" and convs[-2]["T"] == 6


def test_tgrow_rows_are_patched_like_the_reference():
    sd = tw.synth_taehv_state_dict(0)
    big = dict(sd)
    big["decoder.7.conv.weight"] = torch.cat([torch.zeros(256, 256, 1, 1, dtype=torch.bfloat16), sd["decoder.7.conv.weight"]])   # stride-2 checkpoint
    big["encoder.0.weight"] = torch.zeros(1)
    out = tw.patch_tgrow_rows(big)
    assert torch.equal(out["decoder.7.conv.weight"], sd["decoder.7.conv.weight"]) and "encoder.0.weight" in out
    assert big["decoder.7.conv.weight"].shape[0] == 512                          # the caller's dict is left alone


def test_other_upscale_switches_raise():
    with pytest.raises(ValueError, match="decoder_time_upscale"):
        tw.taehv_param_shapes(decoder_time_upscale=(True, False))
    with pytest.raises(ValueError):
        tw.taehv_param_shapes(decoder_space_upscale=(True, True, False))


def test_wrapper_without_checkpoint_raises_and_never_downloads(tmp_path):
    with pytest.raises(FileNotFoundError, match="taew2_1.pth"):
        sfa.TAEHVWrapper(checkpoint_path=str(tmp_path / "taew2_1.pth"), device="cpu")


def test_generate_decoder_flags_are_mutually_exclusive():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(__file__))
    r = subprocess.run([sys.executable, os.path.join(root, "generate.py"), "--config_path", "c", "--data_path", "d", "--output_folder", "o",
                        "--taehv_random_init_seed", "0", "--vae_random_init_seed", "0"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "not together" in r.stderr


def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    assert lib.sf_taehv_conv(None, None) != 0 and b"null" in lib.sf_last_error()
    a = sfa._lib.TaehvConvArgs()
    assert lib.sf_taehv_conv(a, None) != 0 and b"null tensor" in lib.sf_last_error()
    a.x, a.w, a.bias, a.out = 4096, 4096, 4096, 4096
    a.Tout, a.H, a.W, a.Cin, a.Cout, a.kt, a.ldw, a.ldo = 1, 4, 4, 32, 64, 3, 576, 64
    assert lib.sf_taehv_conv(a, None) != 0 and b"kt must be 1 or 2" in lib.sf_last_error()
    a.kt, a.Cin = 2, 48
    assert lib.sf_taehv_conv(a, None) != 0 and b"Cin=48" in lib.sf_last_error()
    a.Cin, a.ldw = 32, 512
    assert lib.sf_taehv_conv(a, None) != 0 and b"weight row stride" in lib.sf_last_error()
    a.ldw, a.epilogue = 576, 9
    assert lib.sf_taehv_conv(a, None) != 0 and b"unknown epilogue" in lib.sf_last_error()
    a.epilogue, a.tgrow = sfa._lib.TAEHV_EPILOGUES["bias_relu"], 2
    assert lib.sf_taehv_conv(a, None) != 0 and b"tgrow" in lib.sf_last_error()
    a.tgrow, a.upsample, a.H = 1, 1, 5
    assert lib.sf_taehv_conv(a, None) != 0 and b"even" in lib.sf_last_error()
    assert lib.sf_taehv_prepare_latent(None, None, 1, 16, 4, 4, 32, None) != 0
    m = sfa._lib.TaehvModel()
    assert lib.sf_taehv_state_bytes(None, 60, 104) == 0 and b"null model" in lib.sf_last_error()
    assert lib.sf_taehv_state_bytes(m, 60, 104) == 0 and b"malformed" in lib.sf_last_error()
    assert lib.sf_taehv_scratch_bytes(m, 60, 104, 3) == 0
    assert lib.sf_taehv_reset(m, None, 0, 60, 104, None) != 0
    assert lib.sf_taehv_decode_frames(None, None, 0, None, 0, None, 60, 104, 1, 0, None, None) != 0
    assert [lib.sf_taehv_pick_nt(c) for c in (256, 128, 64, 3)] == [4, 4, 2, 1]
    assert "taehv_decode_frames" in sfa.torch_ops.OPS
    assert ctypes.sizeof(sfa._lib.TaehvLayer) == 32 and ctypes.sizeof(sfa._lib.TaehvConvArgs) == 6 * 8 + 13 * 4 + 4
