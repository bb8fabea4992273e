"""Host-side tests of the VAE encoder (no GPU): the weight layout against the reference's state_dict, the seeded
encoder weights, the chunk plan, the FLOP count, and the argument checks of the new C entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import vae_weights as vw

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_encoder_param_shapes_match_the_reference_state_dict():
    g = np.load(os.path.join(GOLD, "vae_encode_full.npz"))
    ref = [(str(k), tuple(int(d) for d in str(s).split(","))) for k, s in zip(g["encoder_keys"], g["encoder_shapes"])]
    assert len(ref) == 86
    assert list(vw.encoder_param_shapes(vw.WAN_VAE).items()) == ref
    assert not set(vw.encoder_param_shapes(vw.WAN_VAE)) & set(vw.vae_param_shapes(vw.WAN_VAE))


def test_encoder_weights_leave_the_decoder_weights_unchanged():
    for shape, seed in ((vw.VAE_REDUCED, 0), (vw.WAN_VAE, 1)):
        dec = vw.synth_vae_state_dict(shape, seed=seed)
        both = vw.synth_vae_state_dict(shape, seed=seed, encoder=True)
        assert set(dec) == set(vw.vae_param_shapes(shape))                       # the default stays decoder-only
        assert set(both) == set(dec) | set(vw.encoder_param_shapes(shape))
        assert all(torch.equal(dec[k], both[k]) for k in dec)
        for k, shp in vw.encoder_param_shapes(shape).items():
            assert tuple(both[k].shape) == shp
        assert both["encoder.middle.1.proj.weight"].float().abs().sum() > 0      # the attention block is not the identity
    # the encoder object shares the decoder's weight repacking, not its decode methods
    from self_forcing_amd.vae import WanVAEDecoder, WanVAEEncoder
    encoder = WanVAEEncoder(vw.VAE_REDUCED, vw.synth_vae_state_dict(vw.VAE_REDUCED, seed=0, encoder=True), "cpu")
    assert not issubclass(WanVAEEncoder, WanVAEDecoder)
    assert not hasattr(encoder, "cached_decode")


def test_chunk_plan_matches_the_reference_loop():
    for T in range(1, 30):
        assert vw.encode_chunks(T) == 1 + (T - 1) // 4
    with pytest.raises(ValueError):
        vw.encode_chunks(0)


def test_encode_flops():
    s = vw.WAN_VAE
    first = vw.vae_encode_flops(s, 480, 832, 1)
    assert 2.6e12 < first < 2.8e12
    later = vw.vae_encode_flops(s, 480, 832, 5) - first
    assert vw.vae_encode_flops(s, 480, 832, 8) == vw.vae_encode_flops(s, 480, 832, 5)        # frames past a whole chunk: dropped
    assert vw.vae_encode_flops(s, 480, 832, 81) == pytest.approx(first + 20 * later)
    assert 2.5 * first < later < 4 * first          # 4 frames per chunk until the two downsample3d halve them
    assert vw.vae_encode_flops(s, 240, 416, 1) == pytest.approx(first / 4, rel=0.03)   # all but the attention scale with area


def _lib():
    return sfa._lib.lib()


def _enc():
    e = sfa._lib.VaeEncoder()
    return e


def test_encode_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = _lib()
    err = lambda: lib.sf_last_error().decode()  # noqa: E731
    assert lib.sf_vae_encode_state_bytes(None, 64, 64, 2) == 0
    assert "null encoder" in err()
    e = _enc()
    assert lib.sf_vae_encode_scratch_bytes(ctypes.byref(e), 64, 64, 2) == 0
    assert "stage counts" in err()
    e.n_stages, e.res_per_stage = 4, 2
    assert lib.sf_vae_encode_state_bytes(ctypes.byref(e), 64, 64, 2) == 0
    assert "null weights" in err()
    assert lib.sf_vae_encode_frames(None, None, 0, None, 0, None, 0, 0, 64, 64, 2, 0, 1, 0, 0, None, None) != 0
    assert "null encoder" in err()
    assert lib.sf_vae_encode_reset(ctypes.byref(e), None, 0, 64, 64, 1, None) != 0
    assert "window_frames" in err()
    assert lib.sf_vae_prepare_pixels(None, 0, 0, None, 1, 8, 8, 32, None) != 0
    assert "null tensor" in err()
    fake = ctypes.c_void_p(256)      # never dereferenced: the shape checks fail first
    assert lib.sf_vae_prepare_pixels(fake, 0, 64, fake, 1, 8, 8, 30, None) != 0
    assert "c_pad" in err()
    assert lib.sf_vae_prepare_pixels(fake, 0, 10, fake, 1, 8, 8, 32, None) != 0
    assert "channel stride" in err()
    assert lib.sf_vae_finish_latent(None, 32, 32, None, 32, None, None, None, None, 1, 16, 4, 4, None) != 0
    assert "null tensor" in err()
    assert lib.sf_vae_finish_latent(fake, 32, 128, fake, 32, fake, fake, fake, fake, 1, 16, 4, 4, None) != 0
    assert "cin <= 64" in err()


def test_strided_conv_arguments_are_checked_without_touching_the_gpu():
    lib = _lib()
    a = sfa._lib.ConvArgs()
    fake = 256
    a.x = a.w = a.bias = a.out = fake
    a.Tout, a.H, a.W, a.Hin, a.Win, a.Cin, a.Cout, a.kt, a.kh, a.kw = 1, 4, 4, 8, 8, 32, 32, 1, 3, 3
    a.ldw, a.ldo = 320, 32
    a.stride_hw = 3
    assert lib.sf_conv_igemm(ctypes.byref(a), None) != 0
    assert "strides" in lib.sf_last_error().decode()
    a.stride_hw, a.upsample = 2, 1
    assert lib.sf_conv_igemm(ctypes.byref(a), None) != 0
    assert "stride 2" in lib.sf_last_error().decode()
    a.upsample, a.Hin = 0, 10
    assert lib.sf_conv_igemm(ctypes.byref(a), None) != 0
    assert "does not match" in lib.sf_last_error().decode()
    a.Hin, a.structure = 8, 2
    assert lib.sf_conv_igemm(ctypes.byref(a), None) != 0
    assert "halo structure takes no strided" in lib.sf_last_error().decode()


def test_encode_op_is_registered_with_a_mutation_schema():
    sch = str(torch.ops.sf_hip.vae_encode_frames.default._schema)
    assert "Tensor(a1!) state" in sch and "Tensor(a2!) scratch" in sch and "Tensor(a4!) out" in sch
    assert "vae_encode_frames" in sfa.torch_ops.OPS
