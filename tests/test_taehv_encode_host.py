"""Host-side tests of the TAEHV tiny encoder (no GPU): the weight layout against the reference's state_dict, the seeded
weights (and that the decoder's are what they were), the TPool fold, the stem's weight layout, the launch list, the
FLOP count, and the argument checks of the new C entry points."""
import ctypes
import math
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import taehv_weights as tw

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_encoder_param_shapes_match_the_reference_state_dict():
    g = np.load(os.path.join(GOLD, "taehv_enc_a.npz"))
    ref = [(str(k), tuple(int(d) for d in str(s).split(","))) for k, s in zip(g["encoder_keys"], g["encoder_shapes"])]
    ps = tw.taehv_encoder_param_shapes()
    assert list(ps.items()) == ref
    assert len(ps) == 64 and sum(math.prod(s) for s in ps.values()) == 1_470_928
    assert next(iter(ps)) == "encoder.0.weight" and list(ps)[-1] == "encoder.17.bias"
    assert ps["encoder.2.conv.weight"] == (64, 128, 1, 1) and ps["encoder.12.conv.weight"] == (64, 64, 1, 1)
    assert not set(ps) & set(tw.taehv_param_shapes())


def test_seeded_encoder_weights_and_the_decoder_draws_are_unchanged():
    a, b, c = tw.synth_taehv_encoder_state_dict(3), tw.synth_taehv_encoder_state_dict(3), tw.synth_taehv_encoder_state_dict(4)
    assert list(a) == list(tw.taehv_encoder_param_shapes()) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["encoder.4.conv.0.weight"], c["encoder.4.conv.0.weight"])
    assert all(v.dtype == torch.bfloat16 and tuple(v.shape) == tw.taehv_encoder_param_shapes()[k] for k, v in a.items())
    assert abs(float(a["encoder.0.weight"].float().abs().max()) - math.sqrt(3.0 / 27)) < 2e-3      # U(-a, a), a = sqrt(3 / fan_in)
    # the decoder's dict: decoder tensors only, the bits it had before the encoder existed (CRC-32 over names and bf16
    # bit patterns in order, recorded from the parent commit)
    sd = tw.synth_taehv_state_dict(5)
    assert list(sd) == list(tw.taehv_param_shapes()) and all(k.startswith("decoder.") for k in sd)
    crc = 0
    for k, v in sd.items():
        crc = zlib.crc32(v.view(torch.int16).numpy().tobytes(), zlib.crc32(k.encode(), crc))
    assert crc == 2386531091
    assert sfa.synth_taehv_encoder_state_dict is tw.synth_taehv_encoder_state_dict and tw.has_encoder(a) and not tw.has_encoder(sd)


@pytest.mark.parametrize("stride", [2, 1])
def test_tpool_fold_equals_tpool_then_strided_conv(stride):
    """TPool (frames stacked as channels, 1x1) -> bias-free stride-2 3x3 with zero padding, as the reference places them
    (taehv.py:43-45, :174), in fp64 against the folded convolution: on the stacked frames, and as the (s, 3, 3) temporal
    kernel at temporal stride s that the GPU runs.  The derivation is exact; 1e-12 relative."""
    g = torch.Generator().manual_seed(10 + stride)
    C, O, T, H, W = 8, 6, 4, 6, 10
    x = torch.randn(T, C, H, W, generator=g, dtype=torch.float64)
    wp = torch.randn(C, stride * C, 1, 1, generator=g, dtype=torch.float64) * 0.3
    wc = torch.randn(O, C, 3, 3, generator=g, dtype=torch.float64) * 0.2
    ref = F.conv2d(F.conv2d(x.reshape(-1, stride * C, H, W), wp), wc, stride=2, padding=1)          # [T / s, O, H/2, W/2]
    folded = tw.fold_tpool(wp, wc)
    assert folded.shape == (O, stride * C, 3, 3) and folded.dtype == torch.float64
    got = F.conv2d(x.reshape(-1, stride * C, H, W), folded, stride=2, padding=1)
    assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-12
    taps = tw.tpool_taps(folded, stride)                                                          # [O, C, s, 3, 3]: frame s t + j is tap j
    assert taps.shape == (O, C, stride, 3, 3)
    vol = F.pad(x.permute(1, 0, 2, 3)[None], (1, 1, 1, 1, 0, 0))
    got3 = F.conv3d(vol, taps, stride=(stride, 2, 2))[0].permute(1, 0, 2, 3)
    assert got3.shape == ref.shape and float((got3 - ref).abs().max() / ref.abs().max()) <= 1e-12
    assert tw.fold_tpool(wp.float(), wc.bfloat16()).dtype == torch.float32                        # the product path: fp32, rounded once after
    with pytest.raises(ValueError):
        tw.fold_tpool(wp, torch.zeros(O, C + 1, 3, 3))
    with pytest.raises(ValueError):
        tw.fold_tpool(torch.zeros(C, C + 1, 1, 1), wc)


def test_stem_weight_layout():
    w = torch.arange(64 * 27, dtype=torch.float32).reshape(64, 3, 3, 3)
    rp = tw.repack_stem(w)
    assert rp.shape == (64, 32) and float(rp[:, 27:].abs().sum()) == 0.0
    for (c, dh, dw) in ((0, 0, 0), (2, 1, 0), (1, 2, 2)):
        assert torch.equal(rp[:, (dh * 3 + dw) * 3 + c], w[:, c, dh, dw])
    with pytest.raises(ValueError):
        tw.repack_stem(torch.zeros(64, 4, 3, 3))


def test_encoder_launch_list_geometry():
    convs = tw.encoder_convs(480, 832, 12)
    assert len(convs) == 1 + 3 * (1 + 9) + 1
    assert convs[0] == dict(name="encoder.0", kernel="stem", kt=1, cin=32, cout=64, T=12, H=480, W=832, stride=1, epi="bias_relu")
    downs = [c for c in convs if c["kernel"] == "down"]
    assert [(c["name"], c["kt"], c["T"], c["H"], c["W"]) for c in downs] == [("encoder.2+3", 2, 6, 240, 416), ("encoder.7+8", 2, 3, 120, 208),
                                                                            ("encoder.12+13", 1, 3, 60, 104)]
    assert all(c["stride"] == 2 and c["epi"] == "plain" and c["cin"] == c["cout"] == 64 for c in downs)
    assert [c["T"] for c in convs if c["name"].endswith("conv.0")] == [6] * 3 + [3] * 6
    assert [c["epi"] for c in convs[2:5]] == ["bias_relu", "bias_relu", "bias_resid_relu"] and [c["kt"] for c in convs[2:5]] == [2, 1, 1]
    assert convs[-1] == dict(name="encoder.17", kernel="conv", kt=1, cin=64, cout=16, T=3, H=60, W=104, stride=1, epi="latent_f32")
    ragged = tw.encoder_convs(104, 168, 4)                 # 52 x 84, 26 x 42, 13 x 21: no stage is a whole number of 128-row tiles
    assert [(c["T"], c["H"], c["W"]) for c in ragged if c["kernel"] == "down"] == [(2, 52, 84), (1, 26, 42), (1, 13, 21)]
    assert all((c["T"] * c["H"] * c["W"]) % 128 for c in ragged[1:])
    for bad in ((480, 832, 6), (484, 832, 4), (480, 836, 4)):
        with pytest.raises(ValueError):
            tw.encoder_convs(*bad)


def test_encode_flops_against_a_hand_count():
    hw = 480 * 832
    mem = 2 * 9 * 128 * 64 + 2 * 2 * 9 * 64 * 64                        # one MemBlock per position
    hand = 2 * 9 * 3 * 64 * hw * 4                                      # encoder.0 on 4 frames
    hand += 2 * 128 * 64 * hw * 2                                       # TPool(64, 2) at 480 x 832 -> 2 frames
    hand += (2 * 9 * 64 * 64 + 3 * mem) * (hw // 4) * 2                 # stride-2 conv + 3 MemBlocks at 240 x 416, 2 frames
    hand += 2 * 128 * 64 * (hw // 4) * 1                                # TPool(64, 2) at 240 x 416 -> 1 frame
    hand += (2 * 9 * 64 * 64 + 3 * mem) * (hw // 16)                    # 120 x 208
    hand += 2 * 64 * 64 * (hw // 16)                                    # TPool(64, 1) at 120 x 208
    hand += (2 * 9 * 64 * 64 + 3 * mem) * (hw // 64)                    # 60 x 104
    hand += 2 * 9 * 64 * 16 * (hw // 64)                                # encoder.17
    assert hand == 241_852_416_000
    assert tw.taehv_encode_flops(480, 832, 1) == pytest.approx(hand, rel=1e-12)
    assert tw.taehv_encode_flops(480, 832, 21) == pytest.approx(21 * hand)
    assert sfa.taehv_encode_flops(240, 416, 1) == pytest.approx(hand / 4)


def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    # the stem
    assert lib.sf_taehv_encode_stem(None, 0, 0, 8, 8, 4, 0, None, None, None, None) != 0 and b"null" in lib.sf_last_error()
    assert lib.sf_taehv_encode_stem(4096, 7, 64, 8, 8, 1, 0, 4096, 4096, 4096, None) != 0 and b"dtype" in lib.sf_last_error()
    assert lib.sf_taehv_encode_stem(4096, 0, 64, 8, 8, 4, 4, 4096, 4096, 4096, None) != 0 and b"lead" in lib.sf_last_error()
    assert lib.sf_taehv_encode_stem(4096, 0, 64, 8, 8, 2, 2, 4096, 4096, 4096, None) != 0 and b"lead" in lib.sf_last_error()
    assert lib.sf_taehv_encode_stem(4096, 0, 63, 8, 8, 1, 0, 4096, 4096, 4096, None) != 0 and b"channel stride" in lib.sf_last_error()
    assert lib.sf_taehv_encode_stem(4096, 0, 64, 8, 8, 1, 0, 4100, 4096, 4096, None) != 0 and b"misaligned" in lib.sf_last_error()
    # the strided convolution
    assert lib.sf_taehv_down_conv(None, None) != 0 and b"null" in lib.sf_last_error()
    a = sfa._lib.TaehvDownConvArgs()
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"null tensor" in lib.sf_last_error()
    a.x, a.w, a.out = 4096, 4096, 4096
    a.Tout, a.H, a.W, a.Cin, a.Cout, a.kt, a.ldw, a.ldo = 1, 4, 4, 64, 64, 3, 1152, 64
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"kt must be 1 or 2" in lib.sf_last_error()
    a.kt, a.Cin = 2, 48
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"Cin=48" in lib.sf_last_error()
    a.Cin, a.Cout = 64, 32
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"Cout=32" in lib.sf_last_error()
    a.Cout, a.ldw = 64, 576
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"weight row stride" in lib.sf_last_error()
    a.ldw, a.ldo = 1152, 32
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"ldo" in lib.sf_last_error()
    a.ldo, a.Tout, a.H, a.W = 64, 43, 240, 416                       # 86 frames of 480 x 832 x 64: past the gather's 4 GiB
    assert lib.sf_taehv_down_conv(a, None) != 0 and b"4 GiB" in lib.sf_last_error()
    # the sequencer
    m = sfa._lib.TaehvEncoder()
    assert lib.sf_taehv_encode_state_bytes(None, 480, 832) == 0 and b"null encoder" in lib.sf_last_error()
    assert lib.sf_taehv_encode_state_bytes(m, 480, 832) == 0 and b"malformed" in lib.sf_last_error()
    assert lib.sf_taehv_encode_state_bytes(m, 484, 832) == 0 and b"multiples of 8" in lib.sf_last_error()
    assert lib.sf_taehv_encode_scratch_bytes(m, 480, 832, 4) == 0
    assert lib.sf_taehv_encode_reset(m, None, 0, 480, 832, None) != 0
    assert lib.sf_taehv_encode_frames(None, None, 0, None, 0, None, 0, 0, 480, 832, 4, 0, None, None) != 0
    # a well-formed descriptor (the pointers are never followed by the checks)
    for layer, (cin, cout, kt, ldw) in [(m.stem, (32, 64, 1, 32)), (m.head, (64, 16, 1, 576))]:
        layer.w, layer.bias, layer.cin, layer.cout, layer.kt, layer.ldw = 4096, 4096, cin, cout, kt, ldw
    for s in range(3):
        d = m.down[s]
        d.w, d.cin, d.cout, d.kt, d.ldw = 4096, 64, 64, (2, 2, 1)[s], (1152, 1152, 576)[s]
        for b in range(3):
            for k in range(3):
                l = m.block[s][b][k]
                l.w, l.bias, l.cin, l.cout, l.kt, l.ldw = 4096, 4096, 64, 64, 2 if k == 0 else 1, 1152 if k == 0 else 576
    state = lib.sf_taehv_encode_state_bytes(m, 480, 832)
    assert state == 3 * 64 * 2 * (240 * 416 + 120 * 208 + 60 * 104) and 50e6 < state < 51e6          # nine one-frame histories
    assert lib.sf_taehv_encode_state_bytes(m, 16, 24) == 3 * ((8 * 12 * 128 + 255) // 256 + (4 * 6 * 128 + 255) // 256 + (2 * 3 * 128 + 255) // 256) * 256
    scratch = lib.sf_taehv_encode_scratch_bytes(m, 480, 832, 8)
    assert scratch > 8 * 480 * 832 * 64 * 2
    assert lib.sf_taehv_encode_scratch_bytes(m, 480, 832, 6) == 0 and b"multiple of 4" in lib.sf_last_error()
    assert lib.sf_taehv_encode_scratch_bytes(m, 480, 836, 8) == 0 and b"multiples of 8" in lib.sf_last_error()
    call = lambda **kw: lib.sf_taehv_encode_frames(m, kw.get("state", 4096), kw.get("sb", state), kw.get("scratch", 8192), kw.get("wb", scratch),   # noqa: E731
                                                   kw.get("pix", 4096), 1, 8 * 480 * 832, kw.get("H", 480), 832, kw.get("n", 8), kw.get("lead", 0),
                                                   kw.get("out", 4096), None)
    assert call(n=6) != 0 and b"multiple of 4" in lib.sf_last_error()
    assert call(n=0) != 0 and b"multiple of 4" in lib.sf_last_error()
    assert call(H=476) != 0 and b"multiples of 8" in lib.sf_last_error()
    assert call(lead=4) != 0 and b"lead" in lib.sf_last_error()
    assert call(sb=state - 1) != 0 and b"state of" in lib.sf_last_error()
    assert call(wb=scratch - 1) != 0 and b"scratch of" in lib.sf_last_error()
    assert call(state=None) != 0 and call(scratch=None) != 0 and call(pix=None) != 0 and call(out=None) != 0 and b"null buffer" in lib.sf_last_error()
    assert call(state=4100) != 0 and b"aligned" in lib.sf_last_error()
    assert lib.sf_taehv_encode_reset(m, 4096, state - 1, 480, 832, None) != 0 and b"state of" in lib.sf_last_error()
    m.down[2].kt = 2
    assert lib.sf_taehv_encode_state_bytes(m, 480, 832) == 0 and b"pool 4 frames" in lib.sf_last_error()
    assert lib.sf_abi_version() == 11
    assert ctypes.sizeof(sfa._lib.TaehvDownConvArgs) == 3 * 8 + 8 * 4 and ctypes.sizeof(sfa._lib.TaehvEncoder) == (1 + 3 + 27 + 1) * 32
    assert sfa._lib.TAEHV_EPILOGUES["latent_f32"] == 5 and sfa._lib.TAEHV_EPILOGUES["head_f32"] == 4


def test_the_new_operator_has_a_schema():
    assert "taehv_encode_frames" in sfa.torch_ops.OPS
    sch = str(torch.ops.sf_hip.taehv_encode_frames.default._schema)
    assert sch == ("sf_hip::taehv_encode_frames(SymInt model, Tensor(a1!) state, Tensor(a2!) scratch, Tensor pixels, Tensor(a4!) out, "
                   "SymInt H, SymInt W, SymInt lead) -> ()")


def test_a_partial_encoder_is_reported_by_name():
    """The two halves merge into one 128-tensor dict (what taew2_1.pth holds); an encoder that lacks tensors is a
    KeyError that names them, before anything is uploaded."""
    need = list(tw.taehv_encoder_param_shapes())
    full = {**tw.synth_taehv_state_dict(0), **tw.synth_taehv_encoder_state_dict(0)}
    assert len(full) == 128 and tw.has_encoder(full) and [k for k in full if k.startswith("encoder.")] == need
    part = {k: v for k, v in full.items() if not k.startswith("encoder.17")}
    with pytest.raises(KeyError, match="lacks 2 encoder tensors"):
        sfa.TAEHVEncoder(part, device="cpu")
