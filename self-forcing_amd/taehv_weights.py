"""Layout, seeded weights, weight repacking and FLOP count of the TAEHV tiny decoder and encoder
(demo_utils/taehv.py:159-208).

The decoder is an `nn.Sequential` of 23 modules; its `state_dict()` names are `decoder.<index>...`:

    0  Clamp                       1  conv 16->256 (+bias)        2  ReLU
    3-5   MemBlock(256)            6  Upsample   7  TGrow(256, 1)   8  conv 256->128 (no bias)
    9-11  MemBlock(128)            12 Upsample   13 TGrow(128, 2)   14 conv 128->64  (no bias)
    15-17 MemBlock(64)             18 Upsample   19 TGrow(64, 2)    20 conv 64->64   (no bias)
    21 ReLU                        22 conv 64->3 (+bias)

The encoder is an `nn.Sequential` of 18 modules, 64 channels wide; its names are `encoder.<index>...`:

    0  conv 3->64 (+bias)          1  ReLU
    2  TPool(64, 2)   3  conv 64->64 stride 2 (no bias)    4-6   MemBlock(64)
    7  TPool(64, 2)   8  conv 64->64 stride 2 (no bias)    9-11  MemBlock(64)
    12 TPool(64, 1)   13 conv 64->64 stride 2 (no bias)    14-16 MemBlock(64)
    17 conv 64->16 (+bias)

Pure host code: nothing here touches the GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

from .vae_weights import ENCODER_SEED_OFFSET, _synth, repack_conv

Tensor = torch.Tensor

LATENT_CHANNELS, IMAGE_CHANNELS = 16, 3                  # taehv.py:160-161
N_F = (256, 128, 64, 64)                                 # taehv.py:179
TGROW = (1, 2, 2)                                        # TGrow strides with decoder_time_upscale=(True, True)
STAGE_FIRST = (3, 9, 15)                                 # index of each stage's first MemBlock
TEMPORAL_FACTOR, SPATIAL_FACTOR = 4, 8
FRAMES_TO_TRIM = TEMPORAL_FACTOR - 1                     # taehv.py:180
TAEHV_CHECKPOINT = "checkpoints/taew2_1.pth"             # demo.py:70-76
ENC_C = 64                                               # taehv.py:173-177: every encoder layer is 64 wide
ENC_TPOOL = (2, 2, 1)                                    # TPool strides: 4 pixel frames -> 1 latent frame
ENC_STAGE_FIRST = (2, 7, 12)                             # index of each stage's TPool; +1 the strided conv, +2.. the MemBlocks
ENC_HEAD = 17


def _check_flags(decoder_time_upscale, decoder_space_upscale) -> None:
    if tuple(decoder_time_upscale) != (True, True) or tuple(decoder_space_upscale) != (True, True, True):
        raise ValueError("only the default TAEHV decoder is built: decoder_time_upscale=(True, True), "
                         f"decoder_space_upscale=(True, True, True); got {tuple(decoder_time_upscale)}, {tuple(decoder_space_upscale)}")


def taehv_param_shapes(decoder_time_upscale=(True, True), decoder_space_upscale=(True, True, True)) -> Dict[str, Tuple[int, ...]]:
    """Decoder tensor names -> shapes, in the order of the reference's `state_dict()` (64 tensors, 9 844 611 parameters)."""
    _check_flags(decoder_time_upscale, decoder_space_upscale)
    ps: Dict[str, Tuple[int, ...]] = {"decoder.1.weight": (N_F[0], LATENT_CHANNELS, 3, 3), "decoder.1.bias": (N_F[0],)}
    for s, first in enumerate(STAGE_FIRST):
        c, c_next = N_F[s], N_F[s + 1]
        for b in range(3):
            p = f"decoder.{first + b}.conv."
            ps[p + "0.weight"], ps[p + "0.bias"] = (c, 2 * c, 3, 3), (c,)
            ps[p + "2.weight"], ps[p + "2.bias"] = (c, c, 3, 3), (c,)
            ps[p + "4.weight"], ps[p + "4.bias"] = (c, c, 3, 3), (c,)
        ps[f"decoder.{first + 4}.conv.weight"] = (c * TGROW[s], c, 1, 1)
        ps[f"decoder.{first + 5}.weight"] = (c_next, c, 3, 3)
    ps["decoder.22.weight"], ps["decoder.22.bias"] = (IMAGE_CHANNELS, N_F[3], 3, 3), (IMAGE_CHANNELS,)
    return ps


def synth_taehv_state_dict(seed: int = 0, dtype=torch.bfloat16) -> Dict[str, Tensor]:
    """Seeded random-init decoder weights on the CPU (there is no network for taew2_1.pth): the recipe of
    `vae_weights._synth` -- weights U(-a, a) with a = sqrt(3 / fan_in), biases N(0, 0.02) -- drawn tensor by tensor in
    `taehv_param_shapes` order."""
    return _synth(taehv_param_shapes(), torch.Generator(device="cpu").manual_seed(seed), dtype)


def patch_tgrow_rows(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """`TAEHV.patch_tgrow_layers` (taehv.py:195-208): a TGrow weight with more rows than this decoder's keeps its LAST
    rows (the last-timestep output channels).  Returns a shallow copy; `encoder.*` keys pass through untouched."""
    need = taehv_param_shapes()
    out = dict(sd)
    for s, first in enumerate(STAGE_FIRST):
        key = f"decoder.{first + 4}.conv.weight"
        if key in out and out[key].shape[0] > need[key][0]:
            out[key] = out[key][-need[key][0]:]
    return out


def repack_memblock_conv0(w: Tensor) -> Tensor:
    """MemBlock.conv.0 weight [C, 2C, 3, 3] over cat([x, past]) -> a (2, 3, 3) causal kernel [C, C, 2, 3, 3] over the
    frame axis: temporal tap 0 (frame t-1) = weight[:, C:], tap 1 (frame t) = weight[:, :C]."""
    c = w.shape[0]
    if w.dim() != 4 or w.shape[1] != 2 * c:
        raise ValueError(f"MemBlock conv.0 weight must be [C, 2C, 3, 3], got {tuple(w.shape)}")
    return torch.stack([w[:, c:], w[:, :c]], dim=2)


def fold_tgrow(tgrow_w: Tensor, conv_w: Tensor) -> Tensor:
    """TGrow (bias-free 1x1, [s*C, C, 1, 1]) followed by the bias-free 3x3 conv [C', C, 3, 3] on each of its s
    sub-frames = ONE 3x3 conv [s*C', C, 3, 3] on the TGrow input whose output channels [j*C', (j+1)*C') are sub-frame j:
    W'[j*C' + o, c] = sum_m conv[o, m] * tgrow[j*C + m, c].  Both layers are linear and bias-free and the nearest
    upsample between them commutes with a 1x1 conv, so this is exact up to rounding; computed in float32."""
    sc, c = tgrow_w.shape[:2]
    s = sc // c
    if sc != s * c or conv_w.shape[1] != c:
        raise ValueError(f"fold_tgrow: TGrow {tuple(tgrow_w.shape)} does not feed conv {tuple(conv_w.shape)}")
    g = tgrow_w.float().reshape(s, c, c)                           # [j][m][c]
    out = torch.einsum("omhw,jmc->jochw", conv_w.float(), g)       # [j][o][c][3][3]
    return out.reshape(s * conv_w.shape[0], c, 3, 3)


repack_taehv_conv = repack_conv   # one packer for both convolution kernels: they read the same layout


def frames_out(latent_frames: int, fresh: bool) -> int:
    """Pixel frames a wrapper call returns for `latent_frames` latent frames: 4 per latent frame, minus the 3 the demo
    drops at the start of a stream (demo.py:432-433) -- 1 + 4 (F - 1) after a reset, as the Wan VAE gives."""
    return TEMPORAL_FACTOR * latent_frames - (FRAMES_TO_TRIM if fresh else 0)


def decoder_convs(lat_h: int, lat_w: int, latent_frames: int = 1) -> List[dict]:
    """Every convolution launch of one decode call, in order, as the sequencer issues it: name, kt, cin (padded), cout
    (of the launch: the folded exit convolutions carry tgrow * C'), output frames / size, upsample, tgrow, epilogue."""
    n = latent_frames
    out = [dict(name="decoder.1", kt=1, cin=32, cout=N_F[0], T=n, H=lat_h, W=lat_w, up=0, tgrow=1, epi="bias_relu")]
    h, w, t = lat_h, lat_w, 1
    for s, first in enumerate(STAGE_FIRST):
        c = N_F[s]
        for b in range(3):
            for k, (kt, epi) in enumerate(((2, "bias_relu"), (1, "bias_relu"), (1, "bias_resid_relu"))):
                out.append(dict(name=f"decoder.{first + b}.conv.{2 * k}", kt=kt, cin=c, cout=c, T=n * t, H=h, W=w, up=0, tgrow=1, epi=epi))
        h, w = 2 * h, 2 * w
        out.append(dict(name=f"decoder.{first + 4}+{first + 5}", kt=1, cin=c, cout=TGROW[s] * N_F[s + 1], T=n * t, H=h, W=w, up=1, tgrow=TGROW[s],
                        epi="relu" if s == 2 else "plain"))
        t *= TGROW[s]
    out.append(dict(name="decoder.22", kt=1, cin=N_F[3], cout=IMAGE_CHANNELS, T=n * t, H=h, W=w, up=0, tgrow=1, epi="head_f32"))
    return out


def taehv_decode_flops(lat_h: int, lat_w: int, latent_frames: int) -> float:
    """Algorithmic FLOPs (multiply-add = 2) of the REFERENCE decoder on `latent_frames` latent frames, every
    convolution at its true channel counts (decoder.1 with 16 input channels, MemBlock conv.0 with 2C).  TGrow is
    counted where the reference runs it: a 1x1 conv C -> stride*C at the UPSAMPLED resolution, on the stage's input
    frame count; the 3x3 behind it on stride times as many frames.  (This build folds TGrow into that 3x3, so it
    executes the 3x3 term only; TFLOP/s figures quoted against this count are therefore of the reference's work.)"""
    h, w, t = lat_h, lat_w, 1
    fl = 2.0 * 9 * LATENT_CHANNELS * N_F[0] * h * w
    for s in range(3):
        c, cn = N_F[s], N_F[s + 1]
        fl += 3 * (2.0 * 9 * (2 * c) * c + 2 * 2.0 * 9 * c * c) * h * w * t       # three MemBlocks
        h, w = 2 * h, 2 * w
        fl += 2.0 * c * (c * TGROW[s]) * h * w * t                                 # TGrow after the Upsample
        t *= TGROW[s]
        fl += 2.0 * 9 * c * cn * h * w * t                                         # stage-exit 3x3
    fl += 2.0 * 9 * N_F[3] * IMAGE_CHANNELS * h * w * t
    return fl * latent_frames


# ======================================================================================================== the encoder
def taehv_encoder_param_shapes() -> Dict[str, Tuple[int, ...]]:
    """Encoder tensor names -> shapes, in the order of the reference's `state_dict()` (64 tensors, 1 470 928 parameters)."""
    c = ENC_C
    ps: Dict[str, Tuple[int, ...]] = {"encoder.0.weight": (c, IMAGE_CHANNELS, 3, 3), "encoder.0.bias": (c,)}
    for s, first in enumerate(ENC_STAGE_FIRST):
        ps[f"encoder.{first}.conv.weight"] = (c, c * ENC_TPOOL[s], 1, 1)
        ps[f"encoder.{first + 1}.weight"] = (c, c, 3, 3)
        for b in range(3):
            p = f"encoder.{first + 2 + b}.conv."
            ps[p + "0.weight"], ps[p + "0.bias"] = (c, 2 * c, 3, 3), (c,)
            ps[p + "2.weight"], ps[p + "2.bias"] = (c, c, 3, 3), (c,)
            ps[p + "4.weight"], ps[p + "4.bias"] = (c, c, 3, 3), (c,)
    ps[f"encoder.{ENC_HEAD}.weight"], ps[f"encoder.{ENC_HEAD}.bias"] = (LATENT_CHANNELS, c, 3, 3), (LATENT_CHANNELS,)
    return ps


def synth_taehv_encoder_state_dict(seed: int = 0, dtype=torch.bfloat16) -> Dict[str, Tensor]:
    """Seeded random-init encoder weights on the CPU: the recipe of `synth_taehv_state_dict`, drawn in
    `taehv_encoder_param_shapes` order from a generator of their own, so that the decoder's tensors stay what they are
    without them."""
    return _synth(taehv_encoder_param_shapes(), torch.Generator(device="cpu").manual_seed(seed + ENCODER_SEED_OFFSET), dtype)


def has_encoder(sd: Dict[str, Tensor]) -> bool:
    return any(k.startswith("encoder.") for k in sd)


def fold_tpool(tpool_w: Tensor, conv_w: Tensor) -> Tensor:
    """TPool (bias-free 1x1 over s stacked frames, [C, s*C, 1, 1], taehv.py:37-45) followed by the bias-free stride-2
    3x3 conv [O, C, 3, 3] = ONE stride-2 3x3 conv [O, s*C, 3, 3] on the stacked frames, i.e. a convolution with s temporal
    taps at temporal stride s whose tap j (frame s t + j) reads input channels [j*C, (j+1)*C):
    W'[o, j*C + c, kh, kw] = sum_m conv[o, m, kh, kw] * tpool[m, j*C + c].  Both layers are linear and bias-free, nothing
    sits between them, and a 1x1 conv maps the zero padding to zero, so this is exact up to rounding; computed in the
    wider of float32 and the inputs' dtype.  The counterpart of `fold_tgrow`."""
    c, sc = tpool_w.shape[:2]
    s = sc // c
    if tpool_w.dim() != 4 or sc != s * c or s < 1 or conv_w.dim() != 4 or conv_w.shape[1] != c:
        raise ValueError(f"fold_tpool: TPool {tuple(tpool_w.shape)} does not feed conv {tuple(conv_w.shape)}")
    dt = torch.float64 if torch.float64 in (tpool_w.dtype, conv_w.dtype) else torch.float32
    return torch.einsum("omhw,mi->oihw", conv_w.to(dt), tpool_w.to(dt).reshape(c, sc))


def tpool_taps(folded: Tensor, stride: int) -> Tensor:
    """A `fold_tpool` result [O, s*C, 3, 3] as the (s, 3, 3) kernel [O, C, s, 3, 3] `repack_taehv_conv` packs: temporal tap
    j = input channels [j*C, (j+1)*C), frame s t + j."""
    o, sc = folded.shape[:2]
    return folded.reshape(o, stride, sc // stride, 3, 3).permute(0, 2, 1, 3, 4)


def repack_stem(w: Tensor) -> Tensor:
    """encoder.0 weight [64, 3, 3, 3] -> [64][32] as `sf_taehv_encode_stem` reads it: k = (dh*3 + dw)*3 + c, columns
    27..31 zero."""
    if tuple(w.shape[1:]) != (IMAGE_CHANNELS, 3, 3):
        raise ValueError(f"repack_stem: expected [Cout, 3, 3, 3], got {tuple(w.shape)}")
    out = torch.zeros(w.shape[0], 32, dtype=w.dtype, device=w.device)
    out[:, :27] = w.permute(0, 2, 3, 1).reshape(w.shape[0], 27)
    return out


def encoder_convs(H: int, W: int, frames: int = 4) -> List[dict]:
    """Every kernel launch of one encode call of `frames` pixel frames, in order, as the sequencer issues it: name,
    kernel (stem / down / conv), kt, cin (padded), cout, output frames / size, spatial stride, epilogue."""
    if frames % TEMPORAL_FACTOR or H % SPATIAL_FACTOR or W % SPATIAL_FACTOR:
        raise ValueError(f"encoder_convs: {frames} frames of {H}x{W}: frames % 4 == 0 and H, W % 8 == 0 expected")
    c = ENC_C
    out = [dict(name="encoder.0", kernel="stem", kt=1, cin=32, cout=c, T=frames, H=H, W=W, stride=1, epi="bias_relu")]
    h, w, t = H, W, frames
    for s, first in enumerate(ENC_STAGE_FIRST):
        h, w, t = h // 2, w // 2, t // ENC_TPOOL[s]
        out.append(dict(name=f"encoder.{first}+{first + 1}", kernel="down", kt=ENC_TPOOL[s], cin=c, cout=c, T=t, H=h, W=w, stride=2, epi="plain"))
        for b in range(3):
            for k, (kt, epi) in enumerate(((2, "bias_relu"), (1, "bias_relu"), (1, "bias_resid_relu"))):
                out.append(dict(name=f"encoder.{first + 2 + b}.conv.{2 * k}", kernel="conv", kt=kt, cin=c, cout=c, T=t, H=h, W=w, stride=1, epi=epi))
    out.append(dict(name=f"encoder.{ENC_HEAD}", kernel="conv", kt=1, cin=c, cout=LATENT_CHANNELS, T=t, H=h, W=w, stride=1, epi="latent_f32"))
    return out


def taehv_encode_flops(H: int, W: int, latent_frames: int) -> float:
    """Algorithmic FLOPs (multiply-add = 2) of the REFERENCE encoder for `latent_frames` latent frames of H x W pixels
    (4 pixel frames each), every convolution at its true channel counts (encoder.0 with 3 input channels, MemBlock
    conv.0 with 2C).  TPool is counted where the reference runs it: a 1x1 conv stride*C -> C at the stage's INPUT
    resolution on its output frame count.  (This build folds TPool into the 3x3 behind it, which then has `stride`
    taps; TFLOP/s figures quoted against this count are of the reference's work.)"""
    c = ENC_C
    hw, t = float(H * W), TEMPORAL_FACTOR
    fl = 2.0 * 9 * IMAGE_CHANNELS * c * hw * t
    for s in range(3):
        t //= ENC_TPOOL[s]
        fl += 2.0 * (c * ENC_TPOOL[s]) * c * hw * t                                  # TPool in front of the downsampling
        hw /= 4
        fl += 2.0 * 9 * c * c * hw * t                                               # stride-2 3x3
        fl += 3 * (2.0 * 9 * (2 * c) * c + 2 * 2.0 * 9 * c * c) * hw * t             # three MemBlocks
    fl += 2.0 * 9 * c * LATENT_CHANNELS * hw * t
    return fl * latent_frames
