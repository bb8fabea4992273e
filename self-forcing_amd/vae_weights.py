"""Shape description and weight handling of the Wan VAE: the decoder (latents -> pixels) and the encoder
(pixels -> latents, for image-to-video).

Key names are those of the reference's `WanVAE_.state_dict()`: `vae_param_shapes` lists what `decode` reads
(wan/modules/vae.py:369-429 Decoder3d, :503 conv2), `encoder_param_shapes` what `encode` reads (:265-367 Encoder3d,
:502 conv1), so `Wan2.1_VAE.pth` loads unchanged.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, asdict
from typing import Dict, List, Optional, Tuple

import torch

Tensor = torch.Tensor

# per-channel latent statistics (utils/wan_wrapper.py:59-68; the same numbers as wan/modules/vae.py:634-643)
LATENT_MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508,
               0.4134, -0.0715, 0.5517, -0.3632, -0.1922, -0.9497, 0.2503, -0.2921]
LATENT_STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743,
              3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253, 2.8251, 1.9160]


@dataclass(frozen=True)
class VaeShape:
    """Constructor arguments of WanVAE_ that shape the decoder (wan/modules/vae.py:591-603:
    dim 96, z_dim 16, dim_mult [1,2,4,4], 2 res blocks, temporal upsampling in the first two stages)."""
    dim: int = 96
    z_dim: int = 16
    dim_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    temperal_upsample: Tuple[bool, ...] = (True, True, False)   # reversed temperal_downsample (vae.py:501)

    def as_dict(self) -> dict:
        return asdict(self)

    @property
    def dims(self) -> List[int]:
        return [self.dim * u for u in (self.dim_mult[-1],) + tuple(self.dim_mult[::-1])]

    @property
    def spatial_factor(self) -> int:
        return 2 ** (len(self.dim_mult) - 1)

    @property
    def temporal_factor(self) -> int:
        return 2 ** sum(1 for t in self.temperal_upsample if t)


WAN_VAE = VaeShape()
# reduced decoder for the parity fixtures (every channel count stays a multiple of 32)
VAE_REDUCED = VaeShape(dim=32)


@dataclass(frozen=True)
class ResBlockSpec:
    prefix: str
    in_dim: int
    out_dim: int


@dataclass(frozen=True)
class ResampleSpec:
    prefix: str
    dim: int
    mode: str   # 'upsample2d' | 'upsample3d' | 'downsample2d' | 'downsample3d'


def decoder_layout(s: VaeShape):
    """The module sequence of Decoder3d (vae.py:390-421): returns (middle, upsamples) where middle is
    [ResBlockSpec, 'attn', ResBlockSpec] and upsamples a list of ResBlockSpec / ResampleSpec in order."""
    dims = s.dims
    middle = [ResBlockSpec("decoder.middle.0.", dims[0], dims[0]), "decoder.middle.1.",
              ResBlockSpec("decoder.middle.2.", dims[0], dims[0])]
    ups = []
    idx = 0
    for i, (in_dim, out_dim) in enumerate(zip(dims[:-1], dims[1:])):
        if i in (1, 2, 3):
            in_dim = in_dim // 2
        for _ in range(s.num_res_blocks + 1):
            ups.append(ResBlockSpec(f"decoder.upsamples.{idx}.", in_dim, out_dim))
            idx += 1
            in_dim = out_dim
        if i != len(s.dim_mult) - 1:
            ups.append(ResampleSpec(f"decoder.upsamples.{idx}.", out_dim,
                                    "upsample3d" if s.temperal_upsample[i] else "upsample2d"))
            idx += 1
    return middle, ups


def encoder_dims(s: VaeShape) -> List[int]:
    """Widths of Encoder3d (vae.py:286): dim * [1, *dim_mult] -- [96, 96, 192, 384, 384] for Wan2.1."""
    return [s.dim * u for u in (1,) + tuple(s.dim_mult)]


def temporal_downsample(s: VaeShape) -> Tuple[bool, ...]:
    return tuple(s.temperal_upsample[::-1])        # WanVAE_: temperal_upsample = temperal_downsample[::-1] (vae.py:500)


def encoder_layout(s: VaeShape):
    """The module sequence of Encoder3d (vae.py:286-319): returns (stages, middle) where stages[i] is the list of
    ResBlockSpec of stage i followed by its ResampleSpec ('downsample2d' / 'downsample3d'; none for the last stage) and
    middle is [ResBlockSpec, attention prefix, ResBlockSpec]."""
    dims = encoder_dims(s)
    tdown = temporal_downsample(s)
    stages = []
    idx = 0
    for i, (in_dim, out_dim) in enumerate(zip(dims[:-1], dims[1:])):
        st = []
        for _ in range(s.num_res_blocks):
            st.append(ResBlockSpec(f"encoder.downsamples.{idx}.", in_dim, out_dim))
            idx += 1
            in_dim = out_dim
        if i != len(s.dim_mult) - 1:
            st.append(ResampleSpec(f"encoder.downsamples.{idx}.", out_dim, "downsample3d" if tdown[i] else "downsample2d"))
            idx += 1
        stages.append(st)
    c = dims[-1]
    middle = [ResBlockSpec("encoder.middle.0.", c, c), "encoder.middle.1.", ResBlockSpec("encoder.middle.2.", c, c)]
    return stages, middle


def _res_shapes(out: Dict[str, Tuple[int, ...]], spec: ResBlockSpec) -> None:
    p = spec.prefix
    out[p + "residual.0.gamma"] = (spec.in_dim, 1, 1, 1)
    out[p + "residual.2.weight"] = (spec.out_dim, spec.in_dim, 3, 3, 3)
    out[p + "residual.2.bias"] = (spec.out_dim,)
    out[p + "residual.3.gamma"] = (spec.out_dim, 1, 1, 1)
    out[p + "residual.6.weight"] = (spec.out_dim, spec.out_dim, 3, 3, 3)
    out[p + "residual.6.bias"] = (spec.out_dim,)
    if spec.in_dim != spec.out_dim:
        out[p + "shortcut.weight"] = (spec.out_dim, spec.in_dim, 1, 1, 1)
        out[p + "shortcut.bias"] = (spec.out_dim,)


def _attn_shapes(out: Dict[str, Tuple[int, ...]], a: str, c: int) -> None:
    out[a + "norm.gamma"] = (c, 1, 1)
    out[a + "to_qkv.weight"] = (3 * c, c, 1, 1)
    out[a + "to_qkv.bias"] = (3 * c,)
    out[a + "proj.weight"] = (c, c, 1, 1)
    out[a + "proj.bias"] = (c,)


def encoder_param_shapes(s: VaeShape) -> Dict[str, Tuple[int, ...]]:
    """Every tensor `WanVAE_.encode` reads, in `state_dict()` order: `encoder.*`, then the 1x1x1 `conv1` (2z -> 2z)."""
    out: Dict[str, Tuple[int, ...]] = {}
    dims = encoder_dims(s)
    out["encoder.conv1.weight"] = (dims[0], 3, 3, 3, 3)
    out["encoder.conv1.bias"] = (dims[0],)
    stages, middle = encoder_layout(s)
    for st in stages:
        for spec in st:
            if isinstance(spec, ResBlockSpec):
                _res_shapes(out, spec)
            else:
                out[spec.prefix + "resample.1.weight"] = (spec.dim, spec.dim, 3, 3)
                out[spec.prefix + "resample.1.bias"] = (spec.dim,)
                if spec.mode == "downsample3d":
                    out[spec.prefix + "time_conv.weight"] = (spec.dim, spec.dim, 3, 1, 1)
                    out[spec.prefix + "time_conv.bias"] = (spec.dim,)
    _res_shapes(out, middle[0])
    _attn_shapes(out, middle[1], dims[-1])
    _res_shapes(out, middle[2])
    z2 = 2 * s.z_dim
    out["encoder.head.0.gamma"] = (dims[-1], 1, 1, 1)
    out["encoder.head.2.weight"] = (z2, dims[-1], 3, 3, 3)
    out["encoder.head.2.bias"] = (z2,)
    out["conv1.weight"] = (z2, z2, 1, 1, 1)
    out["conv1.bias"] = (z2,)
    return out


def encode_chunks(frames: int) -> int:
    """Chunks (= latent frames) `WanVAE_.encode` makes of `frames` pixel frames (vae.py:521-522): the first frame
    alone, then whole groups of 4; trailing frames past the last full group are dropped."""
    if frames < 1:
        raise ValueError("encode needs at least one pixel frame")
    return 1 + (frames - 1) // 4


def vae_param_shapes(s: VaeShape) -> Dict[str, Tuple[int, ...]]:
    out: Dict[str, Tuple[int, ...]] = {}
    z, d0 = s.z_dim, s.dims[0]
    out["conv2.weight"] = (z, z, 1, 1, 1)
    out["conv2.bias"] = (z,)
    out["decoder.conv1.weight"] = (d0, z, 3, 3, 3)
    out["decoder.conv1.bias"] = (d0,)

    def res(spec: ResBlockSpec):
        p = spec.prefix
        out[p + "residual.0.gamma"] = (spec.in_dim, 1, 1, 1)
        out[p + "residual.2.weight"] = (spec.out_dim, spec.in_dim, 3, 3, 3)
        out[p + "residual.2.bias"] = (spec.out_dim,)
        out[p + "residual.3.gamma"] = (spec.out_dim, 1, 1, 1)
        out[p + "residual.6.weight"] = (spec.out_dim, spec.out_dim, 3, 3, 3)
        out[p + "residual.6.bias"] = (spec.out_dim,)
        if spec.in_dim != spec.out_dim:
            out[p + "shortcut.weight"] = (spec.out_dim, spec.in_dim, 1, 1, 1)
            out[p + "shortcut.bias"] = (spec.out_dim,)

    middle, ups = decoder_layout(s)
    res(middle[0])
    a = middle[1]
    out[a + "norm.gamma"] = (d0, 1, 1)
    out[a + "to_qkv.weight"] = (3 * d0, d0, 1, 1)
    out[a + "to_qkv.bias"] = (3 * d0,)
    out[a + "proj.weight"] = (d0, d0, 1, 1)
    out[a + "proj.bias"] = (d0,)
    res(middle[2])
    for spec in ups:
        if isinstance(spec, ResBlockSpec):
            res(spec)
        else:
            out[spec.prefix + "resample.1.weight"] = (spec.dim // 2, spec.dim, 3, 3)
            out[spec.prefix + "resample.1.bias"] = (spec.dim // 2,)
            if spec.mode == "upsample3d":
                out[spec.prefix + "time_conv.weight"] = (2 * spec.dim, spec.dim, 3, 1, 1)
                out[spec.prefix + "time_conv.bias"] = (2 * spec.dim,)
    dl = s.dims[-1]
    out["decoder.head.0.gamma"] = (dl, 1, 1, 1)
    out["decoder.head.2.weight"] = (3, dl, 3, 3, 3)
    out["decoder.head.2.bias"] = (3,)
    return out


def _synth(shapes: Dict[str, Tuple[int, ...]], g: torch.Generator, dtype) -> Dict[str, Tensor]:
    sd: Dict[str, Tensor] = {}
    for name, shape in shapes.items():
        if name.endswith("gamma"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            a = math.sqrt(3.0 / fan_in)
            t = torch.empty(shape).uniform_(-a, a, generator=g)
        sd[name] = t.to(dtype)
    return sd


def repack_conv(w: Tensor, cin_pad: Optional[int] = None) -> Tensor:
    """Conv3d / Conv2d weight [Cout, Cin, (kt,) kh, kw] -> the implicit-GEMM layout of `sf_conv_args.w` and
    `sf_taehv_conv_args.w`: [Cout][Kpad] with k = ((dt*kh + dh)*kw + dw)*Cin_pad + ci, Cin padded to a multiple of 32
    and K to a multiple of 64 (zeros).  Public as `vae.repack_conv`; `taehv_weights.repack_taehv_conv` is this function."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin, kt, kh, kw = w.shape
    cp = cin_pad or ((cin + 31) // 32) * 32
    t = torch.zeros(cout, kt, kh, kw, cp, dtype=w.dtype, device=w.device)
    t[..., :cin] = w.permute(0, 2, 3, 4, 1)
    k = kt * kh * kw * cp
    kpad = ((k + 63) // 64) * 64
    out = torch.zeros(cout, kpad, dtype=w.dtype, device=w.device)
    out[:, :k] = t.reshape(cout, k)
    return out


# the encoder's tensors come from a generator of their own, so that the decoder's stay what they were without them
ENCODER_SEED_OFFSET = 0x5EED


def synth_vae_state_dict(s: VaeShape, seed: int = 0, dtype=torch.bfloat16, encoder: bool = False) -> Dict[str, Tensor]:
    """Seeded random-init decoder weights on the CPU (there is no network for Wan2.1_VAE.pth).
    Convolutions ~ U(-a, a) with a = sqrt(3 / fan_in) (unit gain: activations keep their scale through
    the 30-odd layers), biases ~ N(0, .02), RMS-norm gammas ~ 1 + N(0, .1).  The attention projection
    `proj` is NOT zero (the reference zero-initialises it, vae.py:239, which would make the block the
    identity and the test vacuous).  Drawn tensor by tensor in `vae_param_shapes` order.

    `encoder=True` adds the encoder (`encoder_param_shapes`, same recipe, its own proj non-zero too), drawn from a
    separate generator seeded `seed + ENCODER_SEED_OFFSET`: the decoder tensors are bit-identical either way."""
    sd = _synth(vae_param_shapes(s), torch.Generator(device="cpu").manual_seed(seed), dtype)
    if encoder:
        sd.update(_synth(encoder_param_shapes(s), torch.Generator(device="cpu").manual_seed(seed + ENCODER_SEED_OFFSET), dtype))
    return sd


def vae_decode_flops(s: VaeShape, lat_h: int, lat_w: int, latent_frames: int) -> float:
    """Algorithmic FLOPs (multiply-add = 2) of `decode` on `latent_frames` latent frames: every
    convolution at its true channel counts (2 * taps * Cin * Cout per output position), the attention
    block's projections and its two token-by-token products.  The first latent frame runs every stage
    at one frame (no time convolution); later frames double the frame count after each upsample3d."""
    middle, ups = decoder_layout(s)
    d0 = s.dims[0]

    def one(first: bool) -> float:
        h, w, t = lat_h, lat_w, 1
        pos = h * w
        fl = 2.0 * s.z_dim * s.z_dim * pos + 2.0 * 27 * s.z_dim * d0 * pos               # conv2, decoder.conv1
        fl += 2 * (2.0 * 27 * d0 * d0 * pos * 2)                                             # two middle res blocks
        fl += 2.0 * d0 * 3 * d0 * pos + 2.0 * d0 * d0 * pos + 4.0 * pos * pos * d0           # attention block
        for spec in ups:
            pos = t * h * w
            if isinstance(spec, ResBlockSpec):
                fl += 2.0 * 27 * spec.in_dim * spec.out_dim * pos + 2.0 * 27 * spec.out_dim * spec.out_dim * pos
                if spec.in_dim != spec.out_dim:
                    fl += 2.0 * spec.in_dim * spec.out_dim * pos
            else:
                if spec.mode == "upsample3d" and not first:
                    fl += 2.0 * 3 * spec.dim * 2 * spec.dim * pos
                    t *= 2
                h, w = 2 * h, 2 * w
                fl += 2.0 * 9 * spec.dim * (spec.dim // 2) * t * h * w
        fl += 2.0 * 27 * s.dims[-1] * 3 * t * h * w                                          # head
        return fl

    return one(True) + (latent_frames - 1) * one(False)


def vae_encode_flops(s: VaeShape, height: int, width: int, frames: int) -> float:
    """Algorithmic FLOPs (multiply-add = 2) of `encode` on `frames` pixel frames of height x width: every convolution at
    its true channel counts (encoder.conv1 reads 3 channels), the stride-2 convolutions at their output positions, the
    middle attention block, and conv1's mu rows.  The first chunk is one frame at every stage (no time convolution);
    every later chunk is 4 frames, halved by each downsample3d."""
    stages, middle = encoder_layout(s)
    dims = encoder_dims(s)

    def res(spec: ResBlockSpec, pos: float) -> float:
        fl = 2.0 * 27 * spec.in_dim * spec.out_dim * pos + 2.0 * 27 * spec.out_dim * spec.out_dim * pos
        if spec.in_dim != spec.out_dim:
            fl += 2.0 * spec.in_dim * spec.out_dim * pos
        return fl

    def one(first: bool) -> float:
        h, w, t = height, width, 1 if first else 4
        fl = 2.0 * 27 * 3 * dims[0] * t * h * w                                                # encoder.conv1
        for st in stages:
            for spec in st:
                if isinstance(spec, ResBlockSpec):
                    fl += res(spec, t * h * w)
                else:
                    h, w = h // 2, w // 2
                    fl += 2.0 * 9 * spec.dim * spec.dim * t * h * w
                    if spec.mode == "downsample3d" and not first:
                        t //= 2
                        fl += 2.0 * 3 * spec.dim * spec.dim * t * h * w
        pos, c = t * h * w, dims[-1]
        fl += res(middle[0], pos) + res(middle[2], pos)
        fl += t * (2.0 * c * 3 * c * h * w + 2.0 * c * c * h * w + 4.0 * (h * w) ** 2 * c)    # attention block per frame
        fl += 2.0 * 27 * c * 2 * s.z_dim * pos + 2.0 * 2 * s.z_dim * s.z_dim * pos              # head, conv1 (mu rows)
        return fl

    return one(True) + (encode_chunks(frames) - 1) * one(False)
