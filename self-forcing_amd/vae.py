"""Wan VAE decode and encode on the GPU behind the reference's `WanVAEWrapper` surface.

Mirrors `utils/wan_wrapper.py:56-117`:

    vae = WanVAEWrapper(state_dict=..., device="cuda")
    video = vae.decode_to_pixel(latent, use_cache=False)      # [B, F, 16, h, w] -> [B, 1+4(F-1), 3, 8h, 8w]
    vae.model.clear_cache()                                    # inference.py:183
    latent = vae.encode_to_latent(pixel)                       # [B, 3, T, H, W] -> float32 [B, 1+(T-1)//4, 16, H/8, W/8]
    z0 = vae.encoder.begin_clip(image); z = vae.encoder.continue_clip(n)   # the clip "image, then zeros", as it is needed

Every kernel is in csrc/ (conv_igemm.hip, vae_elementwise.hip, gemm_bf16.hip); a group of latent frames is ONE C call
(`sf_vae_decode_frames`), a group of 4-frame chunks likewise (`sf_vae_encode_frames`).  There is no eager/CPU
fallback.  The encoder (image-to-video, inference.py:145) needs the checkpoint's `encoder.*` / `conv1.*` tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib, torch_ops
from .device_model import DeviceModel
from .vae_weights import (LATENT_MEAN, LATENT_STD, ResBlockSpec, ResampleSpec, VaeShape, WAN_VAE, decoder_layout,
                          encode_chunks, encoder_dims, encoder_layout, encoder_param_shapes, repack_conv, vae_param_shapes)

Tensor = torch.Tensor


class _StreamPos:
    """Where one latent size's stream stands since its last reset."""
    __slots__ = ("fresh", "nframes", "slot")

    def __init__(self):
        self.fresh = True      # no chunk decoded since the last clear_cache
        self.nframes = 0       # latent frames decoded since then
        self.slot = 0          # ... of them in the current lap of the sliding history windows (sf_vae_decode_frames)


class _EncodePos:
    """Where one encode stream stands since its reset: its size and window slots, chunks encoded, slots taken in this lap."""
    __slots__ = ("H", "W", "K", "chunks", "slot")

    def __init__(self, H: int, W: int, K: int):
        self.H, self.W, self.K, self.chunks, self.slot = H, W, K, 0, 0


def window_step(slot: int, g: int, K: int):
    """One step of the sliding history windows (sf_vae_decode_frames / sf_vae_encode_frames): the next group of `g`
    frames, with `slot` of the K slots of the current lap taken, goes to slot `window`; the histories it reads are where
    the previous call left them, at `history_at`.  A group that does not fit restarts the lap at slot 0.  The caller
    advances: slot = window + g."""
    if slot + g > K:
        return 0, slot
    return slot, slot


class _VAEWeights(DeviceModel):
    """What the decoder and the encoder share: the repacking of `CausalConv3d` / `ResidualBlock` / `AttentionBlock`
    weights into their C descriptors, and the per-size state + per-stream scratch blocks."""

    def __init__(self, shape: VaeShape, device, frames_per_call: int):
        if not 1 <= frames_per_call <= 63:
            raise ValueError("frames_per_call must be in 1..63")
        super().__init__(device)
        self.shape = shape
        self.frames_per_call = frames_per_call          # latent frames / 4-frame chunks handed to one C call (any value gives the same bits)
        self._state: Dict[tuple, Tensor] = {}

    def _conv(self, dst: _lib.VaeConv, sd, name: str, cin_pad: Optional[int] = None) -> None:
        w = sd[name + ".weight"]
        if w.dim() == 4:
            w = w.unsqueeze(2)
        cout, cin, kt, kh, kw = w.shape
        rp = self._dev(repack_conv(w.float(), cin_pad))
        dst.w, dst.bias = rp.data_ptr(), self._dev(sd[name + ".bias"]).data_ptr()
        dst.cin = cin_pad or ((cin + 31) // 32) * 32
        dst.cout, dst.kt, dst.kh, dst.kw, dst.ldw = cout, kt, kh, kw, rp.shape[1]

    def _res(self, dst: _lib.VaeResBlock, sd, spec: ResBlockSpec) -> None:
        p = spec.prefix
        dst.gamma1 = self._dev(sd[p + "residual.0.gamma"].flatten()).data_ptr()
        dst.gamma2 = self._dev(sd[p + "residual.3.gamma"].flatten()).data_ptr()
        self._conv(dst.conv1, sd, p + "residual.2")
        self._conv(dst.conv2, sd, p + "residual.6")
        if spec.in_dim != spec.out_dim:
            self._conv(dst.shortcut, sd, p + "shortcut")

    def _attn(self, m, sd, a: str, c: int) -> None:
        """AttentionBlock `a` of width c into m.attn_*: to_qkv split into the q|k rows and the v rows, proj."""
        qkv_w, qkv_b = sd[a + "to_qkv.weight"].reshape(3 * c, c), sd[a + "to_qkv.bias"]
        m.attn_gamma = self._dev(sd[a + "norm.gamma"].flatten()).data_ptr()
        m.attn_qk_w, m.attn_qk_b = self._dev(qkv_w[:2 * c]).data_ptr(), self._dev(qkv_b[:2 * c]).data_ptr()
        m.attn_v_w, m.attn_v_b = self._dev(qkv_w[2 * c:]).data_ptr(), self._dev(qkv_b[2 * c:]).data_ptr()
        m.attn_proj_w = self._dev(sd[a + "proj.weight"].reshape(c, c)).data_ptr()
        m.attn_proj_b = self._dev(sd[a + "proj.bias"]).data_ptr()

    def _state_scratch(self, key: tuple, state_bytes: str, scratch_bytes: str, *size):
        """(state, scratch) of `key`, sized by the two C functions named on `size`: the state -- the convolution
        histories -- zeroed on first use, the scratch per stream."""
        if key not in self._state:
            n = getattr(_lib.lib(), state_bytes)(C.byref(self.cmodel), *size)
            if n == 0:
                _lib.check(-1, state_bytes)
            self._state[key] = torch.zeros(n, dtype=torch.uint8, device=self.device)
        return self._state[key], self._stream_bytes(key, lambda: getattr(_lib.lib(), scratch_bytes)(C.byref(self.cmodel), *size))


class WanVAEDecoder(_VAEWeights):
    """Device-resident decoder: repacked bf16 weights, the C model descriptor, and one decode state
    (the convolution histories of one stream).  Counterpart of `WanVAE_` (wan/modules/vae.py:478-617)
    for `decode` / `cached_decode` / `clear_cache`."""

    def __init__(self, shape: VaeShape, state_dict: Dict[str, Tensor], device, frames_per_call: int = 4):
        super().__init__(shape, device, frames_per_call)
        self.window_frames = frames_per_call + 1        # slots of the sliding history windows (the first chunk + one group)
        self._pos: Dict[tuple, _StreamPos] = {}     # per latent size, beside its state: where that stream stands
        self._load(state_dict)

    def _load(self, sd: Dict[str, Tensor]) -> None:
        s = self.shape
        self._check_state_dict(sd, vae_param_shapes(s), "VAE state dict", "decoder tensors")
        if any(d % 32 for d in s.dims) or s.dims[0] % 64:
            raise ValueError(f"decoder widths {s.dims} must be multiples of 32 (first: 64)")
        if len(s.dim_mult) > _lib.VAE_MAX_STAGES:
            raise ValueError("at most 4 decoder stages")
        m = _lib.VaeModel()
        m.z_dim, m.n_stages, m.res_per_stage = s.z_dim, len(s.dim_mult), s.num_res_blocks + 1
        for i, t in enumerate(s.temperal_upsample):
            m.temporal_up[i] = 1 if t else 0
        m.latent_mean = self._dev(torch.tensor(LATENT_MEAN[:s.z_dim]), torch.float32).data_ptr()
        m.latent_std = self._dev(torch.tensor(LATENT_STD[:s.z_dim]), torch.float32).data_ptr()
        m.conv2_w = self._dev(sd["conv2.weight"].reshape(s.z_dim, s.z_dim)).data_ptr()
        m.conv2_b = self._dev(sd["conv2.bias"]).data_ptr()
        self._conv(m.conv1, sd, "decoder.conv1")
        middle, ups = decoder_layout(s)
        self._res(m.mid0, sd, middle[0])
        self._res(m.mid2, sd, middle[2])
        self._attn(m, sd, middle[1], s.dims[0])
        blocks = [u for u in ups if isinstance(u, ResBlockSpec)]
        res = (_lib.VaeResBlock * len(blocks))()
        for i, spec in enumerate(blocks):
            self._res(res[i], sd, spec)
        self._res_array = res
        m.res_host = C.cast(res, C.POINTER(_lib.VaeResBlock))
        for stage, spec in enumerate(u for u in ups if isinstance(u, ResampleSpec)):
            self._conv(m.up_conv[stage], sd, spec.prefix + "resample.1")
            if spec.mode == "upsample3d":
                self._conv(m.time_conv[stage], sd, spec.prefix + "time_conv")
        m.head_gamma = self._dev(sd["decoder.head.0.gamma"].flatten()).data_ptr()
        self._conv(m.head_conv, sd, "decoder.head.2")
        self.cmodel = m
        self._handle = torch_ops.register_model(self)

    # ---------------------------------------------------------------------------------
    def _buffers(self, h: int, w: int):
        key = (h, w)
        sf, tf = self.shape.spatial_factor, self.shape.temporal_factor
        if (2 + self.window_frames * tf) * (sf * h) * (sf * w) * self.cmodel.head_conv.cin * 2 >= 0xFFFFFF00:
            raise ValueError(f"frames_per_call={self.frames_per_call} at {sf * h}x{sf * w}: a convolution's input volume would pass 4 GiB "
                             "(the kernels address a volume through one 32-bit-ranged buffer descriptor); use fewer frames per call")
        bufs = self._state_scratch(key, "sf_vae_state_bytes", "sf_vae_scratch_bytes", h, w, self.window_frames)
        if key not in self._pos:
            self._pos[key] = _StreamPos()          # every latent size streams on its own: counters live beside its state
        return bufs

    def clear_cache(self) -> None:
        """`WanVAE_.clear_cache` (vae.py:610-617): forget every convolution's history."""
        stream = torch.cuda.current_stream(self.device).cuda_stream if self._state else None
        for (h, w), st in self._state.items():
            _lib.check(_lib.lib().sf_vae_reset(C.byref(self.cmodel), st.data_ptr(), st.numel(), h, w, self.window_frames, stream), "sf_vae_reset")
            self._pos[(h, w)] = _StreamPos()

    def frames_out(self, latent_frames: int, h: Optional[int] = None, w: Optional[int] = None) -> int:
        """Pixel frames the next `cached_decode` of `latent_frames` frames of an h x w latent returns (the size may be
        omitted while the decoder has seen at most one)."""
        tf = self.shape.temporal_factor
        if h is None:
            if len(self._pos) > 1:
                raise ValueError("frames_out: this decoder streams several latent sizes; pass h and w")
            pos = next(iter(self._pos.values()), None)
        else:
            pos = self._pos.get((h, w))
        fresh = pos is None or pos.fresh
        return (1 + tf * (latent_frames - 1)) if fresh else tf * latent_frames

    def cached_decode(self, z: Tensor) -> Tensor:
        """`WanVAE_.cached_decode` (vae.py:579-593) for one sample: z [F, z_dim, h, w] bf16 -> float32
        pixels [T, 3, 8h, 8w] in [-1, 1]; continues from the state the previous call left."""
        if z.dim() != 4 or z.shape[1] != self.shape.z_dim:
            raise ValueError(f"expected latents [F, {self.shape.z_dim}, h, w], got {tuple(z.shape)}")
        z = z.to(device=self.device, dtype=torch.bfloat16).contiguous()
        F, _, h, w = z.shape
        state, scratch = self._buffers(h, w)
        pos = self._pos[(h, w)]
        sf, tf = self.shape.spatial_factor, self.shape.temporal_factor
        out = torch.empty(self.frames_out(F, h, w), 3, sf * h, sf * w, dtype=torch.float32, device=self.device)
        t0 = i = 0
        while i < F:
            # the frame that follows a reset is decoded alone (one output frame); after it, groups of up to
            # frames_per_call latent frames per C call -- bit-identical to one call per frame, but the low-resolution
            # stages fill the chip and every launch has a shorter tail
            g = 1 if pos.fresh else min(self.frames_per_call, F - i)
            window, history_at = window_step(pos.slot, g, self.window_frames)
            torch.ops.sf_hip.vae_decode_frames(self._handle, state, scratch, z[i:i + g], out[t0:], h, w, self.window_frames,
                                               pos.nframes, window, history_at)
            pos.slot = window + g
            pos.nframes += g
            t0 += 1 if pos.fresh else tf * g
            i += g
            pos.fresh = False
        return out

    def decode(self, z: Tensor) -> Tensor:
        """`WanVAE_.decode` (vae.py:556-578): cleared caches before and after."""
        self.clear_cache()
        out = self.cached_decode(z)
        self.clear_cache()
        return out


class WanVAEEncoder(_VAEWeights):
    """Device-resident encoder: repacked bf16 weights of `Encoder3d` + `conv1` and the C descriptor; per-(H, W) state
    (the convolution histories) and scratch allocated on first use.  Counterpart of `WanVAE_.encode`
    (wan/modules/vae.py:517-543)."""

    def __init__(self, shape: VaeShape, state_dict: Dict[str, Tensor], device, frames_per_call: int = 4):
        super().__init__(shape, device, frames_per_call)
        self._clip: Optional[_EncodePos] = None      # the clip begin_clip started, until another begin_clip or an encode() over the same (H, W, K) histories ends it
        self._zeros: Dict[tuple, Tensor] = {}        # per (H, W): the zero pixel frames continue_clip feeds
        self._load_encoder(state_dict)

    def _load_encoder(self, sd: Dict[str, Tensor]) -> None:
        s = self.shape
        self._check_state_dict(sd, encoder_param_shapes(s))
        dims = encoder_dims(s)
        if any(d % 32 for d in dims) or dims[-1] % 64:
            raise ValueError(f"encoder widths {dims} must be multiples of 32 (last: 64)")
        if len(s.dim_mult) > _lib.VAE_MAX_STAGES:
            raise ValueError("at most 4 encoder stages")
        stages, middle = encoder_layout(s)
        m = _lib.VaeEncoder()
        m.z_dim, m.n_stages, m.res_per_stage = s.z_dim, len(s.dim_mult), s.num_res_blocks
        m.latent_mean = self._dev(torch.tensor(LATENT_MEAN[:s.z_dim]), torch.float32).data_ptr()
        m.latent_std = self._dev(torch.tensor(LATENT_STD[:s.z_dim]), torch.float32).data_ptr()
        z2 = 2 * s.z_dim
        m.conv1_w = self._dev(sd["conv1.weight"].reshape(z2, z2)[:s.z_dim]).data_ptr()      # mu rows only (vae.py:538)
        m.conv1_b = self._dev(sd["conv1.bias"][:s.z_dim]).data_ptr()
        self._conv(m.in_conv, sd, "encoder.conv1")
        blocks = [spec for st in stages for spec in st if isinstance(spec, ResBlockSpec)]
        res = (_lib.VaeResBlock * len(blocks))()
        for i, spec in enumerate(blocks):
            self._res(res[i], sd, spec)
        self._res_array = res
        m.res_host = C.cast(res, C.POINTER(_lib.VaeResBlock))
        for i, st in enumerate(stages):
            for spec in st:
                if isinstance(spec, ResampleSpec):
                    self._conv(m.down_conv[i], sd, spec.prefix + "resample.1")
                    if spec.mode == "downsample3d":
                        m.temporal_down[i] = 1
                        self._conv(m.time_conv[i], sd, spec.prefix + "time_conv")
        self._res(m.mid0, sd, middle[0])
        self._res(m.mid2, sd, middle[2])
        self._attn(m, sd, middle[1], dims[-1])
        m.head_gamma = self._dev(sd["encoder.head.0.gamma"].flatten()).data_ptr()
        self._conv(m.head_conv, sd, "encoder.head.2")
        self.cmodel = m
        self._handle = torch_ops.register_model(self)

    def _enc_buffers(self, H: int, W: int, K: int):
        if (2 + K * 4) * H * W * encoder_dims(self.shape)[0] * 2 >= 0xFFFFFF00:
            raise ValueError(f"frames_per_call={self.frames_per_call} at {H}x{W}: a convolution's input volume would pass 4 GiB "
                             "(the kernels address a volume through one 32-bit-ranged buffer descriptor); use fewer frames per call")
        return self._state_scratch((H, W, K), "sf_vae_encode_state_bytes", "sf_vae_encode_scratch_bytes", H, W, K)

    def _reset(self, H: int, W: int, K: int) -> "_EncodePos":
        state, _ = self._enc_buffers(H, W, K)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().sf_vae_encode_reset(C.byref(self.cmodel), state.data_ptr(), state.numel(), H, W, K, stream), "sf_vae_encode_reset")
        return _EncodePos(H, W, K)

    def _encode_group(self, pos: "_EncodePos", pixels: Tensor, out: Tensor) -> None:
        """The next `out.shape[0]` chunks of the stream at `pos` (the first: one pixel frame; later ones: 4 each) in one C call."""
        g = out.shape[0]
        state, scratch = self._enc_buffers(pos.H, pos.W, pos.K)
        window, history_at = window_step(pos.slot, g, pos.K)
        torch.ops.sf_hip.vae_encode_frames(self._handle, state, scratch, pixels, out, pos.H, pos.W, pos.K, pos.chunks, window, history_at)
        pos.slot = window + g
        pos.chunks += g

    def encode(self, x: Tensor) -> Tensor:
        """`WanVAE_.encode` (vae.py:517-543) for one sample: x [3, T, H, W] (bf16 or float32, in [-1, 1]) -> float32
        normalised mu [1 + (T-1)//4, z_dim, H/8, W/8].  Starts from cleared histories; frames past the last whole chunk
        of 4 are dropped, as the reference does."""
        if x.dim() != 4 or x.shape[0] != 3:
            raise ValueError(f"expected pixels [3, T, H, W], got {tuple(x.shape)}")
        _, T, H, W = x.shape
        sf = self.shape.spatial_factor
        if H % sf or W % sf:
            raise ValueError(f"encode: height and width must be multiples of {sf}, got {H}x{W}")
        n = encode_chunks(T)
        if x.dtype not in (torch.bfloat16, torch.float32):
            x = x.float()
        x = x.to(self.device)[:, :1 + 4 * (n - 1)].contiguous()
        # histories for the first frame + up to frames_per_call chunks per call; fewer slots when the input is short
        K = min(self.frames_per_call, max(n - 1, 1)) + 1
        if self._clip is not None and (self._clip.H, self._clip.W, self._clip.K) == (H, W, K):
            self._clip = None                  # a clip of begin_clip with these histories (same size, same window slots) ends here
        pos = self._reset(H, W, K)
        out = torch.empty(n, self.shape.z_dim, H // sf, W // sf, dtype=torch.float32, device=self.device)
        f0 = 0
        while pos.chunks < n:
            i = pos.chunks
            g = 1 if i == 0 else min(self.frames_per_call, n - i)
            nf = 1 if i == 0 else 4 * g
            self._encode_group(pos, x[:, f0:f0 + nf], out[i:i + g])
            f0 += nf
        return out

    # --- a clip "one image, then zeros" of open length, encoded as it is needed (i2v_condition.py) ---------------
    def _clip_out(self, out: Optional[Tensor], n: int, H: int, W: int) -> Tensor:
        sf = self.shape.spatial_factor
        want = (n, self.shape.z_dim, H // sf, W // sf)
        if out is None:
            return torch.empty(want, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != want or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 tensor {want} on {self.device}, got {tuple(out.shape)} {out.dtype} {out.device}")
        return out

    def begin_clip(self, image: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """Start the clip whose first pixel frame is `image` [3, H, W] (bf16 or float32 in [-1, 1]) and whose other frames
        are zero: cleared histories, then the one-frame call.  Returns latent frame 0, float32 [1, z_dim, H/8, W/8]
        (written to `out` when given).  `continue_clip` encodes what follows -- the same calls `encode` makes on the whole
        clip, so the same bits."""
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"expected an image [3, H, W], got {tuple(image.shape)}")
        _, H, W = image.shape
        sf = self.shape.spatial_factor
        if H % sf or W % sf:
            raise ValueError(f"begin_clip: height and width must be multiples of {sf}, got {H}x{W}")
        if image.dtype not in (torch.bfloat16, torch.float32):
            image = image.float()
        image = image.to(self.device).unsqueeze(1).contiguous()
        self._clip = None
        out = self._clip_out(out, 1, H, W)
        pos = self._reset(H, W, self.frames_per_call + 1)
        self._encode_group(pos, image, out)
        self._clip = pos
        return out

    def continue_clip(self, n: int, out: Optional[Tensor] = None) -> Tensor:
        """The next `n` latent frames of the clip `begin_clip` started (4 n zero pixel frames), float32
        [n, z_dim, H/8, W/8] (written to `out` when given), carrying the histories.  The zeros are one persistent buffer of
        4 x frames_per_call frames per size: the clip itself never exists in memory."""
        pos = self._clip
        if pos is None:
            raise RuntimeError("continue_clip: no clip in progress (begin_clip starts one; encode() over the same histories ends it)")
        if n < 1:
            raise ValueError(f"continue_clip: n must be positive, got {n}")
        out = self._clip_out(out, n, pos.H, pos.W)
        zeros = self._zero_frames(pos.H, pos.W)
        i = 0
        while i < n:
            g = min(self.frames_per_call, n - i)
            self._encode_group(pos, zeros[:, :4 * g], out[i:i + g])
            i += g
        return out

    def _zero_frames(self, H: int, W: int) -> Tensor:
        if (H, W) not in self._zeros:
            self._zeros[(H, W)] = torch.zeros(3, 4 * self.frames_per_call, H, W, dtype=torch.bfloat16, device=self.device)
        return self._zeros[(H, W)]


VAE_CHECKPOINT = "wan_models/Wan2.1-T2V-1.3B/Wan2.1_VAE.pth"   # utils/wan_wrapper.py:74


class WanVAEWrapper(torch.nn.Module):
    """Drop-in for the reference's `WanVAEWrapper` (utils/wan_wrapper.py:56-117), decode side.

    `state_dict`: the tensors of `Wan2.1_VAE.pth` (or the seeded stand-in of `vae_weights.synth_vae_state_dict`);
    when it holds the encoder tensors as well, `encode_to_latent` works too.  Without one the reference's default checkpoint path is loaded
    (weights-only); FileNotFoundError when it is absent."""

    def __init__(self, state_dict: Optional[Dict[str, Tensor]] = None, device="cuda", shape: VaeShape = WAN_VAE,
                 checkpoint_path: str = VAE_CHECKPOINT, frames_per_call: int = 4):
        super().__init__()
        if state_dict is None:   # `WanVAEWrapper()` as the reference's pipelines construct it (wan_wrapper.py:72-76)
            import os
            if not os.path.exists(checkpoint_path):
                raise FileNotFoundError(f"VAE checkpoint {checkpoint_path!r} not found: download it as the reference's README "
                                        "describes, or construct WanVAEWrapper(state_dict=...) / inject a vae= into the pipeline")
            state_dict = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        self.mean = torch.tensor(LATENT_MEAN, dtype=torch.float32)
        self.std = torch.tensor(LATENT_STD, dtype=torch.float32)
        self.model = WanVAEDecoder(shape, state_dict, device, frames_per_call=frames_per_call)
        self.shape = shape
        missing = [k for k in encoder_param_shapes(shape) if k not in state_dict]
        self.encoder: Optional[WanVAEEncoder] = None
        self._encoder_missing = missing
        if not missing:
            self.encoder = WanVAEEncoder(shape, state_dict, device, frames_per_call=frames_per_call)

    def encode_to_latent(self, pixel: Tensor) -> Tensor:
        """pixel [B, 3, T, H, W] in [-1, 1] -> float32 latents [B, 1 + (T-1)//4, 16, H/8, W/8] (wan_wrapper.py:78-92):
        one `WanVAE_.encode` per sample, histories cleared before and after each."""
        if self.encoder is None:
            m = self._encoder_missing
            raise NotImplementedError(f"this VAE state dict has no encoder: {len(m)} encoder.* / conv1.* tensors are missing, "
                                      f"e.g. {m[:3]} (load Wan2.1_VAE.pth, or synth_vae_state_dict(..., encoder=True))")
        if pixel.dim() != 5 or pixel.shape[1] != 3:
            raise ValueError(f"encode_to_latent expects pixels [B, 3, T, H, W], got {tuple(pixel.shape)}")
        sf = self.shape.spatial_factor
        if pixel.shape[3] % sf or pixel.shape[4] % sf:
            raise ValueError(f"encode_to_latent: height and width must be multiples of {sf}, got {pixel.shape[3]}x{pixel.shape[4]}")
        return torch.stack([self.encoder.encode(u) for u in pixel], dim=0)

    def decode_to_pixel(self, latent: Tensor, use_cache: bool = False) -> Tensor:
        """latent [B, F, C, h, w] -> float32 [B, T, 3, 8h, 8w] clamped to [-1, 1] (wan_wrapper.py:95-117)."""
        if use_cache:
            assert latent.shape[0] == 1, "Batch size must be 1 when using cache"
        fn = self.model.cached_decode if use_cache else self.model.decode
        return torch.stack([fn(u) for u in latent], dim=0)

    def decode_chunk(self, latent: Tensor, chunk_index: int) -> Tensor:
        """Streaming decode used by `CausalInferencePipeline.stream`: chunk 0 starts from cleared caches,
        later chunks continue the stream (demo.py:399-427 does the same with `use_cache=True`)."""
        if chunk_index == 0:
            self.model.clear_cache()
        return self.decode_to_pixel(latent, use_cache=True)
