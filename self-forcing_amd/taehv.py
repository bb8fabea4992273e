"""TAEHV tiny autoencoder on the GPU: the fast preview path of the reference's demo (demo.py:60-100, :319-435;
demo_utils/taehv.py) behind the `WanVAEWrapper` contract.

    vae = TAEHVWrapper(state_dict=..., device="cuda")                     # or checkpoint_path="checkpoints/taew2_1.pth"
    video = vae.decode_to_pixel(latent, use_cache=False)      # [B, F, 16, h, w] -> [B, 1+4(F-1), 3, 8h, 8w] in [-1, 1]
    latent = vae.encode_to_latent(video.transpose(1, 2))      # [B, 3, 1+4k, H, W] -> [B, 1+k, 16, H/8, W/8]
    pipe = CausalInferencePipeline(cfg, device, vae=vae)      # drops in for the Wan VAE; stream() uses decode_chunk

Every kernel is in csrc/ (taehv_conv.hip, taehv_decode.hip, taehv_encode_conv.hip, taehv_encode.hip); a group of latent
frames is ONE C call (`sf_taehv_decode_frames`, `sf_taehv_encode_frames`).  The nine one-frame MemBlock memories of each
half are carried between calls, so a streamed decode or encode is bit-identical to the one-shot one (the demo instead
re-decodes the last 3 latent frames from a fresh memory, demo.py:423-435, which only approximates it).  There is no
eager/CPU fallback.  The encoder is built when the state dict holds `encoder.*` tensors (taew2_1.pth does).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch

from . import _lib, torch_ops
from .device_model import DeviceModel
from .taehv_weights import (ENC_C, ENC_HEAD, ENC_STAGE_FIRST, ENC_TPOOL, FRAMES_TO_TRIM, LATENT_CHANNELS, N_F, SPATIAL_FACTOR, STAGE_FIRST,
                            TAEHV_CHECKPOINT, TEMPORAL_FACTOR, TGROW, fold_tgrow, fold_tpool, has_encoder, patch_tgrow_rows, repack_memblock_conv0,
                            repack_stem, repack_taehv_conv, taehv_encoder_param_shapes, taehv_param_shapes, tpool_taps)

Tensor = torch.Tensor


class TAEHVDecoder(DeviceModel):
    """Device-resident decoder: repacked bf16 weights, the C model descriptor, and per latent size one decode state (the
    nine MemBlock memories of one stream).  Counterpart of `TAEHV.decode_video` (taehv.py:222-234)."""

    def __init__(self, state_dict: Dict[str, Tensor], device="cuda", frames_per_call: int = 3,
                 decoder_time_upscale=(True, True), decoder_space_upscale=(True, True, True)):
        self.param_shapes = taehv_param_shapes(decoder_time_upscale, decoder_space_upscale)   # ValueError on other switches
        if not 1 <= frames_per_call <= 64:
            raise ValueError("frames_per_call must be in 1..64")
        super().__init__(device)
        self.frames_per_call = frames_per_call          # latent frames handed to one C call (any value gives the same bits)
        self._state: Dict[tuple, Tensor] = {}
        self._load(state_dict)

    # ---------------------------------------------------------------------------------
    def _layer(self, dst: _lib.TaehvLayer, w: Tensor, bias: Optional[Tensor], cin_pad: int = 0) -> None:
        if w.dim() == 4:
            w = w.unsqueeze(2)
        cout, cin, kt = w.shape[:3]
        rp = self._dev(repack_taehv_conv(w.float(), cin_pad))
        dst.w = rp.data_ptr()
        dst.bias = self._dev(bias).data_ptr() if bias is not None else None
        dst.cin, dst.cout, dst.kt, dst.ldw = cin_pad or ((cin + 31) // 32) * 32, cout, kt, rp.shape[1]

    def _load(self, sd: Dict[str, Tensor]) -> None:
        sd = patch_tgrow_rows(sd)
        self._check_state_dict(sd, self.param_shapes, "TAEHV state dict", "decoder tensors")
        m = _lib.TaehvModel()
        m.z_dim = LATENT_CHANNELS
        self._layer(m.in_conv, sd["decoder.1.weight"], sd["decoder.1.bias"], cin_pad=32)
        for s, first in enumerate(STAGE_FIRST):
            for b in range(_lib.TAEHV_BLOCKS):
                p = f"decoder.{first + b}.conv."
                self._layer(m.block[s][b][0], repack_memblock_conv0(sd[p + "0.weight"]), sd[p + "0.bias"])
                self._layer(m.block[s][b][1], sd[p + "2.weight"], sd[p + "2.bias"])
                self._layer(m.block[s][b][2], sd[p + "4.weight"], sd[p + "4.bias"])
            self._layer(m.exit_conv[s], fold_tgrow(sd[f"decoder.{first + 4}.conv.weight"], sd[f"decoder.{first + 5}.weight"]), None)
            m.tgrow[s] = TGROW[s]
        self._layer(m.head, sd["decoder.22.weight"], sd["decoder.22.bias"])
        self.cmodel = m
        self._handle = torch_ops.register_model(self)

    def state_bytes(self, h: int, w: int) -> int:
        return int(_lib.lib().sf_taehv_state_bytes(C.byref(self.cmodel), h, w))

    def scratch_bytes(self, h: int, w: int) -> int:
        return int(_lib.lib().sf_taehv_scratch_bytes(C.byref(self.cmodel), h, w, self.frames_per_call))

    # ---------------------------------------------------------------------------------
    def _buffers(self, h: int, w: int):
        key = (h, w)
        if (TEMPORAL_FACTOR * self.frames_per_call) * (SPATIAL_FACTOR * h) * (SPATIAL_FACTOR * w) * N_F[3] * 2 >= 0xFFFFFF00:
            raise ValueError(f"frames_per_call={self.frames_per_call} at {SPATIAL_FACTOR * h}x{SPATIAL_FACTOR * w}: the head's input volume would "
                             "pass 4 GiB (the kernels address a volume through one 32-bit-ranged buffer descriptor); use fewer frames per call")
        if key not in self._state:
            n = self.state_bytes(h, w)
            if n == 0:
                _lib.check(-1, "sf_taehv_state_bytes")
            self._state[key] = torch.zeros(n, dtype=torch.uint8, device=self.device)      # zero = a fresh memory
        return self._state[key], self._stream_bytes(key, lambda: self.scratch_bytes(h, w))

    def clear_cache(self) -> None:
        """Forget every MemBlock's memory: the next frame's `past` is zero (taehv.py:115-116)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream if self._state else None
        for (h, w), st in self._state.items():
            _lib.check(_lib.lib().sf_taehv_reset(C.byref(self.cmodel), st.data_ptr(), st.numel(), h, w, stream), "sf_taehv_reset")

    def cached_decode(self, z: Tensor, clamp: bool = False) -> Tensor:
        """z [F, 16, h, w] (as the generator emits it: no mean / std un-scaling) -> float32 [4F, 3, 8h, 8w] =
        `decode_video(z, parallel=False) * 2 - 1` continued from the memory the previous call left; nothing trimmed."""
        if z.dim() != 4 or z.shape[1] != LATENT_CHANNELS:
            raise ValueError(f"expected latents [F, {LATENT_CHANNELS}, h, w], got {tuple(z.shape)}")
        z = z.to(device=self.device, dtype=torch.bfloat16).contiguous()
        F, _, h, w = z.shape
        state, scratch = self._buffers(h, w)
        out = torch.empty(TEMPORAL_FACTOR * F, 3, SPATIAL_FACTOR * h, SPATIAL_FACTOR * w, dtype=torch.float32, device=self.device)
        for i in range(0, F, self.frames_per_call):
            g = min(self.frames_per_call, F - i)
            torch.ops.sf_hip.taehv_decode_frames(self._handle, state, scratch, z[i:i + g], out[TEMPORAL_FACTOR * i:], h, w, clamp)
        return out

    def decode(self, z: Tensor, clamp: bool = False) -> Tensor:
        """The demo wrapper's `decode_video(...) * 2 - 1` (demo.py:95-98) from a cleared memory, cleared again after."""
        self.clear_cache()
        out = self.cached_decode(z, clamp)
        self.clear_cache()
        return out


class TAEHVEncoder(DeviceModel):
    """Device-resident encoder: repacked bf16 weights (TPool folded into the strided convolutions), the C descriptor,
    and per frame size one encode state (the nine MemBlock memories of one stream).  Counterpart of `TAEHV.encode_video`
    (taehv.py:210-220)."""

    def __init__(self, state_dict: Dict[str, Tensor], device="cuda", frames_per_call: int = 3):
        self.param_shapes = taehv_encoder_param_shapes()
        if not 1 <= frames_per_call <= 64:
            raise ValueError("frames_per_call must be in 1..64")
        super().__init__(device)
        self.frames_per_call = frames_per_call          # LATENT frames (4 pixel frames each) per C call (any value gives the same bits)
        self._state: Dict[tuple, Tensor] = {}
        self._load(state_dict)

    _layer = TAEHVDecoder._layer

    def _load(self, sd: Dict[str, Tensor]) -> None:
        self._check_state_dict(sd, self.param_shapes, "TAEHV state dict", "encoder tensors")
        m = _lib.TaehvEncoder()
        m.stem.w = self._dev(repack_stem(sd["encoder.0.weight"].float())).data_ptr()
        m.stem.bias = self._dev(sd["encoder.0.bias"]).data_ptr()
        m.stem.cin, m.stem.cout, m.stem.kt, m.stem.ldw = 32, ENC_C, 1, 32
        for s, first in enumerate(ENC_STAGE_FIRST):
            folded = fold_tpool(sd[f"encoder.{first}.conv.weight"], sd[f"encoder.{first + 1}.weight"])      # fp32; rounded once, by _layer
            self._layer(m.down[s], tpool_taps(folded, ENC_TPOOL[s]), None)
            for b in range(_lib.TAEHV_BLOCKS):
                p = f"encoder.{first + 2 + b}.conv."
                self._layer(m.block[s][b][0], repack_memblock_conv0(sd[p + "0.weight"]), sd[p + "0.bias"])
                self._layer(m.block[s][b][1], sd[p + "2.weight"], sd[p + "2.bias"])
                self._layer(m.block[s][b][2], sd[p + "4.weight"], sd[p + "4.bias"])
        self._layer(m.head, sd[f"encoder.{ENC_HEAD}.weight"], sd[f"encoder.{ENC_HEAD}.bias"])
        self.cmodel = m
        self._handle = torch_ops.register_model(self)

    def state_bytes(self, H: int, W: int) -> int:
        return int(_lib.lib().sf_taehv_encode_state_bytes(C.byref(self.cmodel), H, W))

    def scratch_bytes(self, H: int, W: int) -> int:
        return int(_lib.lib().sf_taehv_encode_scratch_bytes(C.byref(self.cmodel), H, W, TEMPORAL_FACTOR * self.frames_per_call))

    # ---------------------------------------------------------------------------------
    def _buffers(self, H: int, W: int):
        if H % SPATIAL_FACTOR or W % SPATIAL_FACTOR:
            raise ValueError(f"encode: height and width must be multiples of {SPATIAL_FACTOR}, got {H}x{W}")
        if TEMPORAL_FACTOR * self.frames_per_call * H * W * ENC_C * 2 >= 0xFFFFFF00:
            raise ValueError(f"frames_per_call={self.frames_per_call} at {H}x{W}: the stem's output volume would pass 4 GiB (the kernels "
                             "address a volume through one 32-bit-ranged buffer descriptor); use fewer frames per call")
        key = (H, W)
        if key not in self._state:
            n = self.state_bytes(H, W)
            if n == 0:
                _lib.check(-1, "sf_taehv_encode_state_bytes")
            self._state[key] = torch.zeros(n, dtype=torch.uint8, device=self.device)      # zero = a fresh memory
        return self._state[key], self._stream_bytes(key, lambda: self.scratch_bytes(H, W), "sf_taehv_encode_scratch_bytes")

    def clear_cache(self) -> None:
        """Forget every MemBlock's memory: the next frame's `past` is zero (taehv.py:115-116)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream if self._state else None
        for (H, W), st in self._state.items():
            _lib.check(_lib.lib().sf_taehv_encode_reset(C.byref(self.cmodel), st.data_ptr(), st.numel(), H, W, stream), "sf_taehv_encode_reset")

    def cached_encode(self, pixels: Tensor, lead: int = 0, channels_first: Optional[bool] = None) -> Tensor:
        """pixels [T, 3, H, W], or [3, T, H, W] with any channel stride (`channels_first`; inferred from where the 3 is,
        [T, 3, H, W] when both fit), bf16 or float32 in [-1, 1], with the first frame `lead` (0..3) more times in front;
        (lead + T) % 4 == 0 -> float32 [(lead + T) / 4, 16, H/8, W/8] = `encode_video((pixels + 1) / 2)` continued from the
        memory the previous call left, in the generator's space (no mean / std)."""
        if pixels.dim() != 4 or 3 not in tuple(pixels.shape[:2]):
            raise ValueError(f"expected pixels [T, 3, H, W] or [3, T, H, W], got {tuple(pixels.shape)}")
        if channels_first is None:
            channels_first = pixels.shape[1] != 3
        if pixels.shape[0 if channels_first else 1] != 3:
            raise ValueError(f"expected 3 colour channels, got {tuple(pixels.shape)}")
        x = pixels if channels_first else pixels.transpose(0, 1)
        if x.dtype not in (torch.bfloat16, torch.float32):
            x = x.float()
        x = x.to(self.device)
        if not x[0].is_contiguous():
            x = x.contiguous()
        _, T, H, W = x.shape
        if not 0 <= lead < TEMPORAL_FACTOR or T < 1 or (lead + T) % TEMPORAL_FACTOR:
            raise ValueError(f"cached_encode: lead={lead} + {T} frames is not a whole number of groups of {TEMPORAL_FACTOR}")
        state, scratch = self._buffers(H, W)
        F = (lead + T) // TEMPORAL_FACTOR
        out = torch.empty(F, LATENT_CHANNELS, H // SPATIAL_FACTOR, W // SPATIAL_FACTOR, dtype=torch.float32, device=self.device)
        f0 = 0
        for i in range(0, F, self.frames_per_call):
            g = min(self.frames_per_call, F - i)
            ld = lead if i == 0 else 0
            nf = TEMPORAL_FACTOR * g - ld
            torch.ops.sf_hip.taehv_encode_frames(self._handle, state, scratch, x[:, f0:f0 + nf], out[i:i + g], H, W, ld)
            f0 += nf
        return out

    def encode(self, pixels: Tensor, lead: int = 0, channels_first: Optional[bool] = None) -> Tensor:
        """`encode_video` from a cleared memory, cleared again after."""
        self.clear_cache()
        out = self.cached_encode(pixels, lead, channels_first)
        self.clear_cache()
        return out


class _TrimmingModel:
    """`.model` of the wrapper: the decoder plus the stream's trim bookkeeping, so that `vae.model.clear_cache()`
    (inference.py:183) also restarts the first-3-frames trim -- and clears the encoder, when there is one."""

    def __init__(self, decoder: TAEHVDecoder, encoder: Optional["TAEHVEncoder"] = None):
        self.decoder = decoder
        self.encoder = encoder
        self._fresh: Dict[tuple, bool] = {}

    def clear_cache(self) -> None:
        self.decoder.clear_cache()
        if self.encoder is not None:
            self.encoder.clear_cache()
        self._fresh.clear()

    def _trimmed(self, z: Tensor) -> Tensor:
        key = tuple(z.shape[-2:])
        out = self.decoder.cached_decode(z, clamp=True)
        if self._fresh.get(key, True):
            out = out[FRAMES_TO_TRIM:]
        self._fresh[key] = False
        return out

    def cached_decode(self, z: Tensor) -> Tensor:
        return self._trimmed(z)

    def decode(self, z: Tensor) -> Tensor:
        self.clear_cache()
        out = self._trimmed(z)
        self.clear_cache()
        return out


class TAEHVWrapper(torch.nn.Module):
    """The `WanVAEWrapper` decode contract (utils/wan_wrapper.py:95-117) on the TAEHV decoder, as the demo's
    `TAEHVDiffusersWrapper` offers it (demo.py:88-100): `decode_to_pixel`, `decode_chunk`, `.model.clear_cache()`.

    `state_dict`: the tensors of `taew2_1.pth` or `taehv_weights.synth_taehv_state_dict`; when it holds `encoder.*`
    tensors as well (taew2_1.pth does; `synth_taehv_encoder_state_dict`), `encode_to_latent` works too.  Without one
    `checkpoint_path` is loaded (weights-only), FileNotFoundError when it is absent -- nothing is downloaded."""

    def __init__(self, state_dict: Optional[Dict[str, Tensor]] = None, device="cuda", checkpoint_path: str = TAEHV_CHECKPOINT,
                 frames_per_call: int = 3):
        super().__init__()
        if state_dict is None:
            if not os.path.exists(checkpoint_path):
                raise FileNotFoundError(f"TAEHV checkpoint {checkpoint_path!r} not found: place taew2_1.pth there as the reference's demo "
                                        "expects, or construct TAEHVWrapper(state_dict=...)")
            state_dict = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        self.decoder = TAEHVDecoder(state_dict, device, frames_per_call=frames_per_call)
        self.encoder = TAEHVEncoder(state_dict, device, frames_per_call=frames_per_call) if has_encoder(state_dict) else None
        self._encoder_missing = [] if self.encoder is not None else list(taehv_encoder_param_shapes())
        self.model = _TrimmingModel(self.decoder, self.encoder)

    def encode_to_latent(self, pixel: Tensor) -> Tensor:
        """pixel [B, 3, T, H, W] in [-1, 1], T = 1 + 4k (the `WanVAEWrapper` contract, and the shape `decode_to_pixel`
        returns) -> float32 latents [B, 1 + k, 16, H/8, W/8] in the generator's space, one sample at a time from a cleared
        memory.  TAEHV pools every four frames into one, so the first frame fills the first group of four (it is encoded
        as four copies of itself): the mirror of the three frames the decode drops at the start of a stream.  The
        reference has no encode wrapper for TAEHV; this convention is this project's choice."""
        if self.encoder is None:
            m = self._encoder_missing
            raise NotImplementedError(f"this TAEHV state dict has no encoder: {len(m)} encoder.* tensors are missing, e.g. {m[:3]} "
                                      "(load taew2_1.pth, or add synth_taehv_encoder_state_dict(...)); or encode with WanVAEWrapper")
        if pixel.dim() != 5 or pixel.shape[1] != 3:
            raise ValueError(f"encode_to_latent expects pixels [B, 3, T, H, W], got {tuple(pixel.shape)}")
        if pixel.shape[2] % TEMPORAL_FACTOR != 1:
            raise ValueError(f"encode_to_latent: T = 1 + 4k frames expected, got {pixel.shape[2]}")
        if pixel.shape[3] % SPATIAL_FACTOR or pixel.shape[4] % SPATIAL_FACTOR:
            raise ValueError(f"encode_to_latent: height and width must be multiples of {SPATIAL_FACTOR}, got {pixel.shape[3]}x{pixel.shape[4]}")
        return torch.stack([self.encoder.encode(u, lead=FRAMES_TO_TRIM, channels_first=True) for u in pixel], dim=0)

    def decode_to_pixel(self, latent: Tensor, use_cache: bool = False) -> Tensor:
        """latent [B, F, 16, h, w] -> float32 [B, T, 3, 8h, 8w] clamped to [-1, 1]; T = 1 + 4 (F - 1) from a cleared
        memory (the first 3 frames dropped, demo.py:432-433), 4 F when `use_cache` continues a stream."""
        if latent.dim() != 5:
            raise ValueError(f"decode_to_pixel expects latents [B, F, 16, h, w], got {tuple(latent.shape)}")
        if use_cache:
            assert latent.shape[0] == 1, "Batch size must be 1 when using cache"
        fn = self.model.cached_decode if use_cache else self.model.decode
        return torch.stack([fn(u) for u in latent], dim=0)

    def decode_chunk(self, latent: Tensor, chunk_index: int) -> Tensor:
        """Streaming decode used by `CausalInferencePipeline.stream`: chunk 0 starts from a cleared memory (4F - 3
        frames), later chunks continue the stream (4F frames)."""
        if chunk_index == 0:
            self.model.clear_cache()
        return self.decode_to_pixel(latent, use_cache=True)
