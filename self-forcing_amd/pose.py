"""Pose front end on the GPU: rendered DWPose frames -> pose tokens for the causal generator's `add_condition`
(pipeline/causal_diffusion_inference.py:87-145, :329-347 of the reference).

    emb = PoseEmbedder("checkpoints/pose.pt", device="cuda")             # or a state dict (pose_weights.synth_pose_state_dict)
    tokens, (f, h, w) = emb.embed(dwpose_data)                           # [3, F, H, W] in 0..255 -> [1, f*h*w, 5120]
    pose_emb, ref_map = emb.encode_pose(dwpose_data, random_ref_dwpose)  # the reference's two tensors, its layouts
    pipe = CausalDiffusionInferencePipeline(args, device, ..., pose_embedder=emb)
    pipe.inference(noise, prompts, None, dwpose_data, random_ref_dwpose)

Every kernel is in csrc/ (pose_conv.hip, pose_embed.hip, gemm_bf16.hip); a clip is ONE C call (`sf_pose_embed`).  The
tokens come out token-major, which is already the `add_condition` layout: a chunk's tokens are a contiguous row range.
There is no eager/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple, Union

import torch

from . import _lib
from .device_model import DeviceModel
from .pose_weights import (CIN_STORE, DWPOSE_LAYERS, POSE_DIM, RANDOMREF_DIM, RANDOMREF_LAYERS, pad_pose_bias, pose_plan, ref_plan, repack_pose_conv,
                           repack_pose_embed, split_pose_state_dict)

Tensor = torch.Tensor


def load_pose_state_dict(state_dict_or_path: Union[str, Dict[str, Tensor]]) -> Dict[str, Tensor]:
    """A pose weight file (`args.pose_weights_path`, :124-128) or an already loaded state dict."""
    if isinstance(state_dict_or_path, str):
        return torch.load(state_dict_or_path, map_location="cpu", weights_only=True)
    return state_dict_or_path


class PoseEmbedder(DeviceModel):
    """Device-resident `dwpose_embedding` + `randomref_embedding_pose`: repacked weights and the C model descriptor.
    `state_dict` names carry the `dwpose_embedding.` / `randomref_embedding_pose.` prefixes; `strict` as
    `load_pose_embedding_weights` (:124-145).  A stack the file does not hold cannot be run."""

    def __init__(self, state_dict_or_path: Union[str, Dict[str, Tensor]], device="cuda", strict: bool = True):
        super().__init__(device)
        dw, ref = split_pose_state_dict(load_pose_state_dict(state_dict_or_path), strict=strict)
        m = _lib.PoseModel()
        self.has_dwpose, self.has_randomref = dw is not None, ref is not None
        if dw is not None:
            for i, (idx, _, cout, _, stride, _, act) in enumerate(DWPOSE_LAYERS[:-1]):
                self._layer(m.conv[i], dw[f"{idx}.weight"], dw[f"{idx}.bias"], CIN_STORE if i == 0 else 0, 3, stride[0], stride[1], act)
            last = DWPOSE_LAYERS[-1][0]
            m.embed_w = self._dev(repack_pose_embed(dw[f"{last}.weight"].float()), torch.bfloat16).data_ptr()
            m.embed_b = self._dev(dw[f"{last}.bias"], torch.bfloat16).data_ptr()
            m.pose_dim = POSE_DIM
        if ref is not None:
            for i, (idx, _, cout, _, stride, _, act) in enumerate(RANDOMREF_LAYERS):
                self._layer(m.ref_conv[i], ref[f"{idx}.weight"], ref[f"{idx}.bias"], CIN_STORE if i == 0 else 0, 1, 1, stride[0], act)
        self.cmodel = m

    def _layer(self, dst: _lib.PoseLayer, w: Tensor, b: Tensor, cin_store: int, kt: int, stride_t: int, stride_s: int, act: bool) -> None:
        rp = self._dev(repack_pose_conv(w.float(), cin_store), torch.bfloat16)
        dst.w, dst.bias = rp.data_ptr(), self._dev(pad_pose_bias(b), torch.float32).data_ptr()
        dst.cin, dst.cout, dst.kt = cin_store or w.shape[1], w.shape[0], kt
        dst.stride_t, dst.stride_s, dst.ldw, dst.silu = stride_t, stride_s, rp.shape[1], int(act)

    # ---------------------------------------------------------------------------------
    def scratch_bytes(self, num_frames: int, H: int, W: int) -> int:
        """Scratch of one `embed` call (`num_frames` >= 1) or of `embed_ref` (`num_frames` = 0)."""
        n = int(_lib.lib().sf_pose_scratch_bytes(C.byref(self.cmodel), num_frames, H, W))
        if n == 0:
            _lib.check(-1, "sf_pose_scratch_bytes")
        return n

    def _scratch_for(self, num_frames: int, H: int, W: int) -> Tensor:
        # one clip at a time: a full-size clip's scratch is a few GB
        return self._stream_bytes((num_frames, H, W), lambda: self.scratch_bytes(num_frames, H, W), keep_one=True)

    def _pose_input(self, x: Tensor, what: str) -> Tuple[Tensor, int]:
        name = str(x.dtype).replace("torch.", "")
        if name not in _lib.POSE_DTYPES:
            if not x.is_floating_point():
                raise ValueError(f"{what}: pose data must be uint8 or floating point holding 0..255, got {x.dtype}")
            x, name = x.float(), "float32"
        return x.to(self.device).contiguous(), _lib.POSE_DTYPES[name]

    def embed(self, dwpose_data: Tensor) -> Tuple[Tensor, Tuple[int, int, int]]:
        """dwpose_data [3, F, H, W] (or [B, 3, F, H, W]) in 0..255 -> (tokens bf16 [B, f*h*w, 5120], (f, h, w)): the
        reference's `dwpose_embedding(cat([first x3, clip]) / 255)` (:337-340) as 'b c f h w -> b (f h w) c' (:388-391)."""
        if not self.has_dwpose:
            raise RuntimeError("the pose weights hold no dwpose_embedding.* tensors")
        if dwpose_data.dim() == 5:
            outs = [self.embed(d) for d in dwpose_data]
            return torch.cat([t for t, _ in outs], dim=0), outs[0][1]
        if dwpose_data.dim() != 4 or dwpose_data.shape[0] != 3:
            raise ValueError(f"dwpose_data must be [3, F, H, W], got {tuple(dwpose_data.shape)}")
        x, code = self._pose_input(dwpose_data, "dwpose_data")
        _, F, H, W = x.shape
        f, h, w = pose_plan(F, H, W)
        scratch = self._scratch_for(F, H, W)
        tokens = torch.empty(1, f * h * w, POSE_DIM, dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().sf_pose_embed(C.byref(self.cmodel), x.data_ptr(), code, F, H, W, scratch.data_ptr(), scratch.numel(),
                                                tokens.data_ptr(), f * h * w, stream), "sf_pose_embed")
        x.record_stream(torch.cuda.current_stream(self.device))
        return tokens, (f, h, w)

    def embed_ref(self, random_ref_dwpose: Tensor) -> Tensor:
        """random_ref_dwpose [H, W, 3] in 0..255 -> bf16 [1, 20, 1, H/8, W/8] (:341-343), a view of the channels-last map."""
        if not self.has_randomref:
            raise RuntimeError("the pose weights hold no randomref_embedding_pose.* tensors")
        if random_ref_dwpose.dim() != 3 or random_ref_dwpose.shape[2] != 3:
            raise ValueError(f"random_ref_dwpose must be [H, W, 3], got {tuple(random_ref_dwpose.shape)}")
        x, code = self._pose_input(random_ref_dwpose, "random_ref_dwpose")
        H, W, _ = x.shape
        h, w = ref_plan(H, W)
        scratch = self._scratch_for(0, H, W)
        out = torch.empty(h, w, RANDOMREF_DIM, dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().sf_pose_embed_ref(C.byref(self.cmodel), x.data_ptr(), code, H, W, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                                    stream), "sf_pose_embed_ref")
        x.record_stream(torch.cuda.current_stream(self.device))
        return out.permute(2, 0, 1)[None, :, None]

    def encode_pose(self, dwpose_data: Tensor, random_ref_dwpose: Optional[Tensor]) -> Tuple[Tensor, Optional[Tensor]]:
        """The reference's two tensors in its layouts (:337-343): `dwpose_data_emb` [B, 5120, f, h, w] (a permuted VIEW of
        the tokens) and the reference-pose map [1, 20, 1, H/8, W/8] (None without `random_ref_dwpose`)."""
        tokens, (f, h, w) = self.embed(dwpose_data)
        emb = tokens.view(tokens.shape[0], f, h, w, POSE_DIM).permute(0, 4, 1, 2, 3)
        return emb, (self.embed_ref(random_ref_dwpose) if random_ref_dwpose is not None else None)
