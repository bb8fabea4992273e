"""Pose front end on the GPU: rendered DWPose frames -> pose tokens for the causal generator's `add_condition`
(pipeline/causal_diffusion_inference.py:87-145, :329-347 of the reference).

    emb = PoseEmbedder("checkpoints/pose.pt", device="cuda")             # or a state dict (pose_weights.synth_pose_state_dict)
    tokens, (f, h, w) = emb.embed(dwpose_data)                           # [3, F, H, W] in 0..255 -> [1, f*h*w, 5120]
    pose_emb, ref_map = emb.encode_pose(dwpose_data, random_ref_dwpose)  # the reference's two tensors, its layouts
    pipe = CausalDiffusionInferencePipeline(args, device, ..., pose_embedder=emb)
    pipe.inference(noise, prompts, None, dwpose_data, random_ref_dwpose)

    stream = emb.open_stream(H, W)                                       # a clip in pieces (a live feed, a long clip)
    tokens, m = stream.push(frames)                                      # [3, n, H, W] -> the rows of the m latent frames now final
    tokens, m = stream.close()                                           # the tail, with the clip-end padding
    tokens, (f, h, w) = emb.embed_long(dwpose_data)                      # `embed` through a stream: clips `embed` refuses

Every kernel is in csrc/ (pose_conv.hip, pose_embed.hip, gemm_bf16.hip); a clip is ONE C call (`sf_pose_embed`), a piece
of one ONE call too (`sf_pose_stream_push`), and the pieces' rows are the whole clip's, bit for bit.  The tokens come out
token-major, which is already the `add_condition` layout: a chunk's tokens are a contiguous row range.
There is no eager/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple, Union

import torch

from . import _lib
from .device_model import DeviceModel
from .torch_ops import _dtype_name
from .pose_weights import (CIN_STORE, DWPOSE_LAYERS, POSE_DIM, RANDOMREF_DIM, RANDOMREF_LAYERS, pad_pose_bias, pose_plan, pose_stream_plan,
                           ref_plan, repack_pose_conv, repack_pose_embed, split_pose_state_dict)

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
        name = _dtype_name(x)
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

    # --------------------------------------------------------------------------------- a clip in pieces
    def open_stream(self, H: int, W: int, max_frames_per_push: int = 16) -> "PoseStream":
        """A resumable `embed` for H x W frames: push the clip in pieces, get every latent frame's rows as soon as the
        frames it depends on are in.  Each stream owns its history and scratch; any number may be open."""
        if not self.has_dwpose:
            raise RuntimeError("the pose weights hold no dwpose_embedding.* tensors")
        return PoseStream(self, H, W, max_frames_per_push)

    def embed_long(self, dwpose_data: Tensor, frames_per_push: int = 12) -> Tuple[Tensor, Tuple[int, int, int]]:
        """`embed` through a `PoseStream`, `frames_per_push` frames at a time: the same tokens, bit for bit, with scratch
        that does not grow with the clip -- for clips whose volumes `embed` refuses (4 GiB: ~145 frames of 720x1280)."""
        if dwpose_data.dim() == 5:
            outs = [self.embed_long(d, frames_per_push) for d in dwpose_data]
            return torch.cat([t for t, _ in outs], dim=0), outs[0][1]
        if dwpose_data.dim() != 4 or dwpose_data.shape[0] != 3:
            raise ValueError(f"dwpose_data must be [3, F, H, W], got {tuple(dwpose_data.shape)}")
        if frames_per_push < 1:
            raise ValueError(f"frames_per_push must be at least 1, got {frames_per_push}")
        _, F, H, W = dwpose_data.shape
        f, h, w = pose_plan(F, H, W)
        tokens = torch.empty(1, f * h * w, POSE_DIM, dtype=torch.bfloat16, device=self.device)
        stream = self.open_stream(H, W, frames_per_push)
        for i in range(0, F, frames_per_push):
            stream.push(dwpose_data[:, i:i + frames_per_push], out=tokens, out_row=stream.latent_frames_done * h * w)
        stream.close(out=tokens, out_row=stream.latent_frames_done * h * w)
        assert stream.latent_frames_done == f
        return tokens, (f, h, w)


class PoseStream:
    """One clip going through the dwpose stack piece by piece (`PoseEmbedder.open_stream`).  Latent frame j is final
    once 4j + 5 pixel frames are in; `close` declares the clip ended and flushes the frames that were waiting for
    neighbours.  The history (two frames per layer input) and the scratch are this stream's own."""

    def __init__(self, embedder: PoseEmbedder, H: int, W: int, max_frames_per_push: int = 16):
        if max_frames_per_push < 1:
            raise ValueError(f"max_frames_per_push must be at least 1, got {max_frames_per_push}")
        self.embedder, self.H, self.W, self.max_frames_per_push = embedder, int(H), int(W), int(max_frames_per_push)
        _, self.h, self.w = pose_plan(1, self.H, self.W)
        lib, cm = _lib.lib(), C.byref(embedder.cmodel)
        nbytes = []
        for what, n in (("sf_pose_stream_state_bytes", lib.sf_pose_stream_state_bytes(cm, self.H, self.W)),
                        ("sf_pose_stream_scratch_bytes", lib.sf_pose_stream_scratch_bytes(cm, self.max_frames_per_push, self.H, self.W))):
            if int(n) == 0:
                _lib.check(-1, what)
            nbytes.append(int(n))
        self._state = torch.empty(nbytes[0], dtype=torch.uint8, device=embedder.device)
        self._scratch = torch.empty(nbytes[1], dtype=torch.uint8, device=embedder.device)
        self.frames_pushed = 0
        self.latent_frames_done = 0
        self.closed = False

    @property
    def hw(self) -> Tuple[int, int]:
        return self.h, self.w

    def _call(self, x: Optional[Tensor], code: int, n: int, closing: bool, dst: Tensor, row: int) -> int:
        dev = self.embedder.device
        written = C.c_int32(0)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.lib().sf_pose_stream_push(C.byref(self.embedder.cmodel), self._state.data_ptr(), self.frames_pushed,
                                                      x.data_ptr() if x is not None else None, code, n, self.H, self.W, int(closing),
                                                      self._scratch.data_ptr(), self._scratch.numel(),
                                                      dst.data_ptr() + row * POSE_DIM * 2, dst.shape[1] - row, C.byref(written), stream),
                       "sf_pose_stream_push")
        if x is not None:
            x.record_stream(torch.cuda.current_stream(dev))
        self.frames_pushed += n
        self.latent_frames_done += written.value
        return written.value

    def _run(self, frames: Optional[Tensor], closing: bool, out: Optional[Tensor], out_row: int) -> Tuple[Tensor, int]:
        if self.closed:
            raise RuntimeError("this pose stream is closed: open a new one for the next clip")
        code, n = 0, 0
        if frames is not None:
            if frames.dim() != 4 or frames.shape[0] != 3 or tuple(frames.shape[2:]) != (self.H, self.W):
                raise ValueError(f"pose frames must be [3, n, {self.H}, {self.W}], got {tuple(frames.shape)}")
            frames, code = self.embedder._pose_input(frames, "pose frames")
            n = frames.shape[1]
        if closing and self.frames_pushed + n == 0:
            raise ValueError("a pose stream cannot be closed before its first frame")
        fs = self.h * self.w
        step = self.max_frames_per_push
        pieces = [(i, min(step, n - i)) for i in range(0, n, step)] or [(0, 0)]
        # the rows this call makes final, from the plan alone
        m = sum(pose_stream_plan(self.frames_pushed + i, k, closing and i + k == n)[1][-1] for i, k in pieces)
        if out is None:
            dst, row = torch.empty(1, m * fs, POSE_DIM, dtype=torch.bfloat16, device=self.embedder.device), 0
        else:
            if out.dim() != 3 or out.shape[0] != 1 or out.shape[2] != POSE_DIM or out.dtype != torch.bfloat16 or not out.is_contiguous() \
                    or out.device != self.embedder.device:
                raise ValueError(f"out must be a contiguous bf16 [1, rows, {POSE_DIM}] tensor on {self.embedder.device}, got {tuple(out.shape)} {out.dtype}")
            if out_row < 0 or out_row + m * fs > out.shape[1]:
                raise ValueError(f"out holds {out.shape[1]} rows: {m} latent frames of {fs} rows do not fit at row {out_row}")
            dst, row = out, out_row
        first = row
        for i, k in pieces:
            x = frames[:, i:i + k].contiguous() if k else None
            row += self._call(x, code, k, closing and i + k == n, dst, row) * fs
        assert row - first == m * fs, "the library's plan and pose_weights.pose_stream_plan disagree"
        self.closed = closing
        return dst[:, first:row], m

    def push(self, frames: Tensor, out: Optional[Tensor] = None, out_row: int = 0) -> Tuple[Tensor, int]:
        """frames [3, n, H, W] in 0..255 (uint8 / float / bf16, as `embed`) -> (tokens bf16 [1, m*h*w, 5120], m): the rows
        of the m latent frames this push made final (m may be 0).  More than `max_frames_per_push` frames are split.
        With `out` (bf16 [1, rows, 5120]) the rows are written there from row `out_row` and the result is a view of it."""
        return self._run(frames, False, out, out_row)

    def close(self, out: Optional[Tensor] = None, out_row: int = 0) -> Tuple[Tensor, int]:
        """Declare the clip ended: the remaining latent frames, which see the zero padding behind the last frame as in
        `embed`.  Nothing can be pushed afterwards."""
        return self._run(None, True, out, out_row)
