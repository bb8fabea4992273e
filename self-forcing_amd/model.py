"""Device-resident causal Wan DiT: weights in HBM + the C-ABI descriptor of one forward.

Counterpart of `CausalWanModel` (wan/modules/causal_model.py:370-513) for the KV-cached
inference branch only (`_forward_inference`, :725-893).  It owns the bf16 weights (with `fp8=True`: e4m3 copies of
every Linear's weight plus fp32 column scales instead, fp8.py), laid out for
the kernels (q|k|v and cross k|v projection matrices stacked so that one GEMM serves three / two
Linears), the fp32 RoPE tables and a per-shape workspace; `forward` is ONE C call
(`sf_dit_forward`) that enqueues every kernel of the pass on the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, fp8 as fp8_recipe, torch_ops
from .device_model import DeviceModel
from .kvcache import CachePlan
from .weights import I2V_Y_CHANNELS, WanShape, param_shapes

Tensor = torch.Tensor


def rope_tables(head_dim: int, max_pos: int = 1024, theta: float = 10000.0):
    """cos/sin tables [max_pos, head_dim/2] in the column layout of the reference's `freqs`
    (causal_model.py:481-488; model.py:29-36): [time | height | width] with widths
    (d/2 - 2*(d/6), d/6, d/6)... computed in float64, stored float32."""
    d = head_dim
    parts = []
    for dim in (d - 4 * (d // 6), 2 * (d // 6), 2 * (d // 6)):
        inv = 1.0 / torch.pow(torch.tensor(theta, dtype=torch.float64),
                              torch.arange(0, dim, 2, dtype=torch.float64) / dim)
        parts.append(torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :])
    ang = torch.cat(parts, dim=1)
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


class CausalWanModel(DeviceModel):
    """Inference-only causal DiT on one GPU.  Attributes mirror what the reference pipeline reads
    from `generator.model`: `local_attn_size`, `sink_size`, `num_frame_per_block`, plus the shape."""

    def __init__(self, shape: WanShape, state_dict: Dict[str, Tensor], device, sched_sigmas: Tensor,
                 sched_timesteps: Tensor, fp8: bool = False):
        if shape.head_dim != 128:
            raise ValueError(f"head_dim must be 128 (dim={shape.dim}, heads={shape.num_heads})")
        if tuple(shape.patch_size) != (1, 2, 2):
            raise ValueError("only patch_size (1, 2, 2) is supported")
        super().__init__(device)
        self.shape = shape
        self.dim, self.num_heads, self.num_layers = shape.dim, shape.num_heads, shape.num_layers
        self.local_attn_size = shape.local_attn_size
        self.sink_size = shape.sink_size
        self.num_frame_per_block = 1
        self.independent_first_frame = False
        self.fp8 = bool(fp8)
        self.fp8_weights: Dict[str, tuple] = {}
        self.model_type = shape.model_type
        if shape.is_i2v:
            if self.fp8:
                raise NotImplementedError("fp8=True is not built for the i2v model type (its img_emb / k_img / v_img Linears run in bf16 only)")
            if shape.in_dim != shape.out_dim + I2V_Y_CHANNELS or shape.clip_dim % 64:
                raise ValueError(f"i2v model: in_dim must be {shape.out_dim} + {I2V_Y_CHANNELS} and clip_dim a multiple of 64 "
                                 f"(in_dim={shape.in_dim}, clip_dim={shape.clip_dim})")
        self.y_channels = I2V_Y_CHANNELS if shape.is_i2v else 0
        self._load(state_dict, sched_sigmas, sched_timesteps)
        self._handle = torch_ops.register_model(self)

    # ---------------------------------------------------------------------------------
    def _dev8(self, name: str, parts: List[Tensor]):
        """FP8: the reference Linears `parts` (stacked along N) -> device e4m3 weight + fp32 column scales, quantised on
        the device from the bf16 weights the reference model holds (fp8.py); only these copies are kept
        (`fp8_weights[name]` = (q, s))."""
        q, s = fp8_recipe.quantize_weight([p.detach().to(device=self.device, dtype=torch.bfloat16) for p in parts])
        self._keep += [q, s]
        self.fp8_weights[name] = (q, s)
        return C.c_void_p(q.data_ptr()), C.c_void_p(s.data_ptr())

    def _load(self, sd: Dict[str, Tensor], sigmas: Tensor, timesteps: Tensor) -> None:
        self._check_state_dict(sd, param_shapes(self.shape), "state dict")
        s = self.shape
        if self.fp8:   # every K an fp8 GEMM sees must be a multiple of its 128-deep k-tile: fail here, not at the first call
            for name, k in (("text_embedding.0", s.text_dim), ("the dim-wide Linears", s.dim), ("ffn.2", s.ffn_dim)):
                fp8_recipe.check_k(name, k)
            if "pose_proj.weight" in sd:
                fp8_recipe.check_k("pose_proj", sd["pose_proj.weight"].shape[1])
        m = _lib.Model()
        m.fp8 = int(self.fp8)
        m.dim, m.ffn_dim, m.num_heads, m.num_layers = s.dim, s.ffn_dim, s.num_heads, s.num_layers
        m.in_dim, m.out_dim, m.freq_dim, m.text_dim, m.text_len = s.in_dim, s.out_dim, s.freq_dim, s.text_dim, s.text_len
        m.eps = s.eps
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        pw = sd["patch_embedding.weight"].flatten(1)
        if s.is_i2v:
            # 36 channels x 4 = 144 columns: the GEMM's k-tile wants K % 64 == 0, so the weight is zero-padded to 192
            # columns and the sequencer sees in_dim = 48 (its 12 extra channels are written as zeros by sf_patchify_i2v)
            kpad = -(-pw.shape[1] // 64) * 64
            pw = torch.cat([pw, pw.new_zeros(pw.shape[0], kpad - pw.shape[1])], dim=1)
            m.in_dim = kpad // 4
        m.patch_w = P(self._dev(pw))
        m.patch_b = P(self._dev(sd["patch_embedding.bias"]))
        for dst, src in (("text0", "text_embedding.0"), ("text2", "text_embedding.2"), ("time0", "time_embedding.0"),
                         ("time2", "time_embedding.2"), ("tproj", "time_projection.1"), ("head", "head.head")):
            if self.fp8:
                q8, s8 = self._dev8(src, [sd[src + ".weight"]])
                setattr(m, dst + "_q", q8)
                setattr(m, dst + "_s", s8)
            else:
                setattr(m, dst + "_w", P(self._dev(sd[src + ".weight"])))
            setattr(m, dst + "_b", P(self._dev(sd[src + ".bias"])))
        m.head_mod = P(self._dev(sd["head.modulation"].reshape(2, s.dim)))
        from .weights import POSE_DIM
        self.has_pose_proj = "pose_proj.weight" in sd
        if self.has_pose_proj:   # optional: the fork's pose conditioning (Linear(5120, dim), causal_model.py:493-503)
            if self.fp8:
                m.pose_q, m.pose_s = self._dev8("pose_proj", [sd["pose_proj.weight"]])
            else:
                m.pose_w = P(self._dev(sd["pose_proj.weight"]))
            m.pose_b = P(self._dev(sd["pose_proj.bias"]))
            m.pose_dim = sd["pose_proj.weight"].shape[1]
        elif s.dim == POSE_DIM:  # `pose_proj = nn.Identity()` for dim-5120 models (:500-501): no weights, x += add_condition
            m.pose_dim = s.dim
        self.accepts_pose = self.has_pose_proj or s.dim == POSE_DIM
        layers = (_lib.LayerWeights * s.num_layers)()
        layers8 = (_lib.LayerFp8 * s.num_layers)()
        for i in range(s.num_layers):
            p = f"blocks.{i}."
            lw = layers[i]
            if self.fp8:   # the Linears' weights in e4m3 only; biases, norms and modulation stay bf16 (below)
                for dst, srcs in _lib.FP8_LAYER_LINEARS:
                    q8, s8 = self._dev8(p + dst, [sd[p + src + ".weight"] for src in srcs])
                    setattr(layers8[i], dst + "_q", q8)
                    setattr(layers8[i], dst + "_s", s8)
            lw.modulation = P(self._dev(sd[p + "modulation"].reshape(6, s.dim)))
            lw.norm3_w, lw.norm3_b = P(self._dev(sd[p + "norm3.weight"])), P(self._dev(sd[p + "norm3.bias"]))
            sa, ca = p + "self_attn.", p + "cross_attn."
            W = (lambda t: None) if self.fp8 else (lambda t: P(self._dev(t)))  # noqa: E731  (bf16 Linear weights: bf16 mode only)
            lw.qkv_w = W(torch.cat([sd[sa + "q.weight"], sd[sa + "k.weight"], sd[sa + "v.weight"]], 0))
            lw.qkv_b = P(self._dev(torch.cat([sd[sa + "q.bias"], sd[sa + "k.bias"], sd[sa + "v.bias"]], 0)))
            lw.norm_q_w, lw.norm_k_w = P(self._dev(sd[sa + "norm_q.weight"])), P(self._dev(sd[sa + "norm_k.weight"]))
            lw.o_w, lw.o_b = W(sd[sa + "o.weight"]), P(self._dev(sd[sa + "o.bias"]))
            lw.cq_w, lw.cq_b = W(sd[ca + "q.weight"]), P(self._dev(sd[ca + "q.bias"]))
            lw.ckv_w = W(torch.cat([sd[ca + "k.weight"], sd[ca + "v.weight"]], 0))
            lw.ckv_b = P(self._dev(torch.cat([sd[ca + "k.bias"], sd[ca + "v.bias"]], 0)))
            lw.cnorm_q_w, lw.cnorm_k_w = P(self._dev(sd[ca + "norm_q.weight"])), P(self._dev(sd[ca + "norm_k.weight"]))
            lw.co_w, lw.co_b = W(sd[ca + "o.weight"]), P(self._dev(sd[ca + "o.bias"]))
            lw.ffn0_w, lw.ffn0_b = W(sd[p + "ffn.0.weight"]), P(self._dev(sd[p + "ffn.0.bias"]))
            lw.ffn2_w, lw.ffn2_b = W(sd[p + "ffn.2.weight"]), P(self._dev(sd[p + "ffn.2.bias"]))
        self._layers = layers
        m.layers_host = C.cast(layers, C.POINTER(_lib.LayerWeights))
        if self.fp8:
            self._layers8 = layers8
            m.layers_fp8_host = C.cast(layers8, C.POINTER(_lib.LayerFp8))
        if s.is_i2v:
            im = _lib.I2VModel()
            im.clip_dim, im.clip_len, im.img_eps = s.clip_dim, s.clip_len, 1e-5   # nn.LayerNorm's default eps (model.py:474-477)
            for dst, src in (("img_ln0", "img_emb.proj.0"), ("img_fc1", "img_emb.proj.1"), ("img_fc2", "img_emb.proj.3"),
                             ("img_ln1", "img_emb.proj.4")):
                setattr(im, dst + "_w", P(self._dev(sd[src + ".weight"])))
                setattr(im, dst + "_b", P(self._dev(sd[src + ".bias"])))
            ilayers = (_lib.I2VLayer * s.num_layers)()
            for i in range(s.num_layers):
                ca = f"blocks.{i}.cross_attn."
                ilayers[i].kvimg_w = P(self._dev(torch.cat([sd[ca + "k_img.weight"], sd[ca + "v_img.weight"]], 0)))
                ilayers[i].kvimg_b = P(self._dev(torch.cat([sd[ca + "k_img.bias"], sd[ca + "v_img.bias"]], 0)))
                ilayers[i].norm_k_img_w = P(self._dev(sd[ca + "norm_k_img.weight"]))
            self._i2v_layers = ilayers
            im.layers_host = C.cast(ilayers, C.POINTER(_lib.I2VLayer))
            self.i2v_cmodel = im
        cos, sin = rope_tables(s.head_dim)
        self.rope_cos = cos.to(self.device)
        self.rope_sin = sin.to(self.device)
        self.sched_sigmas = sigmas.to(device=self.device, dtype=torch.float32).contiguous()
        self.sched_timesteps = timesteps.to(device=self.device, dtype=torch.float32).contiguous()
        m.rope_cos, m.rope_sin = self.rope_cos.data_ptr(), self.rope_sin.data_ptr()
        m.sched_sigmas, m.sched_timesteps = self.sched_sigmas.data_ptr(), self.sched_timesteps.data_ptr()
        m.n_table = self.sched_sigmas.numel()
        self.cmodel = m

    # ---------------------------------------------------------------------------------
    def workspace(self, B: int, F: int, H: int, W: int, G: int) -> Tensor:
        # one workspace per shape AND stream: concurrent rollouts on different HIP streams share the
        # weights but must not share activations
        i2v = C.byref(self.i2v_cmodel) if self.shape.is_i2v else None
        return self._stream_bytes((B, F, H, W, G), lambda: _lib.lib().sf_dit_workspace_bytes(C.byref(self.cmodel), i2v, B, F, H, W, G),
                                  zero_is_error="sf_dit_workspace_bytes" if i2v else None)

    def forward(self, noisy: Tensor, timestep: Tensor, prompt_embeds: Optional[Tensor], init_cross: bool,
                k_cache: List[Tensor], v_cache: List[Tensor], ck_cache: List[Tensor], cv_cache: List[Tensor], plan: CachePlan,
                start_frame: int, evict_scratch: Optional[Tensor] = None, cache_only: bool = False,
                add_condition: Optional[Tensor] = None, kv_index: Optional[Tensor] = None,
                cross_fold: Optional[Tuple[Tensor, Tensor]] = None, clip_feature: Optional[Tensor] = None, y: Optional[Tensor] = None,
                kimg_cache: Optional[List[Tensor]] = None, vimg_cache: Optional[List[Tensor]] = None):
        """noisy [B,F,in_dim,H,W] bf16 (contiguous); timestep [B,G] float32|int64 on device; *_cache: per-layer cache
        tensors (mutated in place); kv_index: the shared int64 [L, 2] buffer behind the cache dicts' index tensors (the
        pass ends by setting every row to (plan.global_end, plan.local_end)), or None.  Returns (flow, x0)
        [B,F,out_dim,H,W], or (None, None) with cache_only.
        cross_fold: the cross-attention caches' (keys, log2w) buffers (int32 / float32 [L, B], torch_ops.cross_fold_scan):
        filled by this call with init_cross, read by every layer's cross-attention; None: all text_len keys are attended.
        i2v model type: noisy carries in_dim - 20 channels; y (bf16 [B or 1, 20, F, H, W], strided) and the per-layer image
        caches are required, clip_feature (bf16 [B, clip_len, clip_dim]) with init_cross: torch.ops.sf_hip.dit_forward_i2v.
        ONE custom-op call: torch.ops.sf_hip.dit_forward -> sf_dit_forward."""
        B, F, Cin, H, W = noisy.shape
        ws = self.workspace(B, F, H, W, timestep.shape[1])
        if self.shape.is_i2v:
            if y is None or kimg_cache is None or vimg_cache is None or (init_cross and clip_feature is None):
                raise ValueError("an i2v model needs clip_feature, y and the image caches")
            flow, x0 = torch.ops.sf_hip.dit_forward_i2v(
                self._handle, noisy, timestep, prompt_embeds, clip_feature if init_cross else None, y, add_condition, k_cache, v_cache,
                ck_cache, cv_cache, kimg_cache, vimg_cache, ws, evict_scratch, bool(init_cross), bool(cache_only), plan.sink, plan.evict,
                plan.keep, plan.write_start, plan.attn_start, plan.local_end, start_frame, kv_index, plan.global_end,
                *(cross_fold or (None, None)))
            return (None, None) if cache_only else (flow, x0)
        flow, x0 = torch.ops.sf_hip.dit_forward(
            self._handle, noisy, timestep, prompt_embeds, add_condition, k_cache, v_cache, ck_cache, cv_cache, ws, evict_scratch,
            bool(init_cross), bool(cache_only), plan.sink, plan.evict, plan.keep, plan.write_start, plan.attn_start, plan.local_end,
            start_frame, kv_index, plan.global_end, *(cross_fold or (None, None)))
        return (None, None) if cache_only else (flow, x0)

    def forward_pair(self, ctx_noisy: Tensor, ctx_timestep: Tensor, noisy: Tensor, timestep: Tensor, k_cache: List[Tensor],
                     v_cache: List[Tensor], ck_cache: List[Tensor], cv_cache: List[Tensor], ctx_plan: CachePlan, plan: CachePlan,
                     ctx_start_frame: int, start_frame: int, evict_scratch: Optional[Tensor] = None, kv_index: Optional[Tensor] = None,
                     cross_fold: Optional[Tuple[Tensor, Tensor]] = None,
                     add_conditions: Tuple[Optional[Tensor], Optional[Tensor]] = (None, None)):
        """The context pass of chunk k (cache only) + the first denoising pass of chunk k + 1 as ONE call
        (torch.ops.sf_hip.dit_forward_pair -> sf_dit_forward with two passes): bit-identical to two `forward` calls, but every
        row-wise kernel and GEMM sees both passes' rows at once.  `add_conditions`: the pose tokens of the context pass and
        of the denoising pass (each pass adds its own).  Returns (flow, x0) of the denoising pass."""
        if self.shape.is_i2v:
            raise NotImplementedError("forward_pair is not built for the i2v model type")
        B, F, Cin, H, W = noisy.shape
        ws = self.workspace(2 * B, F, H, W, timestep.shape[1])
        as_list = lambda pl, sf: [pl.sink, pl.evict, pl.keep, pl.write_start, pl.attn_start, pl.local_end, sf]  # noqa: E731
        return torch.ops.sf_hip.dit_forward_pair(self._handle, ctx_noisy, ctx_timestep, noisy, timestep, k_cache, v_cache, ck_cache, cv_cache,
                                                 ws, evict_scratch, as_list(ctx_plan, ctx_start_frame), as_list(plan, start_frame), kv_index,
                                                 plan.global_end, *(cross_fold or (None, None)), *add_conditions)
