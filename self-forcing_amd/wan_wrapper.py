"""`WanDiffusionWrapper` -- drop-in for the reference's generator wrapper on the KV-cached path.

Mirrors utils/wan_wrapper.py:120-177, 253-349 of the reference: same constructor keywords, same
`forward(noisy_image_or_video, conditional_dict, timestep, kv_cache, crossattn_cache,
current_start, ...) -> (flow_pred, pred_x0)`, same cache-dict schema (the callee mutates the
caller's caches in place), `.scheduler`, `.get_scheduler()`, `.model.local_attn_size`,
`.model.num_frame_per_block`.  Everything behind `forward` runs in the HIP kernels.

Differences from the reference, all deliberate:
  * weights: a local checkpoint directory (`model_path`) with `*.safetensors`, an explicit
    `state_dict=`, or `random_init_seed=`; there is no implicit download and no silent random init;
  * LoRA (`lora_rank`, `lora_alpha`, `lora_targets`, `lora_path`: utils/wan_wrapper.py:146-165): adapters found in the
    state dict (`<linear>.base.weight` + `lora_A/lora_B`, the layout `apply_lora` leaves behind) or loaded from
    `lora_path` (.safetensors / weights-only .pt; lora_A/lora_B or lora_up/lora_down pairs, the reference's prefix
    handling) are MERGED into the base matrices at load time, W += alpha/rank * B @ A -- the same function up to one
    bf16 rounding of the merged matrix, without the 14 % of extra run-time FLOPs; `lora_dropout` is inference-inert;
  * the attention window for `local_attn_size == -1` is the cache capacity and for rolling mode
    `local_attn_size * frame_seqlen` of the CURRENT latent size (the reference hard-codes
    32760 / `local_attn_size * 1560`, causal_model.py:77, which is only right for 60x104 latents);
  * FP8 linear layers (`fp8=True`, keyword-only): the counterpart of the reference's optional
    `quantize_(transformer, Float8DynamicActivationFloat8WeightConfig(granularity=PerTensor()))` (demo.py:277-283) --
    every nn.Linear runs as an e4m3 GEMM with a per-tensor weight scale and a dynamic per-pass activation scale
    (fp8.py); off by default, and with it off nothing changes;
  * the non-cached branches (`kv_cache is None`, classify_mode, clean_x teacher forcing) raise NotImplementedError; the
    fork's pose tokens (`add_condition`) are supported;
  * the i2v model type (`shape.model_type == "i2v"`, e.g. model_name="Wan2.1-I2V-14B"): `clip_feature` [B or 1, 257, clip_dim]
    and `y` [B or 1, 20, F, H, W] (channel-first, THIS call's frames) are required, as arguments or in `conditional_dict`
    (utils/wan_wrapper.py:271-274); the image keys / values live in the cross-attention cache dicts as "k_img" / "v_img" and
    are filled with the text K / V.  The reference's own causal i2v path does not run (its WanI2VCrossAttention takes no
    `crossattn_cache`): the semantics are those of its bidirectional i2v model, DESIGN.md section 16.  A t2v model given
    either tensor raises NotImplementedError; `forward_pair` and `fp8=True` are not built for an i2v model (`forward_pair` does
    take the two passes' pose tokens).
"""
from __future__ import annotations

import glob
import os
import time
from typing import Dict, List, Optional

import torch

from .kvcache import add_image_cache, plan_cache_update, read_indices, shared_index_buffer, shift_positions, write_indices
from .model import CausalWanModel
from .scheduler import FlowMatchScheduler
from .weights import (LORA_DEFAULT_TARGETS, NAMED_SHAPES, WanShape, apply_lora_file, load_lora_file, merge_lora, strip_prefix,
                      synth_state_dict)

Tensor = torch.Tensor


def _load_checkpoint_dir(path: str) -> Dict[str, Tensor]:
    files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(
            f"no *.safetensors under {path!r}. Pass state_dict=..., or random_init_seed=<int> for "
            "seeded random weights (benchmarks / tests).")
    from safetensors.torch import load_file
    sd: Dict[str, Tensor] = {}
    for f in files:
        sd.update(load_file(f))
    return sd


class WanDiffusionWrapper(torch.nn.Module):
    def __init__(self, model_name: str = "Wan2.1-T2V-1.3B", model_path: Optional[str] = None, timestep_shift: float = 8.0,
                 is_causal: bool = False, local_attn_size: int = -1, sink_size: int = 0, lora_rank: Optional[int] = None,
                 lora_alpha: float = 1.0, lora_dropout: float = 0.0, lora_targets: Optional[List[str]] = None,
                 lora_path: Optional[str] = None, *, shape: Optional[WanShape] = None,
                 state_dict: Optional[Dict[str, Tensor]] = None, random_init_seed: Optional[int] = None,
                 device="cuda", fp8: bool = False):
        super().__init__()
        if not is_causal:
            raise NotImplementedError("only the causal (KV-cached) generator is implemented on this path")
        if shape is None:
            if model_name not in NAMED_SHAPES:
                raise ValueError(f"unknown model_name {model_name!r}; pass shape=WanShape(...)")
            shape = NAMED_SHAPES[model_name]
        shape = shape.replace(local_attn_size=local_attn_size, sink_size=sink_size)
        if state_dict is None:
            if random_init_seed is not None:
                state_dict = synth_state_dict(shape, seed=random_init_seed)
            else:
                state_dict = _load_checkpoint_dir(model_path or f"wan_models/{model_name}/")
        state_dict = strip_prefix(state_dict)
        if any(".lora_A." in k for k in state_dict):
            if not lora_rank:
                raise ValueError("state dict holds LoRA adapters but lora_rank was not given")
            state_dict = merge_lora(state_dict, alpha=lora_alpha, rank=lora_rank)
        self.lora_loaded = self.lora_skipped = 0
        if lora_rank is not None and lora_rank > 0 and lora_path is not None:
            # utils/wan_wrapper.py:146-165: adapters on `lora_targets` (default q, k, v, o of both attentions), weights
            # from `lora_path`; folded into the base matrices here (W += alpha / rank * B @ A) instead of evaluated as
            # base(x) + B(A(x)) * alpha / rank on every call (utils/lora.py:47-50)
            state_dict, self.lora_loaded, self.lora_skipped = apply_lora_file(
                state_dict, load_lora_file(lora_path), shape, lora_rank, lora_alpha, lora_targets or LORA_DEFAULT_TARGETS)
            print(f"Loaded LoRA weights: {self.lora_loaded} (skipped {self.lora_skipped}).")

        self.uniform_timestep = not is_causal
        self.scheduler = FlowMatchScheduler(shift=timestep_shift, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.model = CausalWanModel(shape, state_dict, device, self.scheduler.sigmas, self.scheduler.timesteps, fp8=fp8)
        self.seq_len = 32760
        self._evict_scratch: Optional[Tensor] = None
        self._cross_fold: Dict[tuple, tuple] = {}
        self._init_throttle()

    # --- host-side pacing ---------------------------------------------------------------------
    # One forward is 25-50 ms of GPU work and ~2 ms of host work, so the calling thread runs far ahead of the GPU until the
    # stream's launch queue is full -- and then SPINS inside the HIP runtime for room (measured: the thread's CPU time inside
    # sf_dit_forward equals its wall time, one busy core per rollout thread).  With one process per GPU and two rollout
    # threads per process that is 16 spinning cores on an 8-GPU node for nothing.  Instead the wrapper keeps at most
    # `max_inflight_forwards` passes enqueued (per wrapper = per stream) and waits for the oldest one by POLLING its event
    # between 1 ms sleeps (hipEventSynchronize spins too, also on events created with blocking sync: measured 2.5 busy cores
    # per rank with it, against 1.7 unpaced).  Two passes in flight keep >= 25 ms of work queued, so the GPU never waits
    # for the host and a millisecond of polling granularity costs nothing.  0 disables the pacing.
    max_inflight_forwards = 2

    def _init_throttle(self) -> None:
        import collections
        self._inflight = collections.deque()

    def _pace(self, device) -> None:
        n = self.max_inflight_forwards
        if n <= 0 or torch.compiler.is_compiling() or torch.cuda.is_current_stream_capturing():
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._inflight.append(ev)
        while len(self._inflight) > n:
            oldest = self._inflight.popleft()
            while not oldest.query():
                time.sleep(0.001)

    def share(self) -> "WanDiffusionWrapper":
        """A second wrapper over the SAME device weights (own pointer tables / scratch), for a second
        rollout running concurrently on another HIP stream."""
        other = WanDiffusionWrapper.__new__(WanDiffusionWrapper)
        torch.nn.Module.__init__(other)
        other.uniform_timestep = self.uniform_timestep
        other.scheduler = self.scheduler
        other.model = self.model
        other.seq_len = self.seq_len
        other._evict_scratch = None
        other._cross_fold = {}
        other._init_throttle()
        return other

    @property
    def fp8(self) -> bool:
        """True when the generator's Linears run in FP8 (constructed with fp8=True)."""
        return self.model.fp8

    # --- reference API ------------------------------------------------------------------------
    def get_scheduler(self):
        return self.scheduler

    def post_init(self):
        self.get_scheduler()

    def enable_gradient_checkpointing(self):
        raise NotImplementedError("inference-only path")

    # --- cache plumbing -----------------------------------------------------------------------
    _write_indices = staticmethod(write_indices)   # (kv_cache, global_end, local_end): set a cache's position by hand

    def _latents(self, x: Tensor) -> Tensor:
        return x.to(device=self.model.device, dtype=torch.bfloat16).contiguous()

    def _timestep(self, t: Tensor) -> Tensor:
        """[B] or [B, G] -> [B, G] on the device, int64 kept, anything else float32."""
        t = t.to(self.model.device)
        if t.dim() == 1:
            t = t.unsqueeze(1)
        return (t if t.dtype == torch.int64 else t.to(torch.float32)).contiguous()

    def _eviction_scratch(self, batch: int, keep: int, cap: int) -> Tensor:
        """Where sf_kv_evict parks the `keep` tokens it moves; sized once for the whole cache."""
        dim = self.model.shape.dim
        if self._evict_scratch is None or self._evict_scratch.numel() < batch * keep * dim * 2:
            self._evict_scratch = torch.empty(batch * cap * dim * 2, dtype=torch.uint8, device=self.model.device)
        return self._evict_scratch

    @torch.no_grad()
    def rebase_positions(self, kv_cache: List[dict], delta_frames: int, frame_seqlen: int) -> None:
        """Move the cache `delta_frames` back in the timeline, between two calls: every layer's cached keys (rows
        [0, local_end), sink rows included: their distance to the rest is kept, their new position is negative and never
        looked up) are rotated back by `delta_frames` (sf_kv_rope_shift), then `global_end_index` drops by
        delta_frames * frame_seqlen.  The caller passes `current_start` values `delta_frames` frames lower from here on."""
        mdl = self.model
        _, local_end = read_indices(kv_cache)
        for kv in kv_cache:
            torch.ops.sf_hip.kv_rope_shift(kv["k"], mdl.rope_cos, mdl.rope_sin, delta_frames, 0, local_end)
        shift_positions(kv_cache, delta_frames * frame_seqlen)

    # --- cross-attention: a prompt's padding keys folded into one ---------------------------------
    # The rows of `prompt_embeds` behind the prompt's tokens are zero (utils/wan_wrapper.py:50-51) and everything from
    # there to the cross-attention K / V caches is row-wise, so a cache's padded rows are identical: one of them, with
    # log2(their number) added to its score, gives the same softmax as all of them, and the kernel walks 1-4 key tiles
    # instead of 8.  The counts are taken from the caches themselves on the device (torch_ops.cross_fold_scan) and live
    # in two small buffers that belong to the caches' tensors: a cache dict keeps the reference's schema.  False: attend
    # every key, as the reference does.
    fold_cross_padding = True

    def _cross_fold_buffers(self, crossattn_cache: List[dict], init_cross: bool):
        """(keys, log2w) of these cache tensors, or None with folding off.  The pass that fills the caches (init_cross) also
        fills the buffers; caches this wrapper has not seen filled -- adopted from elsewhere with is_init set, or rebound to
        other tensors -- are scanned here once.  (A caller that rewrites an initialised cache IN PLACE must clear is_init or
        rebind the tensors: nothing on the host can see that.)"""
        if not self.fold_cross_padding:
            return None
        ck, cv = [c["k"] for c in crossattn_cache], [c["v"] for c in crossattn_cache]
        key = tuple(t.data_ptr() for t in ck) + tuple(t.data_ptr() for t in cv) + tuple(ck[0].shape) \
            + (torch.cuda.current_stream(ck[0].device).cuda_stream,)
        hit = self._cross_fold.get(key)
        if hit is None:
            if len(self._cross_fold) > 16:
                self._cross_fold.clear()
            B = ck[0].shape[0]
            hit = (torch.empty(len(ck), B, dtype=torch.int32, device=ck[0].device),
                   torch.empty(len(ck), B, dtype=torch.float32, device=ck[0].device))
            self._cross_fold[key] = hit
            if not init_cross:
                torch.ops.sf_hip.cross_fold_scan(ck, cv, hit[0], hit[1])
        return hit

    # --- two passes in one call ------------------------------------------------------------------
    def can_pair(self, conditional_dict: dict) -> bool:
        """`forward_pair` covers the text-conditioned rollout, with or without pose tokens (which it takes per pass, as
        `add_conditions=`, never from `conditional_dict`); not the image conditioning of the i2v model type."""
        return conditional_dict.get("clip_feature") is None and conditional_dict.get("y") is None and not self.model.shape.is_i2v

    def _pose_condition(self, add_condition: Tensor, B: int, n_new: int) -> Tensor:
        """pose tokens [B, L_pose, 5120]: x += pose_proj(add_condition), the intent of causal_model.py:786-819 (that branch
        raises in the reference snapshot: parity pinned by the oracle only)"""
        mdl = self.model
        if not mdl.accepts_pose:   # (dim == 5120 models need none: their pose_proj is nn.Identity(), :500-501)
            raise ValueError(f"add_condition needs pose_proj weights in the state dict of a dim-{mdl.shape.dim} model")
        add_condition = add_condition.to(device=mdl.device, dtype=torch.bfloat16).contiguous()
        if add_condition.dim() != 3 or add_condition.shape[0] != B or add_condition.shape[1] != n_new:
            raise ValueError(f"add_condition spatial dim {add_condition.shape[1]} doesn't match "
                             f"x spatial dim {n_new}. Check pose data processing.")
        assert add_condition.shape[2] == mdl.cmodel.pose_dim, "add_condition channel width must match pose_proj"
        return add_condition

    @torch.no_grad()
    def forward_pair(self, context_input: Tensor, context_timestep: Tensor, noisy_image_or_video: Tensor, timestep: Tensor,
                     conditional_dict: dict, kv_cache: List[dict], crossattn_cache: List[dict], context_start: int, current_start: int,
                     add_conditions: Optional[tuple] = None):
        """Extension (no counterpart call in the reference, which runs these back to back, causal_inference.py:226-235 then
        :190-205 of the next chunk): the context pass of one chunk -- `context_input` = its denoised latents at
        `context_timestep`, cache positions from `context_start`, only the KV cache is updated -- and the FIRST denoising
        pass of the next chunk (`noisy_image_or_video`, `timestep`, `current_start`) as one call.  Same results bit for
        bit as `forward(..., cache_only=True)` followed by `forward(...)`; returns (flow_pred, pred_x0) of the second.
        `add_conditions`: the two passes' pose tokens (context pass, denoising pass), each as `forward`'s `add_condition`.
        The passes belong to different chunks, so one `conditional_dict["add_condition"]` cannot serve both: a dict that
        carries one without `add_conditions` is refused rather than run without the tokens."""
        mdl = self.model
        shape = mdl.shape
        if shape.is_i2v:
            raise NotImplementedError("forward_pair is not built for the i2v model type: run the two passes with forward()")
        if add_conditions is None and conditional_dict.get("add_condition") is not None:
            raise ValueError("forward_pair: conditional_dict carries add_condition but the two passes belong to different chunks: pass "
                             "add_conditions=(context pass tokens, denoising pass tokens), or run the passes with forward()")
        xs = []
        for x in (context_input, noisy_image_or_video):
            assert x.dim() == 5 and x.shape[2] == shape.in_dim, "inputs must be [B, F, C, H, W] latents"
            xs.append(self._latents(x))
        assert xs[0].shape == xs[1].shape, "forward_pair: both passes must have the same number of frames"
        B, F, _, H, W = xs[1].shape
        ts = [self._timestep(context_timestep), self._timestep(timestep)]
        assert ts[0].shape == ts[1].shape and ts[0].dtype == ts[1].dtype and ts[0].shape[0] == B, "forward_pair: timesteps must match in shape and dtype"
        assert len(kv_cache) == mdl.num_layers and len(crossattn_cache) == mdl.num_layers
        assert crossattn_cache[0]["is_init"], "forward_pair: the cross-attention cache is filled by the chunk's earlier passes"
        fs = (H // 2) * (W // 2)
        n_new = F * fs
        cap = kv_cache[0]["k"].shape[1]
        window = cap if mdl.local_attn_size == -1 else mdl.local_attn_size * fs
        global_end, local_end = read_indices(kv_cache)
        plan0 = plan_cache_update(local_end, global_end, context_start, n_new, cap, mdl.local_attn_size, mdl.sink_size * fs, window)
        plan1 = plan_cache_update(plan0.local_end, plan0.global_end, current_start, n_new, cap, mdl.local_attn_size, mdl.sink_size * fs, window)
        scratch = self._eviction_scratch(B, max(plan0.keep, plan1.keep), cap) if plan0.evict > 0 or plan1.evict > 0 else None
        index_buf = shared_index_buffer(kv_cache)
        poses = (None, None)
        if add_conditions is not None:
            assert len(add_conditions) == 2 and all(a is not None for a in add_conditions), \
                "forward_pair: add_conditions is (context pass tokens, denoising pass tokens)"
            poses = tuple(self._pose_condition(a, B, n_new) for a in add_conditions)
        flow, x0 = mdl.forward_pair(xs[0], ts[0], xs[1], ts[1], [kv["k"] for kv in kv_cache], [kv["v"] for kv in kv_cache],
                                    [c["k"] for c in crossattn_cache], [c["v"] for c in crossattn_cache], plan0, plan1,
                                    context_start // fs, current_start // fs, scratch, kv_index=index_buf,
                                    cross_fold=self._cross_fold_buffers(crossattn_cache, False), add_conditions=poses)
        write_indices(kv_cache, plan1.global_end, plan1.local_end, done_by_kernel=index_buf is not None)
        self._pace(mdl.device)
        return flow, x0

    # --- the hot call --------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, noisy_image_or_video: Tensor, conditional_dict: dict, timestep: Tensor,
                kv_cache: Optional[List[dict]] = None, crossattn_cache: Optional[List[dict]] = None,
                current_start: Optional[int] = None, classify_mode: Optional[bool] = False,
                concat_time_embeddings: Optional[bool] = False, clean_x: Optional[Tensor] = None,
                aug_t: Optional[Tensor] = None, cache_start: Optional[int] = None,
                add_condition: Optional[Tensor] = None, clip_feature: Optional[Tensor] = None, y: Optional[Tensor] = None,
                cache_only: bool = False):
        """`cache_only=True` (extension): the caller only wants the KV-cache update (context pass,
        initial-latent warm-up) and gets (None, None) back; see sf_forward_args.cache_only."""
        if kv_cache is None or crossattn_cache is None:
            raise NotImplementedError("only the KV-cached inference branch is implemented (kv_cache / crossattn_cache required)")
        if classify_mode or clean_x is not None or aug_t is not None:
            raise NotImplementedError("training-only branches (classify_mode / teacher forcing) are out of scope")
        if add_condition is None:
            add_condition = conditional_dict.get("add_condition")
        if clip_feature is None:
            clip_feature = conditional_dict.get("clip_feature")
        if y is None:
            y = conditional_dict.get("y")
        mdl = self.model
        shape = mdl.shape
        if not shape.is_i2v and (clip_feature is not None or y is not None):
            raise NotImplementedError("image conditioning (clip_feature, y) needs a generator of the i2v model type; this one is "
                                      f"{shape.model_type} (CausalDiffusionInferencePipeline.encode_image produces the two tensors)")
        x = noisy_image_or_video
        assert x.dim() == 5, "noisy_image_or_video must be [B, F, C, H, W]"
        B, F, Cin, H, W = x.shape
        if shape.is_i2v:
            # causal_model.py:767-768: `assert clip_fea is not None and y is not None`
            assert clip_feature is not None and y is not None, "an i2v generator needs clip_feature and y (arguments or conditional_dict)"
            assert y.dim() == 5 and Cin + y.shape[1] == shape.in_dim, \
                f"latent channels {Cin} + y channels {tuple(y.shape)[1:2]} must be in_dim = {shape.in_dim} (y is [B or 1, 20, F, H, W])"
            assert y.shape[0] in (1, B) and tuple(y.shape[2:]) == (F, H, W), \
                f"y must cover this call's frames: [{B} or 1, {y.shape[1]}, {F}, {H}, {W}], got {tuple(y.shape)}"
            assert clip_feature.dim() == 3 and clip_feature.shape[0] in (1, B) and tuple(clip_feature.shape[1:]) == (shape.clip_len, shape.clip_dim), \
                f"clip_feature must be [{B} or 1, {shape.clip_len}, {shape.clip_dim}], got {tuple(clip_feature.shape)}"
        else:
            assert Cin == shape.in_dim, f"expected {shape.in_dim} latent channels, got {Cin}"
        assert len(kv_cache) == mdl.num_layers and len(crossattn_cache) == mdl.num_layers, \
            "cache lists must have one entry per transformer block"
        if current_start is None:
            current_start = 0
        x = self._latents(x)
        t = self._timestep(timestep)
        assert t.shape[0] == B, "timestep must be [B, groups]"

        fs = (H // 2) * (W // 2)
        n_new = F * fs
        cap = kv_cache[0]["k"].shape[1]
        k0 = kv_cache[0]["k"]
        assert tuple(k0.shape) == (B, cap, shape.num_heads, shape.head_dim) and k0.dtype == torch.bfloat16 and k0.is_contiguous(), \
            f"kv cache must be contiguous bf16 [B, S, {shape.num_heads}, {shape.head_dim}], got {tuple(k0.shape)} {k0.dtype}"
        c0 = crossattn_cache[0]["k"]
        assert tuple(c0.shape) == (B, shape.text_len, shape.num_heads, shape.head_dim) and c0.is_contiguous(), \
            f"cross-attention cache must be [B, {shape.text_len}, {shape.num_heads}, {shape.head_dim}]"

        global_end, local_end = read_indices(kv_cache)
        window = cap if mdl.local_attn_size == -1 else mdl.local_attn_size * fs
        plan = plan_cache_update(local_end, global_end, current_start, n_new, cap, mdl.local_attn_size,
                                 mdl.sink_size * fs, window)
        scratch = self._eviction_scratch(B, plan.keep, cap) if plan.evict > 0 else None

        init_cross = not crossattn_cache[0]["is_init"]
        pe = None
        if init_cross:
            pe = conditional_dict["prompt_embeds"].to(device=mdl.device, dtype=torch.bfloat16)
            assert pe.dim() == 3 and pe.shape[0] == B and pe.shape[2] == shape.text_dim and pe.shape[1] <= shape.text_len, \
                f"prompt_embeds must be [B, <= {shape.text_len}, {shape.text_dim}], got {tuple(pe.shape)}"
            if pe.shape[1] < shape.text_len:  # zero-pad to text_len (causal_model.py:838-842)
                pe = torch.cat([pe, pe.new_zeros(B, shape.text_len - pe.shape[1], shape.text_dim)], dim=1)
            pe = pe.contiguous()

        if add_condition is not None:
            add_condition = self._pose_condition(add_condition, B, n_new)
        i2v = {}
        if shape.is_i2v:
            add_image_cache(crossattn_cache, shape, torch.bfloat16, mdl.device)   # (a cache built elsewhere lacks "k_img" / "v_img")
            y = y.to(device=mdl.device, dtype=torch.bfloat16)
            if y.stride(4) != 1 or y.stride(3) != W:    # a frame slice of the clip's y keeps contiguous planes: no copy
                y = y.contiguous()
            i2v = dict(y=y, kimg_cache=[c["k_img"] for c in crossattn_cache], vimg_cache=[c["v_img"] for c in crossattn_cache])
            if init_cross:   # one image for the whole batch is expanded here, once per prompt
                i2v["clip_feature"] = clip_feature.to(device=mdl.device, dtype=torch.bfloat16).expand(B, -1, -1).contiguous()
        index_buf = shared_index_buffer(kv_cache)
        flow, x0 = mdl.forward(x, t, pe, init_cross, [kv["k"] for kv in kv_cache], [kv["v"] for kv in kv_cache],
                               [c["k"] for c in crossattn_cache], [c["v"] for c in crossattn_cache], plan,
                               current_start // fs, scratch, cache_only=cache_only, add_condition=add_condition,
                               kv_index=index_buf, cross_fold=self._cross_fold_buffers(crossattn_cache, init_cross), **i2v)
        if init_cross:
            for c in crossattn_cache:
                c["is_init"] = True
        write_indices(kv_cache, plan.global_end, plan.local_end, done_by_kernel=index_buf is not None)
        self._pace(mdl.device)
        return flow, x0
