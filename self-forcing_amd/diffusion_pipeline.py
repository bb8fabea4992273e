"""`CausalDiffusionInferencePipeline` -- drop-in for pipeline/causal_diffusion_inference.py of the reference: the
many-step (50 by default) classifier-free-guidance sampler over the same causal generator.

Same constructor `(args, device, generator=None, text_encoder=None, vae=None, image_encoder=None)` and the same
`inference(noise, text_prompts, input_image, dwpose_data, random_ref_dwpose, initial_latent=None,
return_latents=False, start_frame_index=0)`; same attributes (`kv_cache_pos/neg`, `crossattn_cache_pos/neg`,
`sampling_steps`, `sample_solver`, `shift`, `num_frame_per_block`, ...) and cache-dict schema.

Per chunk (causal_diffusion_inference.py:370-457): a fresh FlowUniPCMultistepScheduler, then per step the generator
under the prompt and under the negative prompt (two KV / cross-attention cache sets), the guidance blend and one
scheduler step; finally a timestep-0 pass that rewrites the chunk's K/V in both caches.

What differs:
  * the two generator calls of a step are independent, so with `overlap_cfg=True` (default when the generator can
    `share()` its weights) the negative-prompt pass runs on a second HIP stream beside the prompt pass;
  * the blend and the scheduler's tensor arithmetic are `sf_lincomb_bf16` launches with host-evaluated scalars
    (`unipc.py`); timesteps come from the scheduler's host table, so the loop never waits on the device;
  * the constants the reference hard-codes (30 blocks, 1560 tokens per frame, 12x128 heads, 32760-token caches,
    :69-72, :464-487) are derived from the generator's shape and the latent size;
  * image conditioning (:318-357): `encode_image` (:151-172) runs the CLIP image encoder (`clip.CLIPModel`,
    csrc/clip_encoder.hip; injected as `image_encoder=` or loaded lazily from `args.clip_checkpoint_path`) and the VAE
    encoder and returns `clip_feature` and `y`; a generator of the i2v model type consumes them (`img_emb`, `k_img` /
    `v_img`, the 36-channel patch embedding).  `inference(input_image=...)` encodes the image once per clip over the
    whole output timeline, 4 (num_output_frames - 1) + 1 pixel frames, puts `clip_feature` into both condition dicts and
    hands every pass the frames of `y` at its position in `output` -- the reference hands the whole-clip `y` to every
    chunk (:355-357), which its `torch.cat([u, v])` (causal_model.py:772) only survives when a chunk is the whole clip.  An
    i2v generator needs an image; any other generator given one raises NotImplementedError (it has no i2v branch);
  * the pose front end runs on the GPU path (`pose.PoseEmbedder`, csrc/pose_conv.hip): `dwpose_data` [3, F, H, W] with
    `random_ref_dwpose` [H, W, 3] are embedded once per clip with weights loaded lazily from `args.pose_weights_path`
    (`args.pose_weights_strict`, :329-331) or by an injected `pose_embedder=`; the tokens come out token-major, so a
    chunk's `add_condition` is a row range of them (a view; one clip is shared by every sample of the batch).  With
    only one of the two inputs the pose branch is not taken, as in the reference (:336).  The reference-pose map is
    only ever added to `y` (:346-347): it is computed (`embed_ref`) when there is an image, and broadcast over time.
    Already-embedded tokens can still be passed as `dwpose_data_emb` [B, C_pose, F_total, h, w], sliced per chunk
    exactly as :386-394 does;
  * the 'dpm++' solver branch (:526-536) is not implemented; the per-step `print`s are dropped.
"""
from __future__ import annotations

import logging
from typing import List, Optional

import torch

from . import ops
from .kvcache import new_crossattn_cache, new_kv_cache, reset_kv_indices
from .unipc import FlowUniPCMultistepScheduler
from .wan_wrapper import WanDiffusionWrapper

log = logging.getLogger(__name__)


class CausalDiffusionInferencePipeline(torch.nn.Module):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, image_encoder=None,
                 overlap_cfg: Optional[bool] = None, pose_embedder=None):
        super().__init__()
        self.device = torch.device(device)
        self.generator = WanDiffusionWrapper(**getattr(args, "model_kwargs", {}), is_causal=True, device=device) \
            if generator is None else generator
        # as the reference (causal_inference.py:19-23): build the default components when none is injected; they load
        # the reference's default checkpoints (weights-only) and raise FileNotFoundError when those are absent
        if text_encoder is None:
            from .text_encoder import WanTextEncoder
            text_encoder = WanTextEncoder(device=device)
        if vae is None:
            from .vae import WanVAEWrapper
            vae = WanVAEWrapper(device=device)
        self.text_encoder = text_encoder
        self.vae = vae
        # used by encode_image; when none is injected it loads lazily from args.clip_checkpoint_path on first need
        self.image_encoder = image_encoder
        self.clip_checkpoint_path = getattr(args, "clip_checkpoint_path", None)
        # pose weights load lazily on the first inference that takes the pose branch (:59-61, :329-331)
        self.pose_embedder = pose_embedder
        self.pose_weights_path = getattr(args, "pose_weights_path", None)
        self.pose_weights_strict = getattr(args, "pose_weights_strict", True)
        self.pose_weights_loaded = pose_embedder is not None

        self.num_train_timesteps = args.num_train_timestep
        self.sampling_steps = 50
        self.sample_solver = "unipc"
        self.shift = args.timestep_shift

        self.num_transformer_blocks = self.generator.model.num_layers
        self.frame_seq_length = 1560  # refined from the latent size at inference()
        self.kv_cache_pos = None
        self.kv_cache_neg = None
        self.crossattn_cache_pos = None
        self.crossattn_cache_neg = None
        self.args = args
        self.torch_dtype = torch.bfloat16
        self.num_frame_per_block = getattr(args, "num_frame_per_block", 1)
        self.independent_first_frame = args.independent_first_frame
        self.local_attn_size = self.generator.model.local_attn_size
        if self.num_frame_per_block > 1:
            self.generator.model.num_frame_per_block = self.num_frame_per_block

        # the negative-prompt pass on a second stream needs its own activation workspace over the same weights
        can_share = hasattr(self.generator, "share")
        self.overlap_cfg = can_share if overlap_cfg is None else bool(overlap_cfg)
        if self.overlap_cfg and not can_share:
            raise ValueError("overlap_cfg=True needs a generator with share() (self_forcing_amd.WanDiffusionWrapper)")
        self._generator_neg = self.generator.share() if self.overlap_cfg else self.generator
        self._side_stream = None
        import inspect
        try:
            self._cache_only_kw = {"cache_only": True} if "cache_only" in inspect.signature(self.generator.forward).parameters else {}
        except (TypeError, ValueError):
            self._cache_only_kw = {}
        self._cache_key = None
        self.timesteps = None

    # ------------------------------------------------------------------------------------------
    def _initialize_sample_scheduler(self, noise):
        """:517-540."""
        if self.sample_solver != "unipc":
            raise NotImplementedError("Unsupported solver." if self.sample_solver != "dpm++"
                                      else "the 'dpm++' branch of the reference is not implemented; use 'unipc'")
        sample_scheduler = FlowUniPCMultistepScheduler(num_train_timesteps=self.num_train_timesteps, shift=1,
                                                       use_dynamic_shifting=False)
        sample_scheduler.set_timesteps(self.sampling_steps, device=None, shift=self.shift)
        self.timesteps = sample_scheduler.timesteps
        return sample_scheduler

    def _cache_tokens(self, total_frames: int) -> int:
        if self.local_attn_size != -1:
            return self.local_attn_size * self.frame_seq_length
        return max(21, total_frames) * self.frame_seq_length

    def _initialize_kv_cache(self, batch_size, dtype, device, cache_tokens: Optional[int] = None):
        shape = self.generator.model.shape
        if cache_tokens is None:
            cache_tokens = self._cache_tokens(0)
        self.kv_cache_pos = new_kv_cache(shape, self.num_transformer_blocks, batch_size, cache_tokens, dtype, device)
        self.kv_cache_neg = new_kv_cache(shape, self.num_transformer_blocks, batch_size, cache_tokens, dtype, device)

    def _initialize_crossattn_cache(self, batch_size, dtype, device):
        shape = self.generator.model.shape
        self.crossattn_cache_pos = new_crossattn_cache(shape, self.num_transformer_blocks, batch_size, dtype, device)
        self.crossattn_cache_neg = new_crossattn_cache(shape, self.num_transformer_blocks, batch_size, dtype, device)

    # ------------------------------------------------------------------------------------------
    def _both(self, x, cond_dict, uncond_dict, timestep, current_start, cache_only: bool):
        """The generator under both conditions on the same input; returns (flow_cond, flow_uncond)."""
        kw = dict(noisy_image_or_video=x, timestep=timestep, current_start=current_start, cache_start=None)
        if cache_only:
            kw.update(self._cache_only_kw)
        if not self.overlap_cfg:
            fc, _ = self.generator(conditional_dict=cond_dict, kv_cache=self.kv_cache_pos,
                                   crossattn_cache=self.crossattn_cache_pos, **kw)
            fu, _ = self.generator(conditional_dict=uncond_dict, kv_cache=self.kv_cache_neg,
                                   crossattn_cache=self.crossattn_cache_neg, **kw)
            return fc, fu
        main = torch.cuda.current_stream(x.device)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=x.device)
        side = self._side_stream
        side.wait_stream(main)                       # x and the timestep tensor are produced on `main`
        fc, _ = self.generator(conditional_dict=cond_dict, kv_cache=self.kv_cache_pos,
                               crossattn_cache=self.crossattn_cache_pos, **kw)
        with torch.cuda.stream(side):
            fu, _ = self._generator_neg(conditional_dict=uncond_dict, kv_cache=self.kv_cache_neg,
                                        crossattn_cache=self.crossattn_cache_neg, **kw)
            if fu is not None:
                fu.record_stream(main)
        x.record_stream(side)
        timestep.record_stream(side)
        main.wait_stream(side)
        return fc, fu

    def _pose_embedder(self):
        """The injected pose embedder, or the one loaded from args.pose_weights_path on first need (:59-61, :329-331)."""
        if self.pose_embedder is None:
            if self.pose_weights_path is None:
                raise ValueError("dwpose_data needs pose weights: set args.pose_weights_path or construct the pipeline with pose_embedder=")
            from .pose import PoseEmbedder
            self.pose_embedder = PoseEmbedder(self.pose_weights_path, device=self.device, strict=self.pose_weights_strict)
            self.pose_weights_loaded = True
        return self.pose_embedder

    def _pose_tokens(self, dwpose_data: torch.Tensor):
        """`dwpose_embedding` over the clip (:337-340) as (tokens [1, F'*h*w, 5120], (F', h, w)); the weights load once."""
        return self._pose_embedder().embed(dwpose_data)

    def _image_encoder(self):
        if self.image_encoder is None:
            if self.clip_checkpoint_path is None:
                raise ValueError("encode_image needs the CLIP image encoder: set args.clip_checkpoint_path or construct the pipeline "
                                 "with image_encoder=")
            from .clip import CLIPModel
            self.image_encoder = CLIPModel(dtype=self.torch_dtype, device=self.device, checkpoint_path=self.clip_checkpoint_path)
        return self.image_encoder

    def encode_image(self, image, num_frames: int, height: int, width: int) -> dict:
        """The conditioning of the i2v model type (:151-172): {"clip_feature": bf16 [1, L, dim], "y": bf16
        [1, 20, (num_frames - 1)//4 + 1, height/8, width/8]}.

        `image`: a tensor [1, 3, height, width] or [3, height, width] in [-1, 1], or a PIL image (resized to width x
        height and scaled by 2/255 - 1, as :147-148 and :158 do).  `clip_feature` is `image_encoder.visual` of the image as
        a one-frame video -- `visual` takes a list of [3, T, H, W] tensors (clip.py:527-536); the reference passes its
        [1, 3, H, W] tensor, which that contract reads as a 3-frame single-channel video and which fails in the patch
        embedding.  `y` = 4 mask channels (first pixel frame known, repeated 4 times so that the mask folds to the latent
        timeline, :160-164 with the stray fourth view dimension of :163 dropped) on top of the 16 latent channels of
        `vae.encode_to_latent` of the clip "image, then zeros" (:166-167)."""
        if num_frames < 1 or (num_frames - 1) % 4:
            raise ValueError(f"num_frames must be 4 k + 1 (the VAE's timeline), got {num_frames}")
        if height % 8 or width % 8:
            raise ValueError(f"height and width must be multiples of 8, got {height}x{width}")
        encoder = self._image_encoder()
        if not torch.is_tensor(image):
            import numpy as np
            image = torch.from_numpy(np.array(image.resize((width, height)), dtype=np.float32) * (2 / 255) - 1).permute(2, 0, 1)
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        if tuple(image.shape) != (3, height, width):
            raise ValueError(f"image must be [1, 3, {height}, {width}] or [3, {height}, {width}], got {tuple(image.shape)}")
        image = image.to(self.device, torch.float32)
        clip_feature = encoder.visual([image.unsqueeze(1)]).to(self.torch_dtype)
        lat_t, h, w = (num_frames - 1) // 4 + 1, height // 8, width // 8
        msk = torch.zeros(4, lat_t, h, w, device=self.device)
        msk[:, 0] = 1
        clip = torch.zeros(1, 3, num_frames, height, width, device=self.device, dtype=self.torch_dtype)
        clip[0, :, 0] = image.to(self.torch_dtype)
        latent = self.vae.encode_to_latent(clip)[0].transpose(0, 1)                 # [16, lat_t, h, w]
        y = torch.cat([msk, latent.float()]).unsqueeze(0).to(self.torch_dtype)
        return {"clip_feature": clip_feature, "y": y}

    def inference(self, noise: torch.Tensor, text_prompts: List[str], input_image=None, dwpose_data=None,
                  random_ref_dwpose=None, initial_latent: Optional[torch.Tensor] = None, return_latents: bool = False,
                  start_frame_index: Optional[int] = 0, dwpose_data_emb: Optional[torch.Tensor] = None):
        """noise [B, F, C, H, W] -> video in [0, 1] (and the latents)."""
        is_i2v = getattr(getattr(getattr(self, "generator", None), "model", None), "model_type", "t2v") == "i2v"
        if input_image is not None and not is_i2v:
            raise NotImplementedError("input_image: this generator has no i2v branch (img_emb, k_img / v_img, the 36-channel patch "
                                      "embedding: model_type 'i2v'), so the rollout cannot consume an image; encode_image() still "
                                      "produces its clip_feature and y")
        if is_i2v and input_image is None:
            raise ValueError("an i2v generator needs input_image: every pass takes its clip_feature and y")
        batch_size, num_frames, num_channels, height, width = noise.shape
        if not self.independent_first_frame or (self.independent_first_frame and initial_latent is not None):
            assert num_frames % self.num_frame_per_block == 0
            num_blocks = num_frames // self.num_frame_per_block
        else:
            assert (num_frames - 1) % self.num_frame_per_block == 0
            num_blocks = (num_frames - 1) // self.num_frame_per_block
        num_input_frames = initial_latent.shape[1] if initial_latent is not None else 0
        num_output_frames = num_frames + num_input_frames
        self.frame_seq_length = (height // 2) * (width // 2)
        use_pose = dwpose_data is not None and random_ref_dwpose is not None      # both, as the reference (:336)
        if use_pose:
            if dwpose_data_emb is not None:
                raise ValueError("pass either dwpose_data (with random_ref_dwpose) or dwpose_data_emb, not both")
            if dwpose_data.dim() != 4 or dwpose_data.shape[0] != 3:
                raise ValueError(f"dwpose_data must be one clip [3, F, H, W] (shared by the batch), got {tuple(dwpose_data.shape)}")
            # the pose tokens must cover the whole output timeline (:362-369); known from the shapes, before any work
            from .pose_weights import pose_plan
            pose_fhw = pose_plan(*dwpose_data.shape[1:])
            expected_pose_frames = (start_frame_index or 0) + num_output_frames
            assert pose_fhw[0] == expected_pose_frames, (
                f"dwpose_data_emb has {pose_fhw[0]} frames, "
                f"but expected {expected_pose_frames} to match the output timeline.")
            if pose_fhw[1] * pose_fhw[2] != self.frame_seq_length:
                raise ValueError(f"dwpose_data gives {pose_fhw[1]}x{pose_fhw[2]} pose tokens per frame, the latents {height // 2}x{width // 2}. "
                                 "Check pose data processing.")
        elif dwpose_data is not None or random_ref_dwpose is not None:
            log.warning("only one of dwpose_data / random_ref_dwpose was given: the pose branch needs both and is not taken")
        conditional_dict = dict(self.text_encoder(text_prompts=text_prompts))
        unconditional_dict = dict(self.text_encoder(text_prompts=[self.args.negative_prompt] * len(text_prompts)))

        y_clip = None
        if is_i2v:
            # once per clip, over the OUTPUT timeline (context frames included): a pass reads y at its position in `output`
            image_emb = self.encode_image(input_image, 4 * (num_output_frames - 1) + 1, height * 8, width * 8)
            y_clip = image_emb["y"]
            assert y_clip.shape[2] >= num_output_frames, (
                f"y has {y_clip.shape[2]} latent frames, but the output timeline has {num_output_frames}.")
            if use_pose:   # the image to be driven by the pose (:341-347); [1, 20, 1, h, w] broadcast over time
                y_clip = y_clip + self._pose_embedder().embed_ref(random_ref_dwpose).to(y_clip.dtype)
            for d in (conditional_dict, unconditional_dict):   # (:352-353) one image: the wrapper expands it to the batch
                d["clip_feature"] = image_emb["clip_feature"]

        def set_y(first_frame: int, n: int) -> None:
            if y_clip is not None:
                conditional_dict["y"] = unconditional_dict["y"] = y_clip[:, :, first_frame:first_frame + n]

        output = torch.zeros([batch_size, num_output_frames, num_channels, height, width], device=noise.device, dtype=noise.dtype)

        # Step 1: caches (:203-231)
        key = (batch_size, self._cache_tokens(num_output_frames), noise.device)
        if self.kv_cache_pos is None or self._cache_key != key:
            self._initialize_kv_cache(batch_size, noise.dtype, noise.device, cache_tokens=key[1])
            self._initialize_crossattn_cache(batch_size, noise.dtype, noise.device)
            self._cache_key = key
        else:
            for block_index in range(self.num_transformer_blocks):
                self.crossattn_cache_pos[block_index]["is_init"] = False
                self.crossattn_cache_neg[block_index]["is_init"] = False
            reset_kv_indices(self.kv_cache_pos)
            reset_kv_indices(self.kv_cache_neg)

        # Step 2: context frames into both caches (:233-297)
        fs = self.frame_seq_length
        current_start_frame = start_frame_index
        cache_start_frame = 0
        if initial_latent is not None:
            timestep = torch.zeros([batch_size, 1], device=noise.device, dtype=torch.int64)
            if self.independent_first_frame:
                assert (num_input_frames - 1) % self.num_frame_per_block == 0
                num_input_blocks = (num_input_frames - 1) // self.num_frame_per_block
                output[:, :1] = initial_latent[:, :1]
                set_y(cache_start_frame, 1)
                self._both(initial_latent[:, :1], conditional_dict, unconditional_dict, timestep,
                           current_start_frame * fs, cache_only=True)
                current_start_frame += 1
                cache_start_frame += 1
            else:
                assert num_input_frames % self.num_frame_per_block == 0
                num_input_blocks = num_input_frames // self.num_frame_per_block
            for _ in range(num_input_blocks):
                ref = initial_latent[:, cache_start_frame:cache_start_frame + self.num_frame_per_block]
                output[:, cache_start_frame:cache_start_frame + self.num_frame_per_block] = ref
                set_y(cache_start_frame, self.num_frame_per_block)
                self._both(ref, conditional_dict, unconditional_dict, timestep, current_start_frame * fs, cache_only=True)
                current_start_frame += self.num_frame_per_block
                cache_start_frame += self.num_frame_per_block

        # Step 3: temporal denoising loop (:359-457)
        all_num_frames = [self.num_frame_per_block] * num_blocks
        if self.independent_first_frame and initial_latent is None:
            all_num_frames = [1] + all_num_frames
        if dwpose_data_emb is not None:
            expected_pose_frames = current_start_frame + sum(all_num_frames)
            assert dwpose_data_emb.shape[2] == expected_pose_frames, (
                f"dwpose_data_emb has {dwpose_data_emb.shape[2]} frames, "
                f"but expected {expected_pose_frames} to match the output timeline.")
        pose_tokens = self._pose_tokens(dwpose_data)[0] if use_pose else None      # [1, F'*h*w, 5120], once per clip
        guidance = float(self.args.guidance_scale)
        for current_num_frames in all_num_frames:
            latents = noise[:, cache_start_frame - num_input_frames:
                            cache_start_frame + current_num_frames - num_input_frames].contiguous()
            if dwpose_data_emb is not None:
                start, end = current_start_frame, current_start_frame + current_num_frames
                if end > dwpose_data_emb.shape[2]:
                    raise ValueError("dwpose_data has fewer frames than required for the current block.")
                condition = dwpose_data_emb[:, :, start:end].permute(0, 2, 3, 4, 1).flatten(1, 3).contiguous()
                conditional_dict["add_condition"] = condition
                unconditional_dict["add_condition"] = condition
            elif pose_tokens is not None:
                # token-major: the chunk's tokens are a row range, no copy (batch > 1: the one clip, expanded)
                condition = pose_tokens[:, current_start_frame * fs:(current_start_frame + current_num_frames) * fs]
                if batch_size > 1:
                    condition = condition.expand(batch_size, -1, -1).contiguous()
                conditional_dict["add_condition"] = condition
                unconditional_dict["add_condition"] = condition
            else:
                conditional_dict.pop("add_condition", None)
                unconditional_dict.pop("add_condition", None)

            set_y(cache_start_frame, current_num_frames)
            sample_scheduler = self._initialize_sample_scheduler(noise)
            for t in sample_scheduler.timesteps_host.tolist():
                timestep = torch.full([batch_size, current_num_frames], float(t), device=noise.device, dtype=torch.float32)
                flow_cond, flow_uncond = self._both(latents, conditional_dict, unconditional_dict, timestep,
                                                    current_start_frame * fs, cache_only=False)
                # uncond + g (cond - uncond), :423-424
                flow_pred = ops.lincomb([flow_uncond, flow_cond], [1.0 - guidance, guidance])
                latents = sample_scheduler.step(flow_pred, t, latents, return_dict=False)[0]

            output[:, cache_start_frame:cache_start_frame + current_num_frames] = latents
            # rerun at timestep zero so both caches hold the clean chunk (:438-455)
            self._both(latents, conditional_dict, unconditional_dict, torch.zeros_like(timestep),
                       current_start_frame * fs, cache_only=True)
            current_start_frame += current_num_frames
            cache_start_frame += current_num_frames

        # Step 4: decode (:461-468)
        video = self.vae.decode_to_pixel(output)
        video = (video * 0.5 + 0.5).clamp(0, 1)
        if return_latents:
            return video, output
        return video
