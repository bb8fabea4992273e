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

from typing import List, Optional

import torch

from . import ops
from .conditioning import Conditioning
from .i2v_condition import prepare_image
from .rollout_base import RolloutBase, chunk_plan
from .unipc import FlowUniPCMultistepScheduler


class _WholeClipY:
    """`encode_image`'s `y` of a whole clip as a `Conditioning` takes it: `begin`, then the next n latent frames, as slices."""
    pose_embedder = None

    def __init__(self, pipe, num_frames: int):
        self.pipe, self.num_frames = pipe, num_frames

    def begin(self, image, height, width, random_ref_dwpose=None):
        # once per clip, over the OUTPUT timeline (context frames included): a pass reads y at its position in `output`
        image_emb = self.pipe.encode_image(image, 4 * (self.num_frames - 1) + 1, height, width)
        self.y, self.position = image_emb["y"], 0
        assert self.y.shape[2] >= self.num_frames, (
            f"y has {self.y.shape[2]} latent frames, but the output timeline has {self.num_frames}.")
        if random_ref_dwpose is not None:   # the image to be driven by the pose (:341-347); [1, 20, 1, h, w] broadcast over time
            self.y = self.y + self.pose_embedder.embed_ref(random_ref_dwpose).to(self.y.dtype)
        return image_emb["clip_feature"]

    def frames(self, n: int):
        self.position += n
        return self.y[:, :, self.position - n:self.position]


class CausalDiffusionInferencePipeline(RolloutBase):
    _cache_sets = (("kv_cache_pos", "crossattn_cache_pos"), ("kv_cache_neg", "crossattn_cache_neg"))
    _image_user = "encode_image"
    _no_i2v_hint = "; encode_image() still produces its clip_feature and y"

    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, image_encoder=None,
                 overlap_cfg: Optional[bool] = None, pose_embedder=None):
        super().__init__(args, device, generator, text_encoder, vae, image_encoder, pose_embedder)
        self.num_train_timesteps = args.num_train_timestep
        self.sampling_steps = 50
        self.sample_solver = "unipc"
        self.shift = args.timestep_shift

        # the negative-prompt pass on a second stream needs its own activation workspace over the same weights
        can_share = hasattr(self.generator, "share")
        self.overlap_cfg = can_share if overlap_cfg is None else bool(overlap_cfg)
        if self.overlap_cfg and not can_share:
            raise ValueError("overlap_cfg=True needs a generator with share() (self_forcing_amd.WanDiffusionWrapper)")
        self._generator_neg = self.generator.share() if self.overlap_cfg else self.generator
        self._side_stream = None
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
        image = prepare_image(image, height, width).to(self.device, torch.float32)
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
        batch_size, num_frames, num_channels, height, width = noise.shape
        num_input_frames = initial_latent.shape[1] if initial_latent is not None else 0
        num_output_frames = num_frames + num_input_frames
        # all checks, then the image (once per clip: `encode_image`) and the pose clip (once per clip: `_pose_tokens`)
        cond = Conditioning(self, lambda: _WholeClipY(self, num_output_frames), batch_size, num_output_frames, height, width,
                            input_image=input_image, dwpose_data=dwpose_data, random_ref_dwpose=random_ref_dwpose,
                            dwpose_data_emb=dwpose_data_emb, pose_offset=start_frame_index or 0)
        warm_up_frames, all_num_frames = chunk_plan(num_frames, num_input_frames, self.independent_first_frame, self.num_frame_per_block)
        self.frame_seq_length = fs = (height // 2) * (width // 2)
        # (:352-353) one image: the wrapper expands clip_feature to the batch
        conditional_dict = dict(self.text_encoder(text_prompts=text_prompts), **cond.clip_entries)
        unconditional_dict = dict(self.text_encoder(text_prompts=[self.args.negative_prompt] * len(text_prompts)), **cond.clip_entries)

        output = torch.zeros([batch_size, num_output_frames, num_channels, height, width], device=noise.device, dtype=noise.dtype)

        # Step 1: caches (:203-231)
        self._prepare_caches(batch_size, num_output_frames, noise.dtype, noise.device)

        # Step 2: context frames into both caches (:233-297)
        current_start_frame = start_frame_index
        cache_start_frame = 0
        timestep = torch.zeros([batch_size, 1], device=noise.device, dtype=torch.int64) if warm_up_frames else None
        for n in warm_up_frames:
            ref = initial_latent[:, cache_start_frame:cache_start_frame + n]
            output[:, cache_start_frame:cache_start_frame + n] = ref
            entries = cond.chunk(cache_start_frame, n, warm_up=True)      # y only
            conditional_dict.update(entries)
            unconditional_dict.update(entries)
            self._both(ref, conditional_dict, unconditional_dict, timestep, current_start_frame * fs, cache_only=True)
            current_start_frame += n
            cache_start_frame += n

        # Step 3: temporal denoising loop (:359-457)
        guidance = float(self.args.guidance_scale)
        for current_num_frames in all_num_frames:
            latents = noise[:, cache_start_frame - num_input_frames:
                            cache_start_frame + current_num_frames - num_input_frames].contiguous()
            # `y` at the chunk's place in `output`; the pose rows `start_frame_index` further on, where its frames stand for RoPE
            entries = cond.chunk(cache_start_frame, current_num_frames)
            for d in (conditional_dict, unconditional_dict):
                d.pop("add_condition", None)
                d.update(entries)
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
