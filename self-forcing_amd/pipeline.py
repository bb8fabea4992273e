"""`CausalInferencePipeline` -- drop-in for pipeline/causal_inference.py of the reference.

Same constructor `(args, device, generator=None, text_encoder=None, vae=None)` (plus `image_encoder=None,
pose_embedder=None`), same `inference(noise, text_prompts, initial_latent=None, return_latents=False, profile=False,
low_memory=False)` (plus the keywords the reference's driver passes to whichever pipeline the config selects,
inference.py:166-174: `input_image=None, dwpose_data=None, random_ref_dwpose=None`, and `dwpose_data_emb=None`), same attributes read by the reference's other callers (`kv_cache1`,
`crossattn_cache`, `denoising_step_list`, `scheduler`, `frame_seq_length`, `num_frame_per_block`,
`num_transformer_blocks`; demo.py:309-404) and the same cache-dict schema.

What differs: the five constants the reference hard-codes for Wan-1.3B/480p
(30 blocks, 1560 tokens/frame, 12x128 heads, 32760-token cache; causal_inference.py:33-34,
:288-293) are derived from the generator's shape and the latent size; when no text encoder / VAE is
injected, `WanTextEncoder()` / `WanVAEWrapper()` are built from the reference's default local
checkpoint paths as causal_inference.py:19-23 does (weights-only loads; FileNotFoundError when the
files are absent -- benchmarks and tests inject the stand-ins of `harness.py` or seeded-weight
instances instead); the per-step `print` is dropped; `low_memory` is accepted and ignored (288 GB HBM).

Image and pose conditioning (the reference's few-step pipeline takes neither): with an i2v generator
`input_image` is encoded by the CLIP image encoder once per clip (`clip_feature`) and by the VAE encoder chunk by chunk --
`y` for chunk k is produced right before chunk k's first pass, on the rollout's stream, by `i2v_condition.I2VConditioner`,
and reused by the chunk's passes; every pass, warm-up passes included, gets the frames of `y` at its position in the
output timeline.  `dwpose_data` [3, F, H, W] with `random_ref_dwpose` [H, W, 3] are embedded once per clip
(`pose.PoseEmbedder`; a chunk's `add_condition` is a row range of the tokens), or already-embedded `dwpose_data_emb`
[B, C_pose, F, h, w] is sliced per chunk; with an image too, the reference-pose map goes into `y`.  The semantics, checks
and messages are those of `CausalDiffusionInferencePipeline`.  With none of these arguments nothing changes.

Open length: `open_session(...)` returns a `live.LiveSession`, `stream` without a fixed frame count -- the
same chunk loop (`_denoise_chunks` takes its chunks from a source) over noise drawn chunk by chunk, a rolling KV cache, re-based
RoPE positions and a bounded pose-token buffer, until the pose feed or the noise feed ends or the caller closes it.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import logging

import torch

from .kvcache import new_crossattn_cache, new_kv_cache, reset_kv_indices
from .wan_wrapper import WanDiffusionWrapper

log = logging.getLogger(__name__)


class CausalInferencePipeline(torch.nn.Module):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, image_encoder=None, pose_embedder=None):
        super().__init__()
        self.device_ = torch.device(device)
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
        # image / pose conditioning: injected, or loaded lazily on first need from args.clip_checkpoint_path /
        # args.pose_weights_path (as CausalDiffusionInferencePipeline does)
        self.image_encoder = image_encoder
        self.clip_checkpoint_path = getattr(args, "clip_checkpoint_path", None)
        self.pose_embedder = pose_embedder
        self.pose_weights_path = getattr(args, "pose_weights_path", None)
        self.pose_weights_strict = getattr(args, "pose_weights_strict", True)
        self.pose_weights_loaded = pose_embedder is not None
        self.conditioner = None      # i2v_condition.I2VConditioner, built on the first inference with an image

        # causal hyper-parameters (causal_inference.py:25-45)
        self.scheduler = self.generator.get_scheduler()
        self.denoising_step_list = torch.tensor(args.denoising_step_list, dtype=torch.long)
        if args.warp_denoising_step:
            timesteps = torch.cat((self.scheduler.timesteps.cpu(), torch.tensor([0], dtype=torch.float32)))
            self.denoising_step_list = timesteps[1000 - self.denoising_step_list]

        self.num_transformer_blocks = self.generator.model.num_layers
        self.frame_seq_length = 1560  # refined from the latent size at inference()
        self.kv_cache1 = None
        self.crossattn_cache = None
        self.args = args
        self.num_frame_per_block = getattr(args, "num_frame_per_block", 1)
        self.independent_first_frame = args.independent_first_frame
        self.local_attn_size = self.generator.model.local_attn_size
        if self.num_frame_per_block > 1:
            self.generator.model.num_frame_per_block = self.num_frame_per_block
        # re-noise source; the reference calls torch.randn_like (causal_inference.py:208).  Tests and
        # the CPU-baseline comparison inject pre-drawn tensors here so both sides consume the same eps.
        self.noise_source: Optional[Callable[[torch.Tensor], torch.Tensor]] = None
        # context / warm-up passes only update the KV cache; a generator that advertises `cache_only`
        # (ours) may skip what nothing reads.  Foreign generators are called exactly as the reference does.
        import inspect
        try:
            self._cache_only_kw = {"cache_only": True} if "cache_only" in inspect.signature(self.generator.forward).parameters else {}
        except (TypeError, ValueError):
            self._cache_only_kw = {}
        self.last_profile = None
        self._cache_key = None
        # run a chunk's context pass together with the next chunk's first denoising pass (one call, same results; see
        # _denoise_chunks); False = one generator call per pass, as the reference
        self.pair_context_with_next = True
        # ... when a pass has at most this many tokens (batch x frames x tokens per frame): pairing pays through the GEMMs'
        # tile quantisation -- one prompt at 480p, 4680 rows: +2.0 % (84.9 -> 86.5, 85.2 -> 86.9 frames/s, same box,
        # alternating runs); at 9360 rows (two prompts per call) the GEMMs' rounds are already full: +-0.3 %, not worth
        # the second workspace
        self.pair_max_rows = 6144

    # ------------------------------------------------------------------------------------------
    def _randn_like(self, t: torch.Tensor) -> torch.Tensor:
        if self.noise_source is not None:
            return self.noise_source(t).to(device=t.device, dtype=t.dtype)
        return torch.randn_like(t)

    # ------------------------------------------------------------------------------------------ image / pose conditioning
    def _pose_embedder(self):
        """The injected pose embedder, or the one loaded from args.pose_weights_path on first need."""
        if self.pose_embedder is None:
            if self.pose_weights_path is None:
                raise ValueError("dwpose_data needs pose weights: set args.pose_weights_path or construct the pipeline with pose_embedder=")
            from .pose import PoseEmbedder
            self.pose_embedder = PoseEmbedder(self.pose_weights_path, device=self.device_, strict=self.pose_weights_strict)
            self.pose_weights_loaded = True
        return self.pose_embedder

    def _image_encoder(self):
        if self.image_encoder is None:
            if self.clip_checkpoint_path is None:
                raise ValueError("input_image needs the CLIP image encoder: set args.clip_checkpoint_path or construct the pipeline "
                                 "with image_encoder=")
            from .clip import CLIPModel
            self.image_encoder = CLIPModel(dtype=torch.bfloat16, device=self.device_, checkpoint_path=self.clip_checkpoint_path)
        return self.image_encoder

    def _conditioner(self):
        if self.conditioner is None:
            from .i2v_condition import I2VConditioner
            self.conditioner = I2VConditioner(self.vae, self._image_encoder(), device=self.device_)
        return self.conditioner

    def _conditioning(self, batch_size, num_output_frames, height, width, input_image, dwpose_data, random_ref_dwpose, dwpose_data_emb,
                      pose_feed=None, live_chunk_frames=None):
        """The clip's conditioning beyond the prompt: (entries of the condition dict that hold for the whole clip,
        chunk_condition(first_frame, n, warm_up=False) -> the entries of the pass(es) over those latent frames), or
        (None, None) when there is none.  All checks come first, before any work; the image is encoded by CLIP and the
        pose clip embedded here, once; `y` is produced by `chunk_condition`, in timeline order, one request per chunk.
        `pose_feed` (an iterable of [3, n, H, W] pieces, `stream` only) replaces the pose clip: its first piece is taken
        here for the size check, every further piece when `chunk_condition` needs rows that are not final yet.
        An open-length session (`open_session`) passes `num_output_frames` None and its chunk length as `live_chunk_frames`:
        the feed's rows then live in a bounded buffer, and `chunk_condition` returns None once the feed has ended."""
        is_i2v = getattr(getattr(getattr(self, "generator", None), "model", None), "model_type", "t2v") == "i2v"
        if input_image is not None and not is_i2v:
            raise NotImplementedError("input_image: this generator has no i2v branch (img_emb, k_img / v_img, the 36-channel patch "
                                      "embedding: model_type 'i2v'), so the rollout cannot consume an image")
        if is_i2v and input_image is None:
            raise ValueError("an i2v generator needs input_image: every pass takes its clip_feature and y")
        fs = self.frame_seq_length
        if pose_feed is not None and (dwpose_data is not None or dwpose_data_emb is not None):
            raise ValueError("pass either pose_feed or a whole pose clip (dwpose_data / dwpose_data_emb), not both")
        use_pose = dwpose_data is not None and random_ref_dwpose is not None      # both, as the reference (:336)
        if use_pose:
            if dwpose_data_emb is not None:
                raise ValueError("pass either dwpose_data (with random_ref_dwpose) or dwpose_data_emb, not both")
            if dwpose_data.dim() != 4 or dwpose_data.shape[0] != 3:
                raise ValueError(f"dwpose_data must be one clip [3, F, H, W] (shared by the batch), got {tuple(dwpose_data.shape)}")
            from .pose_weights import pose_plan
            pose_fhw = pose_plan(*dwpose_data.shape[1:])
            assert pose_fhw[0] == num_output_frames, (
                f"dwpose_data_emb has {pose_fhw[0]} frames, "
                f"but expected {num_output_frames} to match the output timeline.")
            if pose_fhw[1] * pose_fhw[2] != fs:
                raise ValueError(f"dwpose_data gives {pose_fhw[1]}x{pose_fhw[2]} pose tokens per frame, the latents {height // 2}x{width // 2}. "
                                 "Check pose data processing.")
        elif pose_feed is None and (dwpose_data is not None or random_ref_dwpose is not None):
            log.warning("only one of dwpose_data / random_ref_dwpose was given: the pose branch needs both and is not taken")
        feed, feed_first = None, None
        if pose_feed is not None:
            from .pose_weights import POSE_DIM, pose_plan
            feed = iter(pose_feed)
            feed_first = next(feed, None)
            if feed_first is None:
                raise ValueError("pose_feed is empty: chunk 0 needs its first pose frames")
            if feed_first.dim() != 4 or feed_first.shape[0] != 3 or feed_first.shape[1] < 1:
                raise ValueError(f"a pose_feed piece must be [3, n >= 1, H, W] (shared by the batch), got {tuple(feed_first.shape)}")
            _, ph, pw = pose_plan(1, *feed_first.shape[2:])
            if ph * pw != fs:
                raise ValueError(f"dwpose_data gives {ph}x{pw} pose tokens per frame, the latents {height // 2}x{width // 2}. "
                                 "Check pose data processing.")
        if dwpose_data_emb is not None:
            assert dwpose_data_emb.shape[2] == num_output_frames, (
                f"dwpose_data_emb has {dwpose_data_emb.shape[2]} frames, "
                f"but expected {num_output_frames} to match the output timeline.")
        if not (is_i2v or use_pose or dwpose_data_emb is not None or feed is not None):
            return None, None

        clip_entries = {}
        cond = None
        if is_i2v:
            cond = self._conditioner()
            ref_in_y = use_pose or (feed is not None and random_ref_dwpose is not None)
            if ref_in_y and getattr(cond, "pose_embedder", None) is None:
                cond.pose_embedder = self._pose_embedder()      # the image to be driven by the pose: its map goes into y
            # one image: the wrapper expands clip_feature to the batch
            clip_entries["clip_feature"] = cond.begin(input_image, height * 8, width * 8, random_ref_dwpose if ref_in_y else None)
        pose_tokens = self._pose_embedder().embed(dwpose_data)[0] if use_pose else None      # [1, F'*h*w, 5120], once per clip
        next_frame = [0]
        feed_rows = None
        live_rows = None
        if feed is not None and num_output_frames is None:
            # open length: a bounded buffer that holds only the rows of the chunks in flight (live.PoseRows)
            from .live import PoseRows
            live_rows = PoseRows(self._pose_embedder().open_stream(*feed_first.shape[2:]), fs, live_chunk_frames, feed, feed_first)
            pose_tokens = live_rows.buffer
        elif feed is not None:
            # the clip's rows in one buffer, filled as the feed delivers; a chunk's add_condition stays a row range of it
            pose_stream = self._pose_embedder().open_stream(*feed_first.shape[2:])
            pose_tokens = torch.empty(1, num_output_frames * fs, POSE_DIM, dtype=torch.bfloat16, device=pose_stream.embedder.device)
            pending = [feed_first]

            def feed_rows(first: int, upto: int) -> None:
                """Pull pieces until latent frames [0, upto) are final (4*upto + 1 pixel frames in) or the feed ends, which
                closes the clip.  Nothing is pulled ahead of that."""
                while pose_stream.latent_frames_done < upto and not pose_stream.closed:
                    piece = pending.pop() if pending else next(feed, None)
                    row = pose_stream.latent_frames_done * fs
                    if piece is None:
                        pose_stream.close(out=pose_tokens, out_row=row)
                    else:      # frames past 4 F + 1 belong to latent frames the noise does not have
                        pose_stream.push(piece[:, :4 * num_output_frames + 1 - pose_stream.frames_pushed], out=pose_tokens, out_row=row)
                if pose_stream.latent_frames_done < upto:
                    raise ValueError(f"pose_feed ended after {pose_stream.frames_pushed} pose frames: latent frames {first}..{upto - 1} need "
                                     f"{4 * upto - 3} when the clip ends with them ({4 * upto + 1} when it goes on)")

        def chunk_condition(first_frame: int, n: int, warm_up: bool = False) -> dict:
            entries = {}
            if live_rows is not None and not warm_up:
                # an open-length session: the chunk's rows first, since a feed that has ended ends the session (None)
                # before anything of the chunk is encoded
                condition = live_rows.take(first_frame, n)
                if condition is None:
                    return None
                entries["add_condition"] = condition.expand(batch_size, -1, -1).contiguous() if batch_size > 1 else condition
            if cond is not None:
                assert first_frame == next_frame[0], f"y is produced in timeline order: frame {next_frame[0]} is next, not {first_frame}"
                next_frame[0] += n
                entries["y"] = cond.frames(n)
            if warm_up:      # the context frames' passes take y only, as in the multi-step pipeline
                return entries
            if dwpose_data_emb is not None:
                entries["add_condition"] = dwpose_data_emb[:, :, first_frame:first_frame + n].permute(0, 2, 3, 4, 1).flatten(1, 3).contiguous()
            elif pose_tokens is not None and live_rows is None:
                if feed_rows is not None:
                    feed_rows(first_frame, first_frame + n)
                # token-major: the chunk's tokens are a row range, no copy (batch > 1: the one clip, expanded)
                condition = pose_tokens[:, first_frame * fs:(first_frame + n) * fs]
                entries["add_condition"] = condition.expand(batch_size, -1, -1).contiguous() if batch_size > 1 else condition
            return entries
        chunk_condition.live_rows = live_rows
        return clip_entries, chunk_condition

    def inference(self, noise: torch.Tensor, text_prompts: List[str], initial_latent: Optional[torch.Tensor] = None,
                  return_latents: bool = False, profile: bool = False, low_memory: bool = False, input_image=None,
                  dwpose_data: Optional[torch.Tensor] = None, random_ref_dwpose: Optional[torch.Tensor] = None,
                  dwpose_data_emb: Optional[torch.Tensor] = None):
        """noise [B, F, C, H, W] -> video in [0, 1] (and the latents)."""
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
        clip_entries, chunk_condition = self._conditioning(batch_size, num_output_frames, height, width, input_image, dwpose_data,
                                                           random_ref_dwpose, dwpose_data_emb)
        conditional_dict = self.text_encoder(text_prompts=text_prompts)
        if chunk_condition is not None:
            conditional_dict = dict(conditional_dict, **clip_entries)

        output = torch.zeros([batch_size, num_output_frames, num_channels, height, width], device=noise.device, dtype=noise.dtype)

        if profile:
            ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
            init_start, init_end, diffusion_start, diffusion_end, vae_start, vae_end = ev(), ev(), ev(), ev(), ev(), ev()
            block_events = []
            init_start.record()

        # Step 1: (re)initialise the caches (causal_inference.py:111-132)
        key = (batch_size, self._cache_tokens(num_output_frames), noise.device)
        if self.kv_cache1 is None or self._cache_key != key:
            self._initialize_kv_cache(batch_size, noise.dtype, noise.device, cache_tokens=key[1])
            self._initialize_crossattn_cache(batch_size, noise.dtype, noise.device)
            self._cache_key = key
        else:
            for block_index in range(self.num_transformer_blocks):
                self.crossattn_cache[block_index]["is_init"] = False
            self._reset_kv_indices()

        # Step 2: cache the context frames (causal_inference.py:134-169)
        gen = self.generator
        current_start_frame = 0
        if initial_latent is not None:
            timestep = torch.zeros([batch_size, 1], device=noise.device, dtype=torch.int64)
            if self.independent_first_frame:
                assert (num_input_frames - 1) % self.num_frame_per_block == 0
                num_input_blocks = (num_input_frames - 1) // self.num_frame_per_block
                output[:, :1] = initial_latent[:, :1]
                if chunk_condition is not None:
                    conditional_dict.update(chunk_condition(current_start_frame, 1, warm_up=True))
                gen(noisy_image_or_video=initial_latent[:, :1], conditional_dict=conditional_dict, timestep=timestep,
                    kv_cache=self.kv_cache1, crossattn_cache=self.crossattn_cache,
                    current_start=current_start_frame * self.frame_seq_length, **self._cache_only_kw)
                current_start_frame += 1
            else:
                assert num_input_frames % self.num_frame_per_block == 0
                num_input_blocks = num_input_frames // self.num_frame_per_block
            for _ in range(num_input_blocks):
                ref = initial_latent[:, current_start_frame:current_start_frame + self.num_frame_per_block]
                output[:, current_start_frame:current_start_frame + self.num_frame_per_block] = ref
                if chunk_condition is not None:
                    conditional_dict.update(chunk_condition(current_start_frame, self.num_frame_per_block, warm_up=True))
                gen(noisy_image_or_video=ref, conditional_dict=conditional_dict, timestep=timestep,
                    kv_cache=self.kv_cache1, crossattn_cache=self.crossattn_cache,
                    current_start=current_start_frame * self.frame_seq_length, **self._cache_only_kw)
                current_start_frame += self.num_frame_per_block

        if profile:
            init_end.record()
            diffusion_start.record()

        # Step 3: temporal denoising loop (causal_inference.py:176-244)
        all_num_frames = [self.num_frame_per_block] * num_blocks
        if self.independent_first_frame and initial_latent is None:
            all_num_frames = [1] + all_num_frames
        for chunk_idx, start_frame, denoised_pred in self._denoise_chunks(
                self._noise_chunks(noise, all_num_frames), conditional_dict, set(all_num_frames), current_start_frame, skip_last_context=False,
                chunk_condition=chunk_condition, on_chunk_start=(lambda: block_events.append([ev(), ev()]) or block_events[-1][0].record()) if profile else None,
                on_chunk_end=(lambda: block_events[-1][1].record()) if profile else None):
            output[:, start_frame:start_frame + denoised_pred.shape[1]] = denoised_pred

        if profile:
            diffusion_end.record()
            vae_start.record()

        # Step 4: decode (causal_inference.py:254-256)
        video = self.vae.decode_to_pixel(output, use_cache=False)
        video = (video * 0.5 + 0.5).clamp(0, 1)

        if profile:
            vae_end.record()
            torch.cuda.synchronize()
            init_time = init_start.elapsed_time(init_end)
            diffusion_time = diffusion_start.elapsed_time(diffusion_end)
            vae_time = vae_start.elapsed_time(vae_end)
            blocks = [a.elapsed_time(b) for a, b in block_events]
            total = init_time + diffusion_time + vae_time
            self.last_profile = {"init_ms": init_time, "diffusion_ms": diffusion_time, "vae_ms": vae_time,
                                 "block_ms": blocks, "total_ms": total}
            share = lambda part, whole: 100.0 * part / max(whole, 1e-9)  # noqa: E731
            report = [f"rollout profile: {total:.1f} ms = cache setup {init_time:.1f} ms ({share(init_time, total):.1f} %) + "
                      f"denoising {diffusion_time:.1f} ms ({share(diffusion_time, total):.1f} %) + decode {vae_time:.1f} ms "
                      f"({share(vae_time, total):.1f} %)"]
            report += [f"  chunk {i}: {bt:.1f} ms ({share(bt, diffusion_time):.1f} % of denoising)" for i, bt in enumerate(blocks)]
            print("\n".join(report))

        if return_latents:
            return video, output
        return video

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _noise_chunks(noise, all_num_frames):
        """A whole clip's noise [B, F, C, H, W] as `_denoise_chunks` takes it: one slice per chunk."""
        at = 0
        for n in all_num_frames:
            yield noise[:, at:at + n]
            at += n

    def _denoise_chunks(self, chunks, conditional_dict, lengths, current_start_frame, skip_last_context,
                        on_chunk_start=None, on_chunk_end=None, chunk_condition=None, rebase=None):
        """The chunk loop of causal_inference.py:176-244 as a generator: yields
        (chunk_index, start_frame, x0 [B, f, C, H, W]) as soon as a chunk's last denoising step is
        enqueued; the context pass that rewrites the chunk's K/V "clean" follows (and is skipped for
        the final chunk when `skip_last_context`, as demo.py:396 does: nothing reads that update).
        `chunks`: the source of the noise, one [B, f, C, H, W] tensor per chunk -- slices of a clip's noise
        (`_noise_chunks`) or a live session's feed; the loop runs until it ends and looks one chunk ahead (a chunk is the last
        one when nothing follows it).  `lengths`: the chunk lengths the caller expects, whose timestep tables are built
        before the first chunk (any other length gets its own on first use).
        `chunk_condition` (`_conditioning`): asked once per chunk, right before the chunk's first pass, for the chunk's
        `y` / `add_condition`, which then stay in `conditional_dict` for all of the chunk's passes.  An open-length session's
        returns None when its pose source has ended: the loop ends there.
        `rebase` (`live.LiveSession`): asked before every generator call with the highest frame position the call needs
        (for a pair the second pass's start_frame + f); it may move the cache back in the timeline and returns by how
        many frames, which the loop subtracts from the positions it passes on.  `start_frame` as yielded and as
        `chunk_condition` sees it stays the frame of the output timeline."""
        gen = self.generator
        chunks = iter(chunks)
        noisy_input = next(chunks, None)
        if noisy_input is None:
            return
        batch_size, device = noisy_input.shape[0], noisy_input.device
        # Every timestep tensor of the rollout is built HERE, once: the reference builds `ones([B, f], int64) * t` for each
        # forward and `t_next * ones([B * f], long)` for each re-noise (causal_inference.py:190-216, :228) -- three small
        # launches per step of kernels this library does not own.  One host->device copy of the step list, one broadcast
        # per distinct chunk length; the loop below then launches nothing of torch's but `randn_like` (the reference's
        # global-RNG re-noise, :208, which must stay) and the caller's copy of the chunk into `output`.  (A chunk's `y` adds
        # VAE encode calls and sf_i2v_assemble_y, all this library's; one clip's pose tokens are a view.  Only pose tokens for a
        # batch, or already-embedded ones, are copied by torch once per chunk, as in the multi-step pipeline.)
        steps = self.denoising_step_list.to(device)
        ctx_noise = getattr(self.args, "context_noise", 0)
        tables = {}

        def table(f):
            if f not in tables:
                ones = torch.ones([batch_size, f], device=device, dtype=torch.int64)
                per_step = (ones.unsqueeze(0) * steps.reshape(-1, 1, 1)).contiguous()      # [S, B, f], dtype as `ones * t`
                tables[f] = (list(per_step.unbind(0)), [t.flatten() for t in per_step.unbind(0)],
                             torch.ones_like(per_step[0]) * ctx_noise)
            return tables[f]
        for f in lengths:
            table(f)
        n_steps = steps.shape[0]
        # A chunk's context pass and the next chunk's first denoising pass run back to back in the reference (:226-235, then
        # :190-205) and layer l of the second needs only layer l's K / V of the first: a generator that offers `forward_pair`
        # (ours) runs them as ONE call -- bit-identical latents, twice the rows per GEMM (the two-pass sf_dit_forward).  The re-noise
        # draws keep their order: nothing is drawn between a chunk's last step and the next chunk's first.
        # Pose tokens differ between the two passes of a pair: only `chunk_condition` knows both chunks'.  A dict that arrives
        # with its own `add_condition` (the reference's convention) is handed to every pass as it is, unpaired.
        pair_ok = bool(self.pair_context_with_next and self._cache_only_kw and hasattr(gen, "forward_pair")
                       and gen.can_pair(conditional_dict)
                       and (chunk_condition is not None or conditional_dict.get("add_condition") is None)
                       and batch_size * max(lengths) * self.frame_seq_length <= self.pair_max_rows)
        position = current_start_frame      # the chunk's first frame as RoPE and the cache indices see it: behind the timeline by the re-bases

        def place(need):
            nonlocal position
            if rebase is not None:
                position -= rebase(need)
            return position * self.frame_seq_length
        first_pred = None          # x0 of this chunk's first step when the previous chunk's pair has already computed it
        next_entries = None        # ... and the chunk's condition entries, which that pair has already asked for
        chunk_idx = 0
        while noisy_input is not None:
            current_num_frames = noisy_input.shape[1]
            if on_chunk_start is not None:
                on_chunk_start()
            if chunk_condition is not None:
                entries = next_entries if next_entries is not None else chunk_condition(current_start_frame, current_num_frames)
                next_entries = None
                if entries is None:
                    return
                conditional_dict.update(entries)
            step_ts, step_ts_flat, context_timestep = table(current_num_frames)
            for index in range(n_steps):
                if index == 0 and first_pred is not None:
                    denoised_pred, first_pred = first_pred, None
                else:
                    start_tok = place(position + current_num_frames)
                    _, denoised_pred = gen(noisy_image_or_video=noisy_input, conditional_dict=conditional_dict,
                                           timestep=step_ts[index], kv_cache=self.kv_cache1,
                                           crossattn_cache=self.crossattn_cache, current_start=start_tok)
                if index < n_steps - 1:
                    flat = denoised_pred.flatten(0, 1)
                    noisy_input = self.scheduler.add_noise(flat, self._randn_like(flat), step_ts_flat[index + 1]
                                                           ).unflatten(0, denoised_pred.shape[:2])
            yield chunk_idx, current_start_frame, denoised_pred
            # rerun at the context timestep so the cache holds clean K/V (causal_inference.py:226-235)
            next_noise = next(chunks, None)
            if not (skip_last_context and next_noise is None):
                paired = False
                if pair_ok and next_noise is not None and next_noise.shape[1] == current_num_frames:
                    pair_kw = {}
                    if chunk_condition is not None:      # pose tokens: the context pass takes this chunk's, the paired pass the next chunk's
                        next_entries = chunk_condition(current_start_frame + current_num_frames, current_num_frames)
                        if next_entries is None:
                            next_noise = None            # the pose source has ended: this chunk is the last one
                        elif "add_condition" in next_entries:
                            pair_kw["add_conditions"] = (conditional_dict["add_condition"], next_entries["add_condition"])
                    if next_noise is not None:
                        start_tok = place(position + 2 * current_num_frames)
                        first_pred = gen.forward_pair(denoised_pred, context_timestep, next_noise, step_ts[0],
                                                      conditional_dict, self.kv_cache1, self.crossattn_cache, start_tok,
                                                      start_tok + current_num_frames * self.frame_seq_length, **pair_kw)[1]
                        paired = True
                if not paired:
                    start_tok = place(position + current_num_frames)
                    gen(noisy_image_or_video=denoised_pred, conditional_dict=conditional_dict, timestep=context_timestep,
                        kv_cache=self.kv_cache1, crossattn_cache=self.crossattn_cache, current_start=start_tok,
                        **self._cache_only_kw)
            if on_chunk_end is not None:
                on_chunk_end()
            current_start_frame += current_num_frames
            position += current_num_frames
            noisy_input = next_noise
            chunk_idx += 1

    def stream(self, noise: torch.Tensor, text_prompts: List[str], skip_last_context: bool = True,
               overlap_decode: bool = False, frame_encoder=None, input_image=None, dwpose_data: Optional[torch.Tensor] = None,
               random_ref_dwpose: Optional[torch.Tensor] = None, dwpose_data_emb: Optional[torch.Tensor] = None, pose_feed=None):
        """Chunk-at-a-time generation (the streaming boundary; mirrors the inline loop of the
        reference's demo.py:303-468): yields `(chunk_index, latents [B, f, C, H, W], pixels)` per chunk.
        `pixels` comes from `vae.decode_chunk(latents, chunk_index)` when the injected VAE has a streaming
        decoder, else from `decode_to_pixel` on the chunk alone.

        overlap_decode=False: chunk k is decoded right after it is denoised and yielded at once (lowest
        latency to the first frame).  overlap_decode=True: the decode of chunk k runs on a second HIP stream
        while chunk k+1 is being denoised (it fills the CUs the denoiser's single-round kernels leave idle);
        chunk k is then yielded one chunk later, as soon as its decode has finished.

        frame_encoder (a `JpegEncoder`): every chunk's frames are also encoded on the GPU, on the stream that decoded
        them, and the generator yields `(chunk_index, latents, pixels, frames)` with `frames` the chunk's JPEG files
        (B * T of them).  An encoder with value_range (-1, 1) gets the decoder's output (the demo's truncation), one with
        (0, 1) gets `pixels`.  Without one the 3-tuples are exactly what they were.

        input_image / dwpose_data / random_ref_dwpose / dwpose_data_emb: as `inference`.  Chunk k's `y` is encoded on the
        rollout's stream right before chunk k's first pass; nothing is encoded ahead of need.

        pose_feed: an iterable of pose pieces [3, n >= 1, H, W] (any lengths) instead of a whole `dwpose_data` clip -- a
        live source.  It takes the pose branch by itself (`random_ref_dwpose` still only goes into an i2v generator's `y`).
        Pieces are pulled only when a chunk's rows are not final yet: chunk k of three latent frames needs 12 k + 13 pose
        frames, one latent frame beyond its own, or the feed's end, which closes the clip (then 4 (f - 1) + 1 frames
        serve f latent frames, as with `dwpose_data`).  A feed that ends too early is a ValueError.  The latents are the
        whole clip's, bit for bit (`PoseStream`)."""
        batch_size, num_frames, num_channels, height, width = noise.shape
        if self.independent_first_frame:
            assert (num_frames - 1) % self.num_frame_per_block == 0
            all_num_frames = [1] + [self.num_frame_per_block] * ((num_frames - 1) // self.num_frame_per_block)
        else:
            assert num_frames % self.num_frame_per_block == 0
            all_num_frames = [self.num_frame_per_block] * (num_frames // self.num_frame_per_block)
        self.frame_seq_length = (height // 2) * (width // 2)
        clip_entries, chunk_condition = self._conditioning(batch_size, num_frames, height, width, input_image, dwpose_data,
                                                           random_ref_dwpose, dwpose_data_emb, pose_feed)
        conditional_dict = self.text_encoder(text_prompts=text_prompts)
        if chunk_condition is not None:
            conditional_dict = dict(conditional_dict, **clip_entries)
        key = (batch_size, self._cache_tokens(num_frames), noise.device)
        if self.kv_cache1 is None or self._cache_key != key:
            self._initialize_kv_cache(batch_size, noise.dtype, noise.device, cache_tokens=key[1])
            self._initialize_crossattn_cache(batch_size, noise.dtype, noise.device)
            self._cache_key = key
        else:
            for block_index in range(self.num_transformer_blocks):
                self.crossattn_cache[block_index]["is_init"] = False
            self._reset_kv_indices()
        chunks = self._denoise_chunks(self._noise_chunks(noise, all_num_frames), conditional_dict, set(all_num_frames), 0, skip_last_context,
                                      chunk_condition=chunk_condition)
        yield from self._decoded_chunks(chunks, noise.device, overlap_decode, frame_encoder)

    def _decoded_chunks(self, chunks, device, overlap_decode, frame_encoder):
        """What `stream` and a live session yield per chunk of `_denoise_chunks`: `(chunk_index, latents, pixels[, frames])`,
        decoded at once or, with `overlap_decode`, on a second HIP stream while the next chunk is denoised."""
        decode_chunk = getattr(self.vae, "decode_chunk", None)

        def decode(x0, chunk_idx):
            pixels = decode_chunk(x0, chunk_idx) if decode_chunk is not None else self.vae.decode_to_pixel(x0, use_cache=False)
            raw, pixels = pixels, (pixels * 0.5 + 0.5).clamp(0, 1)
            if frame_encoder is None:
                return (pixels,)
            src = raw if tuple(frame_encoder.value_range) == (-1, 1) else pixels
            return pixels, frame_encoder._encode(src)              # device buffers; read back when the chunk is yielded

        def finish(chunk_idx, x0, decoded):
            if frame_encoder is None:
                return chunk_idx, x0, decoded[0]
            return chunk_idx, x0, decoded[0], frame_encoder._to_host(*decoded[1])

        if not overlap_decode:
            for chunk_idx, start_frame, x0 in chunks:
                yield finish(chunk_idx, x0, decode(x0, chunk_idx))
            return
        if getattr(self, "_decode_stream", None) is None:
            self._decode_stream = torch.cuda.Stream(device=device)
        side, main = self._decode_stream, torch.cuda.current_stream(device)
        pending = None            # (chunk_idx, x0, pixels, done event) of the chunk being decoded on the side stream
        for chunk_idx, start_frame, x0 in chunks:
            ready = torch.cuda.Event()
            ready.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ready)
                x0.record_stream(side)
                decoded = decode(x0, chunk_idx)
                done = torch.cuda.Event()
                done.record(side)
            if pending is not None:
                pending[3].synchronize()
                yield finish(*pending[:3])
            pending = (chunk_idx, x0, decoded, done)
        if pending is not None:
            pending[3].synchronize()
            main.wait_event(pending[3])
            yield finish(*pending[:3])

    def open_session(self, text_prompts: List[str], latent_size, batch_size: int = 1, noise_feed=None, generator=None, input_image=None,
                     random_ref_dwpose: Optional[torch.Tensor] = None, pose_feed=None, frame_encoder=None, overlap_decode: bool = False,
                     rope_limit: Optional[int] = None):
        """An open-length `stream`: a `live.LiveSession`, an iterator that yields what `stream` yields per chunk and goes on
        until `pose_feed` or `noise_feed` ends or the caller closes it.  See live.py."""
        from .live import LiveSession
        return LiveSession(self, text_prompts, latent_size, batch_size=batch_size, noise_feed=noise_feed, generator=generator,
                           input_image=input_image, random_ref_dwpose=random_ref_dwpose, pose_feed=pose_feed, frame_encoder=frame_encoder,
                           overlap_decode=overlap_decode, rope_limit=rope_limit)

    # ------------------------------------------------------------------------------------------
    def _cache_tokens(self, total_frames: Optional[int] = None) -> int:
        """Cache capacity in tokens.  The reference uses 32760 (= 21 frames x 1560) or
        local_attn_size x 1560 (causal_inference.py:283-288); here: frames x tokens-per-frame of the
        actual latent, never less than what the rollout needs."""
        if self.local_attn_size != -1:
            return self.local_attn_size * self.frame_seq_length
        frames = max(21, total_frames or 0)
        return frames * self.frame_seq_length

    def _initialize_kv_cache(self, batch_size, dtype, device, cache_tokens: Optional[int] = None):
        """Per-GPU KV cache, same dict schema as causal_inference.py:278-298.  The 2 x L index
        tensors are views of one [L, 2] buffer so one fill updates them all."""
        shape = self.generator.model.shape
        if cache_tokens is None:
            cache_tokens = self._cache_tokens()
        self.kv_cache1 = new_kv_cache(shape, self.num_transformer_blocks, batch_size, cache_tokens, dtype, device)

    def _reset_kv_indices(self):
        reset_kv_indices(self.kv_cache1)

    def _initialize_crossattn_cache(self, batch_size, dtype, device):
        """causal_inference.py:300-312."""
        shape = self.generator.model.shape
        self.crossattn_cache = new_crossattn_cache(shape, self.num_transformer_blocks, batch_size, dtype, device)
