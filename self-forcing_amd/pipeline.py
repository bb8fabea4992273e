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
and messages are those of `CausalDiffusionInferencePipeline`: both take them from `conditioning.Conditioning`, and what the
two pipelines are beyond their loops from `rollout_base.RolloutBase`.  With none of these arguments nothing changes.

Open length: `open_session(...)` returns a `live.LiveSession`, `stream` without a fixed frame count -- the
same chunk loop (`_denoise_chunks` takes its chunks from a source) over noise drawn chunk by chunk, a rolling KV cache, re-based
RoPE positions and a bounded pose-token buffer, until the pose feed or the noise feed ends or the caller closes it.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

from .conditioning import Conditioning
from .rollout_base import RolloutBase, chunk_plan


class CausalInferencePipeline(RolloutBase):
    _device_field = "device_"
    _cache_sets = (("kv_cache1", "crossattn_cache"),)

    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, image_encoder=None, pose_embedder=None):
        super().__init__(args, device, generator, text_encoder, vae, image_encoder, pose_embedder)
        self.conditioner = None      # i2v_condition.I2VConditioner, built on the first inference with an image
        self.scheduler = self.generator.get_scheduler()
        self.denoising_step_list = torch.tensor(args.denoising_step_list, dtype=torch.long)
        if args.warp_denoising_step:
            timesteps = torch.cat((self.scheduler.timesteps.cpu(), torch.tensor([0], dtype=torch.float32)))
            self.denoising_step_list = timesteps[1000 - self.denoising_step_list]
        # re-noise source; the reference calls torch.randn_like (causal_inference.py:208).  Tests and
        # the CPU-baseline comparison inject pre-drawn tensors here so both sides consume the same eps.
        self.noise_source: Optional[Callable[[torch.Tensor], torch.Tensor]] = None
        self.last_profile = None
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
    def _conditioner(self):
        if self.conditioner is None:
            from .i2v_condition import I2VConditioner
            self.conditioner = I2VConditioner(self.vae, self._image_encoder(), device=self.device_)
        return self.conditioner

    def _begin_clip(self, text_prompts, batch_size, num_frames, height, width, **conditioning):
        """A clip's conditions: (the condition dict of its passes, its `Conditioning` or None when there is none
        beyond the prompt).  `num_frames`: the latent frames of the output timeline, None for an open-length session."""
        self.frame_seq_length = (height // 2) * (width // 2)
        cond = Conditioning(self, self._conditioner, batch_size, num_frames, height, width, **conditioning)
        conditional_dict = self.text_encoder(text_prompts=text_prompts)
        if not cond.active:
            return conditional_dict, None
        return dict(conditional_dict, **cond.clip_entries), cond

    def inference(self, noise: torch.Tensor, text_prompts: List[str], initial_latent: Optional[torch.Tensor] = None,
                  return_latents: bool = False, profile: bool = False, low_memory: bool = False, input_image=None,
                  dwpose_data: Optional[torch.Tensor] = None, random_ref_dwpose: Optional[torch.Tensor] = None,
                  dwpose_data_emb: Optional[torch.Tensor] = None):
        """noise [B, F, C, H, W] -> video in [0, 1] (and the latents)."""
        batch_size, num_frames, num_channels, height, width = noise.shape
        num_input_frames = initial_latent.shape[1] if initial_latent is not None else 0
        warm_up_frames, all_num_frames = chunk_plan(num_frames, num_input_frames, self.independent_first_frame, self.num_frame_per_block)
        num_output_frames = num_frames + num_input_frames
        conditional_dict, chunk_condition = self._begin_clip(
            text_prompts, batch_size, num_output_frames, height, width, input_image=input_image, dwpose_data=dwpose_data,
            random_ref_dwpose=random_ref_dwpose, dwpose_data_emb=dwpose_data_emb)

        output = torch.zeros([batch_size, num_output_frames, num_channels, height, width], device=noise.device, dtype=noise.dtype)

        if profile:
            ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
            init_start, init_end, diffusion_start, diffusion_end, vae_start, vae_end = ev(), ev(), ev(), ev(), ev(), ev()
            block_events = []
            init_start.record()

        # Step 1: (re)initialise the caches (causal_inference.py:111-132)
        self._prepare_caches(batch_size, num_output_frames, noise.dtype, noise.device)

        # Step 2: cache the context frames (causal_inference.py:134-169)
        current_start_frame = 0
        timestep = torch.zeros([batch_size, 1], device=noise.device, dtype=torch.int64) if warm_up_frames else None
        for n in warm_up_frames:
            ref = initial_latent[:, current_start_frame:current_start_frame + n]
            output[:, current_start_frame:current_start_frame + n] = ref
            if chunk_condition is not None:
                conditional_dict.update(chunk_condition.chunk(current_start_frame, n, warm_up=True))
            self.generator(noisy_image_or_video=ref, conditional_dict=conditional_dict, timestep=timestep,
                           kv_cache=self.kv_cache1, crossattn_cache=self.crossattn_cache,
                           current_start=current_start_frame * self.frame_seq_length, **self._cache_only_kw)
            current_start_frame += n

        if profile:
            init_end.record()
            diffusion_start.record()

        # Step 3: temporal denoising loop (causal_inference.py:176-244)
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
        `chunk_condition` (the clip's `Conditioning`): its `chunk` is asked once per chunk, right before the chunk's first pass, for the chunk's
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
                entries = next_entries if next_entries is not None else chunk_condition.chunk(current_start_frame, current_num_frames)
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
                        next_entries = chunk_condition.chunk(current_start_frame + current_num_frames, current_num_frames)
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
        all_num_frames = chunk_plan(num_frames, 0, self.independent_first_frame, self.num_frame_per_block)[1]
        conditional_dict, chunk_condition = self._begin_clip(
            text_prompts, batch_size, num_frames, height, width, input_image=input_image, dwpose_data=dwpose_data,
            random_ref_dwpose=random_ref_dwpose, dwpose_data_emb=dwpose_data_emb, pose_feed=pose_feed)
        self._prepare_caches(batch_size, num_frames, noise.dtype, noise.device)
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
