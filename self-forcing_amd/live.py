"""Open-length generation: `CausalInferencePipeline.open_session`.

`stream(noise, ...)` fixes a clip's length with its `noise`.  A `LiveSession` runs the same chunk loop
(`CausalInferencePipeline._denoise_chunks`) over sources of no fixed length: noise comes chunk by chunk, pose frames from a
feed, and the session goes on until one of them ends or the caller closes it.  Three things keep it bounded:

  * the KV cache is the rolling one (`local_attn_size` frames, `sf_kv_evict`): a global-attention generator is refused;
  * the temporal RoPE positions, which the tables hold for 1024 frames only, are re-based: before a generator call that
    would need a position beyond `rope_limit` the cached keys are rotated back (`WanDiffusionWrapper.rebase_positions`,
    `sf_kv_rope_shift`) so that the oldest frame of the window stands at position 0 again.  Scores depend on
    pos_q - pos_k only, so this changes the latents by the rounding of the rotated keys and nothing else;
  * the pose tokens live in `PoseRows`, a buffer of a few chunks' rows that is reused as the session goes on.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .kvcache import read_indices
from .pose_weights import POSE_DIM, pose_stream_cap, pose_stream_plan

ROPE_TABLE_FRAMES = 1024      # rows of model.rope_tables: positions 0..1023


class PoseRows:
    """The pose tokens of the chunks in flight, in a buffer whose size does not depend on the session's length.

    Latent frames leave the `PoseStream` in order and are written one behind the other; `take` hands a chunk's frames out
    as a contiguous row range, in timeline order.  When the next push would run past the buffer's end, the frames not
    handed out yet (fewer than a chunk and a push) are copied to its front and writing goes on from there.  Rows that were
    handed out are never moved, and the buffer is long enough that the writes which follow reach them only after two further
    chunks were taken -- a chunk's `add_condition` is read by its own passes and, paired, while the next chunk is taken.
    Pieces are split into pushes of at most `PUSH_FRAMES` frames so that a push makes at most `PUSH_LATENT` frames final
    (`pose_weights.pose_stream_cap`); a piece is pulled from the feed only when a chunk's frames are not final yet."""
    PUSH_FRAMES = 8
    PUSH_LATENT = pose_stream_cap(6, PUSH_FRAMES)      # 4

    def __init__(self, stream, frame_seqlen: int, chunk_frames: int, feed, first_piece):
        self.stream, self.fs, self.n = stream, int(frame_seqlen), int(chunk_frames)
        self.frames = 3 * self.n + 2 * self.PUSH_LATENT
        self.buffer = torch.empty(1, self.frames * self.fs, POSE_DIM, dtype=torch.bfloat16, device=stream.embedder.device)
        self.feed, self.queue = feed, list(first_piece.split(self.PUSH_FRAMES, dim=1))
        self.first = 0        # the first latent frame not handed out yet ...
        self.slot = 0         # ... and where it lies (or will lie), in frames from the buffer's start
        self.copies = 0       # how often the waiting frames were moved to the front

    def _room(self, m: int) -> int:
        """The row where the next `m` latent frames go."""
        waiting = self.stream.latent_frames_done - self.first
        if self.slot + waiting + m > self.frames:
            assert waiting <= self.slot and waiting + m <= self.frames, "PoseRows: the buffer is too short for its own plan"
            if waiting:
                self.buffer[:, :waiting * self.fs].copy_(self.buffer[:, self.slot * self.fs:(self.slot + waiting) * self.fs])
            self.slot, self.copies = 0, self.copies + 1
        return (self.slot + waiting) * self.fs

    def take(self, first_frame: int, n: int) -> Optional[torch.Tensor]:
        """The rows [1, n * frame_seqlen, 5120] of latent frames [first_frame, first_frame + n), or None when the feed
        ended before they were final."""
        assert first_frame == self.first and n <= self.n, f"pose rows are taken in timeline order: frame {self.first} is next, not {first_frame}"
        st = self.stream
        while st.latent_frames_done < first_frame + n and not st.closed:
            if not self.queue:
                piece = next(self.feed, None)
                if piece is not None:
                    self.queue = list(piece.split(self.PUSH_FRAMES, dim=1))
            if self.queue:
                piece = self.queue.pop(0)
                m = pose_stream_plan(st.frames_pushed, piece.shape[1], False)[1][-1]
                st.push(piece, out=self.buffer, out_row=self._room(m))
            else:
                m = pose_stream_plan(st.frames_pushed, 0, True)[1][-1]
                st.close(out=self.buffer, out_row=self._room(m))
        if st.latent_frames_done < first_frame + n:
            return None
        rows = self.buffer[:, self.slot * self.fs:(self.slot + n) * self.fs]
        self.first, self.slot = self.first + n, self.slot + n
        return rows


class LiveSession:
    """An iterator over the chunks of one open-length generation: `(chunk_index, latents [B, f, C, H, W], pixels[, frames])`
    as `CausalInferencePipeline.stream` yields them.  It ends when `pose_feed` ends (the chunks its frames still serve are
    generated first), when `noise_feed` ends, or with `close()`, after which nothing more is enqueued.

    noise_feed: an iterable of [B, f, C, H, W] tensors, one per chunk (f = `num_frame_per_block`; 1 for the first chunk of an
    `independent_first_frame` pipeline); without one every chunk's noise is drawn with `torch.randn(..., generator=generator)`.
    pose_feed / random_ref_dwpose / input_image / frame_encoder / overlap_decode: as `stream`.
    rope_limit: the highest temporal position + 1 a generator call may use before the session re-bases (default and maximum:
    the tables' 1024); `rebases` lists the shifts made so far, in frames.

    Every chunk's context pass runs (paired with the next chunk's first pass where `stream` would pair): a session never
    knows that a chunk is its last one before the sources say so."""

    def __init__(self, pipe, text_prompts: List[str], latent_size, batch_size: int = 1, noise_feed=None, generator=None, input_image=None,
                 random_ref_dwpose=None, pose_feed=None, frame_encoder=None, overlap_decode: bool = False, rope_limit: Optional[int] = None):
        self.pipe = pipe
        model = pipe.generator.model
        window, sink, chunk = model.local_attn_size, model.sink_size, pipe.num_frame_per_block
        if window == -1:
            raise ValueError("open_session needs a rolling generator (local_attn_size > 0): with global attention (local_attn_size == -1) the "
                             "KV cache holds every frame of the clip, so it grows with the session and overflows at its capacity")
        if not 0 <= sink < window:
            raise ValueError(f"open_session: sink_size {sink} must leave room for a window in local_attn_size {window}")
        # After a re-base the window's frames stand at 0 .. window - sink - 1 and a call needs at most one chunk beyond the
        # newest of them (a pair's first pass rewrites a chunk that is already in the window)
        need = window - sink + chunk
        rope_limit = ROPE_TABLE_FRAMES if rope_limit is None else int(rope_limit)
        if rope_limit > ROPE_TABLE_FRAMES:
            raise ValueError(f"open_session: rope_limit {rope_limit} exceeds the RoPE tables' {ROPE_TABLE_FRAMES} positions")
        if rope_limit < need:
            raise ValueError(f"open_session: rope_limit {rope_limit} is too small: the window after a re-base ({window} - {sink} sink frames) "
                             f"and the chunk behind it ({chunk}) need {need} positions")
        height, width = (int(v) for v in latent_size)
        self.rope_limit, self.batch_size, self.latent_size = rope_limit, int(batch_size), (height, width)
        self.rebases: List[int] = []
        self.closed = False
        device = pipe.device_
        conditional_dict, chunk_condition = pipe._begin_clip(text_prompts, self.batch_size, None, height, width, input_image=input_image,
                                                             random_ref_dwpose=random_ref_dwpose, pose_feed=pose_feed, live_chunk_frames=chunk)
        self.pose_rows = chunk_condition.live_rows if chunk_condition is not None else None
        dtype = torch.bfloat16
        pipe._prepare_caches(self.batch_size, None, dtype, device)
        channels = getattr(getattr(model, "shape", None), "out_dim", 16)
        lengths = {chunk, 1} if pipe.independent_first_frame else {chunk}

        def noise_chunks():
            feed = iter(noise_feed) if noise_feed is not None else None
            k = 0
            while True:
                f = 1 if pipe.independent_first_frame and k == 0 else chunk
                want = (self.batch_size, f, channels, height, width)
                if feed is not None:
                    x = next(feed, None)
                    if x is None:
                        return
                    if tuple(x.shape) != want:
                        raise ValueError(f"noise_feed: chunk {k} must be {want}, got {tuple(x.shape)}")
                    x = x.to(device=device, dtype=dtype)
                elif generator is not None:
                    x = torch.randn(want, generator=generator, device=generator.device, dtype=dtype).to(device)
                else:
                    x = torch.randn(want, device=device, dtype=dtype)
                yield x
                k += 1

        chunks = pipe._denoise_chunks(noise_chunks(), conditional_dict, lengths, 0, False, chunk_condition=chunk_condition, rebase=self._rebase)
        self._out = pipe._decoded_chunks(chunks, device, overlap_decode, frame_encoder)

    def _rebase(self, need: int) -> int:
        """Asked before every generator call with the highest position + 1 it needs; re-bases when that exceeds `rope_limit`
        and returns the shift in frames (0: none).  The shift is the position of the oldest cached frame behind the sink."""
        if need <= self.rope_limit:
            return 0
        pipe = self.pipe
        fs, sink = pipe.frame_seq_length, pipe.generator.model.sink_size
        global_end, local_end = read_indices(pipe.kv_cache1)
        delta = global_end // fs - max(0, local_end // fs - sink)
        if delta < 1 or need - delta > self.rope_limit:
            raise RuntimeError(f"live session: a call needs position {need} of {self.rope_limit} and a re-base by {delta} frames does not make "
                               f"room (global_end={global_end}, local_end={local_end}, frame_seqlen={fs})")
        pipe.generator.rebase_positions(pipe.kv_cache1, delta, fs)
        self.rebases.append(delta)
        return delta

    def __iter__(self):
        return self

    def __next__(self):
        if self.closed:
            raise StopIteration
        try:
            return next(self._out)
        except StopIteration:
            self.closed = True
            raise

    def close(self) -> None:
        """End the session: nothing more is pulled from the sources or enqueued."""
        self.closed = True
        self._out.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
