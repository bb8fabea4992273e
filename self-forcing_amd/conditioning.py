"""A clip's conditioning beyond the prompt -- image (`clip_feature`, `y`) and pose (`add_condition`) -- for both pipelines
(DESIGN.md section 17).

    cond = Conditioning(pipe, y_source, batch_size, num_frames, height, width, input_image=..., dwpose_data=..., ...)
    cond.clip_entries                       # the entries of the condition dict that hold for the whole clip
    cond.chunk(first_frame, n)              # the entries of the pass(es) over latent frames [first_frame, first_frame + n)

`y` comes from a source with `begin(image, height, width, random_ref_dwpose) -> clip_feature` and `frames(n)` -> the next n
latent frames: `i2v_condition.I2VConditioner` (chunk by chunk, the few-step rollout) or the many-step pipeline's slices of
`encode_image`'s whole-clip tensor.  Pose rows come from a source with `take(first, n)` -> the rows [1, n * tokens per frame,
5120] of latent frames [first, first + n): `ClipRows`, `EmbeddedRows`, `FeedRows`, or `live.PoseRows`, whose `take` returns
None once its feed has ended.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch

from .live import PoseRows
from .pose_weights import POSE_DIM, pose_plan

log = logging.getLogger(__name__)


class ClipRows:
    """A whole clip's token-major pose tokens [1, F * fs, 5120]: a chunk's rows are a row range, no copy."""

    def __init__(self, tokens, frame_seqlen: int):
        self.tokens, self.fs = tokens, frame_seqlen

    def take(self, first: int, n: int):
        return self.tokens[:, first * self.fs:(first + n) * self.fs]


class EmbeddedRows:
    """Already-embedded pose tokens [B, C_pose, F, h, w], sliced per chunk as causal_diffusion_inference.py:386-394 does."""

    def __init__(self, emb):
        self.emb = emb

    def take(self, first: int, n: int):
        return self.emb[:, :, first:first + n].permute(0, 2, 3, 4, 1).flatten(1, 3).contiguous()


class FeedRows(ClipRows):
    """A pose feed's rows in one buffer for the clip, filled as the feed delivers; a chunk's rows stay a row range of it."""

    def __init__(self, stream, frame_seqlen: int, num_frames: int, feed, first_piece):
        super().__init__(torch.empty(1, num_frames * frame_seqlen, POSE_DIM, dtype=torch.bfloat16, device=stream.embedder.device), frame_seqlen)
        self.stream, self.num_frames, self.feed, self.pending = stream, num_frames, feed, [first_piece]

    def take(self, first: int, n: int):
        """Pull pieces until latent frames [0, first + n) are final (4 (first + n) + 1 pixel frames in) or the feed ends, which
        closes the clip.  Nothing is pulled ahead of that."""
        st, upto = self.stream, first + n
        while st.latent_frames_done < upto and not st.closed:
            piece = self.pending.pop() if self.pending else next(self.feed, None)
            row = st.latent_frames_done * self.fs
            if piece is None:
                st.close(out=self.tokens, out_row=row)
            else:      # frames past 4 F + 1 belong to latent frames the noise does not have
                st.push(piece[:, :4 * self.num_frames + 1 - st.frames_pushed], out=self.tokens, out_row=row)
        if st.latent_frames_done < upto:
            raise ValueError(f"pose_feed ended after {st.frames_pushed} pose frames: latent frames {first}..{upto - 1} need "
                             f"{4 * upto - 3} when the clip ends with them ({4 * upto + 1} when it goes on)")
        return super().take(first, n)


class Conditioning:
    """Construction makes all checks, before any work, then the clip's work, once: the image through CLIP (`clip_feature`) with,
    under a pose, its reference-pose map for `y`; the pose clip embedded, or the feed's stream opened.  `y` itself is produced by
    `chunk`, in timeline order, one request per chunk.

    `y_source`: called for the source of `y` when the generator is i2v.  `num_frames`: the latent frames of the output timeline,
    None for an open-length session, which gives its chunk length as `live_chunk_frames`.  `pose_offset`: the clip's first latent
    frame in the pose timeline (the many-step pipeline's `start_frame_index`): the pose input covers `pose_offset + num_frames`
    frames and the rows of frame f of the clip are those of frame `pose_offset + f`.  `pose_feed` (an iterable of [3, n, H, W]
    pieces) replaces the pose clip: its first piece is taken with the checks, for its size, every further piece when `chunk`
    needs rows that are not final yet.  `active`: whether there is any conditioning at all."""

    def __init__(self, pipe, y_source, batch_size, num_frames, height, width, input_image=None, dwpose_data=None, random_ref_dwpose=None,
                 dwpose_data_emb=None, pose_feed=None, live_chunk_frames=None, pose_offset=0):
        is_i2v = getattr(getattr(getattr(pipe, "generator", None), "model", None), "model_type", "t2v") == "i2v"
        if input_image is not None and not is_i2v:
            raise NotImplementedError("input_image: this generator has no i2v branch (img_emb, k_img / v_img, the 36-channel patch "
                                      "embedding: model_type 'i2v'), so the rollout cannot consume an image" + pipe._no_i2v_hint)
        if is_i2v and input_image is None:
            raise ValueError("an i2v generator needs input_image: every pass takes its clip_feature and y")
        fs = (height // 2) * (width // 2)
        pose_frames = None if num_frames is None else pose_offset + num_frames
        if pose_feed is not None and (dwpose_data is not None or dwpose_data_emb is not None):
            raise ValueError("pass either pose_feed or a whole pose clip (dwpose_data / dwpose_data_emb), not both")
        use_pose = dwpose_data is not None and random_ref_dwpose is not None      # both, as the reference (:336)
        if use_pose:
            if dwpose_data_emb is not None:
                raise ValueError("pass either dwpose_data (with random_ref_dwpose) or dwpose_data_emb, not both")
            if dwpose_data.dim() != 4 or dwpose_data.shape[0] != 3:
                raise ValueError(f"dwpose_data must be one clip [3, F, H, W] (shared by the batch), got {tuple(dwpose_data.shape)}")
            # the pose tokens must cover the whole output timeline (:362-369); known from the shapes
            pose_fhw = pose_plan(*dwpose_data.shape[1:])
            assert pose_fhw[0] == pose_frames, (
                f"dwpose_data_emb has {pose_fhw[0]} frames, "
                f"but expected {pose_frames} to match the output timeline.")
            self._check_tokens_per_frame(pose_fhw[1], pose_fhw[2], height, width)
        elif pose_feed is None and (dwpose_data is not None or random_ref_dwpose is not None):
            log.warning("only one of dwpose_data / random_ref_dwpose was given: the pose branch needs both and is not taken")
        feed = feed_first = None
        if pose_feed is not None:
            feed = iter(pose_feed)
            feed_first = next(feed, None)
            if feed_first is None:
                raise ValueError("pose_feed is empty: chunk 0 needs its first pose frames")
            if feed_first.dim() != 4 or feed_first.shape[0] != 3 or feed_first.shape[1] < 1:
                raise ValueError(f"a pose_feed piece must be [3, n >= 1, H, W] (shared by the batch), got {tuple(feed_first.shape)}")
            self._check_tokens_per_frame(*pose_plan(1, *feed_first.shape[2:])[1:], height, width)
        if dwpose_data_emb is not None:
            assert dwpose_data_emb.shape[2] == pose_frames, (
                f"dwpose_data_emb has {dwpose_data_emb.shape[2]} frames, "
                f"but expected {pose_frames} to match the output timeline.")

        self.batch_size, self.pose_offset = batch_size, pose_offset
        self.active = is_i2v or use_pose or dwpose_data_emb is not None or feed is not None
        self.clip_entries = {}      # the entries of the condition dict that hold for the whole clip
        self.y_source = None        # begin() / frames(n): the clip's y, handed out in timeline order ...
        self.next_y_frame = 0       # ... up to this frame
        self.pose_rows = None       # take(first, n): the pose rows of latent frames [first, first + n)
        self.live_rows = None       # the `live.PoseRows` of an open-length session
        if is_i2v:
            self.y_source = y_source()
            ref_in_y = use_pose or (feed is not None and random_ref_dwpose is not None)
            if ref_in_y and getattr(self.y_source, "pose_embedder", None) is None:
                self.y_source.pose_embedder = pipe._pose_embedder()      # the image to be driven by the pose: its map goes into y
            # one image: the wrapper expands clip_feature to the batch
            self.clip_entries["clip_feature"] = self.y_source.begin(input_image, height * 8, width * 8, random_ref_dwpose if ref_in_y else None)
        if use_pose:
            self.pose_rows = ClipRows(pipe._pose_tokens(dwpose_data)[0], fs)      # [1, F'*h*w, 5120], once per clip
        elif dwpose_data_emb is not None:
            self.pose_rows = EmbeddedRows(dwpose_data_emb)
        elif feed is not None:
            stream = pipe._pose_embedder().open_stream(*feed_first.shape[2:])
            if num_frames is None:
                # open length: a bounded buffer that holds only the rows of the chunks in flight
                self.pose_rows = self.live_rows = PoseRows(stream, fs, live_chunk_frames, feed, feed_first)
            else:
                self.pose_rows = FeedRows(stream, fs, num_frames, feed, feed_first)

    @staticmethod
    def _check_tokens_per_frame(h, w, height, width):
        if h * w != (height // 2) * (width // 2):
            raise ValueError(f"dwpose_data gives {h}x{w} pose tokens per frame, the latents {height // 2}x{width // 2}. "
                             "Check pose data processing.")

    def chunk(self, first_frame: int, n: int, warm_up: bool = False) -> Optional[dict]:
        """The condition entries of the pass(es) over latent frames [first_frame, first_frame + n) of the clip, or None when
        an open-length feed has ended.  The context frames' passes (`warm_up`) take `y` only."""
        entries = {}
        if self.pose_rows is not None and not warm_up:
            # the rows first: a feed that has ended ends the session before anything of the chunk is encoded
            rows = self.pose_rows.take(self.pose_offset + first_frame, n)
            if rows is None:
                return None
            # one clip is shared by the batch: expanded
            entries["add_condition"] = rows.expand(self.batch_size, -1, -1).contiguous() if rows.shape[0] != self.batch_size else rows
        if self.y_source is not None:
            assert first_frame == self.next_y_frame, f"y is produced in timeline order: frame {self.next_y_frame} is next, not {first_frame}"
            self.next_y_frame += n
            entries["y"] = self.y_source.frames(n)
        return entries
