"""Host-side checks of the open-length session (no GPU): the argument checks of `sf_kv_rope_shift`, the reference definition's
own properties, the session's position bookkeeping against a stub generator that keeps the real cache plan, the bounded pose
buffer, and the refusals."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import kvcache, pose_weights as pw, rope_shift_reference as rr
from self_forcing_amd.model import rope_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 24          # 8 x 12 latents


# ============================================================================================== the C entry point
def test_kv_rope_shift_argument_checks():
    L = sfa._lib
    lib = L.lib()
    assert lib.sf_abi_version() == 11
    assert len(L.SIGNATURES["sf_kv_rope_shift"][1]) == 10
    p = 0x1000       # never dereferenced: every call below returns before any launch
    err = lambda: lib.sf_last_error().decode()      # noqa: E731
    assert lib.sf_kv_rope_shift(None, 1, 120, 4, 0, 120, p, p, 1, None) != 0 and "null" in err()
    assert lib.sf_kv_rope_shift(p, 1, 120, 4, 0, 120, None, p, 1, None) != 0 and "null" in err()
    assert lib.sf_kv_rope_shift(p, 1, 120, 4, 0, 120, p, None, 1, None) != 0 and "null" in err()
    for delta in (0, 1024, -1):
        assert lib.sf_kv_rope_shift(p, 1, 120, 4, 0, 120, p, p, delta, None) != 0 and "delta_frames" in err()
    for row0, rows in ((0, 121), (100, 21), (121, 0), (-1, 4), (0, -1)):
        assert lib.sf_kv_rope_shift(p, 1, 120, 4, row0, rows, p, p, 1, None) != 0 and "outside the cache" in err()
    assert lib.sf_kv_rope_shift(p, 0, 120, 4, 0, 120, p, p, 1, None) != 0 and lib.sf_kv_rope_shift(p, 1, 120, 0, 0, 120, p, p, 1, None) != 0
    assert lib.sf_kv_rope_shift(p, 1, 120, 4, 7, 0, p, p, 1, None) == 0          # no rows: nothing to do, nothing launched


# ============================================================================================== the reference definition
def test_reference_shifts_compose_and_leave_the_other_columns():
    cos, sin = rope_tables(128)
    g = torch.Generator().manual_seed(3)
    k = (torch.randn(2, 30, 4, 128, generator=g) * 3).bfloat16()
    for d0, d1 in ((1, 6), (4, 999), (500, 523)):
        two = rr.shift_keys(rr.shift_keys(k, cos, sin, d0), cos, sin, d1)
        one = rr.shift_keys(k, cos, sin, d0 + d1)
        assert torch.equal(two[..., 44:], k[..., 44:]) and torch.equal(one[..., 44:], k[..., 44:])
        # per element, of the pair's norm: two bf16 roundings on one side and one on the other (each at most 2^-8 of the norm, 2^-9 to 2^-8.5
        # for most elements) and the fp32 / table errors, far smaller: the bound of tests/test_gpu_live_session.py, on fixed inputs
        norm = torch.hypot(k[..., 0:44:2].float(), k[..., 1:44:2].float()).repeat_interleave(2, dim=-1)
        assert bool(((two[..., :44].float() - one[..., :44].float()).abs() <= 2.0 ** -7 * norm).all())
        assert not torch.equal(one[..., :44], k[..., :44])
    part = rr.shift_keys(k, cos, sin, 7, row0=5, rows=11)
    assert torch.equal(part[:, :5], k[:, :5]) and torch.equal(part[:, 16:], k[:, 16:])
    assert torch.equal(part[:, 5:16], rr.shift_keys(k, cos, sin, 7)[:, 5:16])
    for bad in (0, 1024):
        with pytest.raises(ValueError, match="delta_frames"):
            rr.shift_keys(k, cos, sin, bad)
    with pytest.raises(ValueError, match="outside the cache"):
        rr.shift_keys(k, cos, sin, 1, row0=25, rows=6)


def test_the_rotation_is_the_inverse_of_the_tables_own():
    """A pair rotated forward by the table's row p (what sf_qkv_norm_rope_cache stores) and back by row d stands where row p - d puts it."""
    cos, sin = rope_tables(128)
    p, d = 1000, 999
    a = torch.ones(1, 1, 1, 128, dtype=torch.float64)
    fwd = lambda pos: torch.stack((a[..., 0::2] * cos[pos].double() - a[..., 1::2] * sin[pos].double(),      # noqa: E731
                                   a[..., 0::2] * sin[pos].double() + a[..., 1::2] * cos[pos].double()), -1).flatten(-2)
    back = rr.shift_keys(fwd(p).bfloat16(), cos, sin, d)
    assert (back[..., :44].double() - fwd(p - d)[..., :44]).abs().max() < 2.0 ** -6 and torch.equal(back[..., 44:], fwd(p).bfloat16()[..., 44:])


# ============================================================================================== bookkeeping
class StubGenerator:
    """Keeps the cache indices as `WanDiffusionWrapper.forward` does (`plan_cache_update`) and records every call."""

    def __init__(self, window=3, sink=1, pair=True):
        self.model = SimpleNamespace(num_layers=2, local_attn_size=window, sink_size=sink, num_frame_per_block=1, model_type="t2v", shape=sfa.WAN_REDUCED)
        self.scheduler = sfa.FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.scheduler.add_noise = lambda x0, eps, t: x0 + 0 * eps
        self.calls, self.rebased, self.poses, self.frames, self.pair = [], [], [], [], pair

    def get_scheduler(self):
        return self.scheduler

    def _update(self, kv_cache, current_start, n_new):
        m, cap = self.model, kv_cache[0]["k"].shape[1]
        global_end, local_end = kvcache.read_indices(kv_cache)
        plan = kvcache.plan_cache_update(local_end, global_end, current_start, n_new, cap, m.local_attn_size, m.sink_size * FS, m.local_attn_size * FS)
        kvcache.write_indices(kv_cache, plan.global_end, plan.local_end)
        self.calls.append((current_start, n_new, plan, sum(self.rebased)))

    def forward(self, noisy_image_or_video, conditional_dict, timestep, kv_cache, crossattn_cache, current_start, cache_only=False):
        self._update(kv_cache, current_start, noisy_image_or_video.shape[1] * FS)
        self._pose(conditional_dict.get("add_condition"))
        return noisy_image_or_video, noisy_image_or_video * 0.5

    __call__ = forward

    def can_pair(self, conditional_dict):
        return self.pair

    def forward_pair(self, context_input, context_timestep, noisy, timestep, conditional_dict, kv_cache, crossattn_cache, context_start,
                     current_start, add_conditions=None):
        self._update(kv_cache, context_start, context_input.shape[1] * FS)
        self._update(kv_cache, current_start, noisy.shape[1] * FS)
        for a in add_conditions or (None, None):
            self._pose(a)
        return noisy, noisy * 0.5

    def _pose(self, a):
        """The pose rows of a pass, and -- read now, while the pass would read them -- the latent frames they hold (`FakeStream` writes
        a frame's index into its rows)."""
        self.poses.append(a)
        if a is not None:
            self.frames.append([int(v) for v in a[0, ::FS, 0]])

    def rebase_positions(self, kv_cache, delta_frames, frame_seqlen):
        assert 1 <= delta_frames <= 1023
        kvcache.shift_positions(kv_cache, delta_frames * frame_seqlen)
        self.rebased.append(delta_frames)


def make_pipeline(gen, nfpb=1, **kw):
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=nfpb, context_noise=0)
    return sfa.CausalInferencePipeline(args, "cpu", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": None}, vae=sfa.IdentityVAE(), **kw)


def run_session(rope_limit, pair, chunks=40):
    gen = StubGenerator(pair=pair)
    pipe = make_pipeline(gen)
    pipe.pair_context_with_next = pair
    noise = [torch.zeros(1, 1, 16, 8, 12) for _ in range(chunks)]
    session = pipe.open_session(["p"], (8, 12), noise_feed=noise, rope_limit=rope_limit)
    seen = [k for k, lat, pixels in session]
    assert seen == list(range(chunks)) and session.rebases == gen.rebased
    return gen, pipe


@pytest.mark.parametrize("pair", [True, False], ids=["paired", "single"])
def test_positions_stay_under_the_limit_and_plans_do_not_change(pair):
    limited, pipe = run_session(8, pair)
    free, pipe_free = run_session(1024, pair)
    assert free.rebased == [] and len(limited.calls) == len(free.calls)
    # no call needs a position >= 8 ...
    assert max((start + n) // FS for start, n, _, _ in limited.calls) <= 8 and max((start + n) // FS for start, n, _, _ in free.calls) == 40
    # ... and with the shifts added back every call stands where it stood and plans what it planned
    for (s0, n0, p0, shift), (s1, n1, p1, _) in zip(limited.calls, free.calls):
        assert s0 + shift * FS == s1 and n0 == n1
        assert (p0.evict, p0.keep, p0.sink, p0.local_end, p0.write_start, p0.attn_start) == (p1.evict, p1.keep, p1.sink, p1.local_end, p1.write_start, p1.attn_start)
        assert p0.global_end + shift * FS == p1.global_end
    diffs = lambda calls: [b[0] - a[0] for a, b in zip(calls, calls[1:])]      # noqa: E731
    moved = [i for i, (a, b) in enumerate(zip(diffs(limited.calls), diffs(free.calls))) if a != b]
    assert len(moved) == len(limited.rebased) and all(diffs(limited.calls)[i] == diffs(free.calls)[i] - 6 * FS for i in moved)
    # The window restarts at 0: a re-base moves the oldest frame behind the sink, at position g - 2 with the cache full, to 0.  The first
    # call that needs position 9 comes with 8 frames in the cache (chunk 7's pair, or chunk 8's first pass unpaired): a shift by 6, and
    # then every 6 chunks, while chunks follow: 6 re-bases in 40 chunks either way (chunks 7, 13, .. 37 / 8, 14, .. 38)
    assert limited.rebased == [6] * 6
    assert kvcache.read_indices(pipe.kv_cache1) == (40 * FS - 36 * FS, 3 * FS) and kvcache.read_indices(pipe_free.kv_cache1) == (40 * FS, 3 * FS)
    assert int(pipe.kv_cache1[1]["global_end_index"]) == 4 * FS and int(pipe.kv_cache1[1]["local_end_index"]) == 3 * FS


def test_shift_positions_moves_global_end_only():
    kv = kvcache.new_kv_cache(sfa.WAN_REDUCED, 2, 1, 3 * FS, torch.bfloat16, "cpu")
    kvcache.write_indices(kv, 7 * FS, 3 * FS)
    kvcache.shift_positions(kv, 5 * FS)
    assert kvcache.read_indices(kv) == (2 * FS, 3 * FS)
    assert all(int(d["global_end_index"]) == 2 * FS and int(d["local_end_index"]) == 3 * FS for d in kv)
    with pytest.raises(ValueError, match="cannot move"):
        kvcache.shift_positions(kv, 3 * FS)
    # a cache built the reference's way (plain per-layer tensors)
    foreign = [{"k": torch.zeros(1, 3 * FS, 1, 128), "global_end_index": torch.tensor([7 * FS]), "local_end_index": torch.tensor([3 * FS])} for _ in range(2)]
    kvcache.shift_positions(foreign, 5 * FS)
    assert all(int(d["global_end_index"]) == 2 * FS and int(d["local_end_index"]) == 3 * FS for d in foreign)


def test_close_runs_nothing_more():
    gen = StubGenerator()
    pipe = make_pipeline(gen)
    session = pipe.open_session(["p"], (8, 12), rope_limit=8)            # no feed at all: noise is drawn, the session is endless
    for k, lat, pixels in session:
        assert tuple(lat.shape) == (1, 1, 16, 8, 12) and lat.dtype == torch.bfloat16
        if k == 11:
            break
    calls = len(gen.calls)
    session.close()
    assert len(gen.calls) == calls and list(session) == [] and session.closed


def test_a_session_reuses_the_caches_of_a_clip_of_the_same_key():
    """`open_session` after an `inference` with the same batch size and cache capacity (a rolling cache's does not depend on the
    clip's length) keeps the cache tensors, clears `is_init` and resets the indices; another batch size allocates anew."""
    gen = StubGenerator()
    pipe = make_pipeline(gen)
    pipe.inference(torch.zeros(1, 5, 16, 8, 12), ["p"])
    kv, cross = pipe.kv_cache1, pipe.crossattn_cache
    tensors = [(d, d["k"], d["v"]) for d in kv + cross]
    assert kvcache.read_indices(kv) == (5 * FS, 3 * FS) and tuple(kv[0]["k"].shape[:2]) == (1, 3 * FS)
    for d in cross:
        d["is_init"] = True                                           # as the generator's first pass leaves it
    session = pipe.open_session(["p"], (8, 12), noise_feed=[torch.zeros(1, 1, 16, 8, 12)] * 2)
    assert pipe.kv_cache1 is kv and pipe.crossattn_cache is cross
    assert all(a is b for old, d in zip(tensors, kv + cross) for a, b in zip(old, (d, d["k"], d["v"])))
    assert not any(d["is_init"] for d in cross) and kvcache.read_indices(kv) == (0, 0)
    assert all(int(d["global_end_index"]) == 0 and int(d["local_end_index"]) == 0 for d in kv)
    gen.calls.clear()
    assert [k for k, lat, pixels in session] == [0, 1] and gen.calls[0][0] == 0 and kvcache.read_indices(kv) == (2 * FS, 2 * FS)
    session = pipe.open_session(["p", "q"], (8, 12), batch_size=2, noise_feed=[])
    assert pipe.kv_cache1 is not kv and pipe.crossattn_cache is not cross and pipe.kv_cache1[0]["k"].shape[0] == 2
    assert not any(d["is_init"] for d in pipe.crossattn_cache) and kvcache.read_indices(pipe.kv_cache1) == (0, 0)


# ============================================================================================== the pose buffer
class FakeStream:
    """Stand-in for `PoseStream` that follows the plan and writes the latent frame's index into the rows it is told to fill."""

    def __init__(self, embedder, H, W):
        self.embedder, self.frames_pushed, self.latent_frames_done, self.closed, self.sizes = embedder, 0, 0, False, []
        self.fs = (H // 16) * (W // 16)

    def _run(self, n, closing, out, out_row):
        m = pw.pose_stream_plan(self.frames_pushed, n, closing)[1][-1]
        assert out_row % self.fs == 0 and out_row + m * self.fs <= out.shape[1]
        for j in range(m):
            out[:, out_row + j * self.fs:out_row + (j + 1) * self.fs] = self.latent_frames_done + j
        self.frames_pushed, self.latent_frames_done, self.closed = self.frames_pushed + n, self.latent_frames_done + m, closing
        return out[:, out_row:out_row + m * self.fs], m

    def push(self, frames, out=None, out_row=0):
        self.sizes.append(frames.shape[1])
        return self._run(frames.shape[1], False, out, out_row)

    def close(self, out=None, out_row=0):
        return self._run(0, True, out, out_row)


class FakeEmbedder:
    device = torch.device("cpu")

    def open_stream(self, H, W, max_frames_per_push=16):
        self.stream = FakeStream(self, H, W)
        return self.stream


class Feed:
    def __init__(self, clip, size):
        self.pieces, self.pulled = list(clip.split(size, dim=1)), 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.pulled == len(self.pieces):
            raise StopIteration
        self.pulled += 1
        return self.pieces[self.pulled - 1]


@pytest.mark.parametrize("pair", [True, False], ids=["paired", "single"])
@pytest.mark.parametrize("piece", [1, 16, 50])
def test_pose_buffer_keeps_its_size_and_pulls_nothing_ahead(pair, piece):
    chunks, nfpb = 30, 3
    emb = FakeEmbedder()
    gen = StubGenerator(window=6, sink=0, pair=pair)
    pipe = make_pipeline(gen, nfpb=nfpb, pose_embedder=emb)
    pipe.pair_context_with_next = pair
    frames = 4 * (chunks * nfpb - 1) + 1                      # what serves 90 latent frames once the clip is closed
    feed = Feed(torch.zeros(3, frames, 64, 96, dtype=torch.uint8), piece)
    session = pipe.open_session(["p"], (8, 12), pose_feed=feed, rope_limit=16)
    rows = session.pose_rows
    size, ptr = tuple(rows.buffer.shape), rows.buffer.data_ptr()
    assert size == (1, (3 * nfpb + 2 * rows.PUSH_LATENT) * FS, 5120)
    for k, lat, pixels in session:
        need = min(12 * k + 13, frames)                     # chunk k's last frame is final one latent frame later, or at the clip's end
        assert feed.pulled == -(-need // piece) and need <= emb.stream.frames_pushed < need + rows.PUSH_FRAMES, (k, feed.pulled)
        assert tuple(rows.buffer.shape) == size and rows.buffer.data_ptr() == ptr
    assert k == chunks - 1 and emb.stream.closed and emb.stream.latent_frames_done == chunks * nfpb and max(emb.stream.sizes) <= rows.PUSH_FRAMES
    assert rows.copies >= 5 and len(session.rebases) > 0
    # every pass took its chunk's three frames, a contiguous row range of the buffer, and found them there when it ran: in the paired
    # loop chunk k's rows survive the pushes made for chunk k + 1
    assert len(gen.poses) == chunks * 5 and all(p is not None and tuple(p.shape) == (1, 3 * FS, 5120) for p in gen.poses)
    assert all(p.data_ptr() >= ptr and (p.data_ptr() - ptr) % (FS * 5120 * 2) == 0 for p in gen.poses)
    if not pair:
        want = [3 * (i // 5) for i in range(chunks * 5)]
    else:          # chunk 0: four passes; then per chunk (context of k, first pass of k + 1), three passes of k + 1; the last context alone
        want = [0] * 4
        for c in range(1, chunks):
            want += [3 * (c - 1), 3 * c] + [3 * c] * 3
        want += [3 * (chunks - 1)]
    assert gen.frames == [[f, f + 1, f + 2] for f in want]


# ============================================================================================== refusals
def test_refusals(tmp_path):
    gen = StubGenerator(window=-1, sink=0)
    with pytest.raises(ValueError, match="rolling generator.*global attention"):
        make_pipeline(gen).open_session(["p"], (8, 12))
    pipe = make_pipeline(StubGenerator())                 # window 3, sink 1, chunks of 1: 3 positions after a re-base
    with pytest.raises(ValueError, match="rope_limit 2 is too small"):
        pipe.open_session(["p"], (8, 12), rope_limit=2)
    with pytest.raises(ValueError, match="exceeds the RoPE tables"):
        pipe.open_session(["p"], (8, 12), rope_limit=1025)
    assert list(pipe.open_session(["p"], (8, 12), noise_feed=[], rope_limit=3)) == []
    with pytest.raises(ValueError, match="noise_feed: chunk 0 must be"):
        next(pipe.open_session(["p"], (8, 12), noise_feed=[torch.zeros(1, 2, 16, 8, 12)]))
    with pytest.raises(ValueError, match="pose_feed is empty"):
        make_pipeline(StubGenerator(), pose_embedder=FakeEmbedder()).open_session(["p"], (8, 12), pose_feed=iter([]))
    # the command line: no pose clip, and a config with global attention
    cfg = os.path.join(ROOT, "configs", "tiny_test_hotpath.yaml")
    base = [sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", cfg, "--data_path", "d", "--output_folder", str(tmp_path), "--open_length"]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode != 0 and "--open_length needs --pose_path" in r.stderr
