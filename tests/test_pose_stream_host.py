"""The pose front end in pieces, without a GPU: the push plan against a brute-force dependency walk
and against torch's own convolutions, the C plan against its Python mirror, the argument checks of the new entry points
with a null stream, the unchanged ABI, and the pipeline's early checks and pull order with stand-ins."""
import ctypes
import inspect
import random
from types import SimpleNamespace

import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import pose_weights as pw

ST = [s[0] for _, _, _, _, s, _, _ in pw.DWPOSE_LAYERS[:-1]]      # temporal strides of the six 3x3x3 layers
LEVELS = pw.POSE_LEVELS


# ------------------------------------------------------------------------------------------ the plan
def walk(P, closed):
    """Final frames per level by brute force: an output frame is final when each of its three taps is in front of the
    clip, known, or (clip closed) behind its end."""
    known = [P + pw.LEAD_FRAMES if P > 0 else 0]
    for st in ST:
        n_in = known[-1]
        total = (n_in - 1) // st + 1 if n_in > 0 else 0      # the layer's output size on a closed input of n_in frames
        t = 0
        while n_in > 0 and all(ti < 0 or ti < n_in or closed for ti in (t * st - 1, t * st, t * st + 1)) and (not closed or t < total):
            t += 1
        known.append(t)
    return known


@pytest.mark.parametrize("closed", [False, True])
def test_frontiers_match_a_brute_force_walk(closed):
    for P in range(0, 41):
        f = pw.pose_stream_frontier(P, closed)
        assert f == walk(P, closed), (P, closed)
        if P == 0:
            assert f == [0] * LEVELS
        elif closed:
            assert f[-1] == pw.pose_plan(P, 64, 96)[0] and f == [t for t, _, _ in pw.pose_layer_volumes(P, 64, 96)[:-1]]
        else:
            assert f[-1] == max(0, (P - 1) // 4)
            assert f == [P + 3, P + 2, P + 1, P, P - 1, (P - 1) // 2, (P - 1) // 2 // 2]


def check_push(before, n, closing):
    """One push: every in-range frame a computed output reads lies inside the window of 2 + new frames, the counts stay
    under the caps the scratch is sized for, and the C plan says the same."""
    first, count = pw.pose_stream_plan(before, n, closing)
    end = pw.pose_stream_frontier(before + n, closing)
    for i, st in enumerate(ST):
        lo, hi = first[i] - pw.HISTORY_FRAMES, first[i] + count[i]       # the window of the layer's input
        for t in range(first[i + 1], first[i + 1] + count[i + 1]):
            for ti in (t * st - 1, t * st, t * st + 1):
                if ti < 0:
                    continue
                if ti >= end[i]:
                    assert closing, (before, n, i, t, ti)                 # behind an open clip's frontier: must not be read
                    continue
                assert lo <= ti < hi, (before, n, closing, i, t, ti, lo, hi)
    assert all(0 <= c <= pw.pose_stream_cap(l, n) for l, c in enumerate(count)), (before, n, closing, count)
    plan = sfa._lib.PosePushPlan()
    assert sfa._lib.lib().sf_pose_stream_plan(before, n, int(closing), plan) == 0
    assert (list(plan.first), list(plan.count)) == (first, count)
    return first, count


def test_every_push_reads_inside_its_window_and_the_c_plan_agrees():
    for before in range(0, 41):
        for n in range(0, 18):
            for closing in (False, True):
                if closing and before + n == 0:
                    continue
                check_push(before, n, closing)
    with pytest.raises(ValueError, match="no frames"):
        pw.pose_stream_plan(0, 0, True)
    assert sfa._lib.lib().sf_pose_stream_plan(0, 0, 1, sfa._lib.PosePushPlan()) != 0 and b"clip of no frames" in sfa._lib.lib().sf_last_error()
    assert sfa._lib.lib().sf_pose_stream_plan(-1, 0, 0, sfa._lib.PosePushPlan()) != 0 and b"frames_before=-1" in sfa._lib.lib().sf_last_error()
    assert sfa._lib.lib().sf_pose_stream_plan(0, 1, 0, None) != 0 and b"null plan" in sfa._lib.lib().sf_last_error()


def test_random_partitions_of_33_frames_compose():
    rng = random.Random(18)
    for _ in range(50):
        parts, left = [], 33
        while left:
            parts.append(rng.randint(1, min(left, 9)))
            left -= parts[-1]
        P, front = 0, [0] * LEVELS
        for n in parts:
            first, count = check_push(P, n, False)
            assert first == front                                        # a push goes on where the last one stopped
            P += n
            front = [a + b for a, b in zip(first, count)]
            assert front == [P + 3, P + 2, P + 1, P, P - 1, (P - 1) // 2, (P - 1) // 2 // 2], (parts, P)
        first, count = check_push(P, 0, True)
        assert first == front and [a + b for a, b in zip(first, count)] == [t for t, _, _ in pw.pose_layer_volumes(33, 64, 96)[:-1]]
        assert first[-1] + count[-1] == pw.pose_plan(33, 64, 96)[0] == 9


def test_torch_convolutions_obey_the_dependency_rule():
    """fp64 nn.Conv3d built from the layer table, random weights, a 16 x 16 clip of 25 frames: replacing the frames from
    P on changes every latent frame the rule calls open and none it calls final."""
    torch.manual_seed(4)
    layers = []
    for _, cin, cout, k, s, p, act in pw.DWPOSE_LAYERS:
        layers.append(torch.nn.Conv3d(cin, min(cout, 32), k, stride=s, padding=p).double())     # 32 of the 5120 token channels: the rule is about time
        if act:
            layers.append(torch.nn.SiLU())
    net = torch.nn.Sequential(*layers)
    clip = torch.rand(3, 25, 16, 16, dtype=torch.float64) * 255
    with torch.no_grad():
        whole = net(pw.pose_input_torch(clip).double())
        assert whole.shape[2] == 7
        for P in (1, 2, 4, 5, 6, 8, 9, 12, 13, 16, 17, 21, 24):
            other = clip.clone()
            other[:, P:] = torch.rand(3, 25 - P, 16, 16, dtype=torch.float64) * 255
            out = net(pw.pose_input_torch(other).double())
            final = pw.pose_stream_frontier(P)[-1]
            assert final == max(0, (P - 1) // 4)
            same = [torch.equal(out[:, :, j], whole[:, :, j]) for j in range(7)]
            assert same == [j < final for j in range(7)], (P, same)
    # latent frame j reads pixel frames 4j - 10 .. 4j + 4: frame 3 is deaf to frames 0, 1 and 17 on, and hears 2 and 16
    with torch.no_grad():
        for f, hears in ((1, False), (2, True), (16, True), (17, False)):
            other = clip.clone()
            other[:, f] = 255 - other[:, f]
            assert torch.equal(net(pw.pose_input_torch(other).double())[:, :, 3], whole[:, :, 3]) != hears, f


# ------------------------------------------------------------------------------------------ the entry points
@pytest.fixture(scope="module")
def model():
    return sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device="cpu")


def conv_args(T=4, H=8, W=8, cin=16, st=1, ss=1):
    a = sfa._lib.PoseConvArgs()
    a.x, a.w, a.bias, a.out = 4096, 4096, 4096, 4096
    a.T, a.H, a.W, a.Cin, a.Cout, a.kt, a.stride_t, a.stride_s, a.ldw, a.ldo = T, H, W, cin, 16, 3, st, ss, 448 if cin == 16 else 224, 16
    return a


def test_window_convolution_rejects_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    err = lib.sf_last_error
    W = sfa._lib.PoseWindow
    assert lib.sf_pose_conv_window(None, None, None) != 0 and b"sf_pose_conv_window: null args" in err()
    assert lib.sf_pose_conv_window(sfa._lib.PoseConvArgs(), None, None) != 0 and b"null tensor" in err()
    assert lib.sf_pose_conv_window(conv_args(), None, None) != 0 and b"null window" in err()
    a = conv_args()
    a.x = 4100
    assert lib.sf_pose_conv_window(a, W(0, 4, 1, 0, 4), None) != 0 and b"misaligned" in err()
    a = conv_args()
    a.kt = 1
    assert lib.sf_pose_conv_window(a, W(0, 4, 1, 0, 4), None) != 0 and b"no kernel" in err()
    assert lib.sf_pose_conv_window(conv_args(), W(0, 0, 1, 0, 4), None) != 0 and b"malformed window" in err()
    assert lib.sf_pose_conv_window(conv_args(), W(0, 4, 1, 0, 0), None) != 0 and b"malformed window" in err()
    # x holds frames [3, 7) of a 20-frame timeline: outputs [4, 6) read [3, 7); [3, 5) read frame 2, [5, 7) frame 7
    assert lib.sf_pose_conv_window(conv_args(), W(3, 20, 1, 3, 2), None) != 0 and b"holds input frames [3, 7), output frames [3, 5) read [2, 6)" in err()
    assert lib.sf_pose_conv_window(conv_args(), W(3, 20, 1, 5, 2), None) != 0 and b"read [4, 8)" in err()
    # temporal stride 2: output frame 3 reads frames 5..7, x holds [6, 10)
    assert lib.sf_pose_conv_window(conv_args(st=2, ss=2), W(6, 20, 0, 3, 2), None) != 0 and b"read [5, 10)" in err()
    # an open timeline that ends at frame 7: output frame 6 would read frame 7; closed, frame 7 is padding but frame 8 does not exist
    assert lib.sf_pose_conv_window(conv_args(), W(3, 7, 0, 4, 3), None) != 0 and b"open timeline ends at 7" in err()
    assert lib.sf_pose_conv_window(conv_args(), W(3, 7, 1, 4, 4), None) != 0 and b"closed timeline of 7 frames" in err()
    # the 4 GiB limit is the window's, not the clip's: 340 frames of 480 x 832 x 32 B
    assert lib.sf_pose_conv_window(conv_args(T=340, H=480, W=832), W(0, 10000, 0, 1, 338), None) != 0 and b"exceeds the 4 GiB" in err()
    assert ctypes.sizeof(sfa._lib.PoseWindow) == 20 and ctypes.sizeof(sfa._lib.PosePushPlan) == 56


def test_stream_entry_points_reject_bad_arguments_without_touching_the_gpu(model):
    lib = sfa._lib.lib()
    err = lib.sf_last_error
    cm = ctypes.byref(model.cmodel)
    n_out = ctypes.c_int32(-1)
    wr = ctypes.byref(n_out)
    big = 1 << 40

    def push(m=cm, state=4096, before=0, frames=8192, dtype=0, n=4, H=64, W=96, closing=0, scratch=65536, nbytes=big, out=4096, cap=1 << 20, written=wr):
        return lib.sf_pose_stream_push(m, state, before, frames, dtype, n, H, W, closing, scratch, nbytes, out, cap, written, None)

    assert lib.sf_pose_stream_state_bytes(None, 64, 96) == 0 and b"null model" in err()
    assert lib.sf_pose_stream_scratch_bytes(None, 12, 64, 96) == 0 and b"null model" in err()
    empty = sfa._lib.PoseModel()
    assert lib.sf_pose_stream_state_bytes(empty, 64, 96) == 0 and b"no weights" in err()
    assert lib.sf_pose_stream_scratch_bytes(cm, -1, 64, 96) == 0 and b"n_max=-1" in err()
    assert lib.sf_pose_stream_scratch_bytes(cm, 12, 8, 8) == 0 and b"no tokens" in err()
    assert lib.sf_pose_stream_scratch_bytes(cm, 400, 720, 1280) == 0 and b"push fewer frames" in err()
    # two frames per layer input: 8 channels, three times 16 at full size, then 16 at half and at quarter size
    assert lib.sf_pose_stream_state_bytes(cm, 64, 96) == 2 * 2 * (64 * 96 * (8 + 3 * 16) + 32 * 48 * 16 + 16 * 24 * 16)
    small, large = lib.sf_pose_stream_scratch_bytes(cm, 1, 64, 96), lib.sf_pose_stream_scratch_bytes(cm, 12, 64, 96)
    assert 0 < small < large
    # a full-size push: no clip length enters, and the window of 12 frames is a fraction of the whole clip's scratch
    hd = lib.sf_pose_stream_scratch_bytes(cm, 12, 720, 1280)
    assert 0 < hd < 0.5 * model.scratch_bytes(84, 720, 1280)
    assert 0 < lib.sf_pose_stream_scratch_bytes(cm, 12, 480, 832) < 0.7e9
    assert "F" not in inspect.signature(sfa.PoseEmbedder.open_stream).parameters

    assert push(m=None) != 0 and b"null model" in err()
    assert push(state=None) != 0 and b"null buffer" in err()
    assert push(scratch=None) != 0 and b"null buffer" in err()
    assert push(written=None) != 0 and b"null buffer" in err()
    assert push(frames=None) != 0 and b"null buffer" in err()
    assert push(out=None, before=8) != 0 and b"tokens_out" in err()
    assert push(dtype=7) != 0 and b"dtype" in err()
    assert push(state=4100) != 0 and b"256-byte aligned" in err()
    assert push(scratch=65600) != 0 and b"256-byte aligned" in err()
    assert push(nbytes=small) != 0 and b"needed for a push of 4 frames" in err()
    assert push(n=0, closing=1) != 0 and b"cannot be closed" in err()
    assert push(before=-3) != 0 and b"frames_before=-3" in err()
    assert push(n=-1) != 0 and b"n=-1" in err()
    assert push(before=4, n=5, cap=4 * 6 * 2 - 1) != 0 and b"this push writes 2 x 4 x 6 = 48" in err()       # frames 0 and 1 are final with 9 frames in
    assert push(before=4, n=5, closing=1, cap=2 * 24) != 0 and b"writes 3 x 4 x 6 = 72" in err()
    assert push(H=8, W=8) != 0 and b"no tokens" in err()
    assert n_out.value == -1                                               # nothing was written on a refusal
    assert lib.sf_abi_version() == 11 == sfa._lib.ABI_VERSION


def test_python_stream_checks_without_a_gpu(model):
    sig = inspect.signature(sfa.PoseEmbedder.open_stream)
    assert list(sig.parameters) == ["self", "H", "W", "max_frames_per_push"] and sig.parameters["max_frames_per_push"].default == 16
    assert inspect.signature(sfa.PoseEmbedder.embed_long).parameters["frames_per_push"].default == 12
    assert list(inspect.signature(sfa.PoseStream.push).parameters) == ["self", "frames", "out", "out_row"]
    assert list(inspect.signature(sfa.PoseStream.close).parameters) == ["self", "out", "out_row"]
    with pytest.raises(ValueError, match="max_frames_per_push"):
        model.open_stream(64, 96, 0)
    with pytest.raises(ValueError, match="no tokens"):
        model.open_stream(8, 8)
    only_ref = {k: v for k, v in pw.synth_pose_state_dict(0).items() if k.startswith(pw.RANDOMREF_PREFIX)}
    with pytest.raises(RuntimeError, match="dwpose_embedding"):
        sfa.PoseEmbedder(only_ref, device="cpu").open_stream(64, 96)
    with pytest.raises(ValueError, match=r"\[3, F, H, W\]"):
        model.embed_long(torch.zeros(25, 64, 96))


# ------------------------------------------------------------------------------------------ the pipeline
class Generator:
    def __init__(self, model_type="t2v"):
        self.model = SimpleNamespace(num_layers=2, local_attn_size=-1, sink_size=0, num_frame_per_block=1, model_type=model_type, shape=sfa.WAN_REDUCED)
        self.scheduler = sfa.FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.scheduler.add_noise = lambda x0, eps, t: x0 + 0 * eps
        self.poses = []

    def get_scheduler(self):
        return self.scheduler

    def forward(self, noisy_image_or_video, conditional_dict, timestep, kv_cache, crossattn_cache, current_start, cache_only=False):
        self.poses.append(conditional_dict.get("add_condition"))
        return noisy_image_or_video, noisy_image_or_video * 0.5

    __call__ = forward


class FakeStream:
    """Stand-in for `PoseStream` that follows the plan and writes the latent frame's index into its rows."""

    def __init__(self, embedder, H, W):
        self.embedder, self.frames_pushed, self.latent_frames_done, self.closed, self.sizes = embedder, 0, 0, False, []
        self.fs = (H // 16) * (W // 16)

    def _run(self, n, closing, out, out_row):
        m = pw.pose_stream_plan(self.frames_pushed, n, closing)[1][-1]
        assert out_row == self.latent_frames_done * self.fs and out_row + m * self.fs <= out.shape[1]
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


def make_pipeline(nfpb=3, model_type="t2v", **kw):
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=nfpb, context_noise=0)
    gen = Generator(model_type)
    pipe = sfa.CausalInferencePipeline(args, "cpu", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": None},
                                       vae=sfa.IdentityVAE(), **kw)
    return pipe, gen


class Feed:
    """An iterator over a clip's pieces that counts how many were asked for."""

    def __init__(self, clip, sizes):
        self.pieces, self.pulled = list(clip.split(sizes, dim=1)), 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.pulled == len(self.pieces):
            raise StopIteration
        self.pulled += 1
        return self.pieces[self.pulled - 1]


def test_pipeline_early_checks():
    params = list(inspect.signature(sfa.CausalInferencePipeline.stream).parameters)
    assert params == ["self", "noise", "text_prompts", "skip_last_context", "overlap_decode", "frame_encoder", "input_image", "dwpose_data",
                      "random_ref_dwpose", "dwpose_data_emb", "pose_feed"]
    assert "pose_feed" not in inspect.signature(sfa.CausalInferencePipeline.inference).parameters
    pipe, _ = make_pipeline(pose_embedder=FakeEmbedder())
    noise = torch.zeros(1, 6, 16, 8, 12)
    clip, image = torch.zeros(3, 21, 64, 96, dtype=torch.uint8), torch.zeros(64, 96, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="pose_feed or a whole pose clip"):
        next(pipe.stream(noise, ["p"], dwpose_data=clip, random_ref_dwpose=image, pose_feed=iter([clip])))
    with pytest.raises(ValueError, match="pose_feed or a whole pose clip"):
        next(pipe.stream(noise, ["p"], dwpose_data=clip, pose_feed=iter([clip])))
    with pytest.raises(ValueError, match="pose_feed or a whole pose clip"):
        next(pipe.stream(noise, ["p"], dwpose_data_emb=torch.zeros(1, 5120, 6, 4, 6), pose_feed=iter([clip])))
    with pytest.raises(ValueError, match="gives 8x12 pose tokens per frame, the latents 4x6. Check pose data processing."):
        next(pipe.stream(noise, ["p"], pose_feed=iter([torch.zeros(3, 1, 128, 192, dtype=torch.uint8)])))
    with pytest.raises(ValueError, match="pose_feed is empty"):
        next(pipe.stream(noise, ["p"], pose_feed=iter([])))
    with pytest.raises(ValueError, match=r"\[3, n >= 1, H, W\]"):
        next(pipe.stream(noise, ["p"], pose_feed=iter([torch.zeros(64, 96, 3)])))


@pytest.mark.parametrize("sizes", [[1] * 25, [5, 4, 4, 4, 4, 4], [13, 12], [2, 9, 1, 7, 6]], ids=lambda s: "-".join(map(str, s[:6])))
def test_pipeline_pulls_no_piece_ahead_of_need(sizes):
    emb = FakeEmbedder()
    pipe, gen = make_pipeline(pose_embedder=emb)
    pipe.pair_context_with_next = False
    clip = torch.zeros(3, 25, 64, 96, dtype=torch.uint8)
    feed = Feed(clip, sizes)
    need = lambda k: next(i + 1 for i in range(len(sizes)) if sum(sizes[:i + 1]) >= 12 * k + 13)      # noqa: E731  pieces until 12k + 13 frames are in
    for k, lat, _ in pipe.stream(torch.zeros(1, 6, 16, 8, 12), ["p"], pose_feed=feed):
        assert feed.pulled == need(k) and emb.stream.frames_pushed <= 25, (k, feed.pulled)
    # every pass of chunk k took the rows of latent frames 3k .. 3k + 2, as a view of the one buffer
    assert len(gen.poses) == 4 + 1 + 4 and all(p.shape == (1, 72, 5120) for p in gen.poses)
    for i, p in enumerate(gen.poses):
        k = i // 5
        assert torch.equal(p[0, ::24, 0].float(), torch.tensor([3.0 * k, 3 * k + 1, 3 * k + 2]))
    assert gen.poses[0].data_ptr() == gen.poses[3].data_ptr() and gen.poses[5].data_ptr() == gen.poses[0].data_ptr() + 72 * 5120 * 2
    assert not emb.stream.closed and emb.stream.frames_pushed == 25


def test_pipeline_closes_the_clip_when_the_feed_ends():
    emb = FakeEmbedder()
    pipe, gen = make_pipeline(pose_embedder=emb)
    feed = Feed(torch.zeros(3, 21, 64, 96, dtype=torch.uint8), [1] * 21)         # 4 (6 - 1) + 1 frames: enough once the clip is closed
    chunks = list(pipe.stream(torch.zeros(1, 6, 16, 8, 12), ["p"], pose_feed=feed))
    assert [c[0] for c in chunks] == [0, 1] and emb.stream.closed and emb.stream.latent_frames_done == 6 and feed.pulled == 21
    # a longer feed than the noise: frames past 4 F + 1 are not pushed, whatever the piece size
    emb = FakeEmbedder()
    pipe, gen = make_pipeline(pose_embedder=emb)
    feed = Feed(torch.zeros(3, 48, 64, 96, dtype=torch.uint8), [16] * 3)
    assert len(list(pipe.stream(torch.zeros(1, 6, 16, 8, 12), ["p"], pose_feed=feed))) == 2
    assert emb.stream.sizes == [16, 9] and emb.stream.latent_frames_done == 6 and feed.pulled == 2
    # four frames short: chunk 1 cannot be conditioned
    emb = FakeEmbedder()
    pipe, gen = make_pipeline(pose_embedder=emb)
    feed = Feed(torch.zeros(3, 17, 64, 96, dtype=torch.uint8), [1] * 17)
    it = pipe.stream(torch.zeros(1, 6, 16, 8, 12), ["p"], pose_feed=feed)
    assert next(it)[0] == 0
    with pytest.raises(ValueError, match=r"pose_feed ended after 17 pose frames: latent frames 3..5 need 21 when the clip ends with them \(25 when it goes on\)"):
        next(it)


def test_with_an_image_the_reference_pose_still_goes_into_y():
    """An i2v generator with a feed: `random_ref_dwpose` reaches the conditioner (its map goes into `y`), `y` is asked for
    chunk by chunk as before, and the feed alone takes the pose branch."""
    class Conditioner:
        def __init__(self):
            self.begun, self.asked, self.pose_embedder = [], [], None

        def begin(self, image, height, width, random_ref_dwpose=None):
            self.begun.append(random_ref_dwpose is not None)
            return torch.zeros(1, 257, 320)

        def frames(self, n):
            self.asked.append(n)
            return torch.zeros(1, 20, n, 8, 12)

    for ref in (torch.zeros(64, 96, 3, dtype=torch.uint8), None):
        emb = FakeEmbedder()
        pipe, gen = make_pipeline(model_type="i2v", pose_embedder=emb)
        pipe.conditioner = cond = Conditioner()
        feed = Feed(torch.zeros(3, 21, 64, 96, dtype=torch.uint8), [1] * 21)
        chunks = list(pipe.stream(torch.zeros(1, 6, 16, 8, 12), ["p"], input_image=torch.zeros(3, 64, 96), random_ref_dwpose=ref, pose_feed=feed))
        assert len(chunks) == 2 and cond.begun == [ref is not None] and cond.asked == [3, 3]
        assert (cond.pose_embedder is emb) == (ref is not None) and all(p is not None and p.shape == (1, 72, 5120) for p in gen.poses)
