"""The pose front end in pieces on the GPU.  Everything here is bit equality with the whole-clip
path of the same build, which the golden tests of test_gpu_pose.py pin to the reference: the window mode of the
convolution against the whole-volume kernel, a pushed clip against `embed` for several partitions, dtypes and push
sizes, and `stream(pose_feed=...)` against `stream(dwpose_data=...)`."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import ops, pose_weights as pw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = [1000, 750, 500, 250]
LAT_H, LAT_W = 8, 12                      # the latent size of test_gpu_pose.py: 64 x 96 pose frames, 4 x 6 tokens per frame


@pytest.fixture(scope="module")
def embedder():
    return sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=DEV)


# ======================================================================================================== the kernel
T_IN, H_IN, W_IN = 11, 20, 24             # partial bricks in h and w for both spatial strides; bricks of 4 and of 2 frames
CONFIGS = {"8ch-s11": (0, 1, 1), "16ch-s11": (2, 1, 1), "16ch-s12": (6, 1, 2), "16ch-s22": (8, 2, 2)}      # Sequential index, stride_t, stride_s


@pytest.fixture(scope="module", params=list(CONFIGS), ids=list(CONFIGS))
def layer(request):
    """The layer's packed weights, a random input volume and the whole-volume kernel's output, computed once."""
    idx, st, ss = CONFIGS[request.param]
    sd = pw.synth_pose_state_dict(11)
    w, b = sd[f"dwpose_embedding.{idx}.weight"].to(torch.bfloat16), sd[f"dwpose_embedding.{idx}.bias"]
    cin = w.shape[1]
    cs = 8 if cin == 3 else 16
    g = torch.Generator().manual_seed(idx)
    x = torch.zeros(T_IN, H_IN, W_IN, cs, dtype=torch.bfloat16)
    x[..., :cin] = torch.rand(T_IN, H_IN, W_IN, cin, generator=g).to(torch.bfloat16) if cin == 3 else F.silu(torch.randn(T_IN, H_IN, W_IN, cin, generator=g)).to(torch.bfloat16)
    wp, bp = pw.repack_pose_conv(w.float(), cs).to(torch.bfloat16).to(DEV), pw.pad_pose_bias(b).to(DEV)
    x = x.to(DEV)
    whole = ops.pose_conv(x, wp, bp, 16, kt=3, stride_t=st, stride_s=ss, silu=True)
    torch.cuda.synchronize()
    assert whole.shape[0] == (T_IN if st == 1 else 6)
    return SimpleNamespace(x=x, wp=wp, bp=bp, st=st, ss=ss, whole=whole, To=whole.shape[0])


def window(L, lo, hi, x_lo, x_hi, t_end, closed, poison_front=0):
    """Output frames [lo, hi) from a copy of input frames [x_lo, x_hi) alone (`poison_front` more frames of NaN in front of
    them, standing for the frames in front of the clip, which must never be read)."""
    xs = L.x[max(x_lo, 0):x_hi].clone()
    if poison_front:
        xs = torch.cat([torch.full((poison_front,) + tuple(xs.shape[1:]), float("nan"), dtype=xs.dtype, device=xs.device), xs])
    return ops.pose_conv_window(xs.contiguous(), L.wp, L.bp, 16, x_lo - poison_front, t_end, closed, lo, hi - lo, stride_t=L.st, stride_s=L.ss, silu=True)


def reads(L, lo, hi, t_end):
    """The in-range input frames output frames [lo, hi) read."""
    return max(lo * L.st - 1, 0), min((hi - 1) * L.st + 2, t_end)


def test_window_kernel_equals_the_whole_volume_kernel(layer):
    L = layer
    cases = [("clip start", 0, 3, False), ("middle", 3, min(8, L.To), L.st == 2), ("clip end", L.To - 2, L.To, True)]
    if L.st == 2:
        cases += [("odd start", 1, 4, False), ("even start", 2, 5, False)]
    for name, lo, hi, closed in cases:
        x_lo, x_hi = reads(L, lo, hi, T_IN)
        # open: the timeline is known up to the window's end and no further; closed: it ends where the clip does
        out = window(L, lo, hi, x_lo, x_hi, T_IN if closed else x_hi, closed)
        assert out.shape == L.whole[lo:hi].shape and torch.equal(out, L.whole[lo:hi]), name
    # as the sequencer calls it: two history frames in front, which lie in front of the clip on the first push
    out = window(L, 0, 3, 0, reads(L, 0, 3, T_IN)[1], T_IN, False, poison_front=2)
    assert torch.equal(out, L.whole[:3])
    # ... and a window wider than the outputs need, with the clip's end inside it
    out = window(L, 1, L.To, 0, T_IN, T_IN, True)
    assert torch.equal(out, L.whole[1:])
    # the whole volume through the window entry point
    out = ops.pose_conv_window(L.x, L.wp, L.bp, 16, 0, T_IN, True, 0, L.To, stride_t=L.st, stride_s=L.ss, silu=True)
    assert torch.equal(out, L.whole)
    assert not torch.isnan(L.whole.float()).any() and L.whole.float().abs().max() > 0.1


# ======================================================================================================== the stream
F_CLIP, H_CLIP, W_CLIP = 25, 64, 96       # 7 latent frames of 4 x 6 tokens
FS = 24
PARTITIONS = [[25], [1] * 25, [5, 4, 4, 4, 4, 4], [13, 12], [3, 7, 2, 13]]


@pytest.fixture(scope="module")
def clip():
    return pw.synth_pose_clip(7, F_CLIP, H_CLIP, W_CLIP, "dense")


@pytest.fixture(scope="module")
def whole_tokens(embedder, clip):
    tokens, fhw = embedder.embed(clip)
    torch.cuda.synchronize()
    assert fhw == (7, 4, 6) and tokens.shape == (1, 7 * FS, 5120)
    return tokens.clone()


def run_stream(stream, clip, parts):
    rows, P = [], 0
    for n in parts:
        tokens, m = stream.push(clip[:, P:P + n])
        P += n
        assert stream.frames_pushed == P and stream.latent_frames_done == max(0, (P - 1) // 4) and tokens.shape == (1, m * FS, 5120)
        rows.append(tokens)
    tokens, m = stream.close()
    rows.append(tokens)
    return torch.cat(rows, dim=1)


@pytest.mark.parametrize("parts", PARTITIONS, ids=lambda p: "-".join(map(str, p[:6])))
def test_any_partition_gives_the_whole_clips_bits(embedder, clip, whole_tokens, parts):
    stream = embedder.open_stream(H_CLIP, W_CLIP)
    assert stream.hw == (4, 6) and (stream.h, stream.w) == (4, 6)
    out = run_stream(stream, clip, parts)
    assert stream.latent_frames_done == 7 and stream.closed
    assert out.shape == whole_tokens.shape and torch.equal(out, whole_tokens)
    with pytest.raises(RuntimeError, match="closed"):
        stream.push(clip[:, :1])
    with pytest.raises(RuntimeError, match="closed"):
        stream.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_other_input_dtypes(embedder, clip, whole_tokens, dtype):
    c = clip.to(dtype)
    want = embedder.embed(c)[0].clone()
    assert torch.equal(want, whole_tokens)                      # 0..255 are exact in bf16
    assert torch.equal(run_stream(embedder.open_stream(H_CLIP, W_CLIP), c, [3, 7, 2, 13]), want)


def test_push_sizes_outputs_and_embed_long(embedder, clip, whole_tokens):
    # a push larger than max_frames_per_push is split inside
    assert torch.equal(run_stream(embedder.open_stream(H_CLIP, W_CLIP, max_frames_per_push=4), clip, [25]), whole_tokens)
    tokens, fhw = embedder.embed_long(clip, 12)
    assert fhw == (7, 4, 6) and torch.equal(tokens, whole_tokens)
    assert torch.equal(embedder.embed_long(clip, 5)[0], whole_tokens)
    # rows written straight into the caller's buffer, from a row offset
    buf = torch.zeros(1, 9 * FS, 5120, dtype=torch.bfloat16, device=DEV)
    s = embedder.open_stream(H_CLIP, W_CLIP)
    view, m = s.push(clip[:, :14], out=buf, out_row=FS)
    assert m == 3 and view.data_ptr() == buf[:, FS:].data_ptr() and view.shape == (1, 3 * FS, 5120)
    view, m = s.push(clip[:, 14:], out=buf, out_row=4 * FS)
    view, m = s.close(out=buf, out_row=(1 + s.latent_frames_done) * FS)
    assert m == 1 and torch.equal(buf[:, FS:8 * FS], whole_tokens) and buf[:, :FS].abs().sum() == 0 and buf[:, 8 * FS:].abs().sum() == 0
    with pytest.raises(ValueError, match="do not fit"):
        embedder.open_stream(H_CLIP, W_CLIP).push(clip[:, :9], out=buf, out_row=8 * FS)
    with pytest.raises(ValueError, match=r"\[3, n, 64, 96\]"):
        embedder.open_stream(H_CLIP, W_CLIP).push(clip[:, :9, :32])
    with pytest.raises(ValueError, match="before its first frame"):
        embedder.open_stream(H_CLIP, W_CLIP).close()
    # a clip that ends off the 4k + 1 grid: 10 frames give 4 latent frames, as `embed` says
    short = clip[:, :10].contiguous()
    assert torch.equal(run_stream(embedder.open_stream(H_CLIP, W_CLIP), short, [4, 6]), embedder.embed(short)[0])
    one = clip[:, :1].contiguous()
    assert torch.equal(run_stream(embedder.open_stream(H_CLIP, W_CLIP), one, [1]), embedder.embed(one)[0])


def test_two_streams_do_not_disturb_each_other(embedder, clip, whole_tokens):
    other = pw.synth_pose_clip(8, F_CLIP, H_CLIP, W_CLIP, "skeleton")
    want_other = embedder.embed(other)[0].clone()
    a, b = embedder.open_stream(H_CLIP, W_CLIP), embedder.open_stream(H_CLIP, W_CLIP)
    rows_a, rows_b = [], []
    for i in range(0, F_CLIP, 5):
        rows_a.append(a.push(clip[:, i:i + 5])[0])
        rows_b.append(b.push(other[:, i:i + 5])[0])
    rows_b.append(b.close()[0])
    rows_a.append(a.close()[0])
    assert torch.equal(torch.cat(rows_a, dim=1), whole_tokens) and torch.equal(torch.cat(rows_b, dim=1), want_other)
    assert not torch.equal(want_other, whole_tokens)


# ======================================================================================================== the pipeline
class Feed:
    """An iterator over a clip's pieces that counts how many were asked for."""

    def __init__(self, clip, size=1):
        self.pieces, self.pulled = list(clip.split(size, dim=1)), 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.pulled == len(self.pieces):
            raise StopIteration
        self.pulled += 1
        return self.pieces[self.pulled - 1]


def test_stream_takes_a_pose_feed(embedder):
    shape = sfa.WAN_REDUCED
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0, pose=True), timestep_shift=5.0, is_causal=True, device=DEV)
    g = torch.Generator().manual_seed(91)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(DEV)      # noqa: E731
    noise, pe = bf(1, 6, 16, LAT_H, LAT_W), bf(1, 512, shape.text_dim)
    eps = [bf(3, 16, LAT_H, LAT_W) for _ in range(6)]
    clip = pw.synth_pose_clip(92, 21, 8 * LAT_H, 8 * LAT_W, "skeleton")           # 4 (6 - 1) + 1 pose frames: 6 latent frames, two chunks of 3
    image = pw.synth_pose_image(93, 8 * LAT_H, 8 * LAT_W, "skeleton")
    assert pw.pose_plan(*clip.shape[1:]) == (6, LAT_H // 2, LAT_W // 2)
    args = SimpleNamespace(denoising_step_list=STEPS, warp_denoising_step=True, independent_first_frame=False, num_frame_per_block=3, context_noise=0)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=sfa.IdentityVAE(), pose_embedder=embedder)

    def run(**kw):
        q = list(eps)
        pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
        return pipe.stream(noise, ["p"], **kw)

    for pairing in (True, False):
        pipe.pair_context_with_next = pairing
        want = [c[1].clone() for c in run(dwpose_data=clip, random_ref_dwpose=image)]
        assert len(want) == 2
        # a feed of exactly 4 (f - 1) + 1 frames: chunk 1 is computed after the feed's end has closed the clip
        feed = Feed(clip)
        for k, lat, _ in run(pose_feed=feed):
            assert feed.pulled <= 12 * k + 13, (k, feed.pulled)                   # nothing pulled ahead of chunk k's need
            assert torch.equal(lat, want[k]), (pairing, k)
        assert k == 1 and feed.pulled == 21
        # a longer clip behind the same 21 frames: chunk 1 waits for 25 frames instead, and its last latent frame hears them
        longer = torch.cat([clip, pw.synth_pose_clip(94, 8, 8 * LAT_H, 8 * LAT_W, "dense")], dim=1)
        feed = Feed(longer)
        got = []
        for k, lat, _ in run(pose_feed=feed):
            assert feed.pulled <= 12 * k + 13
            got.append(lat.clone())
        assert feed.pulled == 25 and torch.equal(got[0], want[0]) and not torch.equal(got[1], want[1])
    plain = [c[1].clone() for c in run()]
    assert not torch.equal(plain[0], want[0])                                     # the tokens are live
    # pieces of any length
    got = [c[1].clone() for c in run(pose_feed=iter(clip.split([2, 9, 1, 9], dim=1)))]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # four frames short
    it = run(pose_feed=Feed(clip[:, :17]))
    assert torch.equal(next(it)[1], want[0])
    with pytest.raises(ValueError, match=r"pose_feed ended after 17 pose frames: latent frames 3..5 need 21 .*25"):
        next(it)
