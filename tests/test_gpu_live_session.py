"""GPU tests of the open-length session: `sf_kv_rope_shift` against its reference bit for bit and against the rotating kernel, a
session against `stream()` on the golden `roll` scenario (plain, with a pose feed, with an image), re-based sessions against
the reference's latents, and a long run.  Reduced shapes (8 x 12 latents, 24 tokens per frame; the image test uses the 16 x 16
latents of test_gpu_fewstep_cond.py); run with `-m gpu`."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import clip_weights as cw, kvcache, ops, pose_weights as pw, rope_shift_reference as rr, vae_weights as vw
from self_forcing_amd.model import rope_tables

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAT_H, LAT_W = 8, 12
FS = (LAT_H // 2) * (LAT_W // 2)
TOL = 2e-2          # the project's bound of test_gpu_forward.py


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def tables():
    cos, sin = rope_tables(128)
    return cos, sin, cos.to(DEV), sin.to(DEV)


# ============================================================================================== 1. the kernel, bit for bit
def random_cache(B, S, H, seed):
    """Every finite bf16 bit pattern with equal probability (so +-0, subnormals and values up to 2^127 occur), and a few rows of
    nothing but zeros of both signs and subnormals."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(-32768, 32768, (B, S, H, 128), generator=g, dtype=torch.int32)
    raw = torch.where((raw & 0x7F80) == 0x7F80, raw & ~0x0080, raw)              # inf / NaN -> the binade below
    raw[:, 3] = torch.where(raw[:, 3] % 2 == 0, 0, -32768)                       # +0 / -0
    raw[:, 6] = raw[:, 6] & ~0x7F80                                              # subnormals (and zeros) of both signs
    raw[:, 9, :, 0::2] = 0x7F7F                                                  # the largest finite value beside anything
    return raw.to(torch.int16).view(torch.bfloat16)


@pytest.mark.parametrize("row0,rows", [(0, None), (5, 67)], ids=["all", "inner"])
@pytest.mark.parametrize("delta", [1, 7, 1023])
@pytest.mark.parametrize("H", [4, 40])
def test_kernel_equals_reference_bit_for_bit(tables, H, delta, row0, rows):
    cos, sin, dcos, dsin = tables
    B, S = 2, 5 * FS
    k = random_cache(B, S, H, 100 + H)
    v = random_cache(B, S, H, 200 + H)
    want = rr.shift_keys(k, cos, sin, delta, row0, rows)
    assert not bool(torch.isnan(want.float()).any())
    dk, dv = k.to(DEV), v.to(DEV)
    assert ops.kv_rope_shift(dk, dcos, dsin, delta, row0, rows) is dk
    torch.cuda.synchronize()
    got = dk.cpu()
    assert torch.equal(bits(got), bits(want))
    # what must not change did not, bit for bit: the other columns, the rows outside the range, V
    end = S if rows is None else row0 + rows
    assert torch.equal(bits(got[..., 44:]), bits(k[..., 44:]))
    assert torch.equal(bits(got[:, :row0]), bits(k[:, :row0])) and torch.equal(bits(got[:, end:]), bits(k[:, end:]))
    assert torch.equal(bits(dv.cpu()), bits(v))
    assert not torch.equal(bits(got[:, row0:end, :, :44]), bits(k[:, row0:end, :, :44]))


def test_op_checks_its_tensors(tables):
    cos, sin, dcos, dsin = tables
    k = torch.zeros(1, 8, 2, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        ops.kv_rope_shift(k[:, ::2], dcos, dsin, 1)
    with pytest.raises(ValueError, match="bfloat16"):
        ops.kv_rope_shift(k.float(), dcos, dsin, 1)
    with pytest.raises(ValueError, match=r"\[1024, 64\]"):
        ops.kv_rope_shift(k, dcos[:512], dsin[:512], 1)
    with pytest.raises(sfa._lib.SfHipError, match="delta_frames"):
        ops.kv_rope_shift(k, dcos, dsin, 1024)
    with pytest.raises(sfa._lib.SfHipError, match="outside the cache"):
        ops.kv_rope_shift(k, dcos, dsin, 1, 4, 5)
    assert not bool(k.any())


# ============================================================================================== 2. against the rotating kernel
@pytest.mark.parametrize("s,delta", [(9, 4), (1000, 999)])
def test_shift_agrees_with_rotating_at_the_shifted_position(tables, s, delta):
    """qkv_norm_rope_cache at start_frame s, then a shift by delta, against qkv_norm_rope_cache at s - delta.  Every changed element
    differs by at most 2^-7 of its pair's norm.  The shifted key went through two bf16 roundings and the direct one through one; a
    rounding moves an element by half a unit in its last place, 2^-9 of the next power of two above it -- of the pair's norm at most
    2^-8, just above a power of two, and 2^-9 to 2^-8.5 for most elements -- and the float32 arithmetic and the tables' own error
    (row s against rows s - delta and delta) are a thousand times smaller.  Three roundings at their typical size sum to under 2^-7;
    all three at their largest, with equal sign, would not (3 x 2^-8).  Measured on these inputs (MI355X; the kernels are
    deterministic): 7.64e-3 and 7.75e-3 of the norm against the bound's 7.81e-3."""
    cos, sin, dcos, dsin = tables
    B, f, h, w, H = 1, 2, 4, 6, 4
    C, L = H * 128, f * h * w
    g = torch.Generator().manual_seed(s)
    qkv = (torch.randn(B * L, 3 * C, generator=g) * 2).bfloat16().to(DEV)
    wq, wk = [(1 + 0.1 * torch.randn(C, generator=g)).bfloat16().to(DEV) for _ in range(2)]
    caches = [torch.zeros(B, L + 5, H, 128, dtype=torch.bfloat16, device=DEV) for _ in range(4)]
    ops.qkv_norm_rope_cache(qkv, wq, wk, caches[0], caches[1], dcos, dsin, (f, h, w), 3, s)
    ops.kv_rope_shift(caches[0], dcos, dsin, delta, 3, L)
    ops.qkv_norm_rope_cache(qkv, wq, wk, caches[2], caches[3], dcos, dsin, (f, h, w), 3, s - delta)
    torch.cuda.synchronize()
    shifted, direct = caches[0].float().cpu(), caches[2].float().cpu()
    assert torch.equal(shifted[..., 44:], direct[..., 44:]) and torch.equal(caches[1], caches[3])
    assert torch.equal(shifted[:, :3], direct[:, :3]) and torch.equal(shifted[:, 3 + L:], direct[:, 3 + L:])
    norm = torch.hypot(direct[..., 0:44:2], direct[..., 1:44:2]).repeat_interleave(2, dim=-1)
    err = (shifted[..., :44] - direct[..., :44]).abs()
    worst = float((err / norm.clamp_min(1e-30)).max())
    print(f"shift after rotate vs rotate at s - delta, (s, delta) = ({s}, {delta}): worst error {worst:.3e} of the pair's norm (bound {2.0 ** -7:.3e})")
    assert bool((err <= 2.0 ** -7 * norm).all()) and float(norm.max()) > 1.0


# ============================================================================================== 3. a session equals stream()
@pytest.fixture(scope="module")
def roll():
    """The `roll` scenario of oracle/make_golden.py: 6 one-frame chunks, window 3, sink 1."""
    R = np.load(os.path.join(GOLD, "rollouts_reduced.npz"))
    return SimpleNamespace(pe=T(R["roll_pe"]).bfloat16().to(DEV), noise=T(R["roll_noise"]).bfloat16().to(DEV),
                           eps=[T(R[f"roll_eps{j}"]).bfloat16() for j in range(int(R["roll_neps"]))], lat_f32=T(R["roll_lat_f32"]),
                           local_end=int(R["roll_local_end"]), global_end=int(R["roll_global_end"]))


def make_pipe(gen, pe, vae=None, **kw):
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=1, context_noise=0)
    return sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=vae or sfa.IdentityVAE(), **kw)


def fix_noise(pipe, eps):
    q = list(eps)
    pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
    return q


def indices(pipe):
    host = kvcache.read_indices(pipe.kv_cache1)
    assert all((int(d["global_end_index"]), int(d["local_end_index"])) == host for d in pipe.kv_cache1)
    return host


@pytest.fixture(scope="module")
def rolling_gen():
    return sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0), timestep_shift=5.0,
                                   is_causal=True, local_attn_size=3, sink_size=1, device=DEV)


@pytest.fixture(scope="module")
def roll_stream(rolling_gen, roll):
    """`stream(noise)` on the scenario, once: (latents, final cache indices)."""
    pipe = make_pipe(rolling_gen, roll.pe)
    q = fix_noise(pipe, roll.eps)
    chunks = list(pipe.stream(roll.noise, ["p"]))
    torch.cuda.synchronize()
    assert not q and [c[0] for c in chunks] == list(range(6))
    lat = torch.cat([c[1] for c in chunks], dim=1)
    assert rel(lat, roll.lat_f32) < TOL and indices(pipe) == (roll.global_end, roll.local_end)
    return lat, indices(pipe)


def test_session_equals_stream(rolling_gen, roll, roll_stream):
    lat, idx = roll_stream
    pipe = make_pipe(rolling_gen, roll.pe)
    q = fix_noise(pipe, roll.eps)
    session = pipe.open_session(["p"], (LAT_H, LAT_W), noise_feed=roll.noise.split(1, dim=1))
    chunks = list(session)
    torch.cuda.synchronize()
    assert not q and [c[0] for c in chunks] == list(range(6)) and session.rebases == [] and session.closed
    mine = torch.cat([c[1] for c in chunks], dim=1)
    assert torch.equal(mine, lat) and indices(pipe) == idx
    assert all(torch.equal(c[2], (c[1] * 0.5 + 0.5).clamp(0, 1)) for c in chunks)
    # the same pipeline again, and unpaired: the caches are reset, and one call per pass gives the same bits
    pipe.pair_context_with_next = False
    fix_noise(pipe, roll.eps)
    again = torch.cat([c[1] for c in pipe.open_session(["p"], (LAT_H, LAT_W), noise_feed=roll.noise.split(1, dim=1))], dim=1)
    assert torch.equal(again, lat) and indices(pipe) == idx


def test_session_with_a_pose_feed_equals_stream(roll):
    shape = sfa.WAN_REDUCED
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sfa.synth_state_dict(shape, seed=0, pose=True), timestep_shift=5.0, is_causal=True,
                                  local_attn_size=3, sink_size=1, device=DEV)
    embedder = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device=DEV)
    clip = pw.synth_pose_clip(92, 21, 8 * LAT_H, 8 * LAT_W, "skeleton")            # 4 (6 - 1) + 1 frames: six latent frames once it has ended
    pieces = list(clip.split(1, dim=1))
    pipe = make_pipe(gen, roll.pe, pose_embedder=embedder)
    fix_noise(pipe, roll.eps)
    want = torch.cat([c[1] for c in pipe.stream(roll.noise, ["p"], pose_feed=iter(pieces))], dim=1)
    idx = indices(pipe)
    q = fix_noise(pipe, roll.eps)
    session = pipe.open_session(["p"], (LAT_H, LAT_W), noise_feed=roll.noise.split(1, dim=1), pose_feed=iter(pieces))
    rows = tuple(session.pose_rows.buffer.shape)
    mine = torch.cat([c[1] for c in session], dim=1)
    torch.cuda.synchronize()
    assert not q and torch.equal(mine, want) and indices(pipe) == idx and tuple(session.pose_rows.buffer.shape) == rows
    # the pose clip, not the noise, ends a session: endless noise, 21 pose frames, six chunks
    fix_noise(pipe, roll.eps + roll.eps)
    g = torch.Generator().manual_seed(5)
    session = pipe.open_session(["p"], (LAT_H, LAT_W), generator=g, pose_feed=iter(pieces))
    assert [c[0] for c in session] == list(range(6)) and session.closed
    # the tokens matter: without them the latents differ
    fix_noise(pipe, roll.eps)
    bare = torch.cat([c[1] for c in pipe.stream(roll.noise, ["p"])], dim=1)
    assert not torch.equal(bare, want)


def test_session_with_an_image_equals_stream():
    """A reduced i2v generator (unpaired: `forward_pair` is not built for it), 16 x 16 latents, built as test_gpu_fewstep_cond.py does."""
    S = sfa.WAN_I2V_REDUCED
    gold = np.load(os.path.join(GOLD, "i2v_reduced.npz"))
    gc = np.load(os.path.join(GOLD, "clip_reduced_257.npz"))
    cs = cw.ClipVisionShape(**{str(k): (float(v) if k == "eps" else int(v)) for k, v in zip(gc["shape_fields"], gc["shape_values"])})
    clip_model = sfa.CLIPModel(state_dict=cw.synth_clip_state_dict(cs, int(gc["seed"])), shape=cs, device=DEV)
    vae = sfa.WanVAEWrapper(vw.synth_vae_state_dict(vw.VAE_REDUCED, seed=0, encoder=True), device=DEV, shape=vw.VAE_REDUCED)
    gen = sfa.WanDiffusionWrapper(shape=S, state_dict=sfa.synth_state_dict(S, seed=int(gold["seed"]), pose=True), timestep_shift=5.0, is_causal=True,
                                  local_attn_size=3, sink_size=1, device=DEV)
    image = cw.synth_frames(21, 1, 128, 128)[:, 0]
    g = torch.Generator().manual_seed(31)
    noise = torch.randn(1, 6, 16, 16, 16, generator=g).bfloat16().to(DEV)
    pe = torch.randn(1, 512, S.text_dim, generator=g).bfloat16().to(DEV)
    eps = [torch.randn(1, 16, 16, 16, generator=g).bfloat16() for _ in range(18)]
    pipe = make_pipe(gen, pe, vae=vae, image_encoder=clip_model)
    fix_noise(pipe, eps)
    want = list(pipe.stream(noise, ["p"], input_image=image))
    idx = indices(pipe)
    q = fix_noise(pipe, eps)
    session = pipe.open_session(["p"], (16, 16), noise_feed=noise.split(1, dim=1), input_image=image)
    mine = list(session)
    torch.cuda.synchronize()
    assert not q and len(mine) == 6 and indices(pipe) == idx == (6 * 64, 3 * 64)
    assert torch.equal(torch.cat([c[1] for c in mine], dim=1), torch.cat([c[1] for c in want], dim=1))
    assert all(torch.equal(a[2], b[2]) for a, b in zip(mine, want))            # the decoded frames too
    # re-based: the image branch goes through the same bookkeeping
    fix_noise(pipe, eps)
    session = pipe.open_session(["p"], (16, 16), noise_feed=noise.split(1, dim=1), input_image=image, rope_limit=4)
    moved = torch.cat([c[1] for c in session], dim=1)
    assert session.rebases == [2] and rel(moved, torch.cat([c[1] for c in want], dim=1)) < TOL


# ============================================================================================== 4. re-based sessions
@pytest.mark.parametrize("rope_limit,shifts", [(4, [2]), (3, [1, 1, 1])], ids=["limit4", "limit3"])
def test_rebased_session_stays_within_the_tolerance(rolling_gen, roll, roll_stream, rope_limit, shifts):
    """Window 3 with one sink frame: after a re-base the two frames behind the sink stand at 0 and 1.  With rope_limit 4 the pair of
    chunk 3 (context at 3, chunk 4's first pass at 4) needs position 5: one shift by 2, and the rest fits.  With rope_limit 3 the
    pairs of chunks 2, 3 and 4 each need one position more than there is: three shifts by 1.  Measured (MI355X): see DESIGN.md
    section 27."""
    lat, idx = roll_stream
    pipe = make_pipe(rolling_gen, roll.pe)
    q = fix_noise(pipe, roll.eps)
    session = pipe.open_session(["p"], (LAT_H, LAT_W), noise_feed=roll.noise.split(1, dim=1), rope_limit=rope_limit)
    mine = torch.cat([c[1] for c in session], dim=1)
    torch.cuda.synchronize()
    vs_ref, vs_plain = rel(mine, roll.lat_f32), rel(mine, lat)
    print(f"rope_limit {rope_limit}: re-bases {session.rebases}; rel(re-based, reference fp32) = {vs_ref:.3e} (un-re-based: {rel(lat, roll.lat_f32):.3e}); "
          f"rel(re-based, un-re-based) = {vs_plain:.3e}")
    assert not q and session.rebases == shifts
    assert indices(pipe) == (idx[0] - sum(shifts) * FS, idx[1])
    assert vs_ref < TOL and vs_plain < TOL
    assert not torch.equal(mine, lat)            # the keys were rotated: bits may move, within the bound


# ============================================================================================== 5. a long run
def test_long_run_is_finite_and_its_memory_does_not_grow(rolling_gen, roll):
    pipe = make_pipe(rolling_gen, roll.pe)
    g = torch.Generator(device=DEV).manual_seed(11)
    pipe.noise_source = lambda t: torch.randn(t.shape, generator=g, device=DEV, dtype=torch.float32).to(t.dtype)
    session = pipe.open_session(["p"], (LAT_H, LAT_W), generator=g, rope_limit=8)
    allocated, finite = {}, []
    for out in session:
        k = out[0]
        finite.append(bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[2]).all()))
        del out
        if k in (10, 40):
            torch.cuda.synchronize()
            allocated[k] = torch.cuda.memory_allocated()
        if k == 40:
            session.close()
    assert len(finite) == 41 and all(finite)
    assert allocated[10] == allocated[40], allocated
    # as test_live_session_host.py derives: the pair of chunk 7 is the first call that needs position 9, and then every 6 chunks
    assert session.rebases == [6] * 6 and indices(pipe)[1] == 3 * FS


# ============================================================================================== 6. the CLI
@pytest.mark.parametrize("video_format", ["pt", "mjpeg"])
def test_generate_cli_open_length(tmp_path, video_format):
    """generate.py --open_length: the 17-frame pose clip decides the length (5 latent frames, 17 video frames), not --num_output_frames;
    a config with global attention is refused before any weights are built."""
    torch.save({"dwpose_data": pw.synth_pose_clip(92, 17, 64, 96, "skeleton"), "random_ref_dwpose": pw.synth_pose_image(93, 64, 96, "skeleton")},
               tmp_path / "pose.pt")
    (tmp_path / "prompts.txt").write_text("a red fox\n")
    keys = "denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 1\nindependent_first_frame: false\n"
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(keys + "model_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n  local_attn_size: 3\n  sink_size: 1\n")
    out = tmp_path / "out"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "generate.py"), "--config_path", str(cfg), "--data_path",
           str(tmp_path / "prompts.txt"), "--output_folder", str(out), "--random_init_seed", "0", "--num_output_frames", "3", "--latent_height", "8",
           "--latent_width", "12", "--seed", "5", "--vae_random_init_seed", "0", "--pose_path", str(tmp_path / "pose.pt"),
           "--pose_random_init_seed", "0", "--open_length", "--video_format", video_format]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stderr[-2000:]
    lat = torch.load(out / "0-0.pt")
    assert lat.shape == (5, 16, 8, 12) and bool(lat.float().abs().sum() > 0) and bool(torch.isfinite(lat.float()).all())
    if video_format == "pt":
        vid = torch.load(out / "0-0.video.pt")
        assert vid.shape == (17, 64, 96, 3) and vid.dtype == torch.uint8
        flat = tmp_path / "global.yaml"
        flat.write_text(keys + "model_kwargs:\n  model_name: reduced\n  timestep_shift: 5.0\n")
        res = subprocess.run(cmd[:cmd.index("--config_path") + 1] + [str(flat)] + cmd[cmd.index("--config_path") + 2:], capture_output=True, text=True,
                             timeout=400)
        assert res.returncode != 0 and "rolling KV cache" in res.stderr
    else:
        frames = sfa.mjpeg.read_avi(str(out / "0-0.avi"))
        assert len(frames) == 17 and all(f[:2] == b"\xff\xd8" for f in frames)
