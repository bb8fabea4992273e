"""GPU tests of the FP8 linear layers: the quantiser against torch bit for bit, the e4m3 GEMM
(every structure, every epilogue) and the small linear against an fp64 emulation on the same e4m3 bytes, the whole
forward against the oracle run through an fp8 emulation of F.linear, and the rollout's determinism contracts in fp8."""
from types import SimpleNamespace

import pytest
import torch

import self_forcing_amd as sfa
from oracle import wan_oracle as wo
from self_forcing_amd import fp8 as f8
from self_forcing_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT_H, LAT_W = 8, 12
FS = (LAT_H // 2) * (LAT_W // 2)
E4M3 = torch.float8_e4m3fn


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("rows_per_segment", [65536, 4096, 1000, 1])
def test_quantize_is_bit_identical_to_torch_over_every_finite_bf16(rows_per_segment):
    """All 65536 bf16 bit patterns minus inf / NaN, as [M, 128] rows, split into segments of several sizes (one segment,
    a few, a ragged last one, one row each): bytes and scales equal torch's recipe (fp8.py) exactly."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    x = bits[torch.isfinite(bits.float())]
    x = torch.cat([x, x[: (-x.numel()) % 128]]).reshape(-1, 128)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(rows_per_segment))
    x = x[perm].contiguous()            # mixes magnitudes across rows, so segment amaxes differ
    q, s = ops.quantize_fp8(x.to(DEV), rows_per_segment)
    q_ref, s_ref = f8.quantize_rows(x, rows_per_segment)
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


def test_quantize_strided_input_and_zero_segment():
    g = torch.Generator().manual_seed(3)
    big = bf((300, 1024), g, 3.0)
    big[100:200] = 0                      # an all-zero segment: scale 1e-12 / 448, bytes 0
    x = big[:, 256:768]
    q, s = ops.quantize_fp8(x.to(DEV), 100)
    q_ref, s_ref = f8.quantize_rows(x, 100)
    assert torch.equal(s.cpu(), s_ref) and torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))
    assert s[1].item() == pytest.approx(1e-12 / 448, rel=1e-6)


# ------------------------------------------------------------------------------------------ GEMM
def emulate(aq, sa, rps, wq, sw, bias=None):
    """fp64 (on the GPU, returned on the host): (aq * sa[seg(m)]) @ (wq * sw[n])^T + bias."""
    M = aq.shape[0]
    sa_row = sa.double().repeat_interleave(rps)[:M, None].to(DEV)
    y = (aq.to(DEV).double() @ wq.to(DEV).double().t()) * sa_row * sw.double().to(DEV)[None]
    y = y if bias is None else y + bias.to(DEV).double()
    return y.cpu()


def epi_ref(epi, y, M, N, g, rps_gate):
    resid, gate_mod, e0 = bf((M, N), g), bf((N,), g, 0.5), bf((3, 6, N), g, 0.5)
    kw = {}
    if epi == "gelu":
        ref = torch.nn.functional.gelu(y, approximate="tanh")
    elif epi == "resid":
        ref, kw = resid.double() + y, {"resid": resid.to(DEV)}
    elif epi == "gate_resid":
        gate = (gate_mod.float()[None] + e0[:, 5].float()).to(torch.bfloat16).double()
        ref = resid.double() + y * gate.repeat_interleave(rps_gate, dim=0)[:M]
        kw = dict(resid=resid.to(DEV), gate_mod=gate_mod.to(DEV), gate_e0=e0.to(DEV)[:, 5], rows_per_group=rps_gate)
    else:
        ref = y
    return ref, kw


SHAPES = [(4680, 4608, 1536), (4680, 1536, 1536), (4680, 8960, 1536), (4680, 1536, 8960),
          (9360, 4608, 1536), (9360, 1536, 1536), (9360, 8960, 1536), (9360, 1536, 8960),
          (3600, 5120, 5120), (3600, 13824, 5120), (1200, 5120, 13824),
          (1000, 1056, 256), (1560, 1536, 384), (333, 200, 512), (77, 64, 1536), (4680, 64, 1536),
          (333, 204, 512)]      # N % 8 == 4: the direct epilogue and the clamped w_scale read on the fp8 path


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("structure", ["pp256", "pp224", "pp192", "pp128", "t128"])
def test_gemm_fp8_every_structure(structure, M, N, K):
    """Every structure on the rollout's shapes (M 4680 / 9360 x qkv / o / ffn.0 / ffn.2), 14B's (C 5120, ffn 13824),
    2- and 3-k-tile prologue / tail cases and ragged ones (M not a multiple of 16, N = 200, N = 64 = the head), with
    two row segments of activation scale and a 3-segment column scale vector (a stacked q|k|v): within 4e-3 of the fp64
    emulation on the same e4m3 bytes, and bit-identical to the 128 x 128 structure and to the automatic choice."""
    g = torch.Generator().manual_seed(M + N + K)
    a, w, bias = bf((M, K), g), bf((N, K), g, 1.0 / K ** 0.5), bf((N,), g, 0.5)
    rps = (M + 1) // 2
    aq, sa = f8.quantize_rows(a, rps)
    thirds = [w[i * N // 3:(i + 1) * N // 3] * (i + 1) for i in range(3)]
    wq, sw = f8.quantize_weight([t.to(torch.bfloat16) for t in thirds])
    y = emulate(aq, sa, rps, wq, sw, bias)
    for epi in ("bias", "gelu", "resid", "gate_resid"):
        ref, kw = epi_ref(epi, y, M, N, g, (M + 2) // 3)
        args = (aq.to(DEV), sa.to(DEV), wq.to(DEV), sw.to(DEV), bias.to(DEV))
        out = ops.gemm_fp8(*args, epilogue=epi, rows_per_segment=rps, structure=structure, **kw)
        assert rel(out, ref) < 4e-3, epi
        assert torch.equal(out, ops.gemm_fp8(*args, epilogue=epi, rows_per_segment=rps, structure="t128", **kw)), epi
        assert torch.equal(out, ops.gemm_fp8(*args, epilogue=epi, rows_per_segment=rps, **kw)), epi
        if M * N > 4e7:
            break      # the big shapes: the epilogues are covered on the others


def test_gemm_fp8_exact_on_integer_data_with_asymmetric_operands():
    """Small integers are exact in e4m3 and their products and sums exact in fp32: the MFMA's lane -> k maps of A and B
    must pair every k with itself.  Asymmetric data (W[n][k] depends on n and k differently from A[m][k])."""
    M, N, K = 256, 256, 512
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None]
    a = ((m * 3 + k * 7) % 9 - 4).float()
    w = ((n * 5 + k * 2) % 7 - 3).float() * ((k % 3) == 0).float() + ((k % 3) != 0).float() * ((n + 2 * k) % 5 - 2).float()
    one = torch.ones(1)
    out = ops.gemm_fp8(a.to(E4M3).to(DEV), one.to(DEV), w.to(E4M3).to(DEV), one.to(DEV), structure="pp256")
    assert torch.equal(out.float().cpu(), (a @ w.t()).to(torch.bfloat16).float())
    out = ops.gemm_fp8(a.to(E4M3).to(DEV), one.to(DEV), w.to(E4M3).to(DEV), one.to(DEV), structure="t128")
    assert torch.equal(out.float().cpu(), (a @ w.t()).to(torch.bfloat16).float())


def test_gemm_fp8_rejects_k_not_multiple_of_128():
    a = torch.zeros(64, 192, dtype=E4M3, device=DEV)
    w = torch.zeros(64, 192, dtype=E4M3, device=DEV)
    one = torch.ones(1, device=DEV)
    with pytest.raises(sfa._lib.SfHipError, match="multiple of 128"):
        ops.gemm_fp8(a, one, w, one)


# ------------------------------------------------------------------------------------------ small linear
@pytest.mark.parametrize("M,N,K,rps,act_in,act_out", [(3, 1536, 256, 3, None, "silu"), (6, 9216, 1536, 3, "silu", None),
                                                      (6, 1536, 1536, 3, None, None), (21, 512, 512, 7, "silu", "gelu"),
                                                      (1, 64, 5120, 1, None, None)])
def test_small_linear_fp8_vs_emulation(M, N, K, rps, act_in, act_out):
    g = torch.Generator().manual_seed(M * N + K)
    x, w, bias = bf((M, K), g, 2.0), bf((N, K), g, 1.0 / K ** 0.5), bf((N,), g, 0.5)
    xa = x.float()
    if act_in == "silu":
        xa = torch.nn.functional.silu(xa)
    xa = xa.to(torch.bfloat16)
    aq, sa = f8.quantize_rows(xa, rps)
    wq, sw = f8.quantize_weight([w])
    y = emulate(aq, sa, rps, wq, sw, bias)
    if act_out == "silu":
        y = torch.nn.functional.silu(y)
    elif act_out == "gelu":
        y = torch.nn.functional.gelu(y, approximate="tanh")
    out = ops.small_linear_fp8(x.to(DEV), wq.to(DEV), sw.to(DEV), bias.to(DEV), act_in, act_out, rows_per_segment=rps)
    assert rel(out, y) < 4e-3


# ------------------------------------------------------------------------------------------ whole forward
class _Fp8Linear:
    """Stand-in for the oracle's `F` module: every F.linear except the patch embedding's runs through the fp8 recipe --
    the bf16 weight and the bf16 activation quantised per tensor (the call's rows = one pass), the product in fp64."""

    def __init__(self, skip_ptr):
        self._skip = skip_ptr

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def linear(self, x, w, b=None):
        if w.data_ptr() == self._skip:
            return torch.nn.functional.linear(x, w, b)
        xs = x.reshape(-1, x.shape[-1]).to(torch.bfloat16)
        aq, sa = f8.quantize_rows(xs, xs.shape[0])
        wq, sw = f8.quantize_weight([w.to(torch.bfloat16)])
        y = emulate(aq, sa, xs.shape[0], wq, sw, None if b is None else b.to(torch.bfloat16))
        return y.to(x.dtype).reshape(*x.shape[:-1], w.shape[0])


def _forward_errors(shape, sd, monkeypatch, F=1, lat=(LAT_H, LAT_W), seed=55):
    g = torch.Generator().manual_seed(seed)
    H, W = lat
    fs = (H // 2) * (W // 2)
    pe = torch.randn(1, 512, shape.text_dim, generator=g).to(torch.bfloat16)
    pe[:, 100:] = 0
    x = torch.randn(1, F, 16, H, W, generator=g).to(torch.bfloat16)
    t = torch.tensor([[937.5] * F])
    outs = {}
    for fp8 in (False, True):
        gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV, fp8=fp8)
        assert gen.fp8 == fp8
        args = SimpleNamespace(denoising_step_list=[1000], warp_denoising_step=False, independent_first_frame=False,
                               num_frame_per_block=1, context_noise=0)
        pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe.to(DEV)), vae=sfa.IdentityVAE())
        pipe.frame_seq_length = fs
        pipe._initialize_kv_cache(1, torch.bfloat16, DEV, cache_tokens=F * fs)
        pipe._initialize_crossattn_cache(1, torch.bfloat16, DEV)
        outs[fp8] = gen(x.to(DEV), {"prompt_embeds": pe.to(DEV)}, t.to(DEV), pipe.kv_cache1, pipe.crossattn_cache, 0)[0].float().cpu()
        del gen, pipe
        torch.cuda.empty_cache()
    Wf = wo.prepare_weights(sd, torch.float32)
    cfg = wo.OracleConfig(dim=shape.dim, ffn_dim=shape.ffn_dim, num_heads=shape.num_heads, num_layers=shape.num_layers,
                          text_dim=shape.text_dim)

    def oracle():
        kv, ca = wo.init_kv_cache(cfg, 1, F * fs, torch.float32), wo.init_crossattn_cache(cfg, 1, torch.float32)
        return wo.wrapper_forward(Wf, cfg, wo.FlowMatchTables(5.0), x.float(), pe.float(), t, kv, ca, 0)[0]

    ref = oracle()
    with monkeypatch.context() as mp:
        mp.setattr(wo, "F", _Fp8Linear(Wf["patch_embedding.weight"].data_ptr()))
        ref8 = oracle()
    return {"bf16_vs_oracle": rel(outs[False], ref), "fp8_vs_emulated": rel(outs[True], ref8),
            "fp8_vs_oracle": rel(outs[True], ref), "emulated_vs_oracle": rel(ref8, ref)}


def _check_forward(e):
    """The kernels quantise THEIR bf16 activations, the emulation the oracle's fp32 ones: values near an e4m3 rounding
    boundary land on different codes, so the two fp8 results differ by a fraction of the fp8 error itself (measured:
    0.5x at the reduced shape, 0.7x at 1.3B) -- not by the bf16 path's error.  Pinned: the fp8
    forward is closer to the fp8 emulation than the emulation is to exact math, and FP8 really ran (its distance to
    the exact oracle is at least 3x the bf16 forward's)."""
    print("fp8 forward errors:", {k: f"{v:.3e}" for k, v in e.items()})
    assert e["fp8_vs_emulated"] < e["emulated_vs_oracle"], e
    assert e["fp8_vs_oracle"] >= 3 * e["bf16_vs_oracle"], e


def test_forward_fp8_reduced_vs_emulated_oracle(monkeypatch):
    sd = sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0)
    _check_forward(_forward_errors(sfa.WAN_REDUCED, sd, monkeypatch, F=2))


def test_forward_fp8_full_1p3b_shape_vs_emulated_oracle(monkeypatch):
    sd = sfa.synth_state_dict(sfa.WAN_1_3B, seed=0)
    _check_forward(_forward_errors(sfa.WAN_1_3B, sd, monkeypatch, F=1, lat=(60, 104)))


def test_fp8_on_a_shape_that_breaks_the_k_rule_fails_at_load():
    shape = sfa.WanShape(dim=512, ffn_dim=1000, num_heads=4, num_layers=1, text_dim=256)
    sd = sfa.synth_state_dict(shape, seed=0)
    with pytest.raises(ValueError, match="ffn.2 has in_features=1000, not a multiple of 128"):
        sfa.WanDiffusionWrapper(shape=shape, state_dict=sd, is_causal=True, device=DEV, fp8=True)


# ------------------------------------------------------------------------------------------ rollout
@pytest.fixture(scope="module")
def sd_reduced():
    return sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0)


def _pipe(sd, nfpb, pe, gen=None):
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True,
                           independent_first_frame=False, num_frame_per_block=nfpb, context_noise=0)
    gen = gen or sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV, fp8=True)
    return sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=sfa.IdentityVAE())


def _inputs(seed, batch, frames, nfpb):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(batch, frames, 16, LAT_H, LAT_W, generator=g).to(torch.bfloat16).to(DEV)
    pe = torch.randn(batch, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    eps = [torch.randn(batch * nfpb, 16, LAT_H, LAT_W, generator=g).to(torch.bfloat16) for _ in range(3 * (frames // nfpb))]
    return noise, pe, eps


def _run(pipe, noise, eps, batch):
    q = list(eps)
    pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
    return pipe.inference(noise, ["p"] * batch, return_latents=True)[1].clone()


@pytest.mark.parametrize("batch", [1, 2])
def test_fp8_rollout_paired_and_unpaired_passes_are_bit_identical(sd_reduced, batch):
    noise, pe, eps = _inputs(7 + batch, batch, 6, 2)
    res = []
    for paired in (True, False):
        pipe = _pipe(sd_reduced, 2, pe)
        pipe.pair_context_with_next = paired
        res.append(_run(pipe, noise, eps, batch))
    assert torch.equal(res[0], res[1])
    bf16 = _pipe(sd_reduced, 2, pe, sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd_reduced, timestep_shift=5.0,
                                                            is_causal=True, device=DEV))
    assert rel(res[0], _run(bf16, noise, eps, batch)) > 1e-3          # and it is not the bf16 result


def test_fp8_rollout_bit_reproducible_beside_a_second_stream(sd_reduced):
    noise, pe, eps = _inputs(17, 1, 6, 2)
    pipe = _pipe(sd_reduced, 2, pe)
    first = _run(pipe, noise, eps, 1)
    side = torch.cuda.Stream()
    junk = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    for _ in range(2):
        with torch.cuda.stream(side):
            for _ in range(20):
                junk = (junk @ junk.t()).clamp(-1, 1)
        assert torch.equal(_run(pipe, noise, eps, 1), first)
    torch.cuda.synchronize()


def test_fp8_streaming_matches_batch_inference(sd_reduced):
    noise, pe, eps = _inputs(31, 1, 6, 3)
    pipe = _pipe(sd_reduced, 3, pe)
    lat = _run(pipe, noise, eps, 1)
    q = list(eps)
    pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
    chunks = list(pipe.stream(noise, ["p"]))
    assert torch.equal(torch.cat([c[1] for c in chunks], dim=1), lat)


def test_fp8_cfg_sampler_runs_and_stays_close_to_bf16(sd_reduced):
    g = torch.Generator().manual_seed(41)
    pe = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    ne = torch.randn(1, 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16).to(DEV)
    noise = torch.randn(1, 2, 16, LAT_H, LAT_W, generator=g).to(torch.bfloat16).to(DEV)

    class Enc:
        def __call__(self, text_prompts):
            return {"prompt_embeds": ne if text_prompts[0] == "NEG" else pe}

    outs = []
    for fp8 in (False, True):
        args = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, num_frame_per_block=1,
                               negative_prompt="NEG", guidance_scale=3.0)
        gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd_reduced, timestep_shift=5.0, is_causal=True, device=DEV, fp8=fp8)
        pipe = sfa.CausalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=Enc(), vae=sfa.IdentityVAE())
        pipe.sampling_steps = 4
        outs.append(pipe.inference(noise, ["p"], return_latents=True)[1].float().cpu())
    assert torch.isfinite(outs[1]).all()
    assert 1e-3 < rel(outs[1], outs[0]) < 0.3
