"""Host-side tests of the FP8 linear layers (no GPU): the recipe of fp8.py on hand-computed cases, the weight
quantisation at load (one scale per reference Linear, stacked weights with per-column scale vectors, the patch
embedding left in bf16, fewer bytes), the fp8 plumbing down to the C struct, and the ctypes mirror of ABI 10."""
import ctypes as C
import os
import re

import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import _lib
from self_forcing_amd import fp8 as f8
from self_forcing_amd.model import CausalWanModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sf_hip.h")
E4M3 = torch.float8_e4m3fn


def codes(q):
    return q.view(torch.uint8).tolist()


# ------------------------------------------------------------------------------------------ the recipe
def test_zero_amax_gives_the_floor_scale_and_zero_bytes():
    x = torch.zeros(3, 8, dtype=torch.bfloat16)
    q, s = f8.quantize_rows(x, 3)
    assert s.tolist() == [pytest.approx(1e-12 / 448, rel=1e-7)] and s.dtype == torch.float32
    assert set(sum(codes(q), [])) == {0}


def test_values_at_plus_minus_448_and_the_largest_code():
    x = torch.tensor([[448.0, -448.0, 224.0, 0.0]], dtype=torch.bfloat16)
    q, s = f8.quantize_rows(x, 1)
    assert s.item() == 1.0
    assert codes(q) == [[0x7E, 0xFE, 0x76, 0x00]]          # 448 = 1.75 x 2^8: exponent 15, mantissa 6
    # past the scale's range (not reachable from the amax, but the clamp is part of the recipe)
    assert codes(f8.quantize(torch.tensor([1000.0, -1e9]), torch.tensor(1.0))) == [0x7E, 0xFE]


def test_e4m3_subnormal_range_rounds_to_nearest_even():
    s = torch.tensor(1.0)
    x = torch.tensor([2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 7 * 2.0 ** -9, 2.0 ** -6, -2.0 ** -9, 2.0 ** -11])
    # 2^-9 is the smallest subnormal (code 1); 2^-10 ties to 0; 1.5 and 2.5 subnormal steps tie to 2; 7 x 2^-9 is the
    # largest subnormal; 2^-6 the smallest normal (exponent 1, code 0x08); 2^-11 rounds to zero
    assert codes(f8.quantize(x, s)) == [0x01, 0x00, 0x02, 0x02, 0x07, 0x08, 0x81, 0x00]


def test_segments_take_their_own_amax():
    x = torch.tensor([[1.0, -2.0], [0.5, 0.25], [4.0, 0.0]], dtype=torch.bfloat16)
    q, s = f8.quantize_rows(x, 2)
    assert torch.equal(s, torch.tensor([2.0 / 448, 4.0 / 448]))
    assert torch.equal(f8.dequantize(q, s.repeat_interleave(2)[:3, None]).float(), x.float())   # powers of two: exact


def test_weight_recipe_stacks_one_scale_per_part():
    g = torch.Generator().manual_seed(0)
    parts = [torch.randn(4, 16, generator=g) * k for k in (1.0, 3.0, 0.5)]
    q, s = f8.quantize_weight(parts)
    assert q.shape == (12, 16) and q.dtype == E4M3 and s.shape == (12,)
    for i, p in enumerate(parts):
        want = p.abs().amax().float() / 448
        assert torch.all(s[4 * i:4 * i + 4] == want)
        assert codes(q[4 * i:4 * i + 4]) == codes(f8.quantize(p, want))


def test_k_rule_message():
    with pytest.raises(ValueError, match="not a multiple of 128"):
        f8.check_k("ffn.2", 1000)
    f8.check_k("ffn.2", 8960)


# ------------------------------------------------------------------------------------------ load + plumbing
@pytest.fixture(scope="module")
def models():
    shape = sfa.WAN_REDUCED
    sd = sfa.synth_state_dict(shape, seed=0)
    s = sfa.FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    s.set_timesteps(1000, training=True)
    return sd, CausalWanModel(shape, sd, "cpu", s.sigmas, s.timesteps), CausalWanModel(shape, sd, "cpu", s.sigmas, s.timesteps, fp8=True)


def test_weights_quantised_per_reference_linear(models):
    sd, m16, m8 = models
    C_ = sfa.WAN_REDUCED.dim
    assert not m16.fp8 and m16.fp8_weights == {} and m8.fp8
    names = {"text_embedding.0", "text_embedding.2", "time_embedding.0", "time_embedding.2", "time_projection.1", "head.head"}
    for i in range(sfa.WAN_REDUCED.num_layers):
        names |= {f"blocks.{i}.{n}" for n in ("qkv", "o", "cq", "ckv", "co", "ffn0", "ffn2")}
    assert set(m8.fp8_weights) == names
    assert not any("patch" in n for n in m8.fp8_weights)
    q, s = m8.fp8_weights["blocks.1.qkv"]
    assert q.dtype == E4M3 and q.shape == (3 * C_, C_) and s.shape == (3 * C_,) and s.dtype == torch.float32
    for j, src in enumerate(("q", "k", "v")):
        w = sd[f"blocks.1.self_attn.{src}.weight"].to(torch.bfloat16)
        assert torch.all(s[j * C_:(j + 1) * C_] == f8.scale_of(w))
        assert codes(q[j * C_:(j + 1) * C_]) == codes(f8.quantize(w, f8.scale_of(w)))
    q, s = m8.fp8_weights["blocks.0.ckv"]
    assert q.shape == (2 * C_, C_)
    for j, src in enumerate(("k", "v")):
        assert torch.all(s[j * C_:(j + 1) * C_] == f8.scale_of(sd[f"blocks.0.cross_attn.{src}.weight"].to(torch.bfloat16)))
    q, s = m8.fp8_weights["head.head"]
    assert q.shape == (64, C_) and torch.all(s == f8.scale_of(sd["head.head.weight"].to(torch.bfloat16)))


def test_param_bytes_shrink(models):
    _, m16, m8 = models
    assert m8.param_bytes() < 0.6 * m16.param_bytes()


def test_fp8_plumbing_down_to_the_c_struct(models):
    _, m16, m8 = models
    c16, c8 = m16.cmodel, m8.cmodel
    assert c16.fp8 == 0 and not c16.layers_fp8_host and not c16.head_q and c16.head_w      # zero = bf16
    assert c8.fp8 == 1 and c8.layers_fp8_host
    assert c8.patch_w                                                     # the patch embedding stays bf16
    for n, (src,) in [(n, s) for n, s in _lib.FP8_MODEL_LINEARS if n != "pose"]:
        q, s = m8.fp8_weights[src]
        assert getattr(c8, n + "_q") == q.data_ptr() and getattr(c8, n + "_s") == s.data_ptr()
        assert not getattr(c8, n + "_w")                                    # only the e4m3 copy is kept
    for i in range(sfa.WAN_REDUCED.num_layers):
        l8, l16 = c8.layers_fp8_host[i], c8.layers_host[i]
        for n, _ in _lib.FP8_LAYER_LINEARS:
            q, s = m8.fp8_weights[f"blocks.{i}.{n}"]
            assert getattr(l8, n + "_q") == q.data_ptr() and getattr(l8, n + "_s") == s.data_ptr()
            assert not getattr(l16, n + "_w") and getattr(l16, n + "_b")      # biases stay bf16


def test_wrapper_keyword_and_attribute():
    import inspect
    sig = inspect.signature(sfa.WanDiffusionWrapper.__init__)
    assert sig.parameters["fp8"].kind == inspect.Parameter.KEYWORD_ONLY and sig.parameters["fp8"].default is False
    sd = sfa.synth_state_dict(sfa.WAN_REDUCED, seed=1)
    w = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd, is_causal=True, device="cpu", fp8=True)
    assert w.fp8 and w.model.cmodel.fp8 == 1 and w.share().fp8
    assert not sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd, is_causal=True, device="cpu").fp8


def test_fp8_on_a_shape_that_breaks_the_k_rule_fails_at_load_on_the_host():
    shape = sfa.WanShape(dim=512, ffn_dim=1000, num_heads=4, num_layers=1, text_dim=256)
    sd = sfa.synth_state_dict(shape, seed=0)
    with pytest.raises(ValueError, match="ffn.2 has in_features=1000"):
        sfa.WanDiffusionWrapper(shape=shape, state_dict=sd, is_causal=True, device="cpu", fp8=True)
    sfa.WanDiffusionWrapper(shape=shape, state_dict=sd, is_causal=True, device="cpu")       # bf16 takes it


# ------------------------------------------------------------------------------------------ the fields ABI 10 appended
def test_abi_version_and_the_ctypes_mirror_of_the_appended_fields():
    text = open(HEADER).read()
    assert int(re.search(r"#define SF_HIP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 11
    assert int(re.search(r"#define SF_FP8_AMAX_PARTS (\d+)", text).group(1)) == _lib.FP8_AMAX_PARTS
    mirror = [f[0] for f in _lib.Model._fields_]      # (equal to the header's: test_host_logic.test_ctypes_mirror_matches_the_header)
    tail = mirror[mirror.index("n_table") + 1:]
    assert tail[0] == "fp8" and tail[-1] == "layers_fp8_host" and len(tail) == 2 + 2 * len(_lib.FP8_MODEL_LINEARS)
    # sf_layer_weights keeps its layout; the append leaves every earlier offset where ABI 9 had it
    assert C.sizeof(_lib.LayerWeights) == 21 * 8
    assert _lib.Model.fp8.offset == _lib.Model.n_table.offset + 4
    assert _lib.Model.layers_fp8_host.offset == C.sizeof(_lib.Model) - 8
    for n in ("sf_quantize_fp8", "sf_gemm_fp8", "sf_small_linear_fp8"):
        assert n in _lib.SIGNATURES and re.search(r"\bint %s\(" % n, text)
