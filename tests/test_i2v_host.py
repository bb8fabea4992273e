"""The generator's i2v model type without a GPU: the CPU restatement `i2v_reference` against the
outputs the reference recorded (tools/make_golden_i2v.py), the conditions the fixture itself must meet, the ctypes mirrors,
the argument checks of the new C entry points, the appended parameter names, and the early checks of wrapper and pipeline.

Tolerance: 1e-5 relative Frobenius for a restatement in fp32 against the reference in fp32."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from oracle import wan_oracle as wo
from self_forcing_amd import i2v_reference as ir
from self_forcing_amd import weights as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "i2v_reduced.npz")
S = wt.WAN_I2V_REDUCED
RESTATEMENT_TOL = 1e-5


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def case(gold):
    c = ir.synthetic_case(S, int(gold["input_seed"]), int(gold["frames"]), int(gold["H"]), int(gold["W"]))
    sums = [c[k].double().abs().sum().item() for k in ("clip", "clip_other", "pe", "attn_x", "attn_ctx", "attn_img")]
    assert sums == list(gold["input_sums"]), "torch CPU generator stream changed; regenerate the fixture"
    bf = lambda a: torch.from_numpy(a.view(np.int16)).view(torch.bfloat16).float()  # noqa: E731
    assert torch.equal(c["x"], bf(gold["x"])) and torch.equal(c["y"], bf(gold["y"]))
    return c


@pytest.fixture(scope="module")
def weights(gold):
    return wo.prepare_weights(wt.synth_state_dict(S, seed=int(gold["seed"])), torch.float32)


@pytest.fixture(scope="module")
def restated(gold, case, weights):
    """One- and two-chunk forwards of the restatement in fp32, with the caches the one-chunk run filled."""
    cfg = ir.oracle_config(S)
    F, fs = int(gold["frames"]), (int(gold["H"]) // 2) * (int(gold["W"]) // 2)
    caches = lambda: (wo.init_kv_cache(cfg, 1, F * fs, torch.float32), wo.init_crossattn_cache(cfg, 1, torch.float32))  # noqa: E731

    def forward(clip, kv, cc, frames, t, start):
        return ir.forward_inference(weights, cfg, case["x"][:, :, frames], case["y"][:, :, frames], torch.full((1, len(range(F)[frames])), t),
                                    case["pe"], clip, kv, cc, start)

    kv, cc = caches()
    one = forward(case["clip"], kv, cc, slice(0, F), float(gold["t_one"]), 0)
    swapped = forward(case["clip_other"], *caches(), slice(0, F), float(gold["t_one"]), 0)
    kv2, cc2 = caches()
    two = torch.cat([forward(case["clip"], kv2, cc2, slice(0, 1), float(gold["t_two"][0]), 0),
                     forward(case["clip"], kv2, cc2, slice(1, F), float(gold["t_two"][1]), fs)], dim=2)
    return SimpleNamespace(one=one, two=two, swapped=swapped, cross=cc, cfg=cfg)


# ------------------------------------------------------------------------------------------ the restatement
def test_reference_modules_fp32(gold, case, weights):
    cfg = ir.oracle_config(S)
    rows = gold["rows"]
    assert rel(ir.img_emb(weights, case["clip"])[0, rows], gold["img_emb"]) <= RESTATEMENT_TOL
    out = ir.cross_attention(weights, "blocks.0.cross_attn.", cfg, case["attn_x"], case["attn_ctx"], case["attn_img"], None)
    assert tuple(out.shape) == gold["cross_attn"].shape and rel(out, gold["cross_attn"]) <= RESTATEMENT_TOL


def test_reference_forwards_fp32(gold, restated):
    assert tuple(restated.one.shape) == gold["one_chunk"].shape == (1, 16, 3, 8, 12)
    assert rel(restated.one, gold["one_chunk"]) <= RESTATEMENT_TOL
    assert rel(restated.two, gold["two_chunk"]) <= RESTATEMENT_TOL
    assert rel(restated.two, restated.one) > 0.05        # the two cases are different computations


def test_reference_image_kv_fp32(gold, restated):
    rows = gold["rows"]
    for name in ("k_img", "v_img"):
        got = torch.stack([c[name] for c in restated.cross])[:, 0, rows].flatten(2)
        assert tuple(got.shape) == gold[name].shape == (S.num_layers, len(rows), S.dim)
        assert rel(got, gold[name]) <= RESTATEMENT_TOL
    assert all(c["is_init"] for c in restated.cross)


def test_reference_bf16_mode_stays_at_the_reference_bf16_distance(gold, case):
    """The bf16 mode follows the reference's rounding points: as far from fp32 as the reference's own bf16 run."""
    cfg = ir.oracle_config(S)
    W16 = wo.prepare_weights(wt.synth_state_dict(S, seed=int(gold["seed"])), torch.bfloat16)
    kv, cc = wo.init_kv_cache(cfg, 1, 72, torch.bfloat16), wo.init_crossattn_cache(cfg, 1, torch.bfloat16)
    one = ir.forward_inference(W16, cfg, case["x"], case["y"], torch.full((1, 3), float(gold["t_one"])), case["pe"], case["clip"], kv, cc, 0)
    assert one.dtype == torch.bfloat16
    assert rel(one.float(), gold["one_chunk"]) <= 2 * float(gold["bf16_vs_fp32"])


# ------------------------------------------------------------------------------------------ conditions on the fixture
def test_fixture_causal_equals_bidirectional(gold):
    """The forwarding shim carries no arithmetic: one chunk from empty caches is the bidirectional i2v forward."""
    assert float(gold["causal_vs_bidirectional"]) <= RESTATEMENT_TOL
    assert rel(gold["one_chunk"], gold["bidirectional"]) <= RESTATEMENT_TOL


def test_fixture_sees_the_image_branch(gold, restated):
    """A condition on the INPUTS: the 2e-2 tolerance of the GPU forwards must not be able to hide a dead image branch."""
    assert float(gold["clip_swap_sensitivity"]) >= 0.1
    assert rel(restated.swapped, restated.one) >= 0.1
    assert float(gold["bf16_vs_fp32"]) < 2e-2 and float(gold["bf16_vs_fp32_kv"]) < 1e-2


# ------------------------------------------------------------------------------------------ C ABI
def test_ctypes_mirrors_match_the_header():
    """(Field names and argument counts against the header: test_host_logic.test_ctypes_mirror_matches_the_header.)"""
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    L = sfa._lib
    assert ctypes.sizeof(L.I2VLayer) == 3 * 8 and ctypes.sizeof(L.I2VModel) == 16 + 9 * 8 and ctypes.sizeof(L.I2VArgs) == 2 * 8 + 3 * 8 + 8 + 2 * 8
    assert L.I2VModel.img_ln0_w.offset == 16 and L.I2VArgs.kimg_cache_host.offset == 48
    assert int(re.search(r"#define SF_HIP_ABI_VERSION (\d+)", text).group(1)) == 11 == L.ABI_VERSION == L.lib().sf_abi_version()
    # the t2v structs keep their layout: everything i2v travels beside them
    assert ctypes.sizeof(L.LayerWeights) == 21 * 8 and L.Model.layers_fp8_host.offset == ctypes.sizeof(L.Model) - 8
    sch = str(torch.ops.sf_hip.attention_accum.default._schema)
    assert "Tensor(a3!) out" in sch and "attention_accum" in sfa.torch_ops.OPS and "dit_forward_i2v" in sfa.torch_ops.OPS
    sch = str(torch.ops.sf_hip.dit_forward_i2v.default._schema)
    assert "Tensor(a11!)[] kimg_cache" in sch and "Tensor(a12!)[] vimg_cache" in sch


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    err = lib.sf_last_error
    p = 1 << 20       # an aligned non-null address: every call below fails its checks before any launch
    def att(structure, out=p):
        a = sfa._lib.AttentionArgs(q=p, k=p, v=p, out=out, B=1, H=2, Lq=72, Lk=257, q_stride=256, q_bstride=72 * 256, kv_stride=256,
                                   kv_bstride=257 * 256, o_stride=256, o_bstride=72 * 256, structure=structure, accumulate=1)
        return lib.sf_attention(a, None)
    assert att(sfa._lib.ATTN_STRUCTURES["r64"]) != 0 and b"r64" in err() and b"accumulate" in err()
    assert att(7) != 0 and b"unknown structure" in err()
    assert att(0, out=None) != 0 and b"null" in err()
    assert lib.sf_patchify_i2v(p, None, p, 1, 1, 16, 20, 48, 8, 12, 0, 96, 96, None) != 0 and b"bad arguments" in err()
    assert lib.sf_patchify_i2v(p, p, p, 1, 1, 16, 20, 48, 7, 12, 0, 84, 84, None) != 0 and b"must be even" in err()
    assert lib.sf_patchify_i2v(p, p, p, 1, 1, 16, 20, 32, 8, 12, 0, 96, 96, None) != 0 and b"do not fit" in err()
    assert lib.sf_patchify_i2v(p, p, p, 1, 1, 16, 20, 48, 8, 12, 0, 95, 96, None) != 0 and b"contiguous" in err()
    assert lib.sf_layernorm_rows(p, p, p, p, 4, 324, 1e-5, None) != 0 and b"multiple of 8" in err()
    assert lib.sf_layernorm_rows(p, None, p, p, 4, 320, 1e-5, None) != 0 and b"null" in err()

    m, im, a, ia = sfa._lib.Model(), sfa._lib.I2VModel(), sfa._lib.ForwardArgs(), sfa._lib.I2VArgs()
    call = sfa._lib.ForwardCall(n_passes=1, i2v_model=ctypes.pointer(im), i2v_args=ctypes.pointer(ia))
    call.passes[0] = ctypes.pointer(a)
    forward = lambda: lib.sf_dit_forward(m, call, None)  # noqa: E731
    assert lib.sf_dit_forward(None, call, None) != 0 and b"null" in err()
    call.i2v_args = None
    assert forward() != 0 and b"null" in err()            # the model's half without the pass's
    call.i2v_args = ctypes.pointer(ia)
    assert lib.sf_dit_workspace_bytes(m, im, 1, 1, 8, 12, 1) == 0
    layers = (sfa._lib.I2VLayer * 2)()
    im.layers_host, im.clip_len, im.clip_dim = ctypes.cast(layers, ctypes.POINTER(sfa._lib.I2VLayer)), 257, 320
    m.dim, m.num_heads, m.num_layers, m.in_dim, m.out_dim = 512, 4, 2, 48, 16
    assert forward() != 0 and b"y is missing" in err()
    ia.y, ia.y_channels = p, 40
    assert forward() != 0 and b"do not fit" in err()
    ia.y_channels = 20
    assert forward() != 0 and b"image cache" in err()
    m.fp8 = 1
    assert forward() != 0 and b"fp8" in err()
    m.fp8, im.clip_dim = 0, 300
    assert forward() != 0 and b"multiple of 64" in err()
    im.clip_dim, call.n_passes = 320, 2
    call.passes[1] = ctypes.pointer(a)
    assert forward() != 0 and b"two-pass call is not built" in err()
    with pytest.raises(ValueError, match="CUDA"):
        z = torch.zeros(1, 4, 1, 128, dtype=torch.bfloat16)
        sfa.ops.attention_accum(z, z, z, z.clone())


# ------------------------------------------------------------------------------------------ weights
def test_param_shapes_append_the_i2v_tensors():
    t2v, i2v = wt.param_shapes(wt.WAN_REDUCED), wt.param_shapes(S)
    names = list(i2v)
    assert names[:len(t2v)] == list(t2v)
    assert {k: v for k, v in i2v.items() if k in t2v and k != "patch_embedding.weight"} == {k: v for k, v in t2v.items() if k != "patch_embedding.weight"}
    assert i2v["patch_embedding.weight"] == (512, 36, 1, 2, 2) and t2v["patch_embedding.weight"] == (512, 16, 1, 2, 2)
    tail = ["img_emb.proj.0.weight", "img_emb.proj.0.bias", "img_emb.proj.1.weight", "img_emb.proj.1.bias", "img_emb.proj.3.weight",
            "img_emb.proj.3.bias", "img_emb.proj.4.weight", "img_emb.proj.4.bias"]
    for i in range(S.num_layers):
        tail += [f"blocks.{i}.cross_attn.{n}" for n in ("k_img.weight", "k_img.bias", "v_img.weight", "v_img.bias", "norm_k_img.weight")]
    assert names[len(t2v):] == tail
    assert i2v["img_emb.proj.1.weight"] == (320, 320) and i2v["img_emb.proj.3.weight"] == (512, 320) and i2v["img_emb.proj.4.weight"] == (512,)
    sd = wt.synth_state_dict(S, seed=0)
    for n in ("img_emb.proj.0.weight", "img_emb.proj.4.weight", "blocks.0.cross_attn.norm_k_img.weight", "blocks.1.cross_attn.norm_k_img.weight"):
        assert abs(sd[n].float().mean().item() - 1) < 0.05 and 0.05 < sd[n].float().std().item() < 0.2, n      # scale vectors ~ 1 + 0.1 N
    # the shapes that existed before are untouched: new fields last, with defaults
    assert wt.WanShape() == wt.WanShape(model_type="t2v", clip_dim=1280, clip_len=257) and not wt.WAN_REDUCED.is_i2v
    assert list(wt.WAN_REDUCED.as_dict())[-3:] == ["model_type", "clip_dim", "clip_len"]
    big = wt.NAMED_SHAPES["Wan2.1-I2V-14B"]
    assert (big.dim, big.ffn_dim, big.num_heads, big.num_layers, big.in_dim, big.clip_dim, big.model_type) == (5120, 13824, 40, 40, 36, 1280, "i2v")
    assert S == wt.WAN_REDUCED.replace(model_type="i2v", in_dim=36, clip_dim=320) and S.clip_dim == sfa.CLIP_REDUCED.dim


# ------------------------------------------------------------------------------------------ wrapper and pipeline, early checks
def _wrapper(shape):
    w = sfa.WanDiffusionWrapper.__new__(sfa.WanDiffusionWrapper)
    torch.nn.Module.__init__(w)
    w.model = SimpleNamespace(shape=shape, num_layers=shape.num_layers, device=torch.device("cpu"), model_type=shape.model_type)
    return w


def test_wrapper_checks_the_image_tensors_first():
    x, kv, cc = torch.zeros(1, 2, 16, 8, 12), [{}] * 2, [{}] * 2
    y, clip = torch.zeros(1, 20, 2, 8, 12), torch.zeros(1, 257, 320)
    call = lambda w, cond=None, **kw: w.forward(x, cond or {}, torch.zeros(1, 2), kv, cc, 0, **kw)  # noqa: E731
    i2v = _wrapper(S)
    with pytest.raises(AssertionError, match="clip_feature and y"):
        call(i2v)
    with pytest.raises(AssertionError, match="clip_feature and y"):
        call(i2v, clip_feature=clip)                                                    # y missing
    with pytest.raises(AssertionError, match="in_dim = 36"):
        call(i2v, {"clip_feature": clip, "y": torch.zeros(1, 16, 2, 8, 12)})          # read from conditional_dict too
    with pytest.raises(AssertionError, match="this call's frames"):
        call(i2v, clip_feature=clip, y=torch.zeros(1, 20, 3, 8, 12))                    # frame mismatch: the whole-clip y
    with pytest.raises(AssertionError, match="this call's frames"):
        call(i2v, clip_feature=clip, y=torch.zeros(3, 20, 2, 8, 12))                    # batch neither 1 nor B
    with pytest.raises(AssertionError, match=r"\[1 or 1, 257, 320\]"):
        call(i2v, clip_feature=torch.zeros(1, 17, 320), y=y)
    with pytest.raises(NotImplementedError, match="forward_pair"):
        i2v.forward_pair(x, torch.zeros(1, 2), x, torch.zeros(1, 2), {}, kv, cc, 0, 0)
    assert not i2v.can_pair({})
    t2v = _wrapper(wt.WAN_REDUCED)
    for kw in ({"clip_feature": clip}, {"y": y}):
        with pytest.raises(NotImplementedError, match="i2v model type"):
            call(t2v, **kw)
        with pytest.raises(NotImplementedError, match="i2v model type"):
            call(t2v, dict(kw))
    assert t2v.can_pair({})


def _pipeline(model):
    gen = SimpleNamespace(model=model, forward=lambda **kw: None)
    a = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, negative_prompt="", guidance_scale=3.0)
    return sfa.CausalDiffusionInferencePipeline(a, "cpu", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": None}, vae=object(),
                                                pose_embedder=object())


def test_pipeline_checks_without_a_gpu():
    noise, image = torch.zeros(1, 3, 16, 16, 16), torch.zeros(3, 128, 128)
    i2v = _pipeline(SimpleNamespace(num_layers=1, local_attn_size=-1, shape=S, model_type="i2v"))
    with pytest.raises(ValueError, match="clip_feature"):
        i2v.inference(noise, ["p"])                                                     # an i2v generator without an image
    for model in (SimpleNamespace(num_layers=1, local_attn_size=-1, shape=wt.WAN_REDUCED, model_type="t2v"),
                  SimpleNamespace(num_layers=1, local_attn_size=-1, shape=wt.WAN_REDUCED)):       # a stand-in without model_type
        with pytest.raises(NotImplementedError, match="i2v branch"):
            _pipeline(model).inference(noise, ["p"], input_image=image)
    asked = []

    def short(img, num_frames, height, width):
        asked.append((num_frames, height, width))
        return {"clip_feature": torch.zeros(1, 257, 320), "y": torch.zeros(1, 20, 2, 16, 16)}
    i2v.encode_image = short
    with pytest.raises(AssertionError, match="y has 2 latent frames, but the output timeline has 3"):
        i2v.inference(noise, ["p"], input_image=image)
    assert asked == [(4 * (3 - 1) + 1, 128, 128)]                                        # once per clip, the whole output timeline


def test_kvcache_holds_the_image_keys():
    from self_forcing_amd.kvcache import add_image_cache, new_crossattn_cache
    cc = new_crossattn_cache(S, 2, 3, torch.bfloat16, "cpu")
    assert all(tuple(c["k_img"].shape) == tuple(c["v_img"].shape) == (3, 257, 4, 128) and c["k_img"].dtype == torch.bfloat16 for c in cc)
    plain = new_crossattn_cache(wt.WAN_REDUCED, 2, 3, torch.bfloat16, "cpu")
    assert all(set(c) == {"k", "v", "is_init"} for c in plain)
    keep = plain[0]["k"]
    add_image_cache(plain, S, torch.bfloat16, "cpu")                                      # a foreign dict gets them added
    assert plain[0]["k"] is keep and tuple(plain[1]["v_img"].shape) == (3, 257, 4, 128)
    kimg = plain[0]["k_img"]
    add_image_cache(plain, S, torch.bfloat16, "cpu")
    assert plain[0]["k_img"] is kimg


def test_pipeline_adds_the_reference_pose_map_to_y():
    """dwpose_data + random_ref_dwpose + input_image: y += embed_ref(random_ref_dwpose), [1, 20, 1, h, w] broadcast over time
    (causal_diffusion_inference.py:341-347), and the first pass gets frame 0 of the sum with the chunk's pose tokens.  The
    stand-in generator stops the rollout at its first call: everything behind it needs the GPU."""
    class Stop(Exception):
        pass

    seen = []

    class Gen:
        model = SimpleNamespace(num_layers=1, local_attn_size=-1, shape=S, model_type="i2v")

        def forward(self, **kw):
            seen.append(kw)
            raise Stop

        __call__ = forward

    g = torch.Generator().manual_seed(3)
    y = torch.randn(1, 20, 3, 8, 12, generator=g).to(torch.bfloat16)
    ref_map = torch.randn(1, 20, 1, 8, 12, generator=g).to(torch.bfloat16)
    tokens = torch.randn(1, 3 * 24, 8, generator=g)
    embedder = SimpleNamespace(embed=lambda d: (tokens, (3, 4, 6)), embed_ref=lambda r: ref_map)
    a = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, negative_prompt="", guidance_scale=3.0)
    pipe = sfa.CausalDiffusionInferencePipeline(a, "cpu", generator=Gen(), text_encoder=lambda text_prompts: {"prompt_embeds": None}, vae=object(),
                                                pose_embedder=embedder)
    pipe.encode_image = lambda img, n, h, w: {"clip_feature": torch.zeros(1, 257, 320), "y": y}
    noise = torch.zeros(1, 3, 16, 8, 12)
    dwpose, ref = torch.zeros(3, 9, 64, 96, dtype=torch.uint8), torch.zeros(64, 96, 3, dtype=torch.uint8)
    with pytest.raises(Stop):
        pipe.inference(noise, ["p"], torch.zeros(3, 64, 96), dwpose, ref)
    cond = seen[0]["conditional_dict"]
    assert torch.equal(cond["y"], (y + ref_map)[:, :, 0:1]) and not torch.equal(cond["y"], y[:, :, 0:1])
    assert torch.equal(cond["add_condition"], tokens[:, :24]) and tuple(cond["clip_feature"].shape) == (1, 257, 320)
    assert torch.equal(y, y.clone()) and pipe.pose_embedder is embedder
    # without the pose pair y goes through as encoded
    seen.clear()
    with pytest.raises(Stop):
        pipe.inference(noise, ["p"], torch.zeros(3, 64, 96), None, None)
    assert torch.equal(seen[0]["conditional_dict"]["y"], y[:, :, 0:1]) and "add_condition" not in seen[0]["conditional_dict"]
