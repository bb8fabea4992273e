"""Host-side checks of the CLIP image encoder (no GPU): the weight table against the reference's recorded names, the
checkpoint filter, the torch restatement against the reference's recorded outputs in both dtype policies, the patch-weight
repack, argument validation of the C entry points, the ctypes mirror, and the pipeline's early checks."""
import ctypes
import dataclasses
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import clip_reference as cr
from self_forcing_amd import clip_weights as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("clip_reduced_17", "clip_reduced_257", "clip_w1280_l16")
_cache = {}


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def fixture(tag):
    """(npz, shape, state dict, videos, recorded output as float32), built once per tag and left unchanged."""
    if tag not in _cache:
        g = np.load(os.path.join(GOLD, tag + ".npz"))
        s = cw.ClipVisionShape(**{str(k): (float(v) if k == "eps" else int(v)) for k, v in zip(g["shape_fields"], g["shape_values"])})
        sd = cw.synth_clip_state_dict(s, int(g["seed"]))
        videos = [cw.synth_frames(*(int(x) for x in v)) for v in g["videos"]]
        _cache[tag] = (g, s, sd, videos, torch.from_numpy(g["out"].astype(np.float32)))
    return _cache[tag]


def test_param_shapes_match_the_reference():
    for tag in ("clip_reduced_17", "clip_w1280_l16"):
        g, s, _, _, _ = fixture(tag)
        want = [(cw.PREFIX + str(k), tuple(int(v) for v in shp.split(","))) for k, shp in zip(g["state_keys"], g["state_shapes"])]
        assert want == list(cw.clip_param_shapes(s).items())
    # the full tower differs from the recorded 16-layer one only in its depth
    g, s, _, _, _ = fixture("clip_w1280_l16")
    assert dataclasses.replace(s, num_layers=32) == cw.CLIP_VIT_H_14
    full, rec = cw.clip_param_shapes(cw.CLIP_VIT_H_14), cw.clip_param_shapes(s)
    assert all(full[k] == v for k, v in rec.items()) and len(full) == len(rec) + 16 * 12
    assert all(full[f"visual.transformer.31.{k}"] == full[f"visual.transformer.0.{k}"] for k in ("attn.to_qkv.weight", "mlp.2.bias", "norm1.weight"))
    n = sum(int(np.prod(v)) for v in full.values())
    assert abs(n - 632e6) < 1e6                                  # ViT-H/14: 632 M parameters
    assert cw.CLIP_VIT_H_14.seq_len == 257 and cw.CLIP_VIT_H_14.patch_kp == 640 and cw.CLIP_VIT_H_14.layers_built == 31
    assert (cw.CLIP_REDUCED.dim, cw.CLIP_REDUCED.num_heads, cw.CLIP_REDUCED.num_layers, cw.CLIP_REDUCED.head_dim) == (320, 4, 3, 80)


def test_synth_state_dict_is_deterministic():
    a, b, c = (cw.synth_clip_state_dict(cw.CLIP_REDUCED, seed) for seed in (0, 0, 1))
    assert list(a) == list(cw.clip_param_shapes(cw.CLIP_REDUCED))
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["visual.cls_embedding"], c["visual.cls_embedding"])
    half = cw.synth_clip_state_dict(cw.CLIP_REDUCED, 0, dtype=torch.bfloat16)
    assert half["visual.transformer.0.mlp.0.weight"].dtype == torch.bfloat16 and half["visual.pre_norm.weight"].dtype == torch.float32
    assert torch.equal(half["visual.transformer.0.mlp.0.weight"], a["visual.transformer.0.mlp.0.weight"].bfloat16())


def test_checkpoint_filter_and_errors():
    s = cw.CLIP_REDUCED
    sd = cw.synth_clip_state_dict(s, 0)
    full = dict(sd)
    full["textual.token_embedding.weight"] = torch.zeros(4, 4)
    full["log_scale"] = torch.zeros(())
    a = cw.visual_state_dict(full, s)
    bare = {k[len(cw.PREFIX):]: v for k, v in sd.items()}
    b = cw.visual_state_dict(bare, s)
    assert list(a) == list(b) == list(bare) and all(a[k] is sd[cw.PREFIX + k] for k in a)
    # what use_31_block never runs may be absent, and is never uploaded
    needed = cw.needed_param_shapes(s)
    trimmed = {k: v for k, v in bare.items() if k in needed}
    assert len(trimmed) == len(bare) - 12 - 3 and list(cw.visual_state_dict(trimmed, s)) == list(trimmed)
    assert not any(k == "head" or k.startswith("post_norm") or k.startswith("transformer.2.") for k in needed)
    enc = sfa.CLIPVisionEncoder(s, full, device="cpu")
    assert enc.param_bytes() == sum((4 if ("norm" in k or "embedding" in k and "patch" not in k) else 2) * int(np.prod(v))
                                    for k, v in needed.items()) + 2 * s.dim * (s.patch_kp - s.patch_k)
    wrong = dict(bare)
    wrong["transformer.1.mlp.0.weight"] = torch.zeros(4, 4)
    with pytest.raises(ValueError, match=r"transformer\.1\.mlp\.0\.weight: expected shape \(1280, 320\)"):
        cw.visual_state_dict(wrong, s)
    missing = {k: v for k, v in full.items() if k != "visual.transformer.0.attn.proj.bias"}
    with pytest.raises(KeyError, match=r"visual\.transformer\.0\.attn\.proj\.bias"):
        cw.visual_state_dict(missing, s)
    with pytest.raises(KeyError, match="pre_norm.weight"):
        sfa.CLIPModel(state_dict={k: v for k, v in bare.items() if k != "pre_norm.weight"}, shape=s, device="cpu")
    with pytest.raises(ValueError, match="head_dim 80"):
        sfa.CLIPVisionEncoder(dataclasses.replace(s, num_heads=5), cw.synth_clip_state_dict(dataclasses.replace(s, num_heads=5), 0), device="cpu")


@pytest.mark.parametrize("tag", FIXTURES)
def test_restatement_reproduces_the_reference_in_fp32(tag):
    """Own fp32 code against the reference's recorded fp32 run: fp32 round-off (1e-5); the float16 fixture adds its storage
    (2^-11 per element, 2.8e-4 in the norm; bound 1e-3)."""
    g, s, sd, videos, gold = fixture(tag)
    out = cr.clip_visual_reference(sd, s, videos, "fp32")
    assert out.shape == gold.shape == (sum(int(v[1]) for v in g["videos"]), s.seq_len, s.dim) and out.dtype == torch.float32
    err = rel(out, gold)
    print(f"{tag}: restatement fp32 vs reference {err:.3e}")
    assert err < (1e-3 if g["out"].dtype == np.float16 else 1e-5)


@pytest.mark.parametrize("tag", FIXTURES)
def test_restatement_autocast_policy_lands_on_the_reference_floor(tag):
    """The `autocast_bf16` policy rounds where the reference's autocast run rounds: its distance from the fp32 run is the
    recorded floor to within 10 %.  A bf16 residual stream (what the fp32 stream kernels avoid) is visibly further out."""
    g, s, sd, videos, gold = fixture(tag)
    floor = float(g["floor"])
    err = rel(cr.clip_visual_reference(sd, s, videos, "autocast_bf16"), gold)
    print(f"{tag}: autocast_bf16 {err:.3e} = {err / floor:.3f} x floor {floor:.3e}")
    assert floor / 1.1 < err < 1.1 * floor
    if tag == "clip_w1280_l16":
        worse = rel(cr.clip_visual_reference(sd, s, videos, "autocast_bf16", residual="bf16"), gold)
        print(f"{tag}: bf16 residual stream {worse / floor:.3f} x floor")
        assert worse > 1.5 * floor


def test_preprocess_restatement_and_patch_repack():
    s = dataclasses.replace(cw.CLIP_REDUCED, image_size=56)
    sd = cw.synth_clip_state_dict(s, 3)
    w = sd["visual.patch_embedding.weight"]
    same = cw.synth_frames(5, 2, 56, 56)
    pre = cr.clip_preprocess([same], 56)
    mean, std = torch.tensor(cw.CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(cw.CLIP_STD).view(1, 3, 1, 1)
    assert torch.equal(pre, (same.transpose(0, 1) * 0.5 + 0.5 - mean) / std)          # bicubic at scale 1 is the identity
    rows = cr.patch_rows(pre, s.patch_size, s.patch_kp)
    packed = cw.repack_patch_weight(w, s.patch_kp)
    assert rows.shape == (2 * 16, 640) and packed.shape == (320, 640)
    assert (packed[:, s.patch_k:] == 0).all() and (rows[:, s.patch_k:] == 0).all()
    conv = F.conv2d(pre, w, stride=s.patch_size).flatten(2).transpose(1, 2).reshape(32, 320)
    assert rel(rows @ packed.t(), conv) < 1e-6
    with pytest.raises(ValueError, match="more than kp"):
        cw.repack_patch_weight(w, 576)


def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    err = lambda: lib.sf_last_error()  # noqa: E731
    p = 4096
    assert lib.sf_clip_preprocess(None, 0, 1, 8, 8, 224, 14, 640, p, None) != 0 and b"null tensor" in err()
    assert lib.sf_clip_preprocess(p, 2, 1, 8, 8, 224, 14, 640, p, None) != 0 and b"dtype" in err()
    assert lib.sf_clip_preprocess(p, 0, 1, 8, 8, 225, 14, 640, p, None) != 0 and b"multiple of patch" in err()
    assert lib.sf_clip_preprocess(p, 0, 1, 8, 8, 224, 14, 576, p, None) != 0 and b"kp=576" in err()
    assert lib.sf_clip_preprocess(p, 0, 0, 8, 8, 224, 14, 640, p, None) != 0 and b"n=0" in err()
    assert lib.sf_clip_embed_norm(p, p, p, p, p, p, p, None, p, 1, 16, 320, 1e-5, None) != 0 and b"null tensor" in err()
    assert lib.sf_clip_embed_norm(p, p, p, p, p, p, None, p, p, 1, 16, 320, 1e-5, None) != 0 and b"ln_w needs" in err()
    assert lib.sf_clip_embed_norm(p, p, p, p, p, p, p, p, p, 1, 16, 322, 1e-5, None) != 0 and b"dim=322" in err()
    assert lib.sf_clip_embed_norm(p, p, p, p + 4, p, p, p, p, p, 1, 16, 320, 1e-5, None) != 0 and b"misaligned" in err()
    assert lib.sf_clip_add_layernorm(None, p, p, p, p, 4, 320, 1e-5, None) != 0 and b"null tensor" in err()
    assert lib.sf_clip_add_layernorm(p, p, p, None, p, 4, 320, 1e-5, None) != 0 and b"ln_w needs" in err()
    assert lib.sf_clip_add_layernorm(p, p, p, p, p, 4, 16384, 1e-5, None) != 0 and b"at most 8192" in err()
    assert lib.sf_clip_add_layernorm(p, p, p, p, p, 0, 320, 1e-5, None) != 0 and b"rows=0" in err()
    assert lib.sf_clip_add_layernorm(p + 8, p, p, p, p, 4, 320, 1e-5, None) != 0 and b"misaligned" in err()
    assert lib.sf_clip_attention(None, p, 1, 17, 4, None) != 0 and b"null tensor" in err()
    assert lib.sf_clip_attention(p, p, 1, 0, 4, None) != 0 and b"L=0" in err()
    assert lib.sf_clip_attention(p, p, 1, 481, 4, None) != 0 and b"L=481" in err()
    assert lib.sf_clip_attention(p, p, 0, 17, 4, None) != 0 and b"n=0" in err()
    assert lib.sf_clip_attention(p + 8, p, 1, 17, 4, None) != 0 and b"misaligned" in err()
    assert lib.sf_clip_gelu(p, p, 12, None) != 0 and b"count=12" in err()
    assert lib.sf_clip_gelu(None, p, 16, None) != 0 and b"count=16" in err()
    assert lib.sf_clip_workspace_bytes(None, 1) == 0 and b"null model" in err()

    def model(**kw):
        m = sfa._lib.ClipModel()
        m.image_size, m.patch, m.dim, m.heads, m.mlp_dim, m.layers_built, m.eps = 224, 14, 320, 4, 1280, 0, 1e-5
        m.patch_w = m.cls = m.pos = m.pre_norm_w = m.pre_norm_b = p
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    assert lib.sf_clip_workspace_bytes(model(), 1) > 0
    assert lib.sf_clip_workspace_bytes(model(), 0) == 0 and b"n=0" in err()
    assert lib.sf_clip_workspace_bytes(model(dim=352, heads=4), 1) == 0 and b"multiple of 64" in err()
    assert lib.sf_clip_workspace_bytes(model(heads=5), 1) == 0 and b"head dimension must be 80" in err()
    assert lib.sf_clip_workspace_bytes(model(image_size=225), 1) == 0 and b"multiple of patch" in err()
    assert lib.sf_clip_workspace_bytes(model(image_size=336), 1) == 0 and b"577 tokens" in err()
    assert lib.sf_clip_workspace_bytes(model(cls=None), 1) == 0 and b"null tensor" in err()
    assert lib.sf_clip_workspace_bytes(model(layers_built=2), 1) == 0 and b"null tensor" in err()
    layers = (sfa._lib.ClipLayer * 2)()
    two = model(layers_built=2, layers_host=ctypes.cast(layers, ctypes.POINTER(sfa._lib.ClipLayer)))
    assert lib.sf_clip_workspace_bytes(two, 1) == 0 and b"null tensor in block 0" in err()

    enc = sfa.CLIPVisionEncoder(cw.CLIP_REDUCED, cw.synth_clip_state_dict(cw.CLIP_REDUCED, 0), device="cpu")
    cm = ctypes.byref(enc.cmodel)
    one, eight = enc.workspace_bytes(1), enc.workspace_bytes(8)
    assert 0 < one < eight <= 8 * one
    assert lib.sf_clip_encode(cm, None, 0, 1, 40, 72, p, p, 1 << 40, None) != 0 and b"null tensor" in err()
    assert lib.sf_clip_encode(cm, p, 3, 1, 40, 72, p, p, 1 << 40, None) != 0 and b"dtype" in err()
    assert lib.sf_clip_encode(cm, p, 0, 1, 0, 72, p, p, 1 << 40, None) != 0 and b"0 x 72" in err()
    assert lib.sf_clip_encode(cm, p, 0, 1, 40, 72, p, p, one - 1, None) != 0 and b"workspace too small" in err()
    assert lib.sf_clip_encode(cm, p, 0, 1, 40, 72, p, None, 0, None) != 0 and b"workspace too small" in err()
    with pytest.raises(sfa._lib.SfHipError, match="n=0"):
        enc.workspace_bytes(0)


def test_ctypes_mirror_matches_the_header():
    """(Field names and argument counts against the header: test_host_logic.test_ctypes_mirror_matches_the_header.)"""
    text = open(os.path.join(ROOT, "include", "sf_hip.h")).read()
    assert ctypes.sizeof(sfa._lib.ClipLayer) == 12 * 8 and ctypes.sizeof(sfa._lib.ClipModel) == 32 + 6 * 8
    assert sfa._lib.ClipModel.patch_w.offset == 32 and sfa._lib.ClipModel.eps.offset == 24
    enum = re.search(r"enum sf_clip_dtype \{(.*?)\}", text).group(1)
    assert re.sub(r"\s", "", enum) == "SF_CLIP_F32=0,SF_CLIP_BF16=1" and sfa._lib.CLIP_DTYPES == {"float32": 0, "bfloat16": 1}
    assert int(re.search(r"#define SF_HIP_ABI_VERSION (\d+)", text).group(1)) == 11
    assert "clip_encode" in sfa.torch_ops.OPS and "Tensor(a2!) workspace" in str(torch.ops.sf_hip.clip_encode.default._schema)


def test_clip_encode_fake_and_model_surface():
    from torch._subclasses.fake_tensor import FakeTensorMode
    model = sfa.CLIPModel(state_dict=cw.synth_clip_state_dict(cw.CLIP_REDUCED, 0), shape=cw.CLIP_REDUCED, device="cpu")
    with FakeTensorMode():
        out = torch.ops.sf_hip.clip_encode(model.model._handle, torch.empty(3, 3, 40, 72, device="cuda"), torch.empty(16, dtype=torch.uint8, device="cuda"))
        assert tuple(out.shape) == (3, 257, 320) and out.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="pos_interpolate"):
        model.visual([torch.zeros(3, 1, 8, 8)], interpolation=True)
    with pytest.raises(NotImplementedError, match="text tower"):
        model.textual(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(ValueError, match=r"\[3, T, H, W\]"):
        model.visual([torch.zeros(1, 3, 8, 8)])
    with pytest.raises(ValueError, match="no CPU fallback"):
        model.visual([torch.zeros(3, 1, 8, 8)])
    with pytest.raises(FileNotFoundError, match="CLIP checkpoint"):
        sfa.CLIPModel(torch.bfloat16, "cpu", "/nonexistent/models_clip.pth", None)


def test_clip_checkpoint_loads_weights_only(tmp_path):
    s = cw.CLIP_REDUCED
    sd = cw.synth_clip_state_dict(s, 0)
    sd["log_scale"] = torch.zeros(())
    path = str(tmp_path / "clip.pth")
    torch.save(sd, path)
    model = sfa.CLIPModel(torch.bfloat16, "cpu", path, None, shape=s)
    assert model.checkpoint_path == path and model.model.param_bytes() > 0
    with pytest.raises(ValueError, match="expected shape"):                    # the default shape is the full ViT-H/14
        sfa.CLIPModel(torch.bfloat16, "cpu", path, None)
    torch.save({"visual.cls_embedding": SimpleNamespace(x=1)}, path)          # a pickled object: refused by weights_only
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|unpickl"):
        sfa.CLIPModel(torch.bfloat16, "cpu", path, None, shape=s)


def test_pipeline_encode_image_needs_an_encoder():
    pipe = sfa.CausalDiffusionInferencePipeline.__new__(sfa.CausalDiffusionInferencePipeline)
    torch.nn.Module.__init__(pipe)
    pipe.device, pipe.torch_dtype, pipe.image_encoder, pipe.clip_checkpoint_path = torch.device("cpu"), torch.bfloat16, None, None
    with pytest.raises(ValueError, match="args.clip_checkpoint_path"):
        pipe.encode_image(torch.zeros(3, 128, 128), 5, 128, 128)
    with pytest.raises(ValueError, match="4 k \\+ 1"):
        pipe.encode_image(torch.zeros(3, 128, 128), 6, 128, 128)
    pipe.clip_checkpoint_path = "/nonexistent/models_clip.pth"
    with pytest.raises(FileNotFoundError, match="CLIP checkpoint"):
        pipe.encode_image(torch.zeros(3, 128, 128), 5, 128, 128)
    with pytest.raises(NotImplementedError, match="encode_image"):
        pipe.inference(torch.zeros(1, 3, 16, 16, 16), ["p"], input_image=torch.zeros(3, 128, 128))
