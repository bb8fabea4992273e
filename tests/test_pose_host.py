"""Host-side checks of the pose front end (no GPU): weight table, the torch restatement against the reference's recorded
outputs, weight repacking in the kernel's K order, the shape plan, weight-file semantics, argument validation of the C
entry points and the pipeline's early checks."""
import ctypes
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import self_forcing_amd as sfa
from self_forcing_amd import pose_weights as pw

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KINDS = ("dense", "skeleton")


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def small(tag, kind):
    g = np.load(os.path.join(GOLD, f"pose_small_{tag}_{kind}.npz"))
    tokens = np.stack([np.load(os.path.join(GOLD, f"pose_small_{tag}_{kind}_f{f}.npz"))["tokens_f32"] for f in range(int(g["plan"][0]))])
    return g, torch.from_numpy(tokens.astype(np.float32))


def test_state_dict_names_and_shapes_match_the_reference():
    g = np.load(os.path.join(GOLD, "pose_small_a_dense.npz"))
    want = [(str(k), tuple(int(v) for v in s.split(","))) for k, s in zip(g["state_keys"], g["state_shapes"])]
    assert want == list(pw.pose_param_shapes().items())
    sd = pw.synth_pose_state_dict(int(g["seed"]))
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want and all(v.dtype == torch.float32 for v in sd.values())
    assert len(want) == 26 and want[12] == ("dwpose_embedding.12.weight", (5120, 16, 1, 2, 2))
    assert torch.equal(sd["dwpose_embedding.0.weight"], pw.synth_pose_state_dict(int(g["seed"]))["dwpose_embedding.0.weight"])
    w = sd["dwpose_embedding.4.weight"]
    assert abs(w.std().item() * (16 * 27) ** 0.5 - 1.6) < 0.05 and abs(sd["dwpose_embedding.12.bias"].std().item() - 0.1) < 0.01


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("kind", KINDS)
def test_torch_restatement_reproduces_the_reference(tag, kind):
    """Own fp32 code (F.conv3d / F.conv2d) against the reference modules' recorded fp32 outputs: fp32 round-off plus the
    fixture's float16 storage (2^-11 relative per element, ~2.8e-4 in the norm) -- so the comparison is against the
    fixture rounded the same way, to 1e-5."""
    g, gold = small(tag, kind)
    sd = pw.synth_pose_state_dict(int(g["seed"]))
    clip, image = torch.from_numpy(g["clip_u8"]), torch.from_numpy(g["image_u8"])
    emb, ref_map = pw.pose_stacks_torch(sd, clip, image)
    f, h, w = (int(v) for v in g["plan"])
    assert emb.shape == (1, 5120, f, h, w) and ref_map.shape == (1, 20, 1) + pw.ref_plan(*image.shape[:2])
    tokens = emb[0].permute(1, 2, 3, 0).flatten(1, 2)
    assert rel(tokens.half().float(), gold) <= 1e-5
    assert rel(ref_map[0, :, 0].half().float(), torch.from_numpy(g["ref_map_f32"].astype(np.float32))) <= 1e-5


def conv_in_kernel_k_order(x, w_packed, bias, cin_store, cout, kt, st, ss):
    """x [T, H, W, cin_store] -> [To, Ho, Wo, cout] tap by tap in the packed K order: k = ((dt*3 + dh)*3 + dw)*cin_store + ci,
    input voxel (t*st - pt + dt, h*ss - 1 + dh, w*ss - 1 + dw), zeros outside."""
    T, H, W, _ = x.shape
    pt = 1 if kt == 3 else 0
    To = (T - 1) // st + 1 if kt == 3 else T
    Ho, Wo = (H - 1) // ss + 1, (W - 1) // ss + 1
    xp = F.pad(x, (0, 0, 1, 1 + ss, 1, 1 + ss, pt, pt + st))
    out = bias[:cout].double().expand(To, Ho, Wo, cout).clone()
    for dt in range(kt):
        for dh in range(3):
            for dw in range(3):
                k0 = ((dt * 3 + dh) * 3 + dw) * cin_store
                patch = xp[dt:dt + (To - 1) * st + 1:st, dh:dh + (Ho - 1) * ss + 1:ss, dw:dw + (Wo - 1) * ss + 1:ss]
                out += patch.double() @ w_packed[:cout, k0:k0 + cin_store].double().t()
    return out


@pytest.mark.parametrize("cin,cout,kt,st,ss", [(3, 16, 3, 1, 1), (16, 16, 3, 1, 1), (16, 16, 3, 1, 2), (16, 16, 3, 2, 2),
                                               (3, 16, 1, 1, 1), (16, 16, 1, 1, 2), (16, 20, 1, 1, 2)])
def test_repacked_weights_in_kernel_k_order_equal_torch_conv(cin, cout, kt, st, ss):
    g = torch.Generator().manual_seed(cin * 100 + cout + kt + st + ss)
    T = 5 if kt == 3 else 1
    x = torch.randn(1, cin, T, 7, 10, generator=g)
    w = torch.randn(cout, cin, kt, 3, 3, generator=g)
    b = torch.randn(cout, generator=g)
    ref = F.conv3d(x, w, b, stride=(st, ss, ss), padding=(1 if kt == 3 else 0, 1, 1))[0].permute(1, 2, 3, 0)
    cs = 8 if cin == 3 else 16
    wp, bp = pw.repack_pose_conv(w if kt == 3 else w[:, :, 0], cs), pw.pad_pose_bias(b)
    assert wp.shape == (16 if cout <= 16 else 32, 32 * pw.pose_k_steps(9 * kt, cs)) and bp.shape[0] == wp.shape[0]
    assert wp[cout:].abs().sum() == 0 and wp[:, 9 * kt * cs:].abs().sum() == 0 and bp[cout:].abs().sum() == 0
    xs = torch.zeros(T, 7, 10, cs)
    xs[..., :cin] = x[0].permute(1, 2, 3, 0)
    out = conv_in_kernel_k_order(xs, wp, bp, cs, cout, kt, st, ss)
    assert out.shape == ref.shape and rel(out, ref) < 1e-6


def test_token_embedding_repack_is_the_2x2_patch_order():
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(1, 16, 2, 5, 6, generator=g), torch.randn(32, 16, 1, 2, 2, generator=g)
    ref = F.conv3d(x, w, None, stride=(1, 2, 2))[0].permute(1, 2, 3, 0)                       # [2, 2, 3, 32]
    xl = x[0].permute(1, 2, 3, 0)
    rows = torch.stack([xl[:, dh:dh + 4:2, dw:dw + 6:2] for dh in range(2) for dw in range(2)], dim=-2).flatten(-2)   # [(dh, dw), ci]
    assert rel(rows @ pw.repack_pose_embed(w).t(), ref) < 1e-6
    assert pw.pose_k_steps(27, 16) == 14 and pw.pose_k_steps(27, 8) == 7 and pw.pose_k_steps(9, 16) == 5 and pw.pose_k_steps(9, 8) == 3


def test_shape_plan():
    assert pw.pose_plan(81, 480, 832) == (21, 30, 52)
    assert pw.pose_plan(9, 120, 208) == (3, 7, 13)
    assert pw.pose_plan(9, 64, 96) == (3, 4, 6)
    assert pw.pose_plan(10, 64, 96) == (4, 4, 6)          # not 4k + 1: (10 + 3) -> 7 -> 4 frames
    assert pw.pose_plan(1, 16, 16) == (1, 1, 1)
    assert pw.pose_layer_volumes(81, 480, 832)[1:7] == [(84, 480, 832)] * 3 + [(84, 240, 416), (42, 120, 208), (21, 60, 104)]
    assert pw.ref_plan(480, 832) == (60, 104) and pw.ref_plan(120, 208) == (15, 26)
    with pytest.raises(ValueError):
        pw.pose_plan(9, 8, 8)
    lib = sfa._lib.lib()
    for n in (1, 2, 7, 15, 84, 480):
        assert lib.sf_pose_out_size(n, 3, 1) == n and lib.sf_pose_out_size(n, 3, 2) == (n - 1) // 2 + 1 and lib.sf_pose_out_size(n, 2, 2) == n // 2
    layers = pw.pose_embed_layers(81, 480, 832)
    full = [l for l in layers if l["name"] in ("dwpose_embedding.2", "dwpose_embedding.4")]
    assert all(abs(l["flops"] / 464e9 - 1) < 0.01 and abs(l["bytes"] / 2.147e9 - 1) < 0.01 for l in full)
    assert abs(pw.pose_embed_flops(81, 480, 832) / 1.17e12 - 1) < 0.03 and 8.0e9 < pw.pose_embed_bytes(81, 480, 832) < 9.0e9   # prepare and the 8-channel input volume included


def test_weight_loading_semantics(tmp_path):
    sd = pw.synth_pose_state_dict(1)
    dw, ref = pw.split_pose_state_dict(sd)
    assert set(dw) == {f"{i}.{p}" for i in range(0, 13, 2) for p in ("weight", "bias")} and set(ref) == {f"{i}.{p}" for i in range(0, 11, 2) for p in ("weight", "bias")}
    only_dw = {k: v for k, v in sd.items() if k.startswith("dwpose_embedding.")}
    assert pw.split_pose_state_dict(dict(only_dw, other=torch.zeros(1)))[1] is None
    with pytest.raises(ValueError, match="No pose embedding weights found"):
        pw.split_pose_state_dict({"generator.x": torch.zeros(1)})
    extra = dict(sd, **{"dwpose_embedding.14.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="unexpected"):
        pw.split_pose_state_dict(extra)
    assert "14.weight" not in pw.split_pose_state_dict(extra, strict=False)[0]
    lacking = {k: v for k, v in sd.items() if k != "dwpose_embedding.4.bias"}
    with pytest.raises(RuntimeError, match="missing"):
        pw.split_pose_state_dict(lacking)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert pw.split_pose_state_dict(lacking, strict=False)[0]["4.bias"].abs().sum() == 0 and len(rec) == 1
    with pytest.raises(RuntimeError, match="size mismatch"):
        pw.split_pose_state_dict(dict(sd, **{"dwpose_embedding.0.weight": torch.zeros(16, 4, 3, 3, 3)}), strict=False)
    # from a file, onto a device; the randomref stack may be absent
    path = str(tmp_path / "pose.pt")
    torch.save(only_dw, path)
    emb = sfa.PoseEmbedder(path, device="cpu")
    assert emb.has_dwpose and not emb.has_randomref and emb.cmodel.pose_dim == 5120 and emb.cmodel.conv[0].cin == 8 and emb.cmodel.conv[5].stride_t == 2
    with pytest.raises(RuntimeError, match="randomref"):
        emb.embed_ref(torch.zeros(16, 16, 3))


def test_pipeline_loads_pose_weights_once(tmp_path, monkeypatch):
    from self_forcing_amd import pose
    calls = []

    class Fake:
        def __init__(self, path, device=None, strict=True):
            calls.append((path, strict))

        def embed(self, d):
            return "tokens", (3, 4, 6)

    monkeypatch.setattr(pose, "PoseEmbedder", Fake)
    pipe = make_pipeline(pose_embedder=None, pose_weights_path="w.pt", pose_weights_strict=False)
    assert not pipe.pose_weights_loaded and pipe.pose_embedder is None
    assert pipe._pose_tokens(torch.zeros(3, 9, 64, 96)) == ("tokens", (3, 4, 6)) and pipe.pose_weights_loaded
    pipe._pose_tokens(torch.zeros(3, 9, 64, 96))
    assert calls == [("w.pt", False)]
    with pytest.raises(ValueError, match="pose_weights_path"):
        make_pipeline(pose_embedder=None)._pose_tokens(torch.zeros(3, 9, 64, 96))


def make_pipeline(pose_embedder=object(), **args):
    gen = SimpleNamespace(model=SimpleNamespace(num_layers=1, local_attn_size=-1, shape=sfa.WAN_REDUCED), forward=lambda **kw: None)
    a = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, independent_first_frame=False, negative_prompt="", guidance_scale=3.0, **args)
    return sfa.CausalDiffusionInferencePipeline(a, "cpu", generator=gen, text_encoder=object(), vae=object(), pose_embedder=pose_embedder)


def test_pipeline_checks_without_a_gpu():
    pipe = make_pipeline()
    noise = torch.zeros(1, 2, 16, 8, 12)
    clip, image = torch.zeros(3, 9, 64, 96, dtype=torch.uint8), torch.zeros(64, 96, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        pipe.inference(noise, ["p"], object(), None, None)
    with pytest.raises(NotImplementedError):
        pipe.inference(noise, ["p"], object(), clip, image)
    with pytest.raises(AssertionError, match="dwpose_data_emb has 3 frames, but expected 2 to match the output timeline."):
        pipe.inference(noise, ["p"], None, clip, image)
    with pytest.raises(ValueError, match="pose tokens per frame"):
        pipe.inference(torch.zeros(1, 3, 16, 16, 12), ["p"], None, clip, image)
    with pytest.raises(ValueError, match="not both"):
        pipe.inference(torch.zeros(1, 3, 16, 8, 12), ["p"], None, clip, image, dwpose_data_emb=torch.zeros(1, 5120, 3, 4, 6))
    import inspect
    params = list(inspect.signature(sfa.CausalDiffusionInferencePipeline.__init__).parameters)
    assert params[:7] == ["self", "args", "device", "generator", "text_encoder", "vae", "image_encoder"] and "pose_embedder" in params


def test_c_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = sfa._lib.lib()
    err = lambda: lib.sf_last_error()  # noqa: E731
    assert lib.sf_pose_conv(None, None) != 0 and b"null args" in err()
    a = sfa._lib.PoseConvArgs()
    assert lib.sf_pose_conv(a, None) != 0 and b"null tensor" in err()
    a.x, a.w, a.bias, a.out = 4096, 4096, 4096, 4096
    a.T, a.H, a.W, a.Cin, a.Cout, a.kt, a.stride_t, a.stride_s, a.ldw, a.ldo = 4, 8, 8, 32, 16, 3, 1, 1, 448, 16
    assert lib.sf_pose_conv(a, None) != 0 and b"Cin=32" in err()
    a.Cin, a.kt = 16, 2
    assert lib.sf_pose_conv(a, None) != 0 and b"kt must be 1 or 3" in err()
    a.kt, a.stride_s = 3, 3
    assert lib.sf_pose_conv(a, None) != 0 and b"strides" in err()
    a.stride_s, a.ldw = 1, 432
    assert lib.sf_pose_conv(a, None) != 0 and b"weight row stride" in err()
    a.ldw, a.Cout = 448, 18
    assert lib.sf_pose_conv(a, None) != 0 and b"Cout=18" in err()
    a.Cout, a.ldo = 16, 12
    assert lib.sf_pose_conv(a, None) != 0 and b"ldo" in err()
    a.ldo, a.x = 16, 4100
    assert lib.sf_pose_conv(a, None) != 0 and b"misaligned" in err()
    a.x, a.Cout, a.ldo = 4096, 20, 20
    assert lib.sf_pose_conv(a, None) != 0 and b"no kernel" in err()                      # 20 channels only on the (16, 1, 1, 2) layer
    a.Cout, a.ldo, a.T, a.H, a.W = 16, 16, 340, 480, 832                                 # 340 frames of 480 x 832 x 32 B = 4.35 GB
    assert lib.sf_pose_conv(a, None) != 0 and b"exceeds the 4 GiB" in err()
    assert lib.sf_pose_prepare(None, 0, 0, 9, 64, 96, 3, None, None) != 0 and b"null" in err()
    assert lib.sf_pose_prepare(4096, 5, 0, 9, 64, 96, 3, 4096, None) != 0 and b"dtype" in err()
    assert lib.sf_pose_prepare(4096, 0, 1, 2, 64, 96, 0, 4096, None) != 0 and b"one image" in err()
    assert lib.sf_pose_prepare(4096, 0, 0, 700, 480, 832, 3, 4096, None) != 0 and b"4 GiB" in err()
    assert lib.sf_pose_scratch_bytes(None, 9, 64, 96) == 0 and b"null model" in err()
    m = sfa._lib.PoseModel()
    assert lib.sf_pose_scratch_bytes(m, 9, 64, 96) == 0 and b"no weights" in err()
    emb = sfa.PoseEmbedder(pw.synth_pose_state_dict(0), device="cpu")
    small_bytes, big_bytes = emb.scratch_bytes(9, 64, 96), emb.scratch_bytes(81, 480, 832)
    assert 0 < small_bytes < big_bytes < 3.5e9 and emb.scratch_bytes(0, 480, 832) > 0
    assert emb.scratch_bytes(84, 720, 1280) > 0                                          # 2.5 GB volumes: still addressable
    with pytest.raises(sfa._lib.SfHipError, match="beyond the 4 GiB"):
        emb.scratch_bytes(200, 720, 1280)
    cm = ctypes.byref(emb.cmodel)
    assert lib.sf_pose_embed(cm, None, 0, 9, 64, 96, None, 0, None, 72, None) != 0 and b"null buffer" in err()
    assert lib.sf_pose_embed(cm, 4096, 0, 9, 64, 96, 4096, 1 << 40, 4096, 71, None) != 0 and b"3 x 4 x 6 = 72" in err()
    assert lib.sf_pose_embed(cm, 4096, 0, 9, 64, 96, 4096, 16, 4096, 72, None) != 0 and b"needed" in err()
    assert lib.sf_pose_embed(cm, 4096, 0, 200, 720, 1280, 4096, 1 << 40, 4096, 72, None) != 0 and b"4 GiB" in err()
    assert lib.sf_pose_embed(cm, 4096, 0, 9, 8, 8, 4096, 1 << 40, 4096, 72, None) != 0 and b"tokens" in err()
    assert lib.sf_pose_embed_ref(cm, None, 0, 64, 96, None, 0, None, None) != 0 and b"null buffer" in err()
    assert lib.sf_pose_embed_ref(cm, 4096, 0, 64, 96, 4096, 16, 4096, None) != 0 and b"needed" in err()
    assert lib.sf_pose_embed_ref(ctypes.byref(m), 4096, 0, 64, 96, 4096, 1 << 40, 4096, None) != 0 and b"no weights" in err()
    assert ctypes.sizeof(sfa._lib.PoseLayer) == 48 and ctypes.sizeof(sfa._lib.PoseConvArgs) == 4 * 8 + 11 * 4 + 4
    assert ctypes.sizeof(sfa._lib.PoseModel) == 6 * 48 + 8 + 8 + 8 + 6 * 48


def test_generate_pose_flags(tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(__file__))
    r = subprocess.run([sys.executable, os.path.join(root, "generate.py"), "--config_path", os.path.join(root, "configs", "tiny_test_hotpath.yaml"),
                        "--data_path", "d", "--output_folder", str(tmp_path), "--pose_path", "p.npy", "--pose_random_init_seed", "0"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "multi-step" in (r.stderr + r.stdout)
