"""Layer tables, seeded weights, weight repacking, shape plan, weight-file semantics and FLOP / byte counts of the pose
front end (pipeline/causal_diffusion_inference.py:87-145, :329-343 of the reference).

`dwpose_embedding` is an `nn.Sequential` of seven `Conv3d` (indices 0, 2, ..., 12; `SiLU` between them),
`randomref_embedding_pose` one of six `Conv2d` (indices 0, 2, ..., 10).  Their `state_dict()` names are
`<index>.weight` / `<index>.bias`; a pose weight file prefixes them with `dwpose_embedding.` /
`randomref_embedding_pose.`.

Pure host code: nothing here touches the GPU.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

Tensor = torch.Tensor

POSE_DIM = 5120            # token width: the last Conv3d's output channels (:102)
POSE_MID = 16              # CONCAT_DIM * 4 (:88)
RANDOMREF_DIM = 20         # :108
LEAD_FRAMES = 3            # the first pose frame is repeated three times in front of the clip (:339)
CIN_STORE = 8              # the three input channels are stored padded to 8 (one 16-byte piece per voxel)
DWPOSE_PREFIX, RANDOMREF_PREFIX = "dwpose_embedding.", "randomref_embedding_pose."

# (Sequential index, cin, cout, kernel, stride, padding, SiLU behind it)
DWPOSE_LAYERS = (
    (0, 3, POSE_MID, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    (2, POSE_MID, POSE_MID, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    (4, POSE_MID, POSE_MID, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    (6, POSE_MID, POSE_MID, (3, 3, 3), (1, 2, 2), (1, 1, 1), True),
    (8, POSE_MID, POSE_MID, (3, 3, 3), (2, 2, 2), (1, 1, 1), True),
    (10, POSE_MID, POSE_MID, (3, 3, 3), (2, 2, 2), (1, 1, 1), True),
    (12, POSE_MID, POSE_DIM, (1, 2, 2), (1, 2, 2), (0, 0, 0), False),
)
RANDOMREF_LAYERS = (
    (0, 3, POSE_MID, (3, 3), (1, 1), (1, 1), True),
    (2, POSE_MID, POSE_MID, (3, 3), (1, 1), (1, 1), True),
    (4, POSE_MID, POSE_MID, (3, 3), (1, 1), (1, 1), True),
    (6, POSE_MID, POSE_MID, (3, 3), (2, 2), (1, 1), True),
    (8, POSE_MID, POSE_MID, (3, 3), (2, 2), (1, 1), True),
    (10, POSE_MID, RANDOMREF_DIM, (3, 3), (2, 2), (1, 1), False),
)


def pose_param_shapes() -> Dict[str, Tuple[int, ...]]:
    """Tensor names -> shapes of a pose weight file, in the order of the reference modules' `state_dict()`s (the dwpose
    stack first)."""
    ps: Dict[str, Tuple[int, ...]] = {}
    for prefix, layers in ((DWPOSE_PREFIX, DWPOSE_LAYERS), (RANDOMREF_PREFIX, RANDOMREF_LAYERS)):
        for idx, cin, cout, k, _, _, _ in layers:
            ps[f"{prefix}{idx}.weight"] = (cout, cin) + tuple(k)
            ps[f"{prefix}{idx}.bias"] = (cout,)
    return ps


def synth_pose_state_dict(seed: int = 0) -> Dict[str, Tensor]:
    """Seeded float32 pose weights on the CPU (there is no trained pose checkpoint to load): weights N(0, (1.6 / sqrt(fan_in))^2),
    biases N(0, 0.1^2), drawn tensor by tensor in `pose_param_shapes` order.  The gain keeps the activation rms near
    constant through the SiLU stack (the default nn.Conv init lets it collapse), so every layer contributes to the
    output the tests compare."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out: Dict[str, Tensor] = {}
    for name, shape in pose_param_shapes().items():
        if name.endswith(".bias"):
            out[name] = 0.1 * torch.randn(shape, generator=g)
        else:
            out[name] = (1.6 / math.sqrt(math.prod(shape[1:]))) * torch.randn(shape, generator=g)
    return out


# ---------------------------------------------------------------------------------------- weight files
def split_pose_state_dict(state_dict: Dict[str, Tensor], strict: bool = True) -> Tuple[Optional[Dict[str, Tensor]], Optional[Dict[str, Tensor]]]:
    """`load_pose_embedding_weights` (:124-145): the tensors under `dwpose_embedding.` and under
    `randomref_embedding_pose.`, prefixes removed; a stack without any tensor is None (the reference leaves it alone),
    ValueError when neither is present.  A present stack is checked as `load_state_dict(strict=...)` does: a shape
    mismatch always raises, missing / unexpected names raise under `strict`; without it unexpected names are dropped and
    a missing tensor is zero (with a warning: the reference would keep its random initialisation)."""
    need = pose_param_shapes()
    out = []
    for prefix in (DWPOSE_PREFIX, RANDOMREF_PREFIX):
        sd = {k.split(prefix, 1)[1]: v for k, v in state_dict.items() if k.startswith(prefix)}
        if not sd:
            out.append(None)
            continue
        want = {k[len(prefix):]: s for k, s in need.items() if k.startswith(prefix)}
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {prefix[:-1]}: missing {missing}, unexpected {unexpected}")
        for k in unexpected:
            del sd[k]
        for k, shape in want.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {prefix}{k}: expected {tuple(shape)}, got {tuple(sd[k].shape)}")
        for k in missing:
            warnings.warn(f"pose weights: {prefix}{k} is missing (strict=False): using zeros")
            sd[k] = torch.zeros(want[k])
        out.append(sd)
    if out[0] is None and out[1] is None:
        raise ValueError("No pose embedding weights found in state_dict.")
    return out[0], out[1]


# ---------------------------------------------------------------------------------------- repacking
def pose_k_steps(ntaps: int, cin_store: int) -> int:
    """32-deep k-steps of a layer: taps * cin_store rounded up (27 taps of 16 channels pad to 28: K = 448)."""
    return (ntaps * cin_store + 31) // 32


def repack_pose_conv(w: Tensor, cin_store: int = 0) -> Tensor:
    """Conv weight [Cout, Cin, kt, 3, 3] (or [Cout, Cin, 3, 3]: kt = 1) -> `sf_pose_conv_args.w`: [16 or 32 rows][Kpad]
    with k = ((dt*3 + dh)*3 + dw)*cin_store + ci; channels Cin..cin_store-1, k past the last tap and rows past Cout are
    zero.  cin_store defaults to Cin rounded up to 8."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin, kt, kh, kw = w.shape
    if (kh, kw) != (3, 3) or kt not in (1, 3) or cout > 32:
        raise ValueError(f"repack_pose_conv: expected a [<=32, Cin, 1|3, 3, 3] weight, got {tuple(w.shape)}")
    cs = cin_store or ((cin + 7) // 8) * 8
    if cs not in (8, 16) or cin > cs:
        raise ValueError(f"repack_pose_conv: {cin} channels cannot be stored as {cs}")
    t = torch.zeros(cout, kt, 3, 3, cs, dtype=w.dtype)
    t[..., :cin] = w.permute(0, 2, 3, 4, 1)
    k = kt * 9 * cs
    out = torch.zeros(16 if cout <= 16 else 32, 32 * pose_k_steps(kt * 9, cs), dtype=w.dtype)
    out[:cout, :k] = t.reshape(cout, k)
    return out


def pad_pose_bias(b: Tensor) -> Tensor:
    """Bias [Cout] -> float32 [16 or 32], zero past Cout."""
    out = torch.zeros(16 if b.numel() <= 16 else 32, dtype=torch.float32)
    out[:b.numel()] = b.float()
    return out


def repack_pose_embed(w: Tensor) -> Tensor:
    """The last Conv3d's weight [5120, 16, 1, 2, 2] -> [5120][64] with k = (dh*2 + dw)*16 + ci, the row order of the
    gathered 2x2 patches."""
    cout, cin, kt, kh, kw = w.shape
    if (kt, kh, kw) != (1, 2, 2) or cin != POSE_MID:
        raise ValueError(f"repack_pose_embed: expected [N, {POSE_MID}, 1, 2, 2], got {tuple(w.shape)}")
    return w[:, :, 0].permute(0, 2, 3, 1).reshape(cout, 4 * cin).contiguous()


# ---------------------------------------------------------------------------------------- shapes
def _out(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def pose_layer_volumes(num_pose_frames: int, H: int, W: int) -> List[Tuple[int, int, int]]:
    """(T, H, W) of the dwpose stack's input (with the three repeated frames) and of every layer's output."""
    v = [(num_pose_frames + LEAD_FRAMES, H, W)]
    for _, _, _, k, s, p, _ in DWPOSE_LAYERS:
        t, h, w = v[-1]
        v.append((_out(t, k[0], s[0], p[0]), _out(h, k[1], s[1], p[1]), _out(w, k[2], s[2], p[2])))
    return v


def pose_plan(num_pose_frames: int, H: int, W: int) -> Tuple[int, int, int]:
    """(F', h, w) of the pose tokens for `num_pose_frames` frames of H x W: (81, 480, 832) -> (21, 30, 52)."""
    if num_pose_frames < 1 or H < 1 or W < 1:
        raise ValueError(f"pose_plan: empty clip {num_pose_frames} x {H} x {W}")
    f, h, w = pose_layer_volumes(num_pose_frames, H, W)[-1]
    if min(f, h, w) < 1:
        raise ValueError(f"pose_plan: {num_pose_frames} frames of {H}x{W} give no tokens")
    return f, h, w


# ---------------------------------------------------------------------------------------- a clip in pieces
# Level 0 is the stack's input (three copies of frame 0, then the pixel frames), level i + 1 the output of Conv3d i.
# Output frame t of a 3-tap layer with padding 1 reads input frames t*st - 1 .. t*st + 1, so of an OPEN clip a layer with
# N final input frames has N - 1 (stride 1) or N // 2 (stride 2) final output frames; a closed clip has them all.
POSE_LEVELS = len(DWPOSE_LAYERS)       # 7: the input and the six 3x3x3 layers' outputs (the last layer is per frame)
HISTORY_FRAMES = 2                     # frames of each layer input a later piece still reads


def pose_stream_frontier(frames_pushed: int, closed: bool = False) -> List[int]:
    """Final frames of every level once `frames_pushed` pixel frames are known: open, (P+3, P+2, P+1, P, P-1, (P-1)//2,
    (P-1)//4); closed, the sizes of `pose_layer_volumes`.  All zero without a frame."""
    f = [frames_pushed + LEAD_FRAMES if frames_pushed > 0 else 0]
    for _, _, _, k, s, p, _ in DWPOSE_LAYERS[:-1]:
        n = f[-1]
        f.append(0 if n <= 0 else _out(n, k[0], s[0], p[0]) if closed else (n - 1 if s[0] == 1 else n // 2))
    return f


def pose_stream_plan(frames_before: int, n: int, closing: bool = False) -> Tuple[List[int], List[int]]:
    """What a push of `n` pixel frames behind `frames_before` computes (`sf_pose_stream_plan`): (first, count) per level
    -- level l gains frames [first[l], first[l] + count[l]), and the layer that reads level l gets a window of
    HISTORY_FRAMES + count[l] frames starting at frame first[l] - HISTORY_FRAMES.  Latent frames made final: count[-1]."""
    if frames_before < 0 or n < 0:
        raise ValueError(f"pose_stream_plan: frames_before={frames_before} n={n}")
    if closing and frames_before + n == 0:
        raise ValueError("pose_stream_plan: closing a clip of no frames")
    f0, f1 = pose_stream_frontier(frames_before), pose_stream_frontier(frames_before + n, closing)
    return f0, [b - a for a, b in zip(f0, f1)]


def pose_stream_cap(level: int, n: int) -> int:
    """The most frames `level` gains in one push of `n` pixel frames, first, middle or closing: what the scratch of
    `sf_pose_stream_scratch_bytes` is sized for."""
    return n + 4 if level <= 4 else (n + 3) // 2 + 2 if level == 5 else (n + 3) // 4 + 2


def ref_plan(H: int, W: int) -> Tuple[int, int]:
    """(h, w) of the reference-pose map for an H x W image: (480, 832) -> (60, 104)."""
    h, w = H, W
    for _, _, _, k, s, p, _ in RANDOMREF_LAYERS:
        h, w = _out(h, k[0], s[0], p[0]), _out(w, k[1], s[1], p[1])
    return h, w


def pose_embed_layers(num_pose_frames: int, H: int, W: int) -> List[dict]:
    """Per launch of `sf_pose_embed`, from the shapes alone: name, FLOPs (multiply-add = 2, the reference's true channel
    counts) and bytes (input volume read once + output volume written once + weights, as this build stores them)."""
    vols = pose_layer_volumes(num_pose_frames, H, W)
    t, h, w = vols[0]
    out = [dict(name="prepare", flops=0.0, bytes=float(3 * num_pose_frames * H * W + t * h * w * CIN_STORE * 2))]
    c_store = CIN_STORE
    for i, (idx, cin, cout, k, _, _, _) in enumerate(DWPOSE_LAYERS):
        (ti, hi, wi), (to, ho, wo) = vols[i], vols[i + 1]
        taps = k[0] * k[1] * k[2]
        if idx == 12:   # the input rows are gathered first (read + write of the [tokens, 64] rows), then the GEMM
            rows = to * ho * wo * taps * cin * 2
            by = 2 * rows + rows + to * ho * wo * cout * 2 + cout * taps * cin * 2
        else:
            by = ti * hi * wi * c_store * 2 + to * ho * wo * cout * 2 + cout * taps * c_store * 2
        out.append(dict(name=f"dwpose_embedding.{idx}", flops=2.0 * taps * cin * cout * to * ho * wo, bytes=float(by)))
        c_store = cout
    return out


def pose_embed_flops(num_pose_frames: int, H: int, W: int) -> float:
    return sum(l["flops"] for l in pose_embed_layers(num_pose_frames, H, W))


def pose_embed_bytes(num_pose_frames: int, H: int, W: int) -> float:
    return sum(l["bytes"] for l in pose_embed_layers(num_pose_frames, H, W))


# ---------------------------------------------------------------------------------------- seeded inputs
def synth_pose_clip(seed: int, num_frames: int, H: int, W: int, kind: str = "skeleton") -> Tensor:
    """Seeded uint8 pose frames [3, F, H, W] (for tests, fixtures and benchmarks): "dense" = uniform 0..255 everywhere;
    "skeleton" = 18 joints drifting over the clip, joined by short coloured segments on black -- a few per cent of
    lit pixels, as rendered DWPose frames are, and the case where padding and bias dominate.  numpy's RandomState
    streams are frozen, so the same seed gives the same clip everywhere."""
    rs = np.random.RandomState(seed)
    if kind == "dense":
        return torch.from_numpy(rs.randint(0, 256, size=(3, num_frames, H, W), dtype=np.uint8))
    if kind != "skeleton":
        raise ValueError(f"synth_pose_clip: kind must be 'dense' or 'skeleton', got {kind!r}")
    joints = 18
    clip = np.zeros((3, num_frames, H, W), dtype=np.uint8)
    centre = np.array([H / 2, W / 2]) + rs.uniform(-0.15, 0.15, 2) * np.array([H, W])
    pos0 = centre + rs.uniform(-0.3, 0.3, (joints, 2)) * min(H, W)
    vel = rs.normal(0.0, 0.004 * min(H, W), (joints, 2))
    colours = rs.randint(64, 256, size=(joints, 3)).astype(np.uint8)
    thick = max(1, min(H, W) // 120)
    n = 2 * max(H, W)
    s = np.linspace(0.0, 1.0, n)[:, None]
    dy, dx = np.meshgrid(np.arange(thick), np.arange(thick), indexing="ij")
    for f in range(num_frames):
        pos = pos0 + f * vel + rs.normal(0.0, 0.5, (joints, 2))
        for j in range(joints):
            a, b = pos[j], pos[(j + 1) % joints]
            b = a + (b - a) * min(1.0, 0.33 * min(H, W) / (np.linalg.norm(b - a) + 1e-6))   # short segments
            pts = np.rint(a + s * (b - a)).astype(np.int64)
            ys = (pts[:, 0, None] + dy.reshape(1, -1)).reshape(-1)
            xs = (pts[:, 1, None] + dx.reshape(1, -1)).reshape(-1)
            ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
            clip[:, f, ys[ok], xs[ok]] = colours[j][:, None]
    return torch.from_numpy(clip)


def synth_pose_image(seed: int, H: int, W: int, kind: str = "skeleton") -> Tensor:
    """Seeded uint8 reference pose image [H, W, 3] of the same two kinds."""
    return synth_pose_clip(seed, 1, H, W, kind)[:, 0].permute(1, 2, 0).contiguous()


# ---------------------------------------------------------------------------------------- restatement (tests, fixtures)
def pose_input_torch(dwpose_data: Tensor) -> Tensor:
    """The input transform of :337-339 in torch: [3, F, H, W] -> float32 [1, 3, F + 3, H, W] in 0..1."""
    x = dwpose_data.unsqueeze(0)
    return torch.cat([x[:, :, :1].repeat(1, 1, LEAD_FRAMES, 1, 1), x], dim=2) / 255.0


def pose_layer_torch(x: Tensor, w: Tensor, b: Tensor, stride, padding, act: bool) -> Tensor:
    """One layer of either stack with torch's own convolution (x [1, C, (T,) H, W]); the yardstick of the per-kernel
    tests.  Never called by the product path."""
    import torch.nn.functional as F
    y = (F.conv3d if w.dim() == 5 else F.conv2d)(x, w, b, stride=stride, padding=padding)
    return F.silu(y) if act else y


def pose_stacks_torch(state_dict: Dict[str, Tensor], dwpose_data: Optional[Tensor] = None, random_ref_dwpose: Optional[Tensor] = None,
                      dtype=torch.float32) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """Plain-torch restatement of both stacks (:87-122, :337-343) for the tests: (dwpose embedding [1, 5120, F', h, w],
    reference-pose map [1, 20, 1, h, w]) in `dtype`.  Never called by the product path."""
    outs = []
    for prefix, layers, x in ((DWPOSE_PREFIX, DWPOSE_LAYERS, None if dwpose_data is None else pose_input_torch(dwpose_data)),
                              (RANDOMREF_PREFIX, RANDOMREF_LAYERS,
                               None if random_ref_dwpose is None else (random_ref_dwpose.unsqueeze(0) / 255.0).permute(0, 3, 1, 2))):
        if x is None:
            outs.append(None)
            continue
        x = x.to(dtype)
        for idx, _, _, _, stride, pad, act in layers:
            x = pose_layer_torch(x, state_dict[f"{prefix}{idx}.weight"].to(dtype), state_dict[f"{prefix}{idx}.bias"].to(dtype), stride, pad, act)
        outs.append(x)
    if outs[1] is not None:
        outs[1] = outs[1].unsqueeze(2)
    return outs[0], outs[1]
