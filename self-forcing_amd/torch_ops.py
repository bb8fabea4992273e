"""PyTorch custom operators over the C-ABI: `torch.ops.sf_hip.*` take Tensors (BASELINE north_star: "Python host code
calling HIP through PyTorch-ROCm custom ops over a thin C-ABI").

Every operator below is a thin shim: it validates shapes / dtypes, allocates the outputs with torch, reads the current
HIP stream, and makes ONE call into `libsf_hip.so` (`include/sf_hip.h`) with raw device pointers.  Registered with
`torch.library.custom_op`, so each has a schema (mutated arguments declared), a fake ("meta") implementation for
tracing, and is opaque-but-legal to `torch.compile` -- which the reference's second caller wraps around the generator
(demo.py:340); a bare ctypes call would be a graph break with unknown side effects.  `ops.py` (per-kernel wrappers),
`model.py` (the fused forward), `vae.py`, `text_encoder.py` route through these.

    sf_hip::attention(q, k, v, structure) -> out
    sf_hip::attention_accum(q, k, v, out!, structure) -> ()         (out += attention: the i2v image keys)
    sf_hip::dit_forward_i2v(model, noisy, timestep, prompt_embeds?, clip_feature?, y, ..., kimg_cache![], vimg_cache![], ...) -> (flow, x0)
    sf_hip::i2v_assemble_y(latent, y!, first_is_frame0, ref_map?) -> ()   (a chunk of the i2v conditioning tensor y)
    sf_hip::gemm(a, w, bias?, epilogue, resid?, gate_mod?, gate_e0?, rows_per_group, structure) -> out
    sf_hip::gemm_out(out!, a, w, ...) -> ()                         (caller-provided / aliased output)
    sf_hip::quantize_fp8(x, rows_per_segment) -> (q e4m3fn, scales)  (FP8 linear layers, fp8.py)
    sf_hip::gemm_fp8(a, a_scale, rows_per_segment, w, w_scale, bias?, epilogue, resid?, gate_mod?, gate_e0?, rows_per_group, structure) -> out
    sf_hip::lincomb(tensors[], coefs[]) -> out ;  sf_hip::lincomb_out(out!, tensors[], coefs[]) -> ()
    sf_hip::add_noise(x0, eps, timestep, sigmas, timesteps) -> out
    sf_hip::dit_forward(model, noisy, timestep, prompt_embeds?, add_condition?, k_cache![], v_cache![], ck_cache![],
                        cv_cache![], workspace!, evict_scratch!?, ..., kv_index!?, global_end, cross_keys!?, cross_log2w!?) -> (flow, x0)
    sf_hip::dit_forward_pair(model, ctx_noisy, ctx_timestep, noisy, timestep, caches![]..., workspace!, evict_scratch!?, ctx_plan[7],
                             plan[7], kv_index!?, global_end, ..., ctx_add_condition?, add_condition?) -> (flow, x0)
                                                                    (context pass of chunk k + first pass of chunk k + 1)
    sf_hip::vae_decode_frames(model, state!, scratch!, z, out!, h, w, window_frames, frame_index, window, history_at) -> ()
    sf_hip::vae_encode_frames(model, state!, scratch!, pixels, out!, H, W, window_frames, chunk_index, window, history_at) -> ()
    sf_hip::taehv_decode_frames(model, state!, scratch!, z, out!, h, w, clamp) -> ()
    sf_hip::taehv_encode_frames(model, state!, scratch!, pixels, out!, H, W, lead) -> ()
    sf_hip::t5_encode(model, ids, mask, buckets, workspace!) -> out
    sf_hip::clip_encode(model, frames, workspace!) -> out
    sf_hip::resize_frames(frames, bounds_h, coefs_h, bounds_v, coefs_v, filter, layout, out_layout, dtype, crop?) -> out
    sf_hip::resize_frames_out(out!, frames, bounds_h, coefs_h, bounds_v, coefs_v, filter, layout, out_layout, crop?) -> ()
    sf_hip::yuv_decode_frames(raw, fmt, height, width, constants, chroma, layout, dtype) -> out
    sf_hip::yuv_encode_frames(frames, fmt, constants, range01) -> out
    sf_hip::pose_render_frames(keypoints, height, width, layout, dtype, normalized, score_threshold) -> out
    sf_hip::pose_render_frames_out(out!, keypoints, layout, normalized, score_threshold) -> ()
    sf_hip::pose_retarget_frames(src, first, ref, src0, out0, n_out, num, den, src_sx, src_sy, ref_sx, ref_sy, score_threshold, align) -> out
    sf_hip::pose_smooth_frames(src, state!, period, min_cutoff, beta, kd, score_threshold, max_gap) -> out
    sf_hip::pose_track_frames(src, state!, slots, gate2, score_threshold, min_points, min_common, max_age) -> (out, ids)
    sf_hip::pose_boxes_decode(head, in_h, in_w, strides, ratio, max_people, class_index, score_threshold, iou_threshold, decoded) -> (boxes, count)
    sf_hip::pose_crop_people(frames, boxes, count, layout, out_h, out_w, padding, mean, std, bgr, dtype) -> out
    sf_hip::pose_simcc_decode(simcc_x, simcc_y, boxes, count, height, width, out_h, out_w, padding, split_ratio, normalized, neck_threshold, order) -> out

Models (weights + C descriptors) are Python objects that own device memory; operators take an integer HANDLE from
`register_model` (a constant to a tracer).  There is no CPU implementation: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import itertools
import threading
import time
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch.library import custom_op

from . import _lib

Tensor = torch.Tensor
NAMESPACE = "sf_hip"

_MODELS: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()


_HANDLES = itertools.count(1)   # never reused: a freed model's handle stays unregistered (id(obj) could come back as a new object's)


def register_model(obj) -> int:
    """Handle of a model object (CausalWanModel / WanVAEDecoder / UMT5Encoder) for the operators that need its weights."""
    h = next(_HANDLES)
    _MODELS[h] = obj
    return h


def _model(handle: int):
    try:
        return _MODELS[handle]
    except KeyError:
        raise RuntimeError(f"sf_hip: model handle {handle} is not registered (or its owner was freed)") from None


def _stream(t: Optional[Tensor] = None) -> int:
    """The current HIP stream of t's device (of the current device without a tensor)."""
    return torch.cuda.current_stream(None if t is None else t.device).cuda_stream


def _dtype_name(t: Tensor) -> str:
    """'bfloat16' for torch.bfloat16: the keys of the `_lib.*_DTYPES` tables."""
    return str(t.dtype).replace("torch.", "")


def _need_gpu(t: Tensor, name: str, dtype=torch.bfloat16) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")


def _need_bytes(op: str, **buffers: Optional[Tensor]) -> None:
    """State / scratch / workspace blocks: their element counts are passed on as BYTE counts."""
    for name, t in buffers.items():
        if t is not None and (not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()):
            raise ValueError(f"{op}: {name} must be a contiguous CUDA uint8 tensor")


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------ attention
@custom_op(f"{NAMESPACE}::attention", mutates_args=())
def attention(q: Tensor, k: Tensor, v: Tensor, structure: int = 0, keys: Optional[Tensor] = None,
              log2w: Optional[Tensor] = None) -> Tensor:
    """softmax(q k^T / sqrt(D)) v.  `keys` (int32 [B]) / `log2w` (float32 [B]), both or neither: sample b attends only its
    first keys[b] key rows and the last of them counts 2^log2w[b] times (sf_attention_args.keys; see cross_fold_scan)."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _need_gpu(t, n)
        if t.dim() != 4 or t.shape[3] != 128 or t.stride(3) != 1 or t.stride(2) != 128:
            raise ValueError(f"attention: {n} must be [B, L, H, 128] with contiguous heads, got {tuple(t.shape)} {t.stride()}")
    B, Lq, H, D = q.shape
    if k.stride() != v.stride() or k.shape != v.shape:
        raise ValueError("attention: k and v must share shape and strides")
    _fold_pair(keys, log2w, (B,), q.device, "attention")
    out = torch.empty(B, Lq, H, D, dtype=torch.bfloat16, device=q.device)
    _attention_launch(q, k, v, out, structure, keys=_ptr(keys), log2w=_ptr(log2w))
    return out


def _attention_launch(q: Tensor, k: Tensor, v: Tensor, out: Tensor, structure: int, **named) -> None:
    """One sf_attention call on validated [B, L, H, 128] tensors; `named`: accumulate / keys / log2w of sf_attention_args."""
    a = _lib.AttentionArgs(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=out.data_ptr(), B=q.shape[0], H=q.shape[2], Lq=q.shape[1],
                           Lk=k.shape[1], q_stride=q.stride(1), q_bstride=q.stride(0), kv_stride=k.stride(1), kv_bstride=k.stride(0),
                           o_stride=out.stride(1), o_bstride=out.stride(0), structure=structure, **named)
    _lib.check(_lib.lib().sf_attention(a, _stream(q)), "sf_attention")


@attention.register_fake
def _(q, k, v, structure=0, keys=None, log2w=None):
    return q.new_empty(q.shape)


@custom_op(f"{NAMESPACE}::attention_accum", mutates_args=("out",))
def attention_accum(q: Tensor, k: Tensor, v: Tensor, out: Tensor, structure: int = 0) -> None:
    """out += softmax(q k^T / sqrt(D)) v, summed in fp32 in the kernel's epilogue and rounded once (sf_attention_args.accumulate):
    the image half of the i2v cross-attention added into the text half's buffer.  structure: auto, w8 or w4."""
    for n, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _need_gpu(t, n)
        if t.dim() != 4 or t.shape[3] != 128 or t.stride(3) != 1 or t.stride(2) != 128:
            raise ValueError(f"attention_accum: {n} must be [B, L, H, 128] with contiguous heads, got {tuple(t.shape)} {t.stride()}")
    B, Lq, H, D = q.shape
    if k.stride() != v.stride() or k.shape != v.shape or k.shape[0] != B or k.shape[2] != H:
        raise ValueError("attention_accum: k and v must share shape and strides, and batch and heads with q")
    if out.shape != q.shape:
        raise ValueError(f"attention_accum: out must have q's shape {tuple(q.shape)}, got {tuple(out.shape)}")
    _attention_launch(q, k, v, out, structure, accumulate=1)


@attention_accum.register_fake
def _(q, k, v, out, structure=0):
    return None


@custom_op(f"{NAMESPACE}::cross_fold_scan", mutates_args=("keys", "log2w"))
def cross_fold_scan(ck_cache: List[Tensor], cv_cache: List[Tensor], keys: Tensor, log2w: Tensor) -> None:
    """Per layer l and sample b of the cross-attention caches (lists of contiguous bf16 [B, text_len, H, D]): how many
    trailing rows repeat the last row bit for bit in both K and V (a zero-padded prompt's padding) -> keys[l, b] =
    text_len - same + 1 (int32) and log2w[l, b] = log2(same) (float32), what `attention` / `dit_forward` take to attend one
    key in place of `same` identical ones (sf_cross_fold_scan)."""
    L = len(ck_cache)
    if L == 0 or len(cv_cache) != L:
        raise ValueError("cross_fold_scan: one K and one V cache per layer expected")
    want = tuple(ck_cache[0].shape)
    for name, ts in (("ck_cache", ck_cache), ("cv_cache", cv_cache)):
        for i, t in enumerate(ts):
            if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 4 or tuple(t.shape) != want or not t.is_contiguous() \
                    or t.device != keys.device:
                raise ValueError(f"cross_fold_scan: {name}[{i}] must be a contiguous bf16 tensor {want} on {keys.device}")
    B, T = want[0], want[1]
    _fold_pair(keys, log2w, (L, B), ck_cache[0].device, "cross_fold_scan")
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])  # noqa: E731
    _lib.check(_lib.lib().sf_cross_fold_scan(arr(ck_cache), arr(cv_cache), L, B, T, want[2] * want[3], keys.data_ptr(), log2w.data_ptr(),
                                             _stream(keys)), "sf_cross_fold_scan")


@cross_fold_scan.register_fake
def _(ck_cache, cv_cache, keys, log2w):
    return None


@custom_op(f"{NAMESPACE}::kv_rope_shift", mutates_args=("k_cache",))
def kv_rope_shift(k_cache: Tensor, rope_cos: Tensor, rope_sin: Tensor, delta_frames: int, row0: int, rows: int) -> None:
    """Rotate the temporal RoPE pairs of rows [row0, row0 + rows) of every sample of the cached keys (contiguous bf16
    [B, S, H, 128]) back by `delta_frames`, in place (sf_kv_rope_shift; rope_shift_reference.shift_keys, bit for bit).
    rope_cos / rope_sin: the model's float32 [1024, 64] tables."""
    _need_gpu(k_cache, "k_cache")
    if k_cache.dim() != 4 or k_cache.shape[3] != 128 or not k_cache.is_contiguous():
        raise ValueError(f"kv_rope_shift: k_cache must be contiguous [B, S, H, 128], got {tuple(k_cache.shape)} {k_cache.stride()}")
    for n, t in (("rope_cos", rope_cos), ("rope_sin", rope_sin)):
        _need_gpu(t, n, torch.float32)
        if tuple(t.shape) != (1024, 64) or not t.is_contiguous() or t.device != k_cache.device:
            raise ValueError(f"kv_rope_shift: {n} must be a contiguous float32 [1024, 64] table on {k_cache.device}, got {tuple(t.shape)}")
    B, S, H, _ = k_cache.shape
    _lib.check(_lib.lib().sf_kv_rope_shift(k_cache.data_ptr(), B, S, H, row0, rows, rope_cos.data_ptr(), rope_sin.data_ptr(), delta_frames,
                                           _stream(k_cache)), "sf_kv_rope_shift")


@kv_rope_shift.register_fake
def _(k_cache, rope_cos, rope_sin, delta_frames, row0, rows):
    return None   # writes only its mutated argument


def _fold_pair(keys: Optional[Tensor], log2w: Optional[Tensor], shape: tuple, device, who: str) -> None:
    """The kernels index these two by sample (and layer) without a bound of their own: check them here."""
    if (keys is None) != (log2w is None):
        raise ValueError(f"{who}: keys and log2w come together")
    if keys is None:
        return
    for name, t, dt in (("keys", keys, torch.int32), ("log2w", log2w, torch.float32)):
        if not t.is_cuda or t.device != device or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dt} tensor {shape} on {device}, got {tuple(t.shape)} {t.dtype} {t.device}")


# ------------------------------------------------------------------------------------------ GEMM
def _gemm_args(out: Tensor, a: Tensor, w: Tensor, bias, epilogue: int, resid, gate_mod, gate_e0, rows_per_group: int,
               structure: int) -> "_lib.GemmArgs":
    """sf_gemm_args of out [M, N] = a [M, K] . w [N, K]^T (shapes checked by the caller); the optional bf16 operands are
    checked for device and dtype here."""
    g = _lib.GemmArgs()
    g.a, g.w, g.bias, g.out = a.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr()
    g.M, g.K = a.shape
    g.N = w.shape[0]
    g.lda, g.ldw, g.ldo = a.stride(0), w.stride(0), out.stride(0)
    g.epilogue, g.rows_per_group, g.structure = epilogue, rows_per_group, structure
    for name, t in (("bias", bias), ("resid", resid), ("gate_mod", gate_mod), ("gate_e0", gate_e0)):
        if t is not None:
            _need_gpu(t, name)
    if resid is not None:
        g.resid, g.ldr = resid.data_ptr(), resid.stride(0)
    g.gate_mod = _ptr(gate_mod)
    if gate_e0 is not None:
        g.gate_e0, g.gate_group_stride = gate_e0.data_ptr(), gate_e0.stride(0)
    return g


def _gemm_launch(out: Tensor, a: Tensor, w: Tensor, bias, epilogue: int, resid, gate_mod, gate_e0, rows_per_group: int,
                 structure: int) -> None:
    for n, t in (("a", a), ("w", w)):
        _need_gpu(t, n)
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"gemm: {n} must be 2-D with contiguous rows, got {tuple(t.shape)} {t.stride()}")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm: a is [{M},{K}] but w is {tuple(w.shape)}")
    want = torch.float32 if epilogue == _lib.EPI_F32 else torch.bfloat16
    _need_gpu(out, "out", want)
    if out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (M, N):
        raise ValueError(f"gemm: out must be [{M},{N}] with contiguous rows, got {tuple(out.shape)} {out.stride()}")
    g = _gemm_args(out, a, w, bias, epilogue, resid, gate_mod, gate_e0, rows_per_group, structure)
    _lib.check(_lib.lib().sf_gemm_bf16(g, _stream(a)), "sf_gemm_bf16")


@custom_op(f"{NAMESPACE}::gemm", mutates_args=())
def gemm(a: Tensor, w: Tensor, bias: Optional[Tensor], epilogue: int, resid: Optional[Tensor], gate_mod: Optional[Tensor],
         gate_e0: Optional[Tensor], rows_per_group: int, structure: int) -> Tensor:
    out = torch.empty(a.shape[0], w.shape[0], dtype=torch.float32 if epilogue == _lib.EPI_F32 else torch.bfloat16, device=a.device)
    _gemm_launch(out, a, w, bias, epilogue, resid, gate_mod, gate_e0, rows_per_group, structure)
    return out


@gemm.register_fake
def _(a, w, bias, epilogue, resid, gate_mod, gate_e0, rows_per_group, structure):
    return a.new_empty((a.shape[0], w.shape[0]), dtype=torch.float32 if epilogue == _lib.EPI_F32 else torch.bfloat16)


@custom_op(f"{NAMESPACE}::gemm_out", mutates_args=("out",))
def gemm_out(out: Tensor, a: Tensor, w: Tensor, bias: Optional[Tensor], epilogue: int, resid: Optional[Tensor],
             gate_mod: Optional[Tensor], gate_e0: Optional[Tensor], rows_per_group: int, structure: int) -> None:
    _gemm_launch(out, a, w, bias, epilogue, resid, gate_mod, gate_e0, rows_per_group, structure)


# ------------------------------------------------------------------------------------------ FP8 (fp8.py)
def _segments(M: int, rows_per_segment: int) -> int:
    if rows_per_segment <= 0:
        raise ValueError("rows_per_segment must be positive")
    return (M + rows_per_segment - 1) // rows_per_segment


@custom_op(f"{NAMESPACE}::quantize_fp8", mutates_args=())
def quantize_fp8(x: Tensor, rows_per_segment: int) -> Tuple[Tensor, Tensor]:
    """x [M, K] bf16 -> (e4m3fn [M, K], fp32 scales [segments]) by sf_quantize_fp8."""
    _need_gpu(x, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"quantize_fp8: x must be 2-D with contiguous rows, got {tuple(x.shape)} {x.stride()}")
    M, K = x.shape
    segs = _segments(M, rows_per_segment)
    q = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=x.device)
    buf = torch.empty(segs * (1 + _lib.FP8_AMAX_PARTS), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().sf_quantize_fp8(x.data_ptr(), x.stride(0), M, K, rows_per_segment, q.data_ptr(), buf.data_ptr(), _stream(x)),
               "sf_quantize_fp8")
    return q, buf[:segs].clone()


@quantize_fp8.register_fake
def _(x, rows_per_segment):
    return x.new_empty(x.shape, dtype=torch.float8_e4m3fn), x.new_empty((_segments(x.shape[0], rows_per_segment),), dtype=torch.float32)


@custom_op(f"{NAMESPACE}::gemm_fp8", mutates_args=())
def gemm_fp8(a: Tensor, a_scale: Tensor, rows_per_segment: int, w: Tensor, w_scale: Tensor, bias: Optional[Tensor], epilogue: int,
             resid: Optional[Tensor], gate_mod: Optional[Tensor], gate_e0: Optional[Tensor], rows_per_group: int, structure: int) -> Tensor:
    """out = epi(acc * (a_scale[m // rows_per_segment] * w_scale[n]) + bias[n]) with e4m3fn a [M, K], w [N, K] (sf_gemm_fp8)."""
    for n, t in (("a", a), ("w", w)):
        _need_gpu(t, n, torch.float8_e4m3fn)
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"gemm_fp8: {n} must be 2-D with contiguous rows, got {tuple(t.shape)} {t.stride()}")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm_fp8: a is [{M},{K}] but w is {tuple(w.shape)}")
    for n, t, size in (("a_scale", a_scale, _segments(M, rows_per_segment)), ("w_scale", w_scale, N)):
        _need_gpu(t, n, torch.float32)
        if t.dim() != 1 or t.numel() != size or not t.is_contiguous():
            raise ValueError(f"gemm_fp8: {n} must be a contiguous fp32 vector of {size}, got {tuple(t.shape)}")
    out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    g = _gemm_args(out, a, w, bias, epilogue, resid, gate_mod, gate_e0, rows_per_group, structure)
    _lib.check(_lib.lib().sf_gemm_fp8(g, a_scale.data_ptr(), rows_per_segment, w_scale.data_ptr(), _stream(a)), "sf_gemm_fp8")
    return out


@gemm_fp8.register_fake
def _(a, a_scale, rows_per_segment, w, w_scale, bias, epilogue, resid, gate_mod, gate_e0, rows_per_group, structure):
    return a.new_empty((a.shape[0], w.shape[0]), dtype=torch.bfloat16)


# ------------------------------------------------------------------------------------------ lincomb / add_noise
def _lincomb_launch(out: Tensor, tensors: Sequence[Tensor], coefs: Sequence[float]) -> None:
    n = len(tensors)
    if not 1 <= n <= 6 or n != len(coefs):
        raise ValueError(f"lincomb: 1..6 tensors with one coefficient each, got {n} / {len(coefs)}")
    for i, t in enumerate(tensors):
        _need_gpu(t, f"tensors[{i}]")
        if not t.is_contiguous() or t.shape != tensors[0].shape or t.device != tensors[0].device:
            raise ValueError("lincomb: tensors must be contiguous and share shape and device")
    if out.shape != tensors[0].shape or out.dtype != torch.bfloat16 or not out.is_contiguous():
        raise ValueError("lincomb: out must be a contiguous bf16 tensor of the inputs' shape")
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    cf = (C.c_float * n)(*[float(c) for c in coefs])
    _lib.check(_lib.lib().sf_lincomb_bf16(out.data_ptr(), ptrs, cf, n, tensors[0].numel(), _stream(out)), "sf_lincomb_bf16")


@custom_op(f"{NAMESPACE}::lincomb", mutates_args=())
def lincomb(tensors: List[Tensor], coefs: List[float]) -> Tensor:
    if not tensors:
        raise ValueError("lincomb: 1..6 tensors with one coefficient each, got 0")
    out = torch.empty_like(tensors[0], memory_format=torch.contiguous_format)
    _lincomb_launch(out, tensors, coefs)
    return out


@lincomb.register_fake
def _(tensors, coefs):
    return torch.empty_like(tensors[0])


@custom_op(f"{NAMESPACE}::lincomb_out", mutates_args=("out",))
def lincomb_out(out: Tensor, tensors: List[Tensor], coefs: List[float]) -> None:
    _lincomb_launch(out, tensors, coefs)


@custom_op(f"{NAMESPACE}::add_noise", mutates_args=())
def add_noise(x0: Tensor, eps: Tensor, timestep: Tensor, sigmas: Tensor, timesteps: Tensor) -> Tensor:
    _need_gpu(x0, "x0"), _need_gpu(eps, "eps"), _need_gpu(sigmas, "sigmas", torch.float32), _need_gpu(timesteps, "timesteps", torch.float32)
    if not (x0.is_contiguous() and eps.is_contiguous() and timestep.is_contiguous()):
        raise ValueError("add_noise: contiguous tensors expected")
    n = x0.shape[0]
    if timestep.numel() != n or timestep.dtype not in (torch.float32, torch.int64):
        raise ValueError(f"add_noise: {n} samples need {n} float32 / int64 timesteps, got {timestep.numel()} of {timestep.dtype}")
    out = torch.empty_like(eps)
    _lib.check(_lib.lib().sf_add_noise(x0.data_ptr(), eps.data_ptr(), timestep.data_ptr(), int(timestep.dtype == torch.int64),
                                       sigmas.data_ptr(), timesteps.data_ptr(), sigmas.numel(), out.data_ptr(), n, x0.numel() // n,
                                       _stream(x0)), "sf_add_noise")
    return out


@add_noise.register_fake
def _(x0, eps, timestep, sigmas, timesteps):
    return torch.empty_like(eps)


# ------------------------------------------------------------------------------------------ fused DiT forward
_TABLES: Dict[str, Dict[tuple, tuple]] = {}    # per operator: {(model handle, stream): (key, pointer arrays)}

# Host time spent INSIDE sf_dit_forward (the C call that enqueues the ~430 launches of a pass), per calling thread:
# {thread id: [calls, wall seconds, CPU seconds of the thread]}.  Wall time includes waiting for room in the stream's
# launch queue when the host runs ahead of the GPU (it does: a pass is ~25-50 ms of GPU work); the thread's CPU time is
# what the call really costs the host.  bench.py reports both -- with one process per GPU and `streams` enqueuing
# threads per process, 8 ranks x that many threads must fit the node's cores.
HOST_ENQUEUE: Dict[int, list] = {}


def host_enqueue_stats(reset: bool = False):
    """(forwards, wall seconds, CPU seconds, threads) summed over the threads that called dit_forward since the last reset."""
    calls = sum(v[0] for v in HOST_ENQUEUE.values())
    wall = sum(v[1] for v in HOST_ENQUEUE.values())
    cpu = sum(v[2] for v in HOST_ENQUEUE.values())
    n = sum(1 for v in HOST_ENQUEUE.values() if v[0])
    if reset:
        HOST_ENQUEUE.clear()
    return calls, wall, cpu, n


def _cache_tables(slot_kind: str, handle: int, named_lists, device):
    """Per-layer cache pointer arrays for the C call, one per (name, tensors, expected shape) of `named_lists`; rebuilt --
    and every tensor validated (bf16, contiguous, the expected [B, S, H, D] on the call's device: the kernels WRITE
    through these pointers) -- only when a cache tensor was re-allocated / rebound or the expected shape changed.
    `slot_kind` names the operator (in the messages); each operator keeps its own tables, at most 64 of them."""
    key = tuple(want for _, _, want in named_lists) + tuple(t.data_ptr() for _, ts, _ in named_lists for t in ts)
    tables = _TABLES.setdefault(slot_kind, {})
    slot = (handle, torch.cuda.current_stream(device).cuda_stream)
    hit = tables.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    for name, tensors, want in named_lists:
        for i, t in enumerate(tensors):
            if not t.is_cuda or t.dtype != torch.bfloat16 or tuple(t.shape) != want or not t.is_contiguous() or t.device != device:
                raise ValueError(f"{slot_kind}: {name}[{i}] must be a contiguous bf16 tensor {want} on {device}, got "
                                 f"{tuple(t.shape)} {t.dtype} {t.device}")
    tabs = tuple((C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) for _, ts, _ in named_lists)
    if len(tables) > 64:
        tables.clear()
    tables[slot] = (key, tabs)
    return tabs


def _forward_args(m, model: int, noisy: Tensor, timestep: Tensor, prompt_embeds: Optional[Tensor], add_condition: Optional[Tensor],
                  k_cache, v_cache, ck_cache, cv_cache, workspace: Tensor, evict_scratch: Optional[Tensor], init_cross: bool,
                  cache_only: bool, sink: int, evict: int, keep: int, write_start: int, attn_start: int, attn_end: int,
                  start_frame: int, kv_index: Optional[Tensor], global_end: int, in_channels: Optional[int] = None):
    """Validate one pass's tensors and fill its sf_forward_args; returns (args, flow, x0) with empty outputs for cache_only."""
    _need_gpu(noisy, "noisy")
    _need_gpu(timestep, "timestep", None)
    if noisy.dim() != 5 or not noisy.is_contiguous() or timestep.dim() != 2 or not timestep.is_contiguous():
        raise ValueError("dit_forward: noisy must be contiguous [B, F, C, H, W], timestep contiguous [B, groups]")
    if timestep.dtype not in (torch.float32, torch.int64):
        raise ValueError(f"dit_forward: timestep must be float32 or int64, got {timestep.dtype}")
    L = m.num_layers
    if not (len(k_cache) == len(v_cache) == len(ck_cache) == len(cv_cache) == L):
        raise ValueError(f"dit_forward: cache lists must have {L} entries")
    B, F, _, H, W = noisy.shape
    sh = m.shape
    if in_channels is None:   # (dit_forward_i2v names its own: the latent channels in front of y's)
        if getattr(sh, "is_i2v", False):
            raise ValueError("dit_forward: an i2v model runs through dit_forward_i2v (clip_feature and y are required)")
        in_channels = sh.in_dim
    if noisy.shape[2] != in_channels or timestep.shape[0] != B:
        raise ValueError(f"dit_forward: noisy must carry {in_channels} channels and timestep one row per sample")
    cap = k_cache[0].shape[1] if k_cache[0].dim() == 4 else -1
    # the C call writes through these pointers: every cache tensor must really be what the kernels assume (checked when
    # the pointer tables are (re)built, i.e. whenever any cache tensor is new to this model / stream)
    want_kv, want_cross = (B, cap, sh.num_heads, sh.head_dim), (B, sh.text_len, sh.num_heads, sh.head_dim)
    n_new = F * (H // 2) * (W // 2)
    if not (0 <= attn_start < attn_end <= cap and 0 <= write_start and write_start + n_new == attn_end):
        raise ValueError(f"dit_forward: cache plan does not fit the cache (write_start {write_start} + {n_new} new tokens, "
                         f"window [{attn_start}, {attn_end}), capacity {cap})")
    if init_cross:
        if prompt_embeds is None:
            raise ValueError("dit_forward: init_cross needs prompt_embeds")
        _need_gpu(prompt_embeds, "prompt_embeds")
        if tuple(prompt_embeds.shape) != (B, sh.text_len, sh.text_dim) or not prompt_embeds.is_contiguous():
            raise ValueError(f"dit_forward: prompt_embeds must be contiguous [{B}, {sh.text_len}, {sh.text_dim}], got {tuple(prompt_embeds.shape)}")
    if add_condition is not None:
        _need_gpu(add_condition, "add_condition")
        if add_condition.dim() != 3 or add_condition.shape[:2] != (B, n_new) or not add_condition.is_contiguous():
            raise ValueError(f"dit_forward: add_condition must be contiguous [{B}, {n_new}, pose_dim], got {tuple(add_condition.shape)}")
    _need_bytes("dit_forward", workspace=workspace, evict_scratch=evict_scratch)
    k_ptrs, v_ptrs, ck_ptrs, cv_ptrs = _cache_tables("dit_forward", model, (("k_cache", k_cache, want_kv), ("v_cache", v_cache, want_kv),
                                                                            ("ck_cache", ck_cache, want_cross), ("cv_cache", cv_cache, want_cross)),
                                                     noisy.device)
    a = _lib.ForwardArgs()
    a.batch, a.frames, a.lat_h, a.lat_w, a.groups = B, F, H, W, timestep.shape[1]
    a.noisy, a.timestep = noisy.data_ptr(), timestep.data_ptr()
    a.t_is_int64 = 1 if timestep.dtype == torch.int64 else 0
    a.prompt_embeds = _ptr(prompt_embeds)
    a.init_cross = 1 if init_cross else 0
    a.add_condition = _ptr(add_condition)
    a.k_cache_host, a.v_cache_host, a.ck_cache_host, a.cv_cache_host = k_ptrs, v_ptrs, ck_ptrs, cv_ptrs
    a.cache_tokens = cap
    a.sink_tokens, a.evict, a.keep = sink, evict, keep
    a.write_start, a.attn_start, a.attn_end, a.start_frame = write_start, attn_start, attn_end, start_frame
    if evict_scratch is not None:
        a.evict_scratch, a.evict_scratch_bytes = evict_scratch.data_ptr(), evict_scratch.numel() * evict_scratch.element_size()
    a.cache_only = 1 if cache_only else 0
    if cache_only:
        flow = torch.empty(0, dtype=torch.bfloat16, device=noisy.device)
        x0 = torch.empty(0, dtype=torch.bfloat16, device=noisy.device)
    else:
        flow = torch.empty(B, F, m.shape.out_dim, H, W, dtype=torch.bfloat16, device=noisy.device)
        x0 = torch.empty_like(flow)
        a.flow_out, a.x0_out = flow.data_ptr(), x0.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if kv_index is not None:
        if kv_index.dtype != torch.int64 or not kv_index.is_cuda or not kv_index.is_contiguous() or tuple(kv_index.shape) != (L, 2):
            raise ValueError(f"dit_forward: kv_index must be a contiguous CUDA int64 [{L}, 2] tensor")
        a.kv_index_out, a.global_end = kv_index.data_ptr(), global_end
    return a, flow, x0


def _forward_call(m, passes, cross_keys: Optional[Tensor], cross_log2w: Optional[Tensor], stream: int, i2v_args=None) -> None:
    """sf_dit_forward over one or two filled sf_forward_args, with its wall and CPU time booked to the calling thread
    (HOST_ENQUEUE)."""
    call = _lib.ForwardCall()
    for i, a in enumerate(passes):
        call.passes[i] = C.pointer(a)
    call.n_passes = len(passes)
    call.cross_keys, call.cross_log2w = _ptr(cross_keys), _ptr(cross_log2w)
    if i2v_args is not None:
        call.i2v_model, call.i2v_args = C.pointer(m.i2v_cmodel), C.pointer(i2v_args)
    fn = _lib.lib().sf_dit_forward
    t0, c0 = time.perf_counter(), time.thread_time()
    rc = fn(C.byref(m.cmodel), C.byref(call), stream)
    dt, dc = time.perf_counter() - t0, time.thread_time() - c0
    rec = HOST_ENQUEUE.setdefault(threading.get_ident(), [0, 0.0, 0.0])
    rec[0] += 1
    rec[1] += dt
    rec[2] += dc
    _lib.check(rc, "sf_dit_forward")


@custom_op(f"{NAMESPACE}::dit_forward",
           mutates_args=("k_cache", "v_cache", "ck_cache", "cv_cache", "workspace", "evict_scratch", "kv_index", "cross_keys", "cross_log2w"))
def dit_forward(model: int, noisy: Tensor, timestep: Tensor, prompt_embeds: Optional[Tensor], add_condition: Optional[Tensor],
                k_cache: List[Tensor], v_cache: List[Tensor], ck_cache: List[Tensor], cv_cache: List[Tensor],
                workspace: Tensor, evict_scratch: Optional[Tensor], init_cross: bool, cache_only: bool, sink: int, evict: int,
                keep: int, write_start: int, attn_start: int, attn_end: int, start_frame: int,
                kv_index: Optional[Tensor], global_end: int, cross_keys: Optional[Tensor],
                cross_log2w: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """One denoiser pass (CausalWanModel._forward_inference + flow -> x0, sf_dit_forward).  Writes the new K/V rows
    into k_cache / v_cache (and, with init_cross, the text K/V into ck_cache / cv_cache); returns (flow, x0), or two
    empty tensors with cache_only.  kv_index (optional, int64 [num_layers, 2]): every row <- (global_end, attn_end),
    the cache dicts' index tensors when they are views of one buffer.  cross_keys / cross_log2w (int32 / float32
    [num_layers, B], both or neither): the cross-attention caches' folded key counts (cross_fold_scan), written with
    init_cross and read by every layer's cross-attention; None: every text key is attended.  (No default: torch drops a
    trailing argument left at its default before it bumps the version counters of the mutated ones, and then fails.)"""
    m = _model(model)
    a, flow, x0 = _forward_args(m, model, noisy, timestep, prompt_embeds, add_condition, k_cache, v_cache, ck_cache, cv_cache, workspace,
                                evict_scratch, init_cross, cache_only, sink, evict, keep, write_start, attn_start, attn_end, start_frame,
                                kv_index, global_end)
    _fold_pair(cross_keys, cross_log2w, (m.num_layers, noisy.shape[0]), noisy.device, "dit_forward")
    _forward_call(m, (a,), cross_keys, cross_log2w, _stream(noisy))
    return flow, x0


@custom_op(f"{NAMESPACE}::dit_forward_i2v",
           mutates_args=("k_cache", "v_cache", "ck_cache", "cv_cache", "kimg_cache", "vimg_cache", "workspace", "evict_scratch", "kv_index",
                         "cross_keys", "cross_log2w"))
def dit_forward_i2v(model: int, noisy: Tensor, timestep: Tensor, prompt_embeds: Optional[Tensor], clip_feature: Optional[Tensor], y: Tensor,
                    add_condition: Optional[Tensor], k_cache: List[Tensor], v_cache: List[Tensor], ck_cache: List[Tensor],
                    cv_cache: List[Tensor], kimg_cache: List[Tensor], vimg_cache: List[Tensor], workspace: Tensor,
                    evict_scratch: Optional[Tensor], init_cross: bool, cache_only: bool, sink: int, evict: int, keep: int,
                    write_start: int, attn_start: int, attn_end: int, start_frame: int, kv_index: Optional[Tensor], global_end: int,
                    cross_keys: Optional[Tensor] = None, cross_log2w: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One pass of an i2v generator (sf_dit_forward with sf_i2v_args): dit_forward plus y (bf16 [B or 1, 20, F, H, W], any batch /
    channel / frame strides over contiguous H x W planes: a frame slice of the clip's y needs no copy) in the patch
    embedding and the image keys behind every layer's text cross-attention.  clip_feature (bf16 [B, clip_len, clip_dim],
    contiguous) is read with init_cross only, which fills kimg_cache / vimg_cache ([B, clip_len, H, D] per layer)."""
    m = _model(model)
    sh = m.shape
    if not sh.is_i2v:
        raise ValueError("dit_forward_i2v: the model is not of the i2v type")
    if noisy.dim() != 5 or noisy.shape[2] + m.y_channels != sh.in_dim:
        raise ValueError(f"dit_forward_i2v: noisy must carry {sh.in_dim - m.y_channels} channels ([B, F, C, H, W]), got {tuple(noisy.shape)}")
    a, flow, x0 = _forward_args(m, model, noisy, timestep, prompt_embeds, add_condition, k_cache, v_cache, ck_cache, cv_cache, workspace,
                                evict_scratch, init_cross, cache_only, sink, evict, keep, write_start, attn_start, attn_end, start_frame,
                                kv_index, global_end, in_channels=noisy.shape[2])
    B, F, _, H, W = noisy.shape
    _need_gpu(y, "y")
    if y.dim() != 5 or y.shape[0] not in (1, B) or y.shape[1] != m.y_channels or tuple(y.shape[2:]) != (F, H, W) \
            or y.stride(4) != 1 or y.stride(3) != W:
        raise ValueError(f"dit_forward_i2v: y must be [{B} or 1, {m.y_channels}, {F}, {H}, {W}] with contiguous H x W planes, got "
                         f"{tuple(y.shape)} {y.stride()}")
    ia = _lib.I2VArgs()
    ia.y, ia.y_channels = y.data_ptr(), m.y_channels
    ia.y_bstride, ia.y_cstride, ia.y_fstride = (0 if y.shape[0] == 1 else y.stride(0)), y.stride(1), y.stride(2)
    if init_cross:
        if clip_feature is None:
            raise ValueError("dit_forward_i2v: init_cross needs clip_feature")
        _need_gpu(clip_feature, "clip_feature")
        if tuple(clip_feature.shape) != (B, sh.clip_len, sh.clip_dim) or not clip_feature.is_contiguous():
            raise ValueError(f"dit_forward_i2v: clip_feature must be contiguous [{B}, {sh.clip_len}, {sh.clip_dim}], got {tuple(clip_feature.shape)}")
        ia.clip_feature = clip_feature.data_ptr()
    if len(kimg_cache) != m.num_layers or len(vimg_cache) != m.num_layers:
        raise ValueError(f"dit_forward_i2v: image cache lists must have {m.num_layers} entries")
    want = (B, sh.clip_len, sh.num_heads, sh.head_dim)
    ia.kimg_cache_host, ia.vimg_cache_host = _cache_tables("dit_forward_i2v", model, (("kimg_cache", kimg_cache, want), ("vimg_cache", vimg_cache, want)),
                                                           noisy.device)
    _fold_pair(cross_keys, cross_log2w, (m.num_layers, B), noisy.device, "dit_forward_i2v")
    _forward_call(m, (a,), cross_keys, cross_log2w, _stream(noisy), i2v_args=ia)
    return flow, x0


@dit_forward_i2v.register_fake
def _(model, noisy, timestep, prompt_embeds, clip_feature, y, add_condition, k_cache, v_cache, ck_cache, cv_cache, kimg_cache, vimg_cache,
      workspace, evict_scratch, init_cross, cache_only, sink, evict, keep, write_start, attn_start, attn_end, start_frame, kv_index, global_end,
      cross_keys=None, cross_log2w=None):
    return _dit_forward_fake(model, noisy, cache_only)


@custom_op(f"{NAMESPACE}::i2v_assemble_y", mutates_args=("y",))
def i2v_assemble_y(latent: Tensor, y: Tensor, first_is_frame0: bool, ref_map: Optional[Tensor] = None) -> None:
    """A chunk of an i2v generator's conditioning tensor in one launch (sf_i2v_assemble_y): latent float32 [f, 16, h, w] (the
    VAE encoder's rows) -> y bf16 [20, f, h, w], any channel / frame strides over contiguous h x w planes (a frame range of a
    longer buffer): channels 0..3 the mask (1 in the clip's frame 0 when `first_is_frame0`), 4..19 bf16(latent); with
    ref_map (bf16 [h, w, 20] channels-last, `PoseEmbedder.embed_ref`'s storage) bf16(float(that) + float(map))."""
    _need_gpu(latent, "latent", torch.float32)
    _need_gpu(y, "y")
    if latent.dim() != 4 or not latent.is_contiguous():
        raise ValueError(f"i2v_assemble_y: latent must be contiguous [f, C, h, w], got {tuple(latent.shape)} {latent.stride()}")
    f, cl, h, w = latent.shape
    if y.dim() != 4 or y.shape[0] <= cl or tuple(y.shape[1:]) != (f, h, w) or y.stride(3) != 1 or y.stride(2) != w \
            or y.stride(1) < h * w or y.stride(0) < h * w or y.device != latent.device:
        raise ValueError(f"i2v_assemble_y: y must be [mask + {cl}, {f}, {h}, {w}] with contiguous h x w planes on {latent.device}, got "
                         f"{tuple(y.shape)} {y.stride()}")
    (n_in, s_in), (n_out, s_out) = sorted(((y.shape[0], y.stride(0)), (f, y.stride(1))), key=lambda d: (d[0] == 1, d[1]))
    if n_out > 1 and s_out < n_in * s_in:     # the kernel writes every plane: no two may share memory
        raise ValueError(f"i2v_assemble_y: y's planes overlap (strides {y.stride()})")
    if ref_map is not None:
        _need_gpu(ref_map, "ref_map")
        if tuple(ref_map.shape) != (h, w, y.shape[0]) or not ref_map.is_contiguous() or ref_map.device != latent.device:
            raise ValueError(f"i2v_assemble_y: ref_map must be contiguous [{h}, {w}, {y.shape[0]}] (channels-last), got {tuple(ref_map.shape)}")
    _lib.check(_lib.lib().sf_i2v_assemble_y(latent.data_ptr(), _ptr(ref_map), y.data_ptr(), f, y.shape[0] - cl, cl, h, w, y.stride(0), y.stride(1),
                                            int(first_is_frame0), _stream(latent)), "sf_i2v_assemble_y")


@i2v_assemble_y.register_fake
def _(latent, y, first_is_frame0, ref_map=None):
    return None   # writes only its mutated argument


@custom_op(f"{NAMESPACE}::dit_forward_pair",
           mutates_args=("k_cache", "v_cache", "ck_cache", "cv_cache", "workspace", "evict_scratch", "kv_index"))
def dit_forward_pair(model: int, ctx_noisy: Tensor, ctx_timestep: Tensor, noisy: Tensor, timestep: Tensor,
                     k_cache: List[Tensor], v_cache: List[Tensor], ck_cache: List[Tensor], cv_cache: List[Tensor],
                     workspace: Tensor, evict_scratch: Optional[Tensor], ctx_plan: List[int], plan: List[int],
                     kv_index: Optional[Tensor], global_end: int, cross_keys: Optional[Tensor] = None,
                     cross_log2w: Optional[Tensor] = None, ctx_add_condition: Optional[Tensor] = None,
                     add_condition: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The context pass of one chunk (cache_only) and the first denoising pass of the next in ONE call
    (sf_dit_forward with two passes): bit-identical to the two calls, twice the rows per GEMM.  `ctx_plan` / `plan` =
    [sink, evict, keep, write_start, attn_start, attn_end, start_frame] of the two passes; workspace sized for 2 x batch.
    cross_keys / cross_log2w as in dit_forward (read only); ctx_add_condition / add_condition: each pass's pose tokens, as
    dit_forward's add_condition.  Returns (flow, x0) of the denoising pass."""
    m = _model(model)
    if len(ctx_plan) != 7 or len(plan) != 7 or ctx_noisy.shape != noisy.shape or ctx_timestep.shape != timestep.shape:
        raise ValueError("dit_forward_pair: two passes of one shape with 7 plan integers each expected")
    a0, _, _ = _forward_args(m, model, ctx_noisy, ctx_timestep, None, ctx_add_condition, k_cache, v_cache, ck_cache, cv_cache, workspace, evict_scratch,
                             False, True, *ctx_plan, None, 0)
    a1, flow, x0 = _forward_args(m, model, noisy, timestep, None, add_condition, k_cache, v_cache, ck_cache, cv_cache, workspace, evict_scratch,
                                 False, False, *plan, kv_index, global_end)
    _fold_pair(cross_keys, cross_log2w, (m.num_layers, noisy.shape[0]), noisy.device, "dit_forward_pair")
    _forward_call(m, (a0, a1), cross_keys, cross_log2w, _stream(noisy))
    return flow, x0


@dit_forward_pair.register_fake
def _(model, ctx_noisy, ctx_timestep, noisy, timestep, k_cache, v_cache, ck_cache, cv_cache, workspace, evict_scratch, ctx_plan, plan,
      kv_index, global_end, cross_keys=None, cross_log2w=None, ctx_add_condition=None, add_condition=None):
    B, F, _, H, W = noisy.shape
    out_dim = _model(model).shape.out_dim
    return noisy.new_empty((B, F, out_dim, H, W)), noisy.new_empty((B, F, out_dim, H, W))


@dit_forward.register_fake
def _(model, noisy, timestep, prompt_embeds, add_condition, k_cache, v_cache, ck_cache, cv_cache, workspace, evict_scratch,
      init_cross, cache_only, sink, evict, keep, write_start, attn_start, attn_end, start_frame, kv_index, global_end,
      cross_keys, cross_log2w):
    return _dit_forward_fake(model, noisy, cache_only)


def _dit_forward_fake(model, noisy, cache_only):
    if cache_only:
        return noisy.new_empty((0,)), noisy.new_empty((0,))
    B, F, _, H, W = noisy.shape
    out_dim = _model(model).shape.out_dim
    return noisy.new_empty((B, F, out_dim, H, W)), noisy.new_empty((B, F, out_dim, H, W))


# ------------------------------------------------------------------------------------------ VAE decode / T5 encode
@custom_op(f"{NAMESPACE}::vae_decode_frames", mutates_args=("state", "scratch", "out"))
def vae_decode_frames(model: int, state: Tensor, scratch: Tensor, z: Tensor, out: Tensor, h: int, w: int, window_frames: int,
                      frame_index: int, window: int, history_at: int) -> None:
    """Consecutive latent frames z [F, z_dim, h, w] -> 1 (frame_index 0: F = 1) or 4 F pixel frames written to the front
    of `out` (float32 [T, 3, 8h, 8w]); `state` carries every convolution's two-frame history between calls; `frame_index`
    counts the latent frames decoded into it since its reset, `window` / `history_at` place the sliding history windows
    (sf_vae_decode_frames in include/sf_hip.h; `WanVAEDecoder.cached_decode` does the bookkeeping)."""
    m = _model(model)
    _need_gpu(z, "z")
    _need_gpu(out, "out", torch.float32)
    if z.dim() != 4 or not z.is_contiguous() or not out.is_contiguous():
        raise ValueError("vae_decode_frames: contiguous z [F, z_dim, h, w] and out expected")
    if tuple(z.shape[1:]) != (m.shape.z_dim, h, w):
        raise ValueError(f"vae_decode_frames: z must be [F, {m.shape.z_dim}, {h}, {w}], got {tuple(z.shape)}")
    _need_bytes("vae_decode_frames", state=state, scratch=scratch)
    sf_, tf_ = m.shape.spatial_factor, m.shape.temporal_factor
    frames = 1 if frame_index == 0 else tf_ * z.shape[0]
    if frame_index == 0 and z.shape[0] != 1:
        raise ValueError("vae_decode_frames: the frame that follows a reset (frame_index 0) is decoded alone")
    if out.numel() < frames * 3 * (sf_ * h) * (sf_ * w):
        raise ValueError(f"vae_decode_frames: out holds {out.numel()} floats, {frames} frames of 3 x {sf_ * h} x {sf_ * w} need "
                         f"{frames * 3 * sf_ * h * sf_ * w}")
    _lib.check(_lib.lib().sf_vae_decode_frames(C.byref(m.cmodel), state.data_ptr(), state.numel(), scratch.data_ptr(), scratch.numel(),
                                               z.data_ptr(), h, w, window_frames, frame_index, z.shape[0], window, history_at,
                                               out.data_ptr(), _stream(z)),
               "sf_vae_decode_frames")


@custom_op(f"{NAMESPACE}::taehv_decode_frames", mutates_args=("state", "scratch", "out"))
def taehv_decode_frames(model: int, state: Tensor, scratch: Tensor, z: Tensor, out: Tensor, h: int, w: int, clamp: bool) -> None:
    """Consecutive latent frames z [F, 16, h, w] -> 4 F pixel frames written to the front of `out` (float32
    [T, 3, 8h, 8w] = decode_video * 2 - 1, clamped to [-1, 1] when `clamp`); `state` carries the one-frame memory of the
    nine MemBlocks between calls (sf_taehv_decode_frames in include/sf_hip.h; `TAEHVDecoder.cached_decode` drives it)."""
    m = _model(model)
    _need_gpu(z, "z")
    _need_gpu(out, "out", torch.float32)
    if z.dim() != 4 or not z.is_contiguous() or not out.is_contiguous():
        raise ValueError("taehv_decode_frames: contiguous z [F, z_dim, h, w] and out expected")
    zc = m.cmodel.z_dim
    if tuple(z.shape[1:]) != (zc, h, w):
        raise ValueError(f"taehv_decode_frames: z must be [F, {zc}, {h}, {w}], got {tuple(z.shape)}")
    _need_bytes("taehv_decode_frames", state=state, scratch=scratch)
    need = 4 * z.shape[0] * 3 * (8 * h) * (8 * w)
    if out.numel() < need:
        raise ValueError(f"taehv_decode_frames: out holds {out.numel()} floats, {4 * z.shape[0]} frames of 3 x {8 * h} x {8 * w} need {need}")
    _lib.check(_lib.lib().sf_taehv_decode_frames(C.byref(m.cmodel), state.data_ptr(), state.numel(), scratch.data_ptr(), scratch.numel(),
                                                 z.data_ptr(), h, w, z.shape[0], int(clamp), out.data_ptr(), _stream(z)),
               "sf_taehv_decode_frames")


@custom_op(f"{NAMESPACE}::vae_encode_frames", mutates_args=("state", "scratch", "out"))
def vae_encode_frames(model: int, state: Tensor, scratch: Tensor, pixels: Tensor, out: Tensor, H: int, W: int, window_frames: int,
                      chunk_index: int, window: int, history_at: int) -> None:
    """Consecutive chunks of pixel frames [3, T, H, W] (bf16 or float32; T = 1 for chunk_index 0, else 4 per chunk; any
    channel stride, frames contiguous) -> float32 normalised latents written to `out` [n_chunks, z_dim, H/8, W/8];
    `state` carries every convolution's history between calls (sf_vae_encode_frames in include/sf_hip.h;
    `WanVAEEncoder.encode` does the bookkeeping)."""
    m = _model(model)
    _need_gpu(pixels, "pixels", None)
    _need_gpu(out, "out", torch.float32)
    if pixels.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"vae_encode_frames: pixels must be bf16 or float32, got {pixels.dtype}")
    if pixels.dim() != 4 or pixels.shape[0] != 3 or tuple(pixels.shape[2:]) != (H, W) or not pixels[0].is_contiguous():
        raise ValueError(f"vae_encode_frames: pixels must be [3, T, {H}, {W}] with contiguous frames, got {tuple(pixels.shape)}")
    _need_bytes("vae_encode_frames", state=state, scratch=scratch)
    T = pixels.shape[1]
    if chunk_index == 0:
        if T != 1:
            raise ValueError("vae_encode_frames: the chunk that follows a reset (chunk_index 0) is one pixel frame")
        n = 1
    else:
        if T % 4 or T == 0:
            raise ValueError(f"vae_encode_frames: {T} pixel frames is not a whole number of 4-frame chunks")
        n = T // 4
    sf_ = m.shape.spatial_factor
    if tuple(out.shape) != (n, m.shape.z_dim, H // sf_, W // sf_) or not out.is_contiguous():
        raise ValueError(f"vae_encode_frames: out must be contiguous [{n}, {m.shape.z_dim}, {H // sf_}, {W // sf_}], got {tuple(out.shape)}")
    _lib.check(_lib.lib().sf_vae_encode_frames(C.byref(m.cmodel), state.data_ptr(), state.numel(), scratch.data_ptr(), scratch.numel(),
                                               pixels.data_ptr(), int(pixels.dtype == torch.float32), pixels.stride(0), H, W, window_frames,
                                               chunk_index, n, window, history_at, out.data_ptr(), _stream(pixels)),
               "sf_vae_encode_frames")


@vae_encode_frames.register_fake
def _(model, state, scratch, pixels, out, H, W, window_frames, chunk_index, window, history_at):
    return None   # writes only its mutated arguments


@custom_op(f"{NAMESPACE}::taehv_encode_frames", mutates_args=("state", "scratch", "out"))
def taehv_encode_frames(model: int, state: Tensor, scratch: Tensor, pixels: Tensor, out: Tensor, H: int, W: int, lead: int) -> None:
    """Pixel frames [3, T, H, W] (bf16 or float32 in [-1, 1]; any channel stride, frames contiguous) with the first frame
    `lead` more times in front, lead + T a multiple of 4 -> float32 latents written to `out` [(lead + T) / 4, 16, H/8,
    W/8]; `state` carries the one-frame memory of the nine MemBlocks between calls (sf_taehv_encode_frames in
    include/sf_hip.h; `TAEHVEncoder.cached_encode` drives it)."""
    m = _model(model)
    _need_gpu(pixels, "pixels", None)
    _need_gpu(out, "out", torch.float32)
    if pixels.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"taehv_encode_frames: pixels must be bf16 or float32, got {pixels.dtype}")
    if pixels.dim() != 4 or pixels.shape[0] != 3 or pixels.shape[1] < 1 or tuple(pixels.shape[2:]) != (H, W) or not pixels[0].is_contiguous():
        raise ValueError(f"taehv_encode_frames: pixels must be [3, T, {H}, {W}] with contiguous frames, got {tuple(pixels.shape)}")
    _need_bytes("taehv_encode_frames", state=state, scratch=scratch)
    n = lead + pixels.shape[1]
    if not 0 <= lead <= 3 or n % 4:
        raise ValueError(f"taehv_encode_frames: lead={lead} + {pixels.shape[1]} pixel frames is not a whole number of 4-frame groups")
    zc = m.cmodel.head.cout
    if tuple(out.shape) != (n // 4, zc, H // 8, W // 8) or not out.is_contiguous():
        raise ValueError(f"taehv_encode_frames: out must be contiguous [{n // 4}, {zc}, {H // 8}, {W // 8}], got {tuple(out.shape)}")
    _lib.check(_lib.lib().sf_taehv_encode_frames(C.byref(m.cmodel), state.data_ptr(), state.numel(), scratch.data_ptr(), scratch.numel(),
                                                 pixels.data_ptr(), _lib.TAEHV_PIXEL_DTYPES[_dtype_name(pixels)],
                                                 pixels.stride(0), H, W, n, lead, out.data_ptr(), _stream(pixels)),
               "sf_taehv_encode_frames")


@taehv_encode_frames.register_fake
def _(model, state, scratch, pixels, out, H, W, lead):
    return None   # writes only its mutated arguments


@custom_op(f"{NAMESPACE}::t5_encode", mutates_args=("workspace",))
def t5_encode(model: int, ids: Tensor, mask: Tensor, buckets: Tensor, workspace: Tensor) -> Tensor:
    """umT5 encoder pass: ids, mask int64 [B, L] -> bf16 [B, L, dim], rows past each prompt's length zeroed (sf_t5_encode)."""
    m = _model(model)
    _need_gpu(ids, "ids", torch.int64), _need_gpu(mask, "mask", torch.int64), _need_gpu(buckets, "buckets", torch.int32)
    if ids.dim() != 2 or ids.shape != mask.shape or not ids.is_contiguous() or not mask.is_contiguous():
        raise ValueError("t5_encode: ids and mask must be contiguous [B, L]")
    B, L = ids.shape
    out = torch.empty(B, L, m.shape.dim, dtype=torch.bfloat16, device=ids.device)
    _lib.check(_lib.lib().sf_t5_encode(C.byref(m.cmodel), ids.data_ptr(), mask.data_ptr(), buckets.data_ptr(), B, L, out.data_ptr(),
                                       workspace.data_ptr(), workspace.numel(), _stream(ids)), "sf_t5_encode")
    return out


@t5_encode.register_fake
def _(model, ids, mask, buckets, workspace):
    return ids.new_empty((ids.shape[0], ids.shape[1], _model(model).shape.dim), dtype=torch.bfloat16)


@custom_op(f"{NAMESPACE}::clip_encode", mutates_args=("workspace",))
def clip_encode(model: int, frames: Tensor, workspace: Tensor) -> Tensor:
    """CLIP vision tower: frames [n, 3, H, W] float32 or bfloat16 in [-1, 1] -> float32 [n, L, dim] (sf_clip_encode)."""
    m = _model(model)
    _need_gpu(frames, "frames", None)
    if frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"clip_encode: frames must be float32 or bfloat16, got {frames.dtype}")
    if frames.dim() != 4 or frames.shape[1] != 3 or not frames.is_contiguous():
        raise ValueError(f"clip_encode: frames must be contiguous [n, 3, H, W], got {tuple(frames.shape)}")
    n, _, H, W = frames.shape
    out = torch.empty(n, m.shape.seq_len, m.shape.dim, dtype=torch.float32, device=frames.device)
    _lib.check(_lib.lib().sf_clip_encode(C.byref(m.cmodel), frames.data_ptr(), _lib.CLIP_DTYPES[_dtype_name(frames)], n, H, W,
                                         out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(frames)), "sf_clip_encode")
    return out


@clip_encode.register_fake
def _(model, frames, workspace):
    s = _model(model).shape
    return frames.new_empty((frames.shape[0], s.seq_len, s.dim), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ frame resizer
_RESIZE_DTYPES = {torch.uint8: "uint8", torch.float32: "float32", torch.bfloat16: "bfloat16"}


def _frame_shape(layout: str, n: int, h: int, w: int) -> Tuple[int, int, int, int]:
    if layout not in _lib.JPEG_LAYOUTS:
        raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
    return {"hwc": (n, h, w, 3), "pose": (3, n, h, w), "chw": (n, 3, h, w)}[layout]


def _frame_geometry(frames: Tensor, layout: str) -> Tuple[int, int, int]:
    """(n, h, w) of a uint8 frame tensor in `layout`."""
    if layout not in _lib.JPEG_LAYOUTS:
        raise ValueError(f"layout must be 'hwc', 'pose' or 'chw', got {layout!r}")
    if frames.dim() != 4 or frames.shape[{"hwc": 3, "pose": 0, "chw": 1}[layout]] != 3:
        raise ValueError(f"resize_frames: frames in layout {layout!r} must be {'[N, H, W, 3]' if layout == 'hwc' else '[3, N, H, W]' if layout == 'pose' else '[N, 3, H, W]'}, "
                         f"got {tuple(frames.shape)}")
    dims = {"hwc": (0, 1, 2), "pose": (1, 2, 3), "chw": (0, 2, 3)}[layout]
    return tuple(int(frames.shape[d]) for d in dims)


def _resize_launch(out: Tensor, frames: Tensor, bounds_h: Tensor, coefs_h: Tensor, bounds_v: Tensor, coefs_v: Tensor, filter: str, layout: str,
                   out_layout: str, crop: Optional[Sequence[int]]) -> None:
    if frames.dtype != torch.uint8:
        raise ValueError(f"resize_frames: frames must be uint8, got {frames.dtype}")
    n, h, w = _frame_geometry(frames, layout)
    if filter not in _lib.RESIZE_FILTERS:
        raise ValueError(f"filter must be 'bilinear' or 'bicubic', got {filter!r}")
    if out.dtype not in _RESIZE_DTYPES:
        raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {out.dtype}")
    if out_layout not in _lib.JPEG_LAYOUTS or out.dim() != 4:
        raise ValueError(f"resize_frames: out must be a 4-d tensor in layout 'hwc', 'pose' or 'chw', got {out_layout!r} {tuple(out.shape)}")
    on, oh, ow = _frame_geometry(out, out_layout)
    if on != n:
        raise ValueError(f"resize_frames: out holds {on} frames, frames {n}")
    _need_gpu(frames, "frames", torch.uint8), _need_gpu(out, "out", None)
    if not frames.is_contiguous() or not out.is_contiguous() or frames.data_ptr() % 4 or out.data_ptr() % 16:
        raise ValueError("resize_frames: frames and out must be contiguous, frames 4-byte and out 16-byte aligned")
    ch, cw = (h, w) if crop is None else (int(crop[2]), int(crop[3]))
    lib = _lib.lib()
    fcode = _lib.RESIZE_FILTERS[filter]
    for name, b, k, size_in, size_out in (("horizontal", bounds_h, coefs_h, cw, ow), ("vertical", bounds_v, coefs_v, ch, oh)):
        ks = lib.sf_resize_kernel_size(size_in, size_out, fcode)
        if ks == 0:
            _lib.check(-1, "sf_resize_kernel_size")
        for t in (b, k):
            _need_gpu(t, f"the {name} table", torch.int32)
        if tuple(b.shape) != (size_out, 2) or tuple(k.shape) != (size_out, ks) or not b.is_contiguous() or not k.is_contiguous():
            raise ValueError(f"resize_frames: the {name} table must be bounds [{size_out}, 2] and coefs [{size_out}, {ks}] for {size_in} -> {size_out} {filter}, "
                             f"got {tuple(b.shape)} and {tuple(k.shape)}")
    ccrop = None if crop is None else (C.c_int32 * 4)(*[int(v) for v in crop])
    _lib.check(lib.sf_resize_frames(frames.data_ptr(), _lib.JPEG_LAYOUTS[layout], n, h, w, ccrop, bounds_h.data_ptr(), coefs_h.data_ptr(), bounds_v.data_ptr(),
                                    coefs_v.data_ptr(), fcode, out.data_ptr(), _lib.JPEG_LAYOUTS[out_layout], _lib.JPEG_DTYPES[_RESIZE_DTYPES[out.dtype]], oh, ow,
                                    _stream(frames)), "sf_resize_frames")


@custom_op(f"{NAMESPACE}::resize_frames", mutates_args=())
def resize_frames(frames: Tensor, bounds_h: Tensor, coefs_h: Tensor, bounds_v: Tensor, coefs_v: Tensor, filter: str, layout: str, out_layout: str,
                  dtype: torch.dtype, crop: Optional[List[int]] = None) -> Tensor:
    """uint8 frames in `layout` -> frames of bounds_v.shape[0] x bounds_h.shape[0] in `out_layout` / `dtype`, with Pillow's bits
    (sf_resize_frames).  The tables are `resize_reference.coefficients` of the two axes, on the device."""
    n, _, _ = _frame_geometry(frames, layout)
    out = torch.empty(_frame_shape(out_layout, n, bounds_v.shape[0], bounds_h.shape[0]), dtype=dtype, device=frames.device)
    _resize_launch(out, frames, bounds_h, coefs_h, bounds_v, coefs_v, filter, layout, out_layout, crop)
    return out


@resize_frames.register_fake
def _(frames, bounds_h, coefs_h, bounds_v, coefs_v, filter, layout, out_layout, dtype, crop=None):
    n, _, _ = _frame_geometry(frames, layout)
    return frames.new_empty(_frame_shape(out_layout, n, bounds_v.shape[0], bounds_h.shape[0]), dtype=dtype)


@custom_op(f"{NAMESPACE}::resize_frames_out", mutates_args=("out",))
def resize_frames_out(out: Tensor, frames: Tensor, bounds_h: Tensor, coefs_h: Tensor, bounds_v: Tensor, coefs_v: Tensor, filter: str, layout: str,
                      out_layout: str, crop: Optional[List[int]] = None) -> None:
    """`resize_frames` into a caller's tensor (its shape gives the output size, its dtype the output type)."""
    _resize_launch(out, frames, bounds_h, coefs_h, bounds_v, coefs_v, filter, layout, out_layout, crop)


@resize_frames_out.register_fake
def _(out, frames, bounds_h, coefs_h, bounds_v, coefs_v, filter, layout, out_layout, crop=None):
    return None


# ------------------------------------------------------------------------------------------ raw YUV frames
def _yuv_frame_bytes(fmt: str, h: int, w: int) -> int:
    if fmt not in _lib.YUV_FORMATS:
        raise ValueError(f"format must be one of {', '.join(_lib.YUV_FORMATS)}, got {fmt!r}")
    need = _lib.lib().sf_yuv_frame_bytes(_lib.YUV_FORMATS[fmt], h, w)
    if need == 0:
        _lib.check(-1, "sf_yuv_frame_bytes")
    return need


def _yuv_constants(constants: Sequence[int]):
    if len(constants) != 16:
        raise ValueError(f"constants must be the sixteen integers of yuv_reference.constants, got {len(constants)}")
    return (C.c_int32 * 16)(*[int(v) for v in constants])


def _yuv_raw_frames(raw: Tensor, fmt: str, h: int, w: int) -> int:
    """n of uint8 raw [n, frame_bytes]."""
    if raw.dtype != torch.uint8 or raw.dim() != 2 or raw.shape[0] < 1:
        raise ValueError(f"yuv_decode_frames: raw must be uint8 [n, frame_bytes], got {raw.dtype} {tuple(raw.shape)}")
    return int(raw.shape[0])


@custom_op(f"{NAMESPACE}::yuv_decode_frames", mutates_args=())
def yuv_decode_frames(raw: Tensor, fmt: str, height: int, width: int, constants: List[int], chroma: str, layout: str, dtype: torch.dtype) -> Tensor:
    """uint8 raw [n, frame_bytes] of `fmt` frames -> n frames of height x width in `layout` / `dtype` as `yuv_reference.decode`
    defines them (sf_yuv_decode_frames).  constants: `yuv_reference.constants(matrix, range)`."""
    n = _yuv_raw_frames(raw, fmt, height, width)
    need = _yuv_frame_bytes(fmt, height, width)
    if raw.shape[1] != need:
        raise ValueError(f"yuv_decode_frames: a {height}x{width} {fmt} frame has {need} bytes, raw holds {raw.shape[1]} per frame")
    if chroma not in _lib.YUV_CHROMAS:
        raise ValueError(f"chroma must be 'nearest' or 'triangle', got {chroma!r}")
    if dtype not in _RESIZE_DTYPES:
        raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
    _need_gpu(raw, "raw", torch.uint8)
    if not raw.is_contiguous():
        raise ValueError("yuv_decode_frames: raw must be contiguous")
    out = torch.empty(_frame_shape(layout, n, height, width), dtype=dtype, device=raw.device)
    _lib.check(_lib.lib().sf_yuv_decode_frames(raw.data_ptr(), _lib.YUV_FORMATS[fmt], n, height, width, _yuv_constants(constants), _lib.YUV_CHROMAS[chroma],
                                               out.data_ptr(), _lib.JPEG_LAYOUTS[layout], _lib.JPEG_DTYPES[_RESIZE_DTYPES[dtype]], _stream(raw)),
               "sf_yuv_decode_frames")
    return out


@yuv_decode_frames.register_fake
def _(raw, fmt, height, width, constants, chroma, layout, dtype):
    return raw.new_empty(_frame_shape(layout, raw.shape[0], height, width), dtype=dtype)


def _yuv_encode_geometry(frames: Tensor) -> Tuple[int, int, int]:
    """(n, h, w) of uint8 [n, h, w, 3] or float32 / bfloat16 [n, 3, h, w]."""
    if frames.dtype not in _RESIZE_DTYPES:
        raise ValueError(f"yuv_encode_frames: frames must be uint8, float32 or bfloat16, got {frames.dtype}")
    u8 = frames.dtype == torch.uint8
    if frames.dim() != 4 or frames.shape[3 if u8 else 1] != 3 or frames.shape[0] < 1:
        raise ValueError(f"yuv_encode_frames: expected {'uint8 [n, h, w, 3]' if u8 else 'float [n, 3, h, w]'}, got {tuple(frames.shape)}")
    return (int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])) if u8 else (int(frames.shape[0]), int(frames.shape[2]), int(frames.shape[3]))


@custom_op(f"{NAMESPACE}::yuv_encode_frames", mutates_args=())
def yuv_encode_frames(frames: Tensor, fmt: str, constants: List[int], range01: bool) -> Tensor:
    """uint8 [n, h, w, 3] or float32 / bfloat16 [n, 3, h, w] frames (range01: in (0, 1), else in (-1, 1)) -> uint8
    [n, frame_bytes] of `fmt` as `yuv_reference.encode` defines them (sf_yuv_encode_frames)."""
    n, h, w = _yuv_encode_geometry(frames)
    need = _yuv_frame_bytes(fmt, h, w)
    _need_gpu(frames, "frames", None)
    if not frames.is_contiguous():
        raise ValueError("yuv_encode_frames: frames must be contiguous")
    out = torch.empty((n, need), dtype=torch.uint8, device=frames.device)
    _lib.check(_lib.lib().sf_yuv_encode_frames(frames.data_ptr(), _lib.JPEG_DTYPES[_RESIZE_DTYPES[frames.dtype]],
                                               _lib.JPEG_RANGES[(0, 1) if range01 else (-1, 1)], n, h, w, _yuv_constants(constants), out.data_ptr(),
                                               _lib.YUV_FORMATS[fmt], _stream(frames)), "sf_yuv_encode_frames")
    return out


@yuv_encode_frames.register_fake
def _(frames, fmt, constants, range01):
    n, h, w = _yuv_encode_geometry(frames)
    from . import yuv_reference
    return frames.new_empty((n, yuv_reference.frame_bytes(fmt, h, w)), dtype=torch.uint8)


# ------------------------------------------------------------------------------------------ pose renderer
def _pose_render_geometry(keypoints: Tensor) -> Tuple[int, int]:
    """(F, P) of float32 keypoints [F, P, 134, 3]."""
    if keypoints.dim() != 4 or tuple(keypoints.shape[2:]) != (134, 3) or keypoints.shape[0] < 1 or not 1 <= keypoints.shape[1] <= _lib.POSE_RENDER_MAX_PEOPLE:
        raise ValueError(f"pose_render_frames: keypoints must be [F, P, 134, 3] with F >= 1 and 1 <= P <= {_lib.POSE_RENDER_MAX_PEOPLE}, "
                         f"got {tuple(keypoints.shape)}")
    return int(keypoints.shape[0]), int(keypoints.shape[1])


def _pose_render_launch(out: Tensor, keypoints: Tensor, layout: str, normalized: bool, score_threshold: float) -> None:
    if keypoints.dtype != torch.float32:
        raise ValueError(f"pose_render_frames: keypoints must be float32, got {keypoints.dtype}")
    f, p = _pose_render_geometry(keypoints)
    if out.dtype not in _RESIZE_DTYPES:
        raise ValueError(f"dtype must be torch.uint8, float32 or bfloat16, got {out.dtype}")
    if layout not in _lib.JPEG_LAYOUTS or out.dim() != 4:
        raise ValueError(f"pose_render_frames: out must be a 4-d tensor in layout 'hwc', 'pose' or 'chw', got {layout!r} {tuple(out.shape)}")
    on, h, w = _frame_geometry(out, layout)
    if on != f:
        raise ValueError(f"pose_render_frames: out holds {on} frames, keypoints {f}")
    _need_gpu(keypoints, "keypoints", torch.float32), _need_gpu(out, "out", None)
    if out.device != keypoints.device:
        raise ValueError(f"pose_render_frames: keypoints on {keypoints.device}, out on {out.device}")
    if not keypoints.is_contiguous() or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError("pose_render_frames: keypoints and out must be contiguous, out 16-byte aligned")
    args = _lib.PoseRenderArgs(keypoints=keypoints.data_ptr(), out=out.data_ptr(), F=f, P=p, H=h, W=w, layout=_lib.JPEG_LAYOUTS[layout],
                               dtype=_lib.JPEG_DTYPES[_RESIZE_DTYPES[out.dtype]], normalized=int(bool(normalized)), score_threshold=score_threshold)
    _lib.check(_lib.lib().sf_pose_render_frames(C.byref(args), _stream(keypoints)), "sf_pose_render_frames")


@custom_op(f"{NAMESPACE}::pose_render_frames", mutates_args=())
def pose_render_frames(keypoints: Tensor, height: int, width: int, layout: str, dtype: torch.dtype, normalized: bool = True,
                       score_threshold: float = 0.3) -> Tensor:
    """float32 keypoints [F, P, 134, 3] on the device -> F skeleton frames of height x width in `layout` / `dtype`, every
    pixel as `pose_render_reference.render` defines it (sf_pose_render_frames)."""
    f, _ = _pose_render_geometry(keypoints)
    out = torch.empty(_frame_shape(layout, f, height, width), dtype=dtype, device=keypoints.device)
    _pose_render_launch(out, keypoints, layout, normalized, score_threshold)
    return out


@pose_render_frames.register_fake
def _(keypoints, height, width, layout, dtype, normalized=True, score_threshold=0.3):
    f, _ = _pose_render_geometry(keypoints)
    return keypoints.new_empty(_frame_shape(layout, f, height, width), dtype=dtype)


@custom_op(f"{NAMESPACE}::pose_render_frames_out", mutates_args=("out",))
def pose_render_frames_out(out: Tensor, keypoints: Tensor, layout: str, normalized: bool = True, score_threshold: float = 0.3) -> None:
    """`pose_render_frames` into a caller's tensor (its shape gives the frame size, its dtype the output type)."""
    _pose_render_launch(out, keypoints, layout, normalized, score_threshold)


@pose_render_frames_out.register_fake
def _(out, keypoints, layout, normalized=True, score_threshold=0.3):
    return None


# ------------------------------------------------------------------------------------------ pose retargeter
def _pose_retarget_geometry(src: Tensor, first: Tensor, ref: Tensor, n_out: int) -> Tuple[int, int, int]:
    """(n_src, P, Pr) of src [n, P, 134, 3], first [P, 134, 3] and ref [Pr, 134, 3]."""
    _pose_render_geometry(src)
    n, p = int(src.shape[0]), int(src.shape[1])
    if tuple(first.shape) != (p, 134, 3):
        raise ValueError(f"pose_retarget_frames: first must be [{p}, 134, 3] (the clip's frame 0), got {tuple(first.shape)}")
    if ref.dim() != 3 or tuple(ref.shape[1:]) != (134, 3) or ref.shape[0] not in (1, p):
        raise ValueError(f"pose_retarget_frames: ref must be [Pr, 134, 3] with Pr = 1 or {p}, got {tuple(ref.shape)}")
    if not 1 <= n_out <= _lib.POSE_RETARGET_MAX_FRAMES:
        raise ValueError(f"pose_retarget_frames: n_out={n_out} (1..{_lib.POSE_RETARGET_MAX_FRAMES})")
    return n, p, int(ref.shape[0])


@custom_op(f"{NAMESPACE}::pose_retarget_frames", mutates_args=())
def pose_retarget_frames(src: Tensor, first: Tensor, ref: Tensor, src0: int, out0: int, n_out: int, num: int, den: int, src_sx: float,
                         src_sy: float, ref_sx: float, ref_sy: float, score_threshold: float = 0.3, align: bool = True) -> Tensor:
    """float32 source frames src0 .. of a clip [n, P, 134, 3], its frame 0 [P, 134, 3] and the reference [Pr, 134, 3], all on
    one device -> output frames out0 .. out0 + n_out - 1 at source_fps / target_fps = num / den, float32 [n_out, P, 134, 3] in
    output pixels, every number as `pose_retarget_reference.frames` defines it (sf_pose_retarget_frames)."""
    n, p, pr = _pose_retarget_geometry(src, first, ref, n_out)
    for name, t in (("src", src), ("first", first), ("ref", ref)):
        _need_gpu(t, name, torch.float32)
        if t.device != src.device or not t.is_contiguous():
            raise ValueError(f"pose_retarget_frames: {name} must be contiguous and on src's device {src.device}")
    out = torch.empty((n_out, p, 134, 3), dtype=torch.float32, device=src.device)
    args = _lib.PoseRetargetArgs(src=src.data_ptr(), first=first.data_ptr(), ref=ref.data_ptr(), out=out.data_ptr(), src0=src0, out0=out0, n_src=n,
                                 n_out=n_out, people=p, ref_people=pr, num=num, den=den, src_sx=src_sx, src_sy=src_sy, ref_sx=ref_sx, ref_sy=ref_sy,
                                 score_threshold=score_threshold, align=int(bool(align)))
    _lib.check(_lib.lib().sf_pose_retarget_frames(C.byref(args), _stream(src)), "sf_pose_retarget_frames")
    return out


@pose_retarget_frames.register_fake
def _(src, first, ref, src0, out0, n_out, num, den, src_sx, src_sy, ref_sx, ref_sy, score_threshold=0.3, align=True):
    _, p, _ = _pose_retarget_geometry(src, first, ref, n_out)
    return src.new_empty((n_out, p, 134, 3), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ pose smoother
def _pose_clip_geometry(op: str, src: Tensor) -> Tuple[int, int]:
    """(n, P) of a clip src [n, P, 134, 3], for the operator `op`."""
    if src.dim() != 4 or tuple(src.shape[2:]) != (134, 3) or not 1 <= src.shape[0] <= _lib.POSE_RETARGET_MAX_FRAMES \
            or not 1 <= src.shape[1] <= _lib.POSE_RENDER_MAX_PEOPLE:
        raise ValueError(f"{op}: src must be [n, P, 134, 3] with 1 <= n <= {_lib.POSE_RETARGET_MAX_FRAMES} and 1 <= P <= "
                         f"{_lib.POSE_RENDER_MAX_PEOPLE}, got {tuple(src.shape)}")
    return int(src.shape[0]), int(src.shape[1])


def _pose_smooth_geometry(src: Tensor, state: Tensor) -> Tuple[int, int]:
    """(n, P) of src [n, P, 134, 3] and its state, int32 [P, 134, 8]."""
    n, p = _pose_clip_geometry("pose_smooth_frames", src)
    if state.dtype != torch.int32 or tuple(state.shape) != (p, 134, 8):
        raise ValueError(f"pose_smooth_frames: state must be int32 [{p}, 134, 8], got {state.dtype} {tuple(state.shape)}")
    return n, p


@custom_op(f"{NAMESPACE}::pose_smooth_frames", mutates_args=("state",))
def pose_smooth_frames(src: Tensor, state: Tensor, period: float, min_cutoff: float, beta: float, kd: float, score_threshold: float = 0.3,
                       max_gap: int = 0) -> Tensor:
    """float32 frames [n, P, 134, 3] of a clip and the packed filter state int32 [P, 134, 8] it has reached (zeros before the
    first frame), on one device -> the frames smoothed, float32 [n, P, 134, 3], every number as
    `pose_smooth_reference.frames` defines it; `state` is advanced in place (sf_pose_smooth_frames)."""
    n, p = _pose_smooth_geometry(src, state)
    _need_gpu(src, "src", torch.float32)
    _need_gpu(state, "state", torch.int32)
    if state.device != src.device or not src.is_contiguous() or not state.is_contiguous() or state.data_ptr() % 16:
        raise ValueError(f"pose_smooth_frames: src and state must be contiguous and on one device, state 16-byte aligned (src on {src.device}, "
                         f"state on {state.device})")
    out = torch.empty((n, p, 134, 3), dtype=torch.float32, device=src.device)
    args = _lib.PoseSmoothArgs(src=src.data_ptr(), out=out.data_ptr(), state=state.data_ptr(), n=n, people=p, period=period, min_cutoff=min_cutoff,
                               beta=beta, kd=kd, score_threshold=score_threshold, max_gap=max_gap)
    _lib.check(_lib.lib().sf_pose_smooth_frames(C.byref(args), _stream(src)), "sf_pose_smooth_frames")
    return out


@pose_smooth_frames.register_fake
def _(src, state, period, min_cutoff, beta, kd, score_threshold=0.3, max_gap=0):
    n, p = _pose_smooth_geometry(src, state)
    return src.new_empty((n, p, 134, 3), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ pose tracker
def _pose_track_geometry(src: Tensor, state: Tensor, slots: int) -> Tuple[int, int]:
    """(n, P) of src [n, P, 134, 3]; its state is int32 [slots + 1, 40]."""
    n, p = _pose_clip_geometry("pose_track_frames", src)
    if not 1 <= slots <= _lib.POSE_RENDER_MAX_PEOPLE:
        raise ValueError(f"pose_track_frames: slots must be 1..{_lib.POSE_RENDER_MAX_PEOPLE}, got {slots}")
    if state.dtype != torch.int32 or tuple(state.shape) != (slots + 1, _lib.POSE_TRACK_STATE_WORDS):
        raise ValueError(f"pose_track_frames: state must be int32 [{slots + 1}, {_lib.POSE_TRACK_STATE_WORDS}], got {state.dtype} {tuple(state.shape)}")
    return n, p


@custom_op(f"{NAMESPACE}::pose_track_frames", mutates_args=("state",))
def pose_track_frames(src: Tensor, state: Tensor, slots: int, gate2: float, score_threshold: float = 0.3, min_points: int = 4,
                      min_common: int = 3, max_age: int = 2) -> Tuple[Tensor, Tensor]:
    """float32 detections [n, P, 134, 3] of a clip, in any order per frame, and the packed tracker state int32 [slots + 1, 40]
    it has reached (zeros before the first frame), on one device -> (the frames with each person in one slot, float32
    [n, slots, 134, 3], and the track ids int32 [n, slots]), as `pose_track_reference.frames` defines them; `state` is
    advanced in place (sf_pose_track_frames; its scratch of n * slots int32 is allocated here)."""
    n, p = _pose_track_geometry(src, state, slots)
    _need_gpu(src, "src", torch.float32)
    _need_gpu(state, "state", torch.int32)
    if state.device != src.device or not src.is_contiguous() or not state.is_contiguous() or state.data_ptr() % 16:
        raise ValueError(f"pose_track_frames: src and state must be contiguous and on one device, state 16-byte aligned (src on {src.device}, "
                         f"state on {state.device})")
    out = torch.empty((n, slots, 134, 3), dtype=torch.float32, device=src.device)
    ids = torch.empty((n, slots), dtype=torch.int32, device=src.device)
    assign = torch.empty((n, slots), dtype=torch.int32, device=src.device)
    args = _lib.PoseTrackArgs(src=src.data_ptr(), out=out.data_ptr(), ids=ids.data_ptr(), state=state.data_ptr(), assign=assign.data_ptr(), n=n,
                              people=p, slots=slots, min_points=min_points, min_common=min_common, max_age=max_age, gate2=gate2,
                              score_threshold=score_threshold)
    _lib.check(_lib.lib().sf_pose_track_frames(C.byref(args), _stream(src)), "sf_pose_track_frames")
    return out, ids


@pose_track_frames.register_fake
def _(src, state, slots, gate2, score_threshold=0.3, min_points=4, min_common=3, max_age=2):
    n, _p = _pose_track_geometry(src, state, slots)
    return src.new_empty((n, slots, 134, 3), dtype=torch.float32), src.new_empty((n, slots), dtype=torch.int32)


# ------------------------------------------------------------------------------------------ DWPose glue
def _pose_boxes_geometry(head: Tensor, in_h: int, in_w: int, strides: Sequence[int], max_people: int) -> Tuple[int, int, int]:
    """(F, A, C) of a head [F, A, 5 + C] for the detector's input size and strides."""
    if not 1 <= len(strides) <= _lib.POSE_BOXES_MAX_STRIDES or any(s < 1 or in_h % s or in_w % s for s in strides) or in_h < 1 or in_w < 1:
        raise ValueError(f"pose_boxes_decode: strides must be 1..{_lib.POSE_BOXES_MAX_STRIDES} divisors of the input size {in_h} x {in_w}, got {list(strides)}")
    anchors = sum((in_h // s) * (in_w // s) for s in strides)
    if anchors > _lib.POSE_BOXES_MAX_ANCHORS:
        raise ValueError(f"pose_boxes_decode: {anchors} anchors, at most {_lib.POSE_BOXES_MAX_ANCHORS}")
    if head.dim() != 3 or not 1 <= head.shape[0] <= _lib.POSE_BOXES_MAX_FRAMES or head.shape[1] != anchors \
            or not 6 <= head.shape[2] <= 5 + _lib.POSE_BOXES_MAX_CLASSES:
        raise ValueError(f"pose_boxes_decode: head must be [F, {anchors}, 5 + C] with 1 <= F <= {_lib.POSE_BOXES_MAX_FRAMES} and 1 <= C <= "
                         f"{_lib.POSE_BOXES_MAX_CLASSES}, got {tuple(head.shape)}")
    if not 1 <= max_people <= _lib.POSE_RENDER_MAX_PEOPLE:
        raise ValueError(f"pose_boxes_decode: max_people must be 1..{_lib.POSE_RENDER_MAX_PEOPLE}, got {max_people}")
    return int(head.shape[0]), anchors, int(head.shape[2]) - 5


@custom_op(f"{NAMESPACE}::pose_boxes_decode", mutates_args=())
def pose_boxes_decode(head: Tensor, in_h: int, in_w: int, strides: List[int], ratio: float, max_people: int, class_index: int = 0,
                      score_threshold: float = 0.3, iou_threshold: float = 0.45, decoded: bool = False) -> Tuple[Tensor, Tensor]:
    """A YOLOX head float32 [F, A, 5 + C] on the device -> (boxes float32 [F, P, 5] = (x1, y1, x2, y2, score) in source-frame
    pixels, count int32 [F]) after greedy NMS, as `pose_estimate_reference.decode_boxes` defines them (sf_pose_boxes_decode;
    its scratch of F * A * 5 floats is allocated here)."""
    f, a, c = _pose_boxes_geometry(head, in_h, in_w, strides, max_people)
    _need_gpu(head, "head", torch.float32)
    if not head.is_contiguous():
        raise ValueError("pose_boxes_decode: head must be contiguous")
    boxes = torch.empty((f, max_people, 5), dtype=torch.float32, device=head.device)
    count = torch.empty((f,), dtype=torch.int32, device=head.device)
    scratch = torch.empty((f, 5, a), dtype=torch.float32, device=head.device)
    args = _lib.PoseBoxesArgs(head=head.data_ptr(), boxes=boxes.data_ptr(), count=count.data_ptr(), scratch=scratch.data_ptr(), F=f, A=a, C=c,
                              P=max_people, in_h=in_h, in_w=in_w, n_strides=len(strides),
                              strides=(C.c_int32 * _lib.POSE_BOXES_MAX_STRIDES)(*strides), class_index=class_index, decoded=int(bool(decoded)),
                              ratio=ratio, score_threshold=score_threshold, iou_threshold=iou_threshold)
    _lib.check(_lib.lib().sf_pose_boxes_decode(C.byref(args), _stream(head)), "sf_pose_boxes_decode")
    return boxes, count


@pose_boxes_decode.register_fake
def _(head, in_h, in_w, strides, ratio, max_people, class_index=0, score_threshold=0.3, iou_threshold=0.45, decoded=False):
    f, _a, _c = _pose_boxes_geometry(head, in_h, in_w, strides, max_people)
    return head.new_empty((f, max_people, 5), dtype=torch.float32), head.new_empty((f,), dtype=torch.int32)


def _pose_people_geometry(op: str, boxes: Tensor, count: Tensor) -> Tuple[int, int]:
    """(F, P) of boxes float32 [F, P, 5] and count int32 [F]."""
    if boxes.dim() != 3 or boxes.shape[2] != 5 or not 1 <= boxes.shape[0] <= _lib.POSE_BOXES_MAX_FRAMES \
            or not 1 <= boxes.shape[1] <= _lib.POSE_RENDER_MAX_PEOPLE or boxes.dtype != torch.float32:
        raise ValueError(f"{op}: boxes must be float32 [F, P, 5] with 1 <= F <= {_lib.POSE_BOXES_MAX_FRAMES} and 1 <= P <= "
                         f"{_lib.POSE_RENDER_MAX_PEOPLE}, got {boxes.dtype} {tuple(boxes.shape)}")
    if count.dtype != torch.int32 or tuple(count.shape) != (boxes.shape[0],):
        raise ValueError(f"{op}: count must be int32 [{boxes.shape[0]}], got {count.dtype} {tuple(count.shape)}")
    return int(boxes.shape[0]), int(boxes.shape[1])


def _pose_crop_size(op: str, out_h: int, out_w: int) -> None:
    if not 1 <= out_h <= _lib.POSE_CROP_MAX_SIZE or not 1 <= out_w <= _lib.POSE_CROP_MAX_SIZE:
        raise ValueError(f"{op}: out_size must be 1..{_lib.POSE_CROP_MAX_SIZE} each way, got {out_h} x {out_w}")


def _pose_crop_geometry(frames: Tensor, boxes: Tensor, count: Tensor, layout: str, out_h: int, out_w: int, dtype: torch.dtype) -> Tuple[int, int, int, int]:
    f, p = _pose_people_geometry("pose_crop_people", boxes, count)
    n, h, w = _frame_geometry(frames, layout)
    if frames.dtype != torch.uint8 or n != f or not 1 <= h <= _lib.POSE_CROP_MAX_FRAME or not 1 <= w <= _lib.POSE_CROP_MAX_FRAME:
        raise ValueError(f"pose_crop_people: frames must be {f} uint8 frames of at most {_lib.POSE_CROP_MAX_FRAME} pixels each way, got {frames.dtype} "
                         f"{tuple(frames.shape)} in layout {layout!r}")
    _pose_crop_size("pose_crop_people", out_h, out_w)
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"pose_crop_people: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    return f, p, h, w


def _same_device(op: str, first: Tensor, **others: Tensor) -> None:
    for name, t in others.items():
        if not t.is_cuda or t.device != first.device or not t.is_contiguous():
            raise ValueError(f"{op}: {name} must be contiguous and on {first.device} (the HIP path has no CPU fallback), got {t.device}")


@custom_op(f"{NAMESPACE}::pose_crop_people", mutates_args=())
def pose_crop_people(frames: Tensor, boxes: Tensor, count: Tensor, layout: str, out_h: int, out_w: int, padding: float, mean: List[float],
                     std: List[float], bgr: bool, dtype: torch.dtype) -> Tensor:
    """uint8 frames in `layout` and the people of `pose_boxes_decode` -> the pose network's input [F * P, 3, out_h, out_w] in
    `dtype`, zeros for the rows without a person, as `pose_estimate_reference.crop_people` defines it (sf_pose_crop_people)."""
    f, p, h, w = _pose_crop_geometry(frames, boxes, count, layout, out_h, out_w, dtype)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("pose_crop_people: mean and std must be three numbers each")
    _need_gpu(frames, "frames", torch.uint8)
    _same_device("pose_crop_people", frames, frames=frames, boxes=boxes, count=count)
    out = torch.empty((f * p, 3, out_h, out_w), dtype=dtype, device=frames.device)
    args = _lib.PoseCropArgs(frames=frames.data_ptr(), boxes=boxes.data_ptr(), count=count.data_ptr(), out=out.data_ptr(), F=f, P=p, H=h, W=w,
                             layout=_lib.JPEG_LAYOUTS[layout], out_h=out_h, out_w=out_w, dtype=_lib.JPEG_DTYPES[_RESIZE_DTYPES[dtype]],
                             bgr=int(bool(bgr)), padding=padding, mean=(C.c_float * 3)(*mean), std=(C.c_float * 3)(*std))
    _lib.check(_lib.lib().sf_pose_crop_people(C.byref(args), _stream(frames)), "sf_pose_crop_people")
    return out


@pose_crop_people.register_fake
def _(frames, boxes, count, layout, out_h, out_w, padding, mean, std, bgr, dtype):
    f, p, _h, _w = _pose_crop_geometry(frames, boxes, count, layout, out_h, out_w, dtype)
    return frames.new_empty((f * p, 3, out_h, out_w), dtype=dtype)


def _pose_simcc_geometry(simcc_x: Tensor, simcc_y: Tensor, boxes: Tensor, count: Tensor, height: int, width: int, out_h: int, out_w: int,
                         order: Tensor) -> Tuple[int, int]:
    f, p = _pose_people_geometry("pose_simcc_decode", boxes, count)
    for name, t in (("simcc_x", simcc_x), ("simcc_y", simcc_y)):
        if t.dim() != 3 or t.shape[0] != f * p or t.shape[1] != _lib.POSE_SIMCC_POINTS or not 1 <= t.shape[2] <= _lib.POSE_SIMCC_MAX_BINS:
            raise ValueError(f"pose_simcc_decode: {name} must be [{f * p}, {_lib.POSE_SIMCC_POINTS}, bins] with 1 <= bins <= {_lib.POSE_SIMCC_MAX_BINS}, "
                             f"got {tuple(t.shape)}")
    if simcc_x.dtype != simcc_y.dtype or _dtype_name(simcc_x) not in _lib.POSE_SIMCC_DTYPES:
        raise ValueError(f"pose_simcc_decode: simcc_x and simcc_y must both be float32 or both float16, got {simcc_x.dtype} and {simcc_y.dtype}")
    if not 1 <= height <= _lib.POSE_CROP_MAX_FRAME or not 1 <= width <= _lib.POSE_CROP_MAX_FRAME:
        raise ValueError(f"pose_simcc_decode: the frame size must be 1..{_lib.POSE_CROP_MAX_FRAME} each way, got {height} x {width}")
    _pose_crop_size("pose_simcc_decode", out_h, out_w)
    if order.dtype != torch.uint8 or tuple(order.shape) != (134,):
        raise ValueError(f"pose_simcc_decode: order must be a host uint8 tensor [134] of indices below 134, got {order.dtype} {tuple(order.shape)}")
    return f, p


@custom_op(f"{NAMESPACE}::pose_simcc_decode", mutates_args=())
def pose_simcc_decode(simcc_x: Tensor, simcc_y: Tensor, boxes: Tensor, count: Tensor, height: int, width: int, out_h: int, out_w: int,
                      padding: float, split_ratio: float, normalized: bool, neck_threshold: float, order: Tensor) -> Tensor:
    """SimCC logits [F * P, 133, Wx] and [F * P, 133, Wy] (float32 or float16) and the people they were cropped for -> keypoints
    float32 [F, P, 134, 3] in the renderer's layout, as `pose_estimate_reference.decode_simcc` defines them (sf_pose_simcc_decode).  order: uint8 [134] in HOST memory,
    `pose_estimate_reference.reorder_table` (the library reads it before it launches)."""
    f, p = _pose_simcc_geometry(simcc_x, simcc_y, boxes, count, height, width, out_h, out_w, order)
    _need_gpu(simcc_x, "simcc_x", None)
    _same_device("pose_simcc_decode", simcc_x, simcc_x=simcc_x, simcc_y=simcc_y, boxes=boxes, count=count)
    out = torch.empty((f, p, 134, 3), dtype=torch.float32, device=simcc_x.device)
    if order.is_cuda or not order.is_contiguous():
        raise ValueError("pose_simcc_decode: order must be a contiguous host tensor")
    args = _lib.PoseSimccArgs(simcc_x=simcc_x.data_ptr(), simcc_y=simcc_y.data_ptr(), boxes=boxes.data_ptr(), count=count.data_ptr(),
                              out=out.data_ptr(), order=order.data_ptr(), F=f, P=p, H=height, W=width, Wx=simcc_x.shape[2], Wy=simcc_y.shape[2],
                              dtype=_lib.POSE_SIMCC_DTYPES[_dtype_name(simcc_x)], out_h=out_h, out_w=out_w, normalized=int(bool(normalized)),
                              padding=padding, split_ratio=split_ratio, neck_threshold=neck_threshold)
    _lib.check(_lib.lib().sf_pose_simcc_decode(C.byref(args), _stream(simcc_x)), "sf_pose_simcc_decode")
    return out


@pose_simcc_decode.register_fake
def _(simcc_x, simcc_y, boxes, count, height, width, out_h, out_w, padding, split_ratio, normalized, neck_threshold, order):
    f, p = _pose_simcc_geometry(simcc_x, simcc_y, boxes, count, height, width, out_h, out_w, order)
    return simcc_x.new_empty((f, p, 134, 3), dtype=torch.float32)


# every operator this module registered, by its name under torch.ops.sf_hip
OPS = tuple(op._name for op in list(globals().values()) if isinstance(op, torch.library.CustomOpDef))
