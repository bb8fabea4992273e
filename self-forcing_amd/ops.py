"""Per-kernel Python entry points over the C-ABI (torch tensors in, torch tensors out).

torch is used only for device memory and the current stream; every computation below runs in
the hand-written HIP kernels of csrc/.  The operators that also exist as PyTorch custom ops (`torch_ops.py`:
gemm, attention, lincomb, add_noise) are called through `torch.ops.sf_hip.*`; the remaining per-kernel test entry
points bind the C-ABI directly.  All functions require CUDA(ROCm) bf16 tensors and
raise if the library is missing -- there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.sf_hip.*)
from .torch_ops import _dtype_name, _ptr, _stream
from ._lib import (ACT_GELU, ACT_NONE, ACT_SILU, CONV_BIAS, CONV_BIAS_CLAMP_F32, CONV_BIAS_RESID, EPI_BIAS,
                   EPI_BIAS_GATE_RESID, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_F32, ConvArgs, GemmArgs, check, lib)

Tensor = torch.Tensor
_EPI = {"bias": EPI_BIAS, "gelu": EPI_BIAS_GELU, "resid": EPI_BIAS_RESID, "gate_resid": EPI_BIAS_GATE_RESID,
        "f32": EPI_F32}
_ACT = {None: ACT_NONE, "none": ACT_NONE, "silu": ACT_SILU, "gelu": ACT_GELU}


def stream_handle() -> int:
    return _stream()


def _bf16(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{name}: expected bfloat16, got {t.dtype}")
    return t


def _rows(t: Tensor, name: str, dtype=torch.bfloat16) -> Tensor:
    """2-D view with unit inner stride."""
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D tensor with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


def _timestep(t: Tensor):
    if t.dtype == torch.int64:
        return t.contiguous(), 1
    return t.to(torch.float32).contiguous(), 0


# --------------------------------------------------------------------------------------
def gemm(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, epilogue: str = "bias",
         resid: Optional[Tensor] = None, gate_mod: Optional[Tensor] = None, gate_e0: Optional[Tensor] = None,
         rows_per_group: int = 1, out: Optional[Tensor] = None, structure: str = "auto") -> Tensor:
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias).  gate_e0: [groups, N] view (row stride free).
    `structure` ("auto" | "t128" | "pp256" | "pp224" | "pp192" | "pp128") forces a tiling (tests / A-B timing)."""
    a, w = _rows(a, "a"), _rows(w, "w")
    epi, st = _EPI[epilogue], _lib.GEMM_STRUCTURES[structure]
    if out is None:
        return torch.ops.sf_hip.gemm(a, w, bias, epi, resid, gate_mod, gate_e0, rows_per_group, st)
    torch.ops.sf_hip.gemm_out(out, a, w, bias, epi, resid, gate_mod, gate_e0, rows_per_group, st)
    return out


def small_linear(x: Tensor, w: Tensor, bias: Optional[Tensor], act_in=None, act_out=None) -> Tensor:
    x, w = _rows(x, "x").contiguous(), _rows(w, "w").contiguous()
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    check(lib().sf_small_linear(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), M, N, K,
                                _ACT[act_in], _ACT[act_out], _stream(x)), "sf_small_linear")
    return out


def quantize_fp8(x: Tensor, rows_per_segment: Optional[int] = None):
    """x [M, K] bf16 -> (e4m3fn [M, K], fp32 scales [segments]): one dynamic scale per `rows_per_segment` rows (default:
    all of them), fp8.py's recipe on the device."""
    x = _rows(x, "x")
    return torch.ops.sf_hip.quantize_fp8(x, rows_per_segment or x.shape[0])


def gemm_fp8(a: Tensor, a_scale: Tensor, w: Tensor, w_scale: Tensor, bias: Optional[Tensor] = None, epilogue: str = "bias",
             resid: Optional[Tensor] = None, gate_mod: Optional[Tensor] = None, gate_e0: Optional[Tensor] = None,
             rows_per_group: int = 1, rows_per_segment: Optional[int] = None, structure: str = "auto") -> Tensor:
    """out[M,N] = epi((a @ w^T) * (a_scale[m // rows_per_segment] * w_scale[n]) + bias) on e4m3fn operands; w_scale is
    fp32 [N] (a scalar tensor is expanded)."""
    a, w = _rows(a, "a", torch.float8_e4m3fn), _rows(w, "w", torch.float8_e4m3fn)
    if w_scale.numel() == 1:
        w_scale = w_scale.reshape(1).expand(w.shape[0])
    return torch.ops.sf_hip.gemm_fp8(a, a_scale.float().contiguous(), rows_per_segment or a.shape[0], w, w_scale.float().contiguous(), bias,
                                     _EPI[epilogue], resid, gate_mod, gate_e0, rows_per_group, _lib.GEMM_STRUCTURES[structure])


def small_linear_fp8(x: Tensor, w_q: Tensor, w_scale: Tensor, bias: Optional[Tensor], act_in=None, act_out=None,
                     rows_per_segment: Optional[int] = None) -> Tensor:
    """small_linear on e4m3fn weights [N, K] with fp32 column scales [N]; the activation is quantised in the kernel,
    one scale per `rows_per_segment` rows (default: all)."""
    x, w_q = _rows(x, "x").contiguous(), _rows(w_q, "w_q", torch.float8_e4m3fn).contiguous()
    M, K = x.shape
    N = w_q.shape[0]
    w_scale = (w_scale.reshape(1).expand(N) if w_scale.numel() == 1 else w_scale).float().contiguous()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    check(lib().sf_small_linear_fp8(x.data_ptr(), w_q.data_ptr(), w_scale.data_ptr(), _ptr(bias), out.data_ptr(), M, N, K,
                                    rows_per_segment or M, _ACT[act_in], _ACT[act_out], _stream(x)), "sf_small_linear_fp8")
    return out


def sinusoid_embedding(t: Tensor, dim: int) -> Tensor:
    tt, is64 = _timestep(t.flatten())
    out = torch.empty(tt.numel(), dim, dtype=torch.bfloat16, device=t.device)
    check(lib().sf_sinusoid_embedding(tt.data_ptr(), is64, out.data_ptr(), tt.numel(), dim, _stream(t)),
          "sf_sinusoid_embedding")
    return out


def layernorm_modulate(x: Tensor, mod_shift: Tensor, mod_scale: Tensor, e0_shift: Tensor, e0_scale: Tensor,
                       rows_per_group: int, eps: float = 1e-6) -> Tensor:
    """x [M,C]; mod_* [C]; e0_* [groups, C] views sharing one row stride."""
    x = _rows(x, "x").contiguous()
    M, Cc = x.shape
    _rows(e0_shift, "e0_shift"), _rows(e0_scale, "e0_scale")
    if e0_shift.stride(0) != e0_scale.stride(0):
        raise ValueError("layernorm_modulate: e0_shift / e0_scale must share a row stride")
    out = torch.empty_like(x)
    check(lib().sf_layernorm_modulate(x.data_ptr(), out.data_ptr(), M, Cc, eps, mod_shift.data_ptr(), mod_scale.data_ptr(),
                                      e0_shift.data_ptr(), e0_scale.data_ptr(), e0_shift.stride(0), rows_per_group,
                                      _stream(x)), "sf_layernorm_modulate")
    return out


def layernorm_affine(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-6) -> Tensor:
    x = _rows(x, "x").contiguous()
    out = torch.empty_like(x)
    check(lib().sf_layernorm_affine(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                    eps, _stream(x)), "sf_layernorm_affine")
    return out


def rmsnorm(x: Tensor, weight: Tensor, eps: float = 1e-6, out: Optional[Tensor] = None) -> Tensor:
    x = _rows(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().sf_rmsnorm(x.data_ptr(), x.stride(0), weight.data_ptr(), out.data_ptr(), out.stride(0), x.shape[0], x.shape[1],
                           eps, _stream(x)), "sf_rmsnorm")
    return out


def qkv_norm_rope_cache(qkv: Tensor, norm_q_w: Tensor, norm_k_w: Tensor, k_cache: Tensor, v_cache: Tensor,
                        rope_cos: Tensor, rope_sin: Tensor, grid, write_start: int, start_frame: int,
                        eps: float = 1e-6) -> Tensor:
    """qkv [B*L, 3C]; caches [B, S, H, D]; returns roped q [B*L, C]; writes K/V rows in place."""
    qkv = _rows(qkv, "qkv").contiguous()
    B, S, H, D = k_cache.shape
    f, h, w = grid
    Cc = H * D
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("qkv_norm_rope_cache: caches must be contiguous [B, S, H, D]")
    q = torch.empty(qkv.shape[0], Cc, dtype=torch.bfloat16, device=qkv.device)
    check(lib().sf_qkv_norm_rope_cache(qkv.data_ptr(), norm_q_w.data_ptr(), norm_k_w.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                                       v_cache.data_ptr(), rope_cos.data_ptr(), rope_sin.data_ptr(), B, f, h, w, Cc, H, S,
                                       write_start, start_frame, eps, _stream(qkv)), "sf_qkv_norm_rope_cache")
    return q


def kv_evict(cache: Tensor, sink: int, evict: int, keep: int, scratch: Tensor) -> None:
    B, S, H, D = cache.shape
    check(lib().sf_kv_evict(cache.data_ptr(), B, S, H * D, sink, evict, keep, scratch.data_ptr(),
                            scratch.numel() * scratch.element_size(), _stream(cache)), "sf_kv_evict")


def kv_rope_shift(k_cache: Tensor, rope_cos: Tensor, rope_sin: Tensor, delta_frames: int, row0: int = 0,
                  rows: Optional[int] = None) -> Tensor:
    """Re-base the temporal RoPE of cached keys [B, S, H, 128] in place: rows [row0, row0 + rows) (default: to the end) of
    every sample are rotated back by `delta_frames` (1..1023).  Returns `k_cache`."""
    torch.ops.sf_hip.kv_rope_shift(k_cache, rope_cos, rope_sin, delta_frames, row0, k_cache.shape[1] - row0 if rows is None else rows)
    return k_cache


def attention(q: Tensor, k: Tensor, v: Tensor, structure: str = "auto", keys: Optional[Tensor] = None,
              log2w: Optional[Tensor] = None) -> Tensor:
    """q [B,Lq,H,128], k/v [B,Lk,H,128] (token/batch strides free, [H,D] contiguous) -> [B,Lq,H,128].
    `structure` ("auto" | "r64" | "w8" | "w4") forces a kernel structure (tests / A-B timing).
    `keys` int32 [B] / `log2w` float32 [B] (both or neither): sample b attends its first keys[b] rows only and the last
    of them weighs 2^log2w[b] rows -- a slab whose trailing rows are identical, folded (`cross_fold_scan`)."""
    return torch.ops.sf_hip.attention(q, k, v, _lib.ATTN_STRUCTURES[structure], keys, log2w)


def attention_accum(q: Tensor, k: Tensor, v: Tensor, out: Tensor, structure: str = "auto") -> Tensor:
    """out += attention(q, k, v), in place: the sum is taken in fp32 in the kernel's epilogue and rounded to bf16 once
    (sf_attention_args.accumulate; the i2v cross-attention's image keys added into the text attention's result).  `structure`:
    "auto" | "w8" | "w4" ("r64" raises: the hand-scheduled kernel has no accumulate epilogue).  Returns `out`."""
    torch.ops.sf_hip.attention_accum(q, k, v, out, _lib.ATTN_STRUCTURES[structure])
    return out


def cross_fold_scan(ck_cache, cv_cache) -> tuple:
    """Lists (one entry per layer) of contiguous bf16 [B, Lk, H, 128] K and V slabs -> (keys int32 [L, B], log2w float32
    [L, B]): per layer and sample, `same` = the trailing rows that repeat the last row bit for bit in K and in V;
    keys = Lk - same + 1, log2w = log2(same)."""
    L, B = len(ck_cache), ck_cache[0].shape[0]
    keys = torch.empty(L, B, dtype=torch.int32, device=ck_cache[0].device)
    log2w = torch.empty(L, B, dtype=torch.float32, device=ck_cache[0].device)
    torch.ops.sf_hip.cross_fold_scan(list(ck_cache), list(cv_cache), keys, log2w)
    return keys, log2w


def patchify(x: Tensor) -> Tensor:
    """x [B, F, Cin, H, W] -> [B*F*(H/2)*(W/2), Cin*4]."""
    x = _bf16(x, "x").contiguous()
    B, F, Cin, H, W = x.shape
    out = torch.empty(B * F * (H // 2) * (W // 2), Cin * 4, dtype=torch.bfloat16, device=x.device)
    check(lib().sf_patchify(x.data_ptr(), out.data_ptr(), B, F, Cin, H, W, _stream(x)), "sf_patchify")
    return out


def unpatchify_x0(head_out: Tensor, xt: Tensor, timestep: Tensor, sigmas: Tensor, timesteps: Tensor):
    """head_out [B*F*h*w, 4*Cout]; xt [B,F,Cout,H,W]; timestep [B, G] -> (flow, x0) [B,F,Cout,H,W]."""
    xt = _bf16(xt, "xt").contiguous()
    B, F, Cout, H, W = xt.shape
    tt, is64 = _timestep(timestep)
    G = tt.shape[1]
    flow = torch.empty_like(xt)
    x0 = torch.empty_like(xt)
    check(lib().sf_unpatchify_x0(_rows(head_out, "head_out").contiguous().data_ptr(), xt.data_ptr(), tt.data_ptr(), is64,
                                 sigmas.data_ptr(), timesteps.data_ptr(), sigmas.numel(), flow.data_ptr(), x0.data_ptr(),
                                 B, F, G, Cout, H, W, _stream(xt)), "sf_unpatchify_x0")
    return flow, x0


def add_noise(x0: Tensor, eps: Tensor, timestep: Tensor, sigmas: Tensor, timesteps: Tensor) -> Tensor:
    """(1 - sigma_t) x0 + sigma_t eps; x0/eps [N, ...], timestep [N]."""
    x0 = _bf16(x0, "x0").contiguous()
    eps = _bf16(eps, "eps").contiguous()
    tt, _ = _timestep(timestep.flatten())
    if tt.numel() != x0.shape[0]:
        raise ValueError(f"add_noise: {x0.shape[0]} samples but {tt.numel()} timesteps")
    return torch.ops.sf_hip.add_noise(x0, eps, tt, sigmas, timesteps)


LINCOMB_MAX = 6


def lincomb(tensors, coefs, out: Optional[Tensor] = None) -> Tensor:
    """out = sum_k coefs[k] * tensors[k]: bf16 tensors of one shape, fp32 accumulation, one final rounding (`out` may be
    one of the inputs).  The tensor arithmetic of the UniPC sampler and of the guidance blend (sf_lincomb_bf16)."""
    if not 1 <= len(tensors) <= LINCOMB_MAX or len(tensors) != len(coefs):
        raise ValueError(f"lincomb: 1..{LINCOMB_MAX} tensors with one coefficient each, got {len(tensors)} / {len(coefs)}")
    xs = [_bf16(t, f"tensors[{i}]").contiguous() for i, t in enumerate(tensors)]
    cf = [float(c) for c in coefs]
    if out is None:
        return torch.ops.sf_hip.lincomb(xs, cf)
    torch.ops.sf_hip.lincomb_out(out, xs, cf)
    return out


# ------------------------------------------------------------------------------------------
# VAE decode kernels (channels-last bf16 volumes)
def conv_igemm(x: Tensor, w_packed: Tensor, bias: Tensor, kernel, t_out: int, upsample: bool = False,
               t_in_offset: int = 0, resid: Optional[Tensor] = None, interleave: bool = False,
               clamp_f32: bool = False, cin: Optional[int] = None, structure: str = "auto", stride=(1, 1)) -> Tensor:
    """Implicit-GEMM convolution (sf_conv_igemm).  x [Tin, Hin, Win, Cin] channels-last with the history
    frames in front; w_packed from `vae.repack_conv`; kernel = (kt, kh, kw).  Returns [Tout, H, W, Cout]
    bf16 -- [2 Tout, H, W, Cout/2] with `interleave` -- or float32 [Tout, Cout, H, W] with `clamp_f32`.
    stride = (temporal, spatial), each 1 or 2: the encoder's downsampling gathers (spatial 2: ZeroPad2d((0,1,0,1)) +
    3x3 stride 2, H = Hin // 2; temporal 2: output frame t reads 2t + dt + t_in_offset)."""
    _bf16(x, "x"), _bf16(w_packed, "w_packed"), _bf16(bias, "bias")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("conv_igemm: x must be a contiguous [T, H, W, C] volume")
    tin, hin, win, c = x.shape
    kt, kh, kw = kernel
    cout = w_packed.shape[0]
    st, sh = stride
    H, W = (2 * hin, 2 * win) if upsample else (hin // 2, win // 2) if sh == 2 else (hin, win)
    if st * (t_out - 1) + kt + t_in_offset > tin:
        raise ValueError(f"conv_igemm: {tin} input frames do not cover {t_out} output frames (kt={kt}, offset={t_in_offset})")
    a = ConvArgs()
    a.x, a.w, a.bias = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr()
    a.Tout, a.H, a.W, a.Hin, a.Win = t_out, H, W, hin, win
    a.Cin, a.Cout, a.kt, a.kh, a.kw = cin or c, cout, kt, kh, kw
    a.upsample, a.t_in_offset, a.ldw = int(upsample), t_in_offset, w_packed.stride(0)
    a.structure = _lib.CONV_STRUCTURES[structure]
    a.stride_t, a.stride_hw = st, sh
    if clamp_f32:
        out = torch.empty(t_out, cout, H, W, dtype=torch.float32, device=x.device)
        a.out_f32, a.epilogue = out.data_ptr(), CONV_BIAS_CLAMP_F32
    else:
        co = cout // 2 if interleave else cout
        out = torch.empty(2 * t_out if interleave else t_out, H, W, co, dtype=torch.bfloat16, device=x.device)
        a.out, a.ldo, a.epilogue = out.data_ptr(), co, CONV_BIAS
        a.interleave_c = co if interleave else 0
        if resid is not None:
            _bf16(resid, "resid")
            if tuple(resid.shape) != tuple(out.shape) or not resid.is_contiguous():
                raise ValueError("conv_igemm: resid must match the output volume")
            a.resid, a.ldr, a.epilogue = resid.data_ptr(), cout, CONV_BIAS_RESID
    check(lib().sf_conv_igemm(a, _stream(x)), "sf_conv_igemm")
    return out


def taehv_conv(x: Tensor, w_packed: Tensor, bias: Optional[Tensor], kt: int, t_out: int, epilogue: str = "bias_relu", upsample: bool = False,
               resid: Optional[Tensor] = None, tgrow: int = 1, clamp: bool = False, cin: Optional[int] = None) -> Tensor:
    """The TAEHV decoder's 3x3 convolution (sf_taehv_conv).  x [t_out - 1 + kt, Hin, Win, Cin] channels-last (kt = 2: the
    history frame in front); w_packed from `taehv_weights.repack_taehv_conv`; epilogue one of `_lib.TAEHV_EPILOGUES`.
    Returns bf16 [tgrow * t_out, H, W, Cout / tgrow], or float32 [t_out, Cout, H, W] = 2 y - 1 for "head_f32" (y for the
    encoder's "latent_f32")."""
    _bf16(x, "x"), _bf16(w_packed, "w_packed")
    if bias is not None:
        _bf16(bias, "bias")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("taehv_conv: x must be a contiguous [T, H, W, C] volume")
    if epilogue not in _lib.TAEHV_EPILOGUES:
        raise ValueError(f"taehv_conv: unknown epilogue {epilogue!r}")
    tin, hin, win, c = x.shape
    if t_out - 1 + kt > tin:
        raise ValueError(f"taehv_conv: {tin} input frames do not cover {t_out} output frames (kt={kt})")
    cout = w_packed.shape[0]
    H, W = (2 * hin, 2 * win) if upsample else (hin, win)
    a = _lib.TaehvConvArgs()
    a.x, a.w, a.bias = x.data_ptr(), w_packed.data_ptr(), None if bias is None else bias.data_ptr()
    a.Tout, a.H, a.W, a.Cin, a.Cout, a.kt = t_out, H, W, cin or c, cout, kt
    a.upsample, a.ldw, a.tgrow, a.epilogue, a.clamp = int(upsample), w_packed.stride(0), tgrow, _lib.TAEHV_EPILOGUES[epilogue], int(clamp)
    if epilogue in ("head_f32", "latent_f32"):
        out = torch.empty(t_out, cout, H, W, dtype=torch.float32, device=x.device)
        a.out_f32 = out.data_ptr()
    else:
        if tgrow < 1 or cout % tgrow:
            raise ValueError(f"taehv_conv: tgrow={tgrow} does not divide Cout={cout}")
        co = cout // tgrow
        out = torch.empty(tgrow * t_out, H, W, co, dtype=torch.bfloat16, device=x.device)
        a.out, a.ldo = out.data_ptr(), co
        if resid is not None:
            _bf16(resid, "resid")
            if tuple(resid.shape) != tuple(out.shape) or not resid.is_contiguous():
                raise ValueError("taehv_conv: resid must match the output volume")
            a.resid, a.ldr = resid.data_ptr(), cout
    check(lib().sf_taehv_conv(a, _stream(x)), "sf_taehv_conv")
    return out


def taehv_encode_stem(pixels: Tensor, w_packed: Tensor, bias: Tensor, lead: int = 0) -> Tensor:
    """The TAEHV encoder's first convolution + ReLU straight from pixels (sf_taehv_encode_stem).  pixels [3, T, H, W] in
    [-1, 1], bf16 or float32, any channel stride with contiguous frames; w_packed from `taehv_weights.repack_stem`.
    Returns bf16 [lead + T, H, W, 64]: the first frame `lead` more times in front."""
    _bf16(w_packed, "w_packed"), _bf16(bias, "bias")
    if not pixels.is_cuda or pixels.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("taehv_encode_stem: pixels must be a CUDA/ROCm bf16 or float32 tensor (the HIP path has no CPU fallback)")
    if pixels.dim() != 4 or pixels.shape[0] != 3 or not pixels[0].is_contiguous():
        raise ValueError(f"taehv_encode_stem: pixels must be [3, T, H, W] with contiguous frames, got {tuple(pixels.shape)}")
    if tuple(w_packed.shape) != (64, 32) or not w_packed.is_contiguous() or bias.numel() != 64:
        raise ValueError("taehv_encode_stem: w_packed [64, 32] and bias [64] expected")
    _, T, H, W = pixels.shape
    out = torch.empty(lead + T, H, W, 64, dtype=torch.bfloat16, device=pixels.device)
    check(lib().sf_taehv_encode_stem(pixels.data_ptr(), _lib.TAEHV_PIXEL_DTYPES[_dtype_name(pixels)], pixels.stride(0), H, W,
                                     lead + T, lead, w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), _stream(pixels)), "sf_taehv_encode_stem")
    return out


def taehv_down_conv(x: Tensor, w_packed: Tensor, kt: int) -> Tensor:
    """The TAEHV encoder's strided convolution with TPool folded in (sf_taehv_down_conv): x [kt * t_out, 2H, 2W, Cin]
    channels-last, kt temporal taps at temporal stride kt, spatial stride 2; w_packed from
    `taehv_weights.repack_taehv_conv(tpool_taps(fold_tpool(...)))`.  Returns bf16 [t_out, H, W, Cout]."""
    _bf16(x, "x"), _bf16(w_packed, "w_packed")
    if x.dim() != 4 or not x.is_contiguous() or x.shape[1] % 2 or x.shape[2] % 2 or kt not in (1, 2) or x.shape[0] % kt:
        raise ValueError(f"taehv_down_conv: x must be a contiguous [kt * T, 2H, 2W, C] volume, got {tuple(x.shape)} with kt={kt}")
    tin, hin, win, c = x.shape
    cout = w_packed.shape[0]
    out = torch.empty(tin // kt, hin // 2, win // 2, cout, dtype=torch.bfloat16, device=x.device)
    a = _lib.TaehvDownConvArgs()
    a.x, a.w, a.out = x.data_ptr(), w_packed.data_ptr(), out.data_ptr()
    a.Tout, a.H, a.W, a.Cin, a.Cout, a.kt, a.ldw, a.ldo = tin // kt, hin // 2, win // 2, c, cout, kt, w_packed.stride(0), cout
    check(lib().sf_taehv_down_conv(a, _stream(x)), "sf_taehv_down_conv")
    return out


def pose_prepare(src: Tensor, lead: int = 3, hwc: bool = False) -> Tensor:
    """The pose input transform (sf_pose_prepare).  src: pose frames [3, F, H, W] holding 0..255 as uint8 / float32 /
    bfloat16, or with `hwc` one image [H, W, 3].  Returns bf16 [lead + F, H, W, 8]: the first frame `lead` more times in
    front, value / 255, channels 3..7 zero."""
    if not src.is_cuda:
        raise ValueError("pose_prepare: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    name = _dtype_name(src)
    if name not in _lib.POSE_DTYPES:
        raise ValueError(f"pose_prepare: pose data must be uint8, float32 or bfloat16, got {src.dtype}")
    if hwc:
        if src.dim() != 3 or src.shape[2] != 3:
            raise ValueError(f"pose_prepare: expected an image [H, W, 3], got {tuple(src.shape)}")
        F, (H, W) = 1, src.shape[:2]
    else:
        if src.dim() != 4 or src.shape[0] != 3:
            raise ValueError(f"pose_prepare: expected pose frames [3, F, H, W], got {tuple(src.shape)}")
        F, H, W = src.shape[1:]
    src = src.contiguous()
    out = torch.empty(lead + F, H, W, 8, dtype=torch.bfloat16, device=src.device)
    check(lib().sf_pose_prepare(src.data_ptr(), _lib.POSE_DTYPES[name], int(hwc), F, H, W, lead, out.data_ptr(), _stream(src)), "sf_pose_prepare")
    return out


def pose_conv(x: Tensor, w_packed: Tensor, bias: Tensor, cout: int, kt: int = 3, stride_t: int = 1, stride_s: int = 1, silu: bool = True) -> Tensor:
    """One convolution of the pose stacks (sf_pose_conv).  x [T, H, W, Cin] channels-last bf16 with Cin 8 or 16; w_packed /
    bias from `pose_weights.repack_pose_conv` / `pad_pose_bias` (bf16 / float32).  Returns bf16 [Tout, Hout, Wout, cout]."""
    _bf16(x, "x"), _bf16(w_packed, "w_packed")
    if not bias.is_cuda or bias.dtype != torch.float32 or bias.numel() != w_packed.shape[0]:
        raise ValueError("pose_conv: bias must be a CUDA float32 tensor padded like the weight rows")
    if x.dim() != 4 or not x.is_contiguous() or not w_packed.is_contiguous():
        raise ValueError("pose_conv: x must be a contiguous [T, H, W, C] volume")
    T, H, W, c = x.shape
    size = lib().sf_pose_out_size
    To = size(T, 3, stride_t) if kt == 3 else T
    out = torch.empty(To, size(H, 3, stride_s), size(W, 3, stride_s), cout, dtype=torch.bfloat16, device=x.device)
    a = _lib.PoseConvArgs()
    a.x, a.w, a.bias, a.out = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr()
    a.T, a.H, a.W, a.Cin, a.Cout, a.kt, a.stride_t, a.stride_s = T, H, W, c, cout, kt, stride_t, stride_s
    a.ldw, a.ldo, a.silu = w_packed.stride(0), cout, int(silu)
    check(lib().sf_pose_conv(a, _stream(x)), "sf_pose_conv")
    return out


def pose_conv_window(x: Tensor, w_packed: Tensor, bias: Tensor, cout: int, x_t0: int, t_end: int, closed: bool, t_out0: int, n_out: int,
                     stride_t: int = 1, stride_s: int = 1, silu: bool = True) -> Tensor:
    """A 3x3x3 convolution of the dwpose stack over a temporal window (sf_pose_conv_window).  x [T, H, W, Cin] holds the
    clip-timeline frames [x_t0, x_t0 + T) of a timeline valid on [0, t_end) (`closed`: zero padding behind it).  Returns
    output frames [t_out0, t_out0 + n_out) as bf16 [n_out, Hout, Wout, cout]: the bits `pose_conv` gives for them on
    the whole clip."""
    _bf16(x, "x"), _bf16(w_packed, "w_packed")
    if not bias.is_cuda or bias.dtype != torch.float32 or bias.numel() != w_packed.shape[0]:
        raise ValueError("pose_conv_window: bias must be a CUDA float32 tensor padded like the weight rows")
    if x.dim() != 4 or not x.is_contiguous() or not w_packed.is_contiguous():
        raise ValueError("pose_conv_window: x must be a contiguous [T, H, W, C] volume")
    T, H, W, c = x.shape
    size = lib().sf_pose_out_size
    out = torch.empty(max(n_out, 0), size(H, 3, stride_s), size(W, 3, stride_s), cout, dtype=torch.bfloat16, device=x.device)
    a = _lib.PoseConvArgs()
    a.x, a.w, a.bias, a.out = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr()
    a.T, a.H, a.W, a.Cin, a.Cout, a.kt, a.stride_t, a.stride_s = T, H, W, c, cout, 3, stride_t, stride_s
    a.ldw, a.ldo, a.silu = w_packed.stride(0), cout, int(silu)
    win = _lib.PoseWindow(x_t0, t_end, int(closed), t_out0, n_out)
    check(lib().sf_pose_conv_window(a, win, _stream(x)), "sf_pose_conv_window")
    return out


def pose_patch_embed(x: Tensor, w_packed: Tensor, bias: Tensor) -> Tensor:
    """The dwpose stack's last layer (sf_pose_patch_embed).  x [T, H, W, 16] channels-last; w_packed [N, 64] from
    `pose_weights.repack_pose_embed`, bias [N], both bf16.  Returns the tokens bf16 [T * (H//2) * (W//2), N]."""
    _bf16(x, "x"), _bf16(w_packed, "w_packed"), _bf16(bias, "bias")
    if x.dim() != 4 or x.shape[3] != 16 or not x.is_contiguous() or not w_packed.is_contiguous() or w_packed.shape[1] != 64:
        raise ValueError("pose_patch_embed: contiguous x [T, H, W, 16] and w_packed [N, 64] expected")
    T, H, W, _ = x.shape
    n = T * (H // 2) * (W // 2)
    rows = torch.empty(n, 64, dtype=torch.bfloat16, device=x.device)
    out = torch.empty(n, w_packed.shape[0], dtype=torch.bfloat16, device=x.device)
    check(lib().sf_pose_patch_embed(x.data_ptr(), T, H, W, w_packed.data_ptr(), bias.data_ptr(), w_packed.shape[0], rows.data_ptr(), out.data_ptr(),
                                    _stream(x)), "sf_pose_patch_embed")
    return out


def rmsnorm_silu_cl(x: Tensor, gamma: Tensor, silu: bool = True) -> Tensor:
    """VAE RMS_norm over the last (channel) dim of a contiguous channels-last tensor, optional SiLU."""
    _bf16(x, "x"), _bf16(gamma, "gamma")
    if not x.is_contiguous():
        raise ValueError("rmsnorm_silu_cl: x must be contiguous")
    out = torch.empty_like(x)
    c = x.shape[-1]
    check(lib().sf_rmsnorm_silu_cl(x.data_ptr(), gamma.data_ptr(), out.data_ptr(), x.numel() // c, c, int(silu), _stream(x)),
          "sf_rmsnorm_silu_cl")
    return out


def softmax_rows(s: Tensor, scale: float, cols_padded: Optional[int] = None) -> Tensor:
    """bf16 softmax(scale * s) over the rows of a float32 matrix; columns up to cols_padded are zero."""
    if s.dtype != torch.float32 or s.dim() != 2 or s.stride(1) != 1 or not s.is_cuda:
        raise ValueError("softmax_rows: expected a CUDA float32 matrix with contiguous rows")
    rows, cols = s.shape
    cp = cols_padded or cols
    out = torch.empty(rows, cp, dtype=torch.bfloat16, device=s.device)
    check(lib().sf_softmax_rows(s.data_ptr(), s.stride(0), out.data_ptr(), cp, rows, cols, cp, float(scale), _stream(s)),
          "sf_softmax_rows")
    return out


# ------------------------------------------------------------------------------------------
# measured ceilings of the box (bench.py: roofline.measured_peak / hbm_measured_peak)
def probe_mfma(operands: Tensor, sink: Tensor, shape: str = "32x32x16", iters: int = 2000, workgroups: int = 256) -> float:
    """Launches the register-only bf16 MFMA loop (sf_probe_mfma) on the current stream; returns the launch's FLOPs.
    operands: >= 4096 bf16 (random); sink: >= workgroups * 256 float32."""
    _bf16(operands, "operands")
    if operands.numel() < 4096 or sink.dtype != torch.float32 or sink.numel() < workgroups * 256 or not sink.is_cuda:
        raise ValueError("probe_mfma: operands >= 4096 bf16 and a CUDA float32 sink of workgroups * 256 elements expected")
    fl = C.c_double(0.0)
    check(lib().sf_probe_mfma({"32x32x16": 0, "16x16x32": 1}[shape], iters, workgroups, operands.data_ptr(), sink.data_ptr(),
                              C.byref(fl), _stream(operands)), "sf_probe_mfma")
    return fl.value


def probe_copy(src: Tensor, dst: Tensor) -> int:
    """Streaming copy src -> dst (sf_probe_copy) on the current stream; returns the bytes READ (as many are written)."""
    if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("probe_copy: contiguous CUDA tensors expected")
    nbytes = src.numel() * src.element_size()
    if nbytes != dst.numel() * dst.element_size() or nbytes % 16:
        raise ValueError("probe_copy: src and dst must hold the same number of bytes, a multiple of 16")
    check(lib().sf_probe_copy(src.data_ptr(), dst.data_ptr(), nbytes, _stream(src)), "sf_probe_copy")
    return nbytes


# -------------------------------------------------------------------------------------- JPEG encoder (csrc/jpeg.hip)
def jpeg_workspace_bytes(n: int, h: int, w: int, subsampling: str, restart_interval: int) -> int:
    """Bytes of workspace (and of a worst-case output buffer) for n frames of h x w (sf_jpeg_workspace_bytes)."""
    need = lib().sf_jpeg_workspace_bytes(n, h, w, _lib.JPEG_SUBSAMPLINGS[subsampling], restart_interval)
    if need == 0:
        check(-1, "sf_jpeg_workspace_bytes")
    return need


def jpeg_transform(frames: Tensor, coef: Tensor, n: int, h: int, w: int, subsampling: str, quality: int, value_range=(-1, 1)) -> Tensor:
    """frames (contiguous float32 / bfloat16 [n, 3, h, w] or uint8 [n, h, w, 3]) -> coef int16 [n, blocks, 64] (sf_jpeg_transform)."""
    dtype = _lib.JPEG_DTYPES[_dtype_name(frames)]
    check(lib().sf_jpeg_transform(frames.data_ptr(), dtype, _lib.JPEG_RANGES[tuple(value_range)], n, h, w, _lib.JPEG_SUBSAMPLINGS[subsampling],
                                  quality, coef.data_ptr(), _stream(frames)), "sf_jpeg_transform")
    return coef


def jpeg_entropy(coef: Tensor, n: int, h: int, w: int, subsampling: str, quality: int, restart_interval: int, workspace: Tensor, out: Tensor,
                 meta: Tensor) -> None:
    """coef -> n files back to back in `out` (uint8); meta int64 [n + 2] receives offsets[n + 1], then the status word
    (sf_jpeg_entropy)."""
    check(lib().sf_jpeg_entropy(coef.data_ptr(), n, h, w, _lib.JPEG_SUBSAMPLINGS[subsampling], quality, restart_interval, workspace.data_ptr(),
                                workspace.numel(), out.data_ptr(), out.numel(), meta.data_ptr(), meta[n + 1:].data_ptr(),
                                _stream(coef)), "sf_jpeg_entropy")


def jpeg_encode_frames(frames: Tensor, n: int, h: int, w: int, subsampling: str, quality: int, restart_interval: int, value_range, workspace: Tensor,
                       out: Tensor, meta: Tensor) -> None:
    """Both steps in one host call (sf_jpeg_encode_frames); arguments as `jpeg_transform` / `jpeg_entropy`."""
    dtype = _lib.JPEG_DTYPES[_dtype_name(frames)]
    check(lib().sf_jpeg_encode_frames(frames.data_ptr(), dtype, _lib.JPEG_RANGES[tuple(value_range)], n, h, w, _lib.JPEG_SUBSAMPLINGS[subsampling],
                                      quality, restart_interval, workspace.data_ptr(), workspace.numel(), out.data_ptr(), out.numel(), meta.data_ptr(),
                                      meta[n + 1:].data_ptr(), _stream(frames)), "sf_jpeg_encode_frames")


# -------------------------------------------------------------------------------------- JPEG decoder (csrc/jpeg_decode.hip)
_IDCT_TABLE = None


def _idct_table():
    """jpeg_reference.IDCT_INT as the host int32 [64] the C side takes: the kernels and their definition share it."""
    global _IDCT_TABLE
    if _IDCT_TABLE is None:
        from . import jpeg_reference as jr
        _IDCT_TABLE = (C.c_int32 * 64)(*[int(v) for v in jr.IDCT_INT.reshape(-1)])
    return _IDCT_TABLE


def jpeg_decode_workspace_bytes(n: int, h: int, w: int, sampling: str, max_intervals: int) -> int:
    """Bytes of workspace for n files of h x w (sf_jpeg_decode_workspace_bytes)."""
    need = lib().sf_jpeg_decode_workspace_bytes(n, h, w, _lib.JPEG_DECODE_SAMPLINGS[sampling], max_intervals)
    if need == 0:
        check(-1, "sf_jpeg_decode_workspace_bytes")
    return need


def jpeg_decode_entropy(upload: Tensor, upload_bytes: int, n: int, h: int, w: int, sampling: str, max_intervals: int, workspace: Tensor, coef: Tensor,
                        status: Tensor) -> Tensor:
    """upload (uint8: the table block, then the scans) -> coef int16 [n, blocks, 64]; status int32 [n] (sf_jpeg_decode_entropy)."""
    check(lib().sf_jpeg_decode_entropy(upload.data_ptr(), upload_bytes, n, h, w, _lib.JPEG_DECODE_SAMPLINGS[sampling], max_intervals, workspace.data_ptr(),
                                       workspace.numel(), coef.data_ptr(), status.data_ptr(), _stream(upload)), "sf_jpeg_decode_entropy")
    return coef


def jpeg_decode_pixels(coef: Tensor, upload: Tensor, upload_bytes: int, n: int, h: int, w: int, sampling: str, workspace: Tensor, out: Tensor,
                       layout: str) -> Tensor:
    """coef -> out (uint8 / float32 / bfloat16, already shaped for `layout`) (sf_jpeg_decode_pixels)."""
    dtype = _lib.JPEG_DTYPES[_dtype_name(out)]
    check(lib().sf_jpeg_decode_pixels(coef.data_ptr(), upload.data_ptr(), upload_bytes, _idct_table(), n, h, w, _lib.JPEG_DECODE_SAMPLINGS[sampling],
                                      workspace.data_ptr(), workspace.numel(), out.data_ptr(), _lib.JPEG_LAYOUTS[layout], dtype, _stream(upload)),
          "sf_jpeg_decode_pixels")
    return out


def jpeg_decode_frames(upload: Tensor, upload_bytes: int, n: int, h: int, w: int, sampling: str, max_intervals: int, workspace: Tensor, out: Tensor,
                       layout: str, status: Tensor) -> Tensor:
    """Both steps in one host call (sf_jpeg_decode_frames); arguments as `jpeg_decode_entropy` / `jpeg_decode_pixels`."""
    dtype = _lib.JPEG_DTYPES[_dtype_name(out)]
    check(lib().sf_jpeg_decode_frames(upload.data_ptr(), upload_bytes, _idct_table(), n, h, w, _lib.JPEG_DECODE_SAMPLINGS[sampling], max_intervals,
                                      workspace.data_ptr(), workspace.numel(), out.data_ptr(), _lib.JPEG_LAYOUTS[layout], dtype, status.data_ptr(),
                                      _stream(upload)), "sf_jpeg_decode_frames")
    return out


# -------------------------------------------------------------------------------------- frame resizer (csrc/resize.hip)
def resize_kernel_size(in_size: int, out_size: int, filter: str) -> int:
    """Columns of one axis' coefficient table (sf_resize_kernel_size); equals resize_reference.kernel_size."""
    ks = lib().sf_resize_kernel_size(in_size, out_size, _lib.RESIZE_FILTERS[filter])
    if ks == 0:
        check(-1, "sf_resize_kernel_size")
    return ks


def resize_frames(frames: Tensor, tables_h, tables_v, filter: str, layout: str = "hwc", out_layout: str = "hwc", dtype=torch.uint8, crop=None,
                  out: Optional[Tensor] = None) -> Tensor:
    """uint8 frames in `layout` -> resized frames in `out_layout` / `dtype` (torch.ops.sf_hip.resize_frames over sf_resize_frames).
    tables_h / tables_v: (bounds, coefs) device int32 tensors of `resize_reference.coefficients` for the crop's width -> the
    output's and its height -> the output's; crop = (top, left, height, width) or None."""
    crop = None if crop is None else [int(v) for v in crop]
    if out is not None:
        torch.ops.sf_hip.resize_frames_out(out, frames, tables_h[0], tables_h[1], tables_v[0], tables_v[1], filter, layout, out_layout, crop)
        return out
    return torch.ops.sf_hip.resize_frames(frames, tables_h[0], tables_h[1], tables_v[0], tables_v[1], filter, layout, out_layout, dtype, crop)


# -------------------------------------------------------------------------------------- raw YUV frames (csrc/yuv.hip)
def yuv_frame_bytes(fmt: str, h: int, w: int) -> int:
    """Bytes of one h x w frame (sf_yuv_frame_bytes); equals yuv_reference.frame_bytes."""
    if fmt not in _lib.YUV_FORMATS:
        raise ValueError(f"format must be one of {', '.join(_lib.YUV_FORMATS)}, got {fmt!r}")
    need = lib().sf_yuv_frame_bytes(_lib.YUV_FORMATS[fmt], h, w)
    if need == 0:
        check(-1, "sf_yuv_frame_bytes")
    return need


def yuv_decode_frames(raw: Tensor, fmt: str, h: int, w: int, constants, chroma: str = "triangle", layout: str = "hwc", dtype=torch.uint8) -> Tensor:
    """uint8 raw [n, frame_bytes] -> n frames in `layout` / `dtype` (torch.ops.sf_hip.yuv_decode_frames over sf_yuv_decode_frames).
    constants: `yuv_reference.constants(matrix, range)`."""
    return torch.ops.sf_hip.yuv_decode_frames(raw, fmt, h, w, [int(v) for v in constants], chroma, layout, dtype)


def yuv_encode_frames(frames: Tensor, fmt: str, constants, value_range=(-1, 1)) -> Tensor:
    """uint8 [n, h, w, 3] or float32 / bfloat16 [n, 3, h, w] in `value_range` -> uint8 [n, frame_bytes]
    (torch.ops.sf_hip.yuv_encode_frames over sf_yuv_encode_frames)."""
    if tuple(value_range) not in _lib.JPEG_RANGES:
        raise ValueError(f"value_range must be (-1, 1) or (0, 1), got {value_range}")
    return torch.ops.sf_hip.yuv_encode_frames(frames, fmt, [int(v) for v in constants], tuple(value_range) == (0, 1))


# -------------------------------------------------------------------------------------- pose renderer (csrc/pose_render.hip)
def pose_render_frames(keypoints: Tensor, height: int, width: int, layout: str = "pose", dtype=torch.uint8, normalized: bool = True,
                       score_threshold: float = 0.3, out: Optional[Tensor] = None) -> Tensor:
    """float32 keypoints [F, P, 134, 3] on the device -> skeleton frames in `layout` / `dtype`
    (torch.ops.sf_hip.pose_render_frames over sf_pose_render_frames); `out`: the tensor to fill, already shaped."""
    if out is not None:
        torch.ops.sf_hip.pose_render_frames_out(out, keypoints, layout, normalized, score_threshold)
        return out
    return torch.ops.sf_hip.pose_render_frames(keypoints, height, width, layout, dtype, normalized, score_threshold)


# -------------------------------------------------------------------------------------- pose retargeter (csrc/pose_retarget.hip)
def pose_retarget_frames(src: Tensor, first: Tensor, ref: Tensor, src0: int, out0: int, n_out: int, num: int, den: int, src_sx: float,
                         src_sy: float, ref_sx: float, ref_sy: float, score_threshold: float = 0.3, align: bool = True) -> Tensor:
    """Source frames src0 .. of a clip (float32 [n, P, 134, 3] on the device), its frame 0 [P, 134, 3] and the reference
    [Pr, 134, 3] -> output frames out0 .. out0 + n_out - 1, float32 [n_out, P, 134, 3] in output pixels
    (torch.ops.sf_hip.pose_retarget_frames over sf_pose_retarget_frames)."""
    return torch.ops.sf_hip.pose_retarget_frames(src, first, ref, src0, out0, n_out, num, den, src_sx, src_sy, ref_sx, ref_sy, score_threshold, align)


def pose_retarget_plan(frames_before: int, n: int, num: int, den: int) -> Tuple[int, int]:
    """(first_out, n_out) of sf_pose_retarget_plan: the output frames final once n more source frames are in."""
    first, count = C.c_int64(), C.c_int64()
    check(lib().sf_pose_retarget_plan(frames_before, n, num, den, C.byref(first), C.byref(count)), "sf_pose_retarget_plan")
    return first.value, count.value


# -------------------------------------------------------------------------------------- pose smoother (csrc/pose_smooth.hip)
def pose_smooth_frames(src: Tensor, state: Tensor, period: float, min_cutoff: float, beta: float, kd: float, threshold: float = 0.3,
                       max_gap: int = 0) -> Tensor:
    """The frames of one piece of a clip (float32 [n, P, 134, 3] on the device) and the packed filter state int32
    [P, 134, 8] the clip has reached -> the frames smoothed, float32 [n, P, 134, 3]; `state` is advanced in place
    (torch.ops.sf_hip.pose_smooth_frames over sf_pose_smooth_frames)."""
    return torch.ops.sf_hip.pose_smooth_frames(src, state, period, min_cutoff, beta, kd, threshold, max_gap)


def pose_smooth_state_bytes(people: int) -> int:
    """sf_pose_smooth_state_bytes: the bytes of the state of `people` people, 0 out of range."""
    return int(lib().sf_pose_smooth_state_bytes(people))


# -------------------------------------------------------------------------------------- pose tracker (csrc/pose_track.hip)
def pose_track_frames(src: Tensor, state: Tensor, slots: int, gate2: float, threshold: float = 0.3, min_points: int = 4, min_common: int = 3,
                      max_age: int = 2) -> Tuple[Tensor, Tensor]:
    """The detections of one piece of a clip (float32 [n, P, 134, 3] on the device, in any order per frame) and the packed
    tracker state int32 [slots + 1, 40] the clip has reached -> (float32 [n, slots, 134, 3] with each person in one slot,
    int32 [n, slots] track ids); `state` is advanced in place (torch.ops.sf_hip.pose_track_frames over sf_pose_track_frames)."""
    return torch.ops.sf_hip.pose_track_frames(src, state, slots, gate2, threshold, min_points, min_common, max_age)


def pose_track_state_bytes(slots: int) -> int:
    """sf_pose_track_state_bytes: the bytes of the state of `slots` slots, 0 out of range."""
    return int(lib().sf_pose_track_state_bytes(slots))


# -------------------------------------------------------------------------------------- DWPose glue (csrc/pose_estimate.hip)
def decode_boxes(head: Tensor, ratio: float, max_people: int, input_size=(640, 640), strides=(8, 16, 32), class_index: int = 0,
                 score_threshold: float = 0.3, iou_threshold: float = 0.45, decoded: bool = False) -> Tuple[Tensor, Tensor]:
    """A YOLOX head float32 [F, A, 5 + C] on the device -> (boxes float32 [F, P, 5] in source-frame pixels, count int32 [F])
    (torch.ops.sf_hip.pose_boxes_decode over sf_pose_boxes_decode); ratio = the letterbox scale min(in_h / H, in_w / W)."""
    return torch.ops.sf_hip.pose_boxes_decode(head, int(input_size[0]), int(input_size[1]), [int(s) for s in strides], float(ratio), max_people,
                                              class_index, float(score_threshold), float(iou_threshold), decoded)


def pose_boxes_scratch_bytes(frames: int, anchors: int) -> int:
    """sf_pose_boxes_scratch_bytes: the bytes of scratch behind `decode_boxes`, 0 out of range."""
    return int(lib().sf_pose_boxes_scratch_bytes(frames, anchors))


def crop_people(frames: Tensor, boxes: Tensor, count: Tensor, layout: str = "hwc", out_size=(384, 288), padding: float = 1.25,
                mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), channels: str = "rgb", dtype=torch.float32) -> Tensor:
    """uint8 frames in `layout` and their people -> the pose network's input [F * P, 3, out_h, out_w] in `dtype`
    (torch.ops.sf_hip.pose_crop_people over sf_pose_crop_people)."""
    if channels not in ("rgb", "bgr"):
        raise ValueError(f"channels must be 'rgb' or 'bgr', got {channels!r}")
    return torch.ops.sf_hip.pose_crop_people(frames, boxes, count, layout, int(out_size[0]), int(out_size[1]), float(padding), [float(v) for v in mean],
                                             [float(v) for v in std], channels == "bgr", dtype)


def decode_simcc(simcc_x: Tensor, simcc_y: Tensor, boxes: Tensor, count: Tensor, frame_size, out_size=(384, 288), padding: float = 1.25,
                 split_ratio: float = 2.0, normalized: bool = True, neck_threshold: float = 0.3, order=None) -> Tensor:
    """SimCC logits and the people they were cropped for -> keypoints float32 [F, P, 134, 3] in the renderer's layout
    (torch.ops.sf_hip.pose_simcc_decode over sf_pose_simcc_decode); order: `pose_estimate_reference.reorder_table` (a host uint8 tensor or array), DWPose's by default."""
    global _POSE_ORDER
    if order is None:
        if _POSE_ORDER is None:
            from .pose_estimate_reference import reorder_table
            _POSE_ORDER = torch.from_numpy(reorder_table())
        order = _POSE_ORDER
    elif not isinstance(order, Tensor):
        order = torch.as_tensor(order, dtype=torch.uint8)
    return torch.ops.sf_hip.pose_simcc_decode(simcc_x, simcc_y, boxes, count, int(frame_size[0]), int(frame_size[1]), int(out_size[0]), int(out_size[1]),
                                              float(padding), float(split_ratio), normalized, float(neck_threshold), order)


_POSE_ORDER: Optional[Tensor] = None          # the default reorder table, uint8 [134] on the host


# -------------------------------------------------------------------------------------- CLIP image encoder (csrc/clip_encoder.hip)
def clip_preprocess(frames: Tensor, image_size: int = 224, patch: int = 14, kp: Optional[int] = None) -> Tensor:
    """frames [n, 3, H, W] float32 / bfloat16 in [-1, 1] -> bf16 patch rows [n * (image_size/patch)^2, kp] (sf_clip_preprocess)."""
    if not frames.is_cuda or frames.dim() != 4 or frames.shape[1] != 3 or not frames.is_contiguous():
        raise ValueError("clip_preprocess: contiguous CUDA frames [n, 3, H, W] expected")
    kp = (3 * patch * patch + 63) // 64 * 64 if kp is None else kp
    n, _, H, W = frames.shape
    rows = torch.empty(n * (image_size // patch) ** 2, kp, dtype=torch.bfloat16, device=frames.device)
    check(lib().sf_clip_preprocess(frames.data_ptr(), _lib.CLIP_DTYPES[_dtype_name(frames)], n, H, W, image_size, patch, kp,
                                   rows.data_ptr(), _stream(frames)), "sf_clip_preprocess")
    return rows


def clip_embed_norm(patch_out: Tensor, cls: Tensor, pos: Tensor, pre_w: Tensor, pre_b: Tensor, ln_w: Optional[Tensor], ln_b: Optional[Tensor],
                    eps: float = 1e-5):
    """patch_out bf16 [n, P, dim] -> (x32 float32 [n, P + 1, dim], xn bf16 or None) (sf_clip_embed_norm)."""
    n, P, dim = patch_out.shape
    _bf16(patch_out, "patch_out")
    x32 = torch.empty(n, P + 1, dim, dtype=torch.float32, device=patch_out.device)
    xn = torch.empty(n, P + 1, dim, dtype=torch.bfloat16, device=patch_out.device) if ln_w is not None else None
    check(lib().sf_clip_embed_norm(patch_out.data_ptr(), cls.data_ptr(), pos.data_ptr(), pre_w.data_ptr(), pre_b.data_ptr(), _ptr(ln_w), _ptr(ln_b),
                                   x32.data_ptr(), _ptr(xn), n, P, dim, eps, _stream(patch_out)), "sf_clip_embed_norm")
    return x32, xn


def clip_add_layernorm(x32: Tensor, y: Tensor, ln_w: Optional[Tensor] = None, ln_b: Optional[Tensor] = None, xn: Optional[Tensor] = None,
                       eps: float = 1e-5) -> Optional[Tensor]:
    """x32 (float32 [rows, dim], updated in place) += y (bf16); with ln_w returns xn = bf16(LN(x32)) (written into `xn` when
    given); without, only adds (sf_clip_add_layernorm)."""
    _bf16(y, "y")
    if x32.dtype != torch.float32 or not x32.is_cuda or not x32.is_contiguous() or x32.shape != y.shape or x32.dim() != 2:
        raise ValueError("clip_add_layernorm: contiguous CUDA float32 x32 [rows, dim] and bf16 y of the same shape expected")
    if ln_w is not None and xn is None:
        xn = torch.empty_like(y)
    check(lib().sf_clip_add_layernorm(x32.data_ptr(), y.data_ptr(), _ptr(ln_w), _ptr(ln_b), _ptr(xn), x32.shape[0], x32.shape[1], eps, _stream(x32)),
          "sf_clip_add_layernorm")
    return xn if ln_w is not None else None


def clip_attention(qkv: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """qkv bf16 [n, L, 3, H, 80] -> bf16 [n, L, H * 80], non-causal softmax attention at scale 1/sqrt(80) (sf_clip_attention)."""
    _bf16(qkv, "qkv")
    if qkv.dim() != 5 or qkv.shape[2] != 3 or qkv.shape[4] != 80:
        raise ValueError(f"clip_attention: qkv [n, L, 3, H, 80] expected, got {tuple(qkv.shape)}")
    n, L, _, H, _ = qkv.shape
    if out is None:
        out = torch.empty(n, L, H * 80, dtype=torch.bfloat16, device=qkv.device)
    check(lib().sf_clip_attention(qkv.data_ptr(), out.data_ptr(), n, L, H, _stream(qkv)), "sf_clip_attention")
    return out


def clip_gelu(x: Tensor) -> Tensor:
    """nn.GELU() (erf form) of a bf16 tensor, evaluated in fp32 (sf_clip_gelu)."""
    _bf16(x, "x")
    out = torch.empty_like(x)
    check(lib().sf_clip_gelu(x.data_ptr(), out.data_ptr(), x.numel(), _stream(x)), "sf_clip_gelu")
    return out
