"""The FP8 recipe of the opt-in FP8 linear layers (`WanDiffusionWrapper(..., fp8=True)`).

The reference's speed option `quantize_(transformer, Float8DynamicActivationFloat8WeightConfig(granularity=PerTensor()))`
(demo.py:277-283) quantises every nn.Linear of the generator to fp8 with one scale per weight tensor and one dynamic
scale per activation tensor.  torchao is not reproduced bit for bit; this module is the definition the kernels and the
tests share (OCP e4m3fn, round to nearest even):

    s = max(amax(|x|) as fp32, 1e-12) / 448          q = e4m3fn(clamp(x.float() / s, -448, 448))

Weights: one scale per reference Linear, applied once at load.  Activations: one scale per SEGMENT of rows -- the rows
of one generator pass (all samples of the call), torchao's per-tensor scope for the reference's call; computed on the
device by `sf_quantize_fp8` / inside `sf_small_linear_fp8` on every call.  The product is
out = epi(acc * (s_a * s_w[n]) + bias[n]) with acc the fp32 sum of the e4m3 products, rounded to bf16 once.

The functions here run on any device (torch ops); the load path uses them on the GPU, the CPU tests on the host.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

Tensor = torch.Tensor
E4M3_MAX = 448.0
E4M3 = torch.float8_e4m3fn
K_ALIGN = 128   # the fp8 GEMM's k-tile: every quantised Linear's in_features must be a multiple of it


def scale_of(x: Tensor) -> Tensor:
    """fp32 scalar tensor s = max(amax(|x|) as fp32, 1e-12) / 448."""
    return x.detach().abs().amax().float().clamp(min=1e-12) / E4M3_MAX


def quantize(x: Tensor, s: Tensor) -> Tensor:
    """e4m3fn(clamp(x.float() / s, -448, 448)); `s` broadcasts (a scalar or a column of per-row scales)."""
    return (x.float() / s).clamp(-E4M3_MAX, E4M3_MAX).to(E4M3)


def quantize_rows(x: Tensor, rows_per_segment: int) -> Tuple[Tensor, Tensor]:
    """The activation recipe of sf_quantize_fp8: x [M, K] -> (e4m3 [M, K], fp32 scales [ceil(M / rows_per_segment)])."""
    M = x.shape[0]
    scales = torch.stack([scale_of(x[r:r + rows_per_segment]) for r in range(0, M, rows_per_segment)])
    per_row = scales.repeat_interleave(rows_per_segment)[:M, None]
    return quantize(x, per_row), scales


def quantize_weight(parts: Sequence[Tensor]) -> Tuple[Tensor, Tensor]:
    """The weight recipe: reference Linears `parts` ([N_i, K] each, stacked along N as the kernels read them) ->
    (e4m3 [sum N_i, K], fp32 column scales [sum N_i]: the scale of part i repeated N_i times)."""
    qs, cols = [], []
    for w in parts:
        s = scale_of(w)
        qs.append(quantize(w, s))
        cols.append(s.expand(w.shape[0]))
    return torch.cat(qs, 0).contiguous(), torch.cat(cols, 0).contiguous()


def dequantize(q: Tensor, s: Tensor) -> Tensor:
    """fp64 values q * s (s broadcasts)."""
    return q.double() * s.double()


def check_k(name: str, k: int) -> None:
    if k % K_ALIGN:
        raise ValueError(f"fp8=True: {name} has in_features={k}, not a multiple of {K_ALIGN} (the fp8 GEMM's k-tile); "
                         "this shape cannot run in FP8, use fp8=False")
