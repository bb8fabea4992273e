"""References, an fp32 emulation and per-row checkers for the DiT row kernels of csrc/elementwise.hip:
layernorm_modulate, layernorm_affine, rmsnorm, sinusoid_embedding.  Host-only, plain torch.

Three layers, all on the same bf16 inputs:

  ref_*    float64, with the reference's rounding points (wan_oracle.layer_norm / rms_norm / sinusoidal_embedding_1d):
             modulate  add = bf16(mod_shift + e0_shift[g]), scl = bf16(mod_scale + e0_scale[g]), g = row // rows_per_group,
                       y = xn (1 + scl) + add, rounded once;
             affine    y = xn w + b, rounded once;
             rmsnorm   bf16(bf16(x r) w), two roundings;
             sinusoid  float64 cos | sin, rounded as torch's `.to(bfloat16)` does (float64 -> float32 -> bf16).
           The LayerNorm references also return the terms `xn m` and `add` the sum is made of.
  emu_*    what a CORRECT fp32 implementation with the kernels' arithmetic gives: per-lane sequential sums over the
           lane's 8-element chunks, a 64-lane pairwise tree, two-pass LayerNorm statistics (mean, then sum (x - mean)^2),
           rsqrt(sum / C + eps).  It is not the code under test; it shows what the caps below leave as headroom.
  check_*  compare an output with a reference row by row and return a Report: one RowReport per row (row, group, family,
           worst element, mismatches) and the list of violated conditions, each naming kernel, width, row, group, family.

Acceptance conditions (set from the arithmetic and the emulation, never from what the kernels give):

  LayerNorm (both modes)  every element: |out - y64| <= 1 bf16 ulp of max(|y64|, |xn m|, |add|) -- the ulp of the larger
                          operand because xn m + add may cancel; at most 1 % of a launch's elements differ from bf16(y64);
                          constant rows equal `add` bit for bit (every x - mean is exactly 0 there).
  RMSNorm                 every element within 2 bf16 steps of the two-rounding float64 value (a tie flip of the inner
                          rounding moves the product by at most 2 steps); at most 0.1 % of the elements differ at all.
  sinusoid                at most 0.5 % of the elements differ from the reference, each difference exactly 1 bf16 step.

Numeric families (FAMILIES; the rows of a launch cycle through them): N(0, 2); mean 8 std 1; mean 100 std 4; scale 1e-3
(var ~ eps); scale 1e4; one 300.0 in 0.05-scale noise; constant 3.25; and "offset", every element 200 or 201.  The last is
there for the one-pass variance E[x^2] - mean^2: in fp32 that costs 0.51 ulp and 0.5 - 0.7 % of a mean-100 row's roundings,
which the caps above allow, but 2.5 - 5 ulp on an offset row (mean / std = 400), where the two-pass emulation stays at 0.503.

Emulation headroom, as tests/test_row_kernels_host.py measures and prints it (`pytest -s`), one family per launch:

  LayerNorm modulate  C = 512 / 2560 / 5120   worst 0.500 / 0.505 / 0.503 ulp of the larger operand (0.500 is the final rounding);
                                              at most 0.006 / 0.353 / 0.259 % of a launch differ, all of that on offset rows
                                              (the first seven families: at most 0.067 %, on mean-100 rows at C = 5120)
  LayerNorm affine    same widths             worst 0.500 / 0.521 / 0.503 ulp; at most 0.012 / 0.453 / 0.335 % differ
  RMSNorm             C = 512 / 4096 / 5120   worst 0 / 0 / 2 steps; at most 0 / 0 / 0.060 % differ (spike rows at C = 5120:
                                              the lane that holds the 300.0 absorbs its small squares)
  on the mixed launches of tests/test_gpu_row_kernels.py, all eight widths:
  LayerNorm modulate  worst 0.853 ulp (C = 3072: x = 100 in a mean-100 row of mean 99.9993, shift exactly 0), then 0.675 (C = 5120),
                      <= 0.502 elsewhere; at most 0.069 % of a launch differ
  RMSNorm             worst 2 steps (C = 5120 only), at most 0.0035 % of a launch differ
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from oracle import wan_oracle as wo

FAMILIES = ("n02", "mean8", "mean100", "tiny", "huge", "spike", "const", "offset")
WIDTHS = (512, 1024, 1536, 2048, 2560, 3072, 4096, 5120)      # 512 * {1,2,3,4,5,6,8,10}: every instantiated width
LN_ULP_CAP, LN_SHARE_CAP = 1.0, 0.01
RMS_STEP_CAP, RMS_SHARE_CAP = 2, 0.001
SIN_STEP_CAP, SIN_SHARE_CAP = 1, 0.005


# ------------------------------------------------------------------------------------------------ inputs
def family_row(name: str, C: int, g: torch.Generator) -> Tensor:
    """One fp32 row of a numeric family (rounded to bf16 by the caller)."""
    n = torch.randn(C, generator=g)
    if name == "n02":
        return n * 2.0
    if name == "mean8":
        return n + 8.0
    if name == "mean100":
        return n * 4.0 + 100.0
    if name == "tiny":                       # var ~ 1e-6: eps matters
        return n * 1e-3
    if name == "huge":
        return n * 1e4
    if name == "spike":                      # one 300.0 in 0.05-scale noise
        n = n * 0.05
        n[int(torch.randint(0, C, (1,), generator=g))] = 300.0
        return n
    if name == "const":
        return torch.full((C,), 3.25)
    if name == "offset":                     # mean / std = 400, exact in bf16: what a one-pass variance cannot do in fp32
        return 200.0 + (torch.rand(C, generator=g) < 0.5).float()
    raise ValueError(name)


def make_rows(M: int, C: int, seed: int, families: Sequence[str] = FAMILIES, first: int = 0):
    """x [M, C] bf16 whose rows cycle through `families`, and the rows' names.  Every pass through the cycle starts one
    family later, so that with an even number of families each still meets both rows of a wave's pair."""
    g = torch.Generator().manual_seed(seed)
    n = len(families)
    names = [families[(first + r + r // n) % n] for r in range(M)]
    return torch.stack([family_row(n, C, g) for n in names]).to(torch.bfloat16), names


def make_params(shape, seed: int) -> Tensor:
    """N(0, 0.3) bf16 parameters."""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 0.3).to(torch.bfloat16)


MOD_LAYOUTS = {"cols01": (0, 1), "cols34": (3, 4), "head": None}


def e0_views(e0: Tensor, layout: str):
    """(e0_shift, e0_scale) [G, C] views of a case's e0 tensor, on whatever device it lives: two columns of [G, 6, C]
    (group stride 6C), or for "head" the one [G, C] tensor as both (group stride C, as the head's LayerNorm passes it)."""
    cols = MOD_LAYOUTS[layout]
    return (e0, e0) if cols is None else (e0[:, cols[0]], e0[:, cols[1]])


def modulate_case(M: int, C: int, rows_per_group: int, layout: str) -> dict:
    """Inputs of one layernorm_modulate launch: x [M, C] over the families, N(0, 0.3) parameters, every group's e0 distinct."""
    x, names = make_rows(M, C, 1000 * M + C)
    G = (M + rows_per_group - 1) // rows_per_group
    e0 = make_params((G, C) if layout == "head" else (G, 6, C), M + rows_per_group)
    for t in e0_views(e0, layout):
        assert torch.unique(t, dim=0).shape[0] == G, "every group's e0 row must be distinct"
    return {"x": x, "names": names, "mod_shift": make_params((C,), 3 * C + 1), "mod_scale": make_params((C,), 3 * C + 2), "e0": e0}


# ------------------------------------------------------------------------------------------------ bf16 arithmetic on float64
def round_bf16(v: Tensor) -> Tensor:
    """float64 -> the nearest bf16 value (ties to even), ONE rounding, returned as float64 (normal range only)."""
    m, e = torch.frexp(v.double())
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def ulp_bf16(v: Tensor) -> Tensor:
    """Spacing of bf16 at |v| (float64); at 0 and below the normal range, the spacing of the smallest normal binade."""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def ordinal(t: Tensor) -> Tensor:
    """bf16 -> int32 that counts bf16 values along the real line (+0 and -0 both 0)."""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b & 0x7FFF), b)


def bits(t: Tensor) -> Tensor:
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ float64 references
def _xn64(x: Tensor, eps: float) -> Tensor:
    xd = x.double()
    d = xd - xd.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)


def mod_params64(mod_shift: Tensor, mod_scale: Tensor, e0_shift: Tensor, e0_scale: Tensor):
    """(add, scl) [G, C]: the bf16 values of mod + e0 (causal_model.py:310 adds two bf16 tensors), as float64."""
    add = round_bf16(mod_shift.double()[None] + e0_shift.double())
    scl = round_bf16(mod_scale.double()[None] + e0_scale.double())
    return add, scl


def row_groups(M: int, rows_per_group: int) -> Tensor:
    return torch.arange(M) // rows_per_group


def ref_layernorm_modulate(x, mod_shift, mod_scale, e0_shift, e0_scale, rows_per_group: int, eps: float) -> dict:
    """x [M, C], mod_* [C], e0_* [G, C], all bf16.  y (unrounded float64), prod = xn (1 + scl), add, group per row."""
    grp = row_groups(x.shape[0], rows_per_group)
    add, scl = mod_params64(mod_shift, mod_scale, e0_shift, e0_scale)
    prod = _xn64(x, eps) * (1.0 + scl[grp])
    return {"y": prod + add[grp], "prod": prod, "add": add[grp], "group": grp}


def ref_layernorm_affine(x, weight, bias, eps: float) -> dict:
    prod = _xn64(x, eps) * weight.double()[None]
    add = bias.double()[None].expand_as(prod)
    return {"y": prod + add, "prod": prod, "add": add, "group": torch.zeros(x.shape[0], dtype=torch.long)}


def ref_rmsnorm(x, weight, eps: float) -> Tensor:
    """bf16 [M, C]: bf16(bf16(x r) w), float64 in between."""
    xd = x.double()
    r = 1.0 / torch.sqrt((xd * xd).mean(-1, keepdim=True) + eps)
    return round_bf16(round_bf16(xd * r) * weight.double()[None]).to(torch.bfloat16)


def ref_sinusoid(t: Tensor, dim: int) -> Tensor:
    """bf16 [n, dim] (cos | sin): wan_oracle's float64 embedding through torch's float64 -> bf16 conversion."""
    return wo.sinusoidal_embedding_1d(dim, t.flatten()).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ fp32 emulation
def lane_tree_sum(t: Tensor) -> Tensor:
    """t [M, C] fp32 -> [M]: lane l sums elements (i * 64 + l) * 8 + j in the order (i, j), then a pairwise 64-lane tree."""
    M, C = t.shape
    v = t.view(M, C // 512, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, C // 64)
    s = torch.zeros(M, 64, dtype=torch.float32)
    for k in range(v.shape[2]):
        s = s + v[:, :, k]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def emu_ln_stats(x32: Tensor, eps: float):
    """Two-pass fp32 statistics: (mean [M, 1], rstd [M, 1])."""
    C = x32.shape[1]
    mean = (lane_tree_sum(x32) / C)[:, None]
    d = x32 - mean
    return mean, torch.rsqrt(lane_tree_sum(d * d) / C + torch.tensor(eps, dtype=torch.float32))[:, None]


def emu_mod_params(mod_shift, mod_scale, e0_shift, e0_scale):
    """(add, scl) [G, C] bf16 from fp32 sums."""
    return ((mod_shift.float()[None] + e0_shift.float()).to(torch.bfloat16),
            (mod_scale.float()[None] + e0_scale.float()).to(torch.bfloat16))


def emu_ln_apply(x32: Tensor, mean: Tensor, rstd: Tensor, mult32: Tensor, add32: Tensor) -> Tensor:
    return ((x32 - mean) * rstd * mult32 + add32).to(torch.bfloat16)


def emu_layernorm_modulate(x, mod_shift, mod_scale, e0_shift, e0_scale, rows_per_group: int, eps: float) -> Tensor:
    grp = row_groups(x.shape[0], rows_per_group)
    add, scl = emu_mod_params(mod_shift, mod_scale, e0_shift, e0_scale)
    mean, rstd = emu_ln_stats(x.float(), eps)
    return emu_ln_apply(x.float(), mean, rstd, 1.0 + scl.float()[grp], add.float()[grp])


def emu_layernorm_affine(x, weight, bias, eps: float) -> Tensor:
    mean, rstd = emu_ln_stats(x.float(), eps)
    return emu_ln_apply(x.float(), mean, rstd, weight.float()[None], bias.float()[None])


def emu_rms_r(x32: Tensor, eps: float, denom: Optional[int] = None) -> Tensor:
    return torch.rsqrt(lane_tree_sum(x32 * x32) / (denom or x32.shape[1]) + torch.tensor(eps, dtype=torch.float32))[:, None]


def emu_rmsnorm(x, weight, eps: float) -> Tensor:
    x32 = x.float()
    return ((x32 * emu_rms_r(x32, eps)).to(torch.bfloat16).float() * weight.float()[None]).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ reports
@dataclass
class RowReport:
    row: int
    group: int
    family: str
    worst_col: int
    worst: float            # LayerNorm: ulps of the larger operand; RMSNorm / sinusoid: bf16 steps
    mismatches: int         # elements that differ from the rounded reference at all
    got: float
    want: float


@dataclass
class Report:
    kernel: str
    width: int
    rows: List[RowReport]
    failures: List[str] = field(default_factory=list)
    blamed: List[int] = field(default_factory=list)        # rows named by a failure, ascending

    @property
    def worst(self) -> float:
        return max(r.worst for r in self.rows)

    @property
    def share(self) -> float:
        return sum(r.mismatches for r in self.rows) / (len(self.rows) * self.width)

    @property
    def ok(self) -> bool:
        return not self.failures

    def figures(self) -> str:
        w = max(self.rows, key=lambda r: r.worst)
        return (f"{self.kernel} C={self.width} M={len(self.rows)}: worst {w.worst:.3f} at row {w.row} (group {w.group}, {w.family}) "
                f"col {w.worst_col}; {self.share * 100:.4f} % of the elements differ")

    def by_family(self) -> dict:
        out = {}
        for r in self.rows:
            w, n, k = out.get(r.family, (0.0, 0, 0))
            out[r.family] = (max(w, r.worst), n + r.mismatches, k + 1)
        return {f: (w, n / (k * self.width)) for f, (w, n, k) in out.items()}

    def assert_ok(self):
        assert self.ok, f"{len(self.failures)} violation(s); first: " + "\n".join(self.failures[:4]) + "\n" + self.figures()


def _finish(rep: Report, cap: float, share_cap: float, unit: str, nan_rows: Tensor) -> Report:
    where = lambda r: f"{rep.kernel} C={rep.width} row {r.row} group {r.group} family {r.family}"  # noqa: E731
    for r in rep.rows:
        if bool(nan_rows[r.row]):
            rep.failures.append(f"{where(r)}: non-finite output at col {r.worst_col}")
            rep.blamed.append(r.row)
        elif r.worst > cap:
            rep.failures.append(f"{where(r)}: col {r.worst_col} is {r.got!r}, reference {r.want!r}: {r.worst:.3f} {unit} > {cap}")
            rep.blamed.append(r.row)
    if rep.share > share_cap:
        # the launch differs too often: the rows that do so themselves carry the blame
        m = max(rep.rows, key=lambda r: r.mismatches)
        rep.failures.append(f"{rep.kernel} C={rep.width}: {rep.share * 100:.3f} % of the launch's elements differ from the rounded reference "
                            f"(> {share_cap * 100:g} %), most in row {m.row} group {m.group} family {m.family} ({m.mismatches})")
        for r in rep.rows:
            if r.mismatches > share_cap * rep.width and r.row not in rep.blamed:
                rep.failures.append(f"{where(r)}: {r.mismatches} of {rep.width} elements differ from the rounded reference "
                                    f"(launch: {rep.share * 100:.3f} % > {share_cap * 100:g} %)")
                rep.blamed.append(r.row)
    rep.blamed.sort()
    return rep


def _rows(kernel, C, err, mism, got, want, groups, families, nan) -> Report:
    err = torch.where(nan, torch.full_like(err, float("inf")), err)
    col = err.argmax(1)
    idx = torch.arange(err.shape[0])
    return Report(kernel, C, [RowReport(r, int(groups[r]), families[r], int(col[r]), float(err[r, col[r]]), int(mism[r]),
                                        float(got[r, col[r]]), float(want[r, col[r]])) for r in idx.tolist()])


def check_layernorm(kernel: str, out: Tensor, ref: dict, families: Sequence[str]) -> Report:
    """out [M, C] bf16 against ref_layernorm_modulate / ref_layernorm_affine."""
    M, C = out.shape
    got, y = out.double(), ref["y"]
    nan = ~torch.isfinite(got)
    scale = ulp_bf16(torch.maximum(y.abs(), torch.maximum(ref["prod"].abs(), ref["add"].abs())))
    err = (got - y).abs() / scale
    want = round_bf16(y)
    rep = _rows(kernel, C, err, (got != want).sum(1), got, want, ref["group"], families, nan)
    _finish(rep, LN_ULP_CAP, LN_SHARE_CAP, "ulp of the larger operand", nan.any(1))
    for r in rep.rows:
        if r.family == "const":
            bad = bits(out[r.row]) != bits(ref["add"][r.row].to(torch.bfloat16))
            if bool(bad.any()):
                c = int(bad.nonzero()[0])
                rep.failures.append(f"{kernel} C={C} row {r.row} group {r.group} family const: col {c} is {float(got[r.row, c])!r}, "
                                    f"not the shift {float(ref['add'][r.row, c])!r} bit for bit")
                if r.row not in rep.blamed:
                    rep.blamed.append(r.row)
    rep.blamed.sort()
    return rep


def _check_steps(kernel, out, ref, families, groups, cap, share_cap) -> Report:
    nan = ~torch.isfinite(out.float())
    steps = (ordinal(out) - ordinal(ref)).abs().double()
    rep = _rows(kernel, out.shape[1], steps, (steps != 0).sum(1), out.double(), ref.double(), groups, families, nan)
    return _finish(rep, cap, share_cap, "bf16 steps", nan.any(1))


def check_rmsnorm(out: Tensor, ref: Tensor, families: Sequence[str], kernel: str = "rmsnorm") -> Report:
    """out, ref [M, C] bf16 (ref from ref_rmsnorm)."""
    return _check_steps(kernel, out, ref, families, torch.zeros(out.shape[0], dtype=torch.long), RMS_STEP_CAP, RMS_SHARE_CAP)


def check_sinusoid(out: Tensor, ref: Tensor, t: Tensor, kernel: str = "sinusoid_embedding") -> List[Report]:
    """out, ref [n, dim] bf16: the cos half and the sin half are reported apart; a row's family is its timestep."""
    half = out.shape[1] // 2
    fam = [f"t={float(v)!r}" for v in t.flatten()]
    grp = torch.zeros(out.shape[0], dtype=torch.long)
    return [_check_steps(f"{kernel}[{name}]", out[:, lo:lo + half], ref[:, lo:lo + half], fam, grp, SIN_STEP_CAP, SIN_SHARE_CAP)
            for name, lo in (("cos", 0), ("sin", half))]
