"""Closed-form inputs, checkers and a tiled float64 emulation for the GEMM kernels of csrc/gemm_bf16.hip: the 128 x 128
kernel (t128), the ping-pong kernels (pp256 / pp224 / pp192: double buffer, pp128: ring of three), their direct and LDS
epilogues and the bf16 and fp8 operand paths.  Host-only, plain torch; tests/test_gpu_gemm_exact.py runs the kernels on
these inputs, tests/test_gemm_cases_host.py validates everything here without a GPU.

Every family is EXACT by construction: every product and every partial sum is exact in fp32 in any accumulation order,
whatever the MFMA's internal rounding, and the epilogue (bias add, gate multiply, residual add in fp32) stays exact too
-- the builders assert that each intermediate survives a round trip through fp32.  The reference is therefore the
exact value rounded ONCE to bf16 and the comparison is equality on every element, as values (-0 equals +0: EpiRegs
adds a zero bias vector where EpiLoads skips the add; a NaN is never equal).  Nothing is exempt.

Family S, selector on A (family="S"): every k, every row.
    A[m, :] is one-hot 1.0 at sigma(m), sigma a seeded permutation of 0..K-1 repeated and cut to M (hits every k when
    M >= K; never affine).  W is random bf16: all 7 mantissa bits random, exponents in [-4, 3], random sign, no zeros or
    denormals.  y[m, n] = W[n, sigma(m)], bit for bit.
Family T, selector on W (family="T"): every k, every column.
    W[n, :] is one-hot at tau(n) (every k when N >= K; else a seeded k-tile and a seeded slot inside it per column, so
    that every k-tile and every slot of a k-tile has one when N >= 128), A random as above.  y[m, n] = A[m, tau(n)].
    S and T together pin both operands' lane-to-k maps, the swizzle, every ring slot and every row and column slot.
Family D, dense integers (family="D"): the sum across all k-tiles.
    A and W hold seeded uniform integers in {-2 .. 2} (exact in e4m3 too); y = A W^T exactly, |y| <= 4 K < 2^24.
    Past K = 1536 (the fp8 form of the 24-k-tile shape, K = 3072) W is drawn from {-1, 0, 1}: with both operands in
    {-2 .. 2} the products have a standard deviation of sqrt(4 K) = 111 there and only 97.96 % stay within 256, which
    would miss the condition below; with the narrower W it is sqrt(4 K / 3) = 64 and 100 % do.
    Sensitivity (a condition on the data, not an exemption): bf16 holds |y| <= 256 exactly, so an error of 1 shows; the
    share of such elements (small_share) is >= 99 % at every shape of the GPU tests (100 % at K <= 448, 99.94 % at
    (1606, 264, 1536)); unit_sensitivity() is the share of elements whose rounded reference changes when y moves by +-1.

fp8 (fp8=True, launched through sf_gemm_fp8): one-hot and small integers are exact in e4m3; the random operand is drawn
    from the e4m3 grid (cast, then the cast values ARE the data).  a_scale[seg] = 2^((seg mod 8) - 4), w_scale[n] =
    2^((n mod 5) - 2): y = value * sa * sw exactly.  With rows_per_segment = 1 every row has a power of two of its own.

Epilogues ("none" = SF_EPI_BIAS without a bias vector, "bias", "gelu", "resid", "gate_resid"):
    bias[n] = (5 n mod 17) - 8 and resid[m, n] = ((7 m + 5 n) mod 17) - 8: integers in [-8, 8] that differ between any two
    columns (rows) whose distance is no multiple of 17.  gate(g, n) = 1 + ((g + n) mod 17) for S and T: it names the group
    (no two rows of a 16-row block share a gate when every row is a group);
    gate_mod[n] = (3 n mod 7) - 2.5, gate_e0[g, n] = gate - gate_mod, so bf16(gate_mod + gate_e0) is the integer exactly.
    Family D: gate(g, n) = 2^((g + n) mod 3), POWERS OF TWO, and the residual is gate x an integer in [-8, 8], so that
    (y + bias) * gate + resid = gate * (y + bias + r0) keeps its 8 significant bits and an error of 1 in y still shows.
    GELU cannot be exact (the kernel uses a fast exp2 and rcp): S and T only, elementwise bound 2^-8 |ref| + 4 e, e the
    largest |gelu_fp32 - gelu_fp64| of torch's CPU tanh-GELU over the case's own y (gelu_fp32_error).

Poison.  Every operand is a window of a larger parent filled with NaN: A [M, K] at (1, 32) of [M + 3, K + 64], W [N, K]
    at (1, 0) of [N + 3, K + 8] (K + 16 for fp8: the same 16 bytes), the residual rows 1 .. M of [M + 3, N + 4], bias,
    gate_mod, every gate_e0 row and w_scale followed by 4 NaN, a_scale by 4 NaN.  The kernels clamp every address into
    the windows, so a correct kernel never reads poison into a stored value and no poisoned address is outside a parent.
    Outputs live in a NaN-patterned Canary, ldo = N + 8 (LDS epilogue, N % 8 == 0) or N + 4 (direct, N % 8 == 4): all
    outside the M x N window must be untouched, and a tile no workgroup wrote keeps the pattern and fails the equality.

emulate(): float64 GEMM that walks the kernels' decomposition -- the tile order of gemm_tile_of on top of sf_xcd_remap,
tiles of 128 / 192 / 224 / 256 rows by 128 / 256 columns, k-tiles of 64 (fp8: 128) through a ring of 2 (pp128: 3), two row
halves per tile, clamped loads, the fp8 scales, the epilogue operands per 16-row block and 4-column piece, the stores --
with injectable DEFECTS.  It is not the code under test; it shows that correct tiled arithmetic passes every checker
and that each defect is rejected."""
import functools
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import List, Optional, Tuple

import torch
from torch import Tensor

# ------------------------------------------------------------------------------------------ canaried outputs
GUARD = 512                                    # elements in front of and behind every output buffer (keeps 16-byte alignment)
FILL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC5A5A5}     # quiet NaNs with a payload
INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def fill_value(dtype):
    v = FILL[dtype]
    return v - (1 << 16) if dtype == torch.bfloat16 and v >= 1 << 15 else v


class Canary:
    """`n` output elements of `dtype` between two guard bands, all pre-filled with the NaN pattern."""

    def __init__(self, n, dtype, device="cuda:0"):
        self.n, self.dtype = n, dtype
        self.raw = torch.full((n + 2 * GUARD,), fill_value(dtype), dtype=INT[dtype], device=device)
        self.region = self.raw[GUARD:GUARD + n].view(dtype)

    def ptr(self):
        return self.region.data_ptr()

    def host(self):
        return self.region.cpu()

    def assert_untouched_outside(self, owned):
        """`owned`: bool [n], the elements the launch may write.  Everything else, guard bands included, is the fill."""
        raw = self.raw.cpu()
        fv = fill_value(self.dtype)
        assert bool((raw[:GUARD] == fv).all()), "guard band in front of the output was written"
        assert bool((raw[GUARD + self.n:] == fv).all()), "guard band behind the output was written"
        stray = (raw[GUARD:GUARD + self.n] != fv) & ~owned
        assert not bool(stray.any()), f"{int(stray.sum())} elements outside the product were written, first at {int(stray.nonzero()[0])}"


def owned_mask(n, M, N, ldo, batch=1, o_bs=0):
    m = torch.zeros(n, dtype=torch.bool)
    for b in range(batch):
        torch.as_strided(m, (M, N), (ldo, 1), b * o_bs).fill_(True)
    return m


# ------------------------------------------------------------------------------------------ the GPU tests' configurations
STRUCTURES = ("t128", "pp256", "pp224", "pp192", "pp128")
# rows x columns of the workgroup tile, GROUP_M of gemm_tile_of, ring depth
TILING = {"t128": (128, 128, 8, 2), "pp256": (256, 256, 4, 2), "pp224": (224, 256, 4, 2), "pp192": (192, 256, 4, 2),
          "pp128": (128, 256, 8, 3)}
PP_COST = (("pp256", 256, 1.00), ("pp224", 224, 1.02), ("pp192", 192, 1.05), ("pp128", 128, 1.14))
EPILOGUES = ("none", "bias", "gelu", "resid", "gate_resid")
EVERY_K_TILES = (1, 2, 3, 4, 5, 6, 7, 24)
EVERY_K_N, EVERY_K_M_T = 264, 200              # family S: M = K + 70; family T: M = 200 (ragged in every tiling)
ROW_EDGE_M = (1, 15, 16, 17, 63, 64, 65, 95, 96, 97, 111, 112, 113, 127, 128, 129, 191, 192, 193, 223, 224, 225, 255, 256, 257,
              383, 384, 385, 447, 449, 513)
ROW_EDGE_N, ROW_EDGE_KT = 264, 2
COL_EDGE_N_LDS = (8, 16, 24, 56, 64, 72, 120, 128, 136, 184, 192, 200, 248, 256, 264, 328, 384, 392, 520)
COL_EDGE_N_DIRECT = (4, 12, 20, 60, 68, 124, 132, 252, 260, 268, 516)
COL_EDGE_M, COL_EDGE_KT = 258, 2
GROUP_M_N_KT = (300, 264, 2)
SUM_SHAPES = ((300, 264, 2), (518, 264, 7), (1606, 264, 24))        # (M, N, k-tiles)
MAP_SHAPES = ((1300, 264), (1300, 776), (2100, 520))
MAP_KT = 2
AUTO_SHAPE = (1100, 1032, 8)
INPLACE_M_N_KT = (300, 264, 2)


D_FULL_RANGE_K = 1536        # family D: past this K, W is drawn from {-1, 0, 1} (the oracle's docstring says why)


def kt_elems(fp8: bool) -> int:
    """Operand elements per k-tile: 128 bytes per row either way."""
    return 128 if fp8 else 64


def rows_per_group_list(M: int) -> Tuple[int, ...]:
    return (1, 37, 100, M, (M + 2) // 3)


def rows_per_segment_list(M: int) -> Tuple[int, ...]:
    return (1, 37, M, (M + 1) // 2)


def resolve_structure(structure: str, M: int, N: int, K: int, fp8: bool = False) -> str:
    """The tiling run_gemm launches for an unbatched bf16-output product: a ping-pong structure needs two k-tiles, `auto`
    takes one from 1024 x 1024 x 512 on, the one with the least cost for its rounds of 256 workgroups."""
    nk = K // kt_elems(fp8)
    if structure == "auto":
        structure = "t128"
        if nk >= 2 and M >= 1024 and N >= 1024 and K >= 512:
            best = 1e30
            for name, rows, rel in PP_COST:
                tiles = ((M + rows - 1) // rows) * ((N + 255) // 256)
                cost = ((tiles + 255) // 256) * (rows / 256.0 * rel + 0.04)
                if cost < best - 1e-9:
                    best, structure = cost, name
    return structure if nk >= 2 else "t128"


def xcd_remap(bid: int, nwg: int) -> int:
    """sf_xcd_remap of csrc/sf_common.h."""
    xcd, q8, r8 = bid & 7, nwg >> 3, nwg & 7
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3)


def tile_of(bid: int, nwg: int, tiles_m: int, tiles_n: int, group_m: int) -> Tuple[int, int]:
    """gemm_tile_of<GROUP_M>: workgroup -> (tm, tn)."""
    wg = xcd_remap(bid, nwg)
    width = group_m * tiles_n
    group = wg // width
    first_m = group * group_m
    gsz = min(tiles_m - first_m, group_m)
    in_group = wg - group * width
    return first_m + in_group % gsz, in_group // gsz


def grid_of(structure: str, M: int, N: int) -> Tuple[int, int, int]:
    """(tiles_m, tiles_n, GROUP_M) of a resolved structure."""
    bm, bn, gm, _ = TILING[structure]
    return (M + bm - 1) // bm, (N + bn - 1) // bn, gm


# ------------------------------------------------------------------------------------------ helpers
def is_bf16(x: Tensor) -> bool:
    """Every element survives the round trip through bf16 (NaN excluded)."""
    return bool((x.double().to(torch.bfloat16).double() == x.double()).all())


def is_e4m3(x: Tensor) -> bool:
    return bool((x.double().float().to(torch.float8_e4m3fn).double() == x.double()).all())


def is_f32(x: Tensor) -> bool:
    return bool((x.double().float().double() == x.double()).all())


def random_bf16(shape, g: torch.Generator) -> Tensor:
    """Random sign, exponent in [-4, 3], all 7 mantissa bits random: no zeros, no denormals."""
    sign = torch.randint(0, 2, shape, generator=g)
    exp = torch.randint(-4, 4, shape, generator=g) + 127
    mant = torch.randint(0, 128, shape, generator=g)
    bits = (sign << 15) | (exp << 7) | mant
    return torch.where(bits >= 1 << 15, bits - (1 << 16), bits).to(torch.int16).view(torch.bfloat16)


def every_k(n: int, K: int, g: torch.Generator) -> Tensor:
    """A seeded permutation of 0 .. K - 1 repeated and cut to n."""
    return torch.cat([torch.randperm(K, generator=g) for _ in range((n + K - 1) // K)])[:n]


def _window(data: Tensor, rows: int, cols: int, r0: int, c0: int) -> Tuple[Tensor, Tensor]:
    """`data` [r, c] as a window at (r0, c0) of a NaN parent [r + rows, c + cols] -> (parent, view)."""
    r, c = data.shape
    if data.dtype == torch.float8_e4m3fn:
        parent = torch.full((r + rows, c + cols), 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn)
    else:
        parent = torch.full((r + rows, c + cols), float("nan"), dtype=data.dtype)
    view = parent[r0:r0 + r, c0:c0 + c]
    view.copy_(data)
    return parent, view


def _tailed(vec: Tensor, dtype) -> Tuple[Tensor, Tensor]:
    """A vector followed by 4 NaN -> (parent, view)."""
    parent = torch.full((vec.numel() + 4,), float("nan"), dtype=dtype)
    parent[:vec.numel()] = vec.to(dtype)
    return parent, parent[:vec.numel()]


# ------------------------------------------------------------------------------------------ the builders
def gate_of(family: str, groups: int, N: int) -> Tensor:
    """[groups, N] float64: 1 + ((g + n) mod 17), or 2^((g + n) mod 3) for family D."""
    s = torch.arange(groups)[:, None] + torch.arange(N)[None, :]
    return (2.0 ** (s % 3).double()) if family == "D" else (1 + s % 17).double()


def apply_epilogue(case, y: Tensor) -> Tensor:
    """float64 [M, N]: the epilogue of `case` on y (the scaled product), before the one rounding.  GELU in float64."""
    z = y
    if case.bias is not None:
        z = z + case.bias.double()[None, :]
    if case.epi == "gelu":
        z = torch.nn.functional.gelu(z, approximate="tanh")
    if case.epi == "gate_resid":
        z = z * case.gate_rows
    if case.epi in ("resid", "gate_resid"):
        z = z + case.resid.double()
    return z


@functools.lru_cache(maxsize=None)
def build(family: str, M: int, N: int, K: int, epi: str = "none", rpg: int = 1, fp8: bool = False, rps: Optional[int] = None):
    """One case: operands as windows of poisoned parents, epilogue operands, scales, the exact reference."""
    assert family in ("S", "T", "D") and epi in EPILOGUES and K % kt_elems(fp8) == 0 and N % 4 == 0
    assert not (family == "D" and epi == "gelu"), "GELU is measured on S and T only"
    g = torch.Generator().manual_seed(1_000_003 * "STD".index(family) + 7919 * M + 31 * N + K + (5 if fp8 else 0))
    opd = torch.float8_e4m3fn if fp8 else torch.bfloat16
    c = SimpleNamespace(family=family, M=M, N=N, K=K, epi=epi, rpg=rpg, fp8=fp8, rps=rps, sigma=None, tau=None)
    if family == "S":
        c.sigma = every_k(M, K, g)
        a = torch.zeros(M, K)
        a[torch.arange(M), c.sigma] = 1.0
        a, w = a.to(opd), random_bf16((N, K), g).float().to(opd)
        y = w.double()[:, c.sigma].T.contiguous()
    elif family == "T":
        kt = kt_elems(fp8)       # N < K: every k-tile and every slot of a k-tile (lane, chunk) still has a column
        c.tau = every_k(N, K, g) if N >= K else every_k(N, K // kt, g) * kt + every_k(N, kt, g)
        w = torch.zeros(N, K)
        w[torch.arange(N), c.tau] = 1.0
        a, w = random_bf16((M, K), g).float().to(opd), w.to(opd)
        y = a.double()[:, c.tau].contiguous()
    else:
        a = torch.randint(-2, 3, (M, K), generator=g).float().to(opd)
        hi = 2 if K <= D_FULL_RANGE_K else 1
        w = torch.randint(-hi, hi + 1, (N, K), generator=g).float().to(opd)
        y = a.double() @ w.double().T
        assert float(y.abs().max()) <= 4 * K < 2 ** 24
    c.y_raw = y
    pad_w = 16 if fp8 else 8
    c.a_parent, c.a = _window(a, 3, 64, 1, 32)
    c.w_parent, c.w = _window(w, 3, pad_w, 1, 0)
    c.lda, c.ldw, c.ldr = K + 64, K + pad_w, N + 4
    c.ldo = N + 8 if N % 8 == 0 else N + 4
    c.lds_epilogue = N % 8 == 0 and c.ldo % 8 == 0
    # fp8 scales
    c.a_scale = c.w_scale = c.a_scale_parent = c.w_scale_parent = c.scale = None
    if fp8:
        c.rps = rps = rps or M
        nseg = (M + rps - 1) // rps
        c.a_scale_parent, c.a_scale = _tailed(2.0 ** ((torch.arange(nseg) % 8) - 4).double(), torch.float32)
        c.w_scale_parent, c.w_scale = _tailed(2.0 ** ((torch.arange(N) % 5) - 2).double(), torch.float32)
        c.scale = c.a_scale.double()[torch.arange(M) // rps][:, None] * c.w_scale.double()[None, :]
        y = y * c.scale
        assert is_f32(y)
    c.y = y
    # epilogue operands
    c.bias = c.resid = c.gate_mod = c.gate_e0 = c.gate_rows = None
    c.bias_parent = c.resid_parent = c.gate_mod_parent = c.gate_e0_parent = None
    n_idx, m_idx = torch.arange(N), torch.arange(M)
    if epi != "none":
        c.bias_parent, c.bias = _tailed(((5 * n_idx) % 17 - 8).double(), torch.bfloat16)
    steps = [y]
    if c.bias is not None:
        steps.append(y + c.bias.double()[None, :])
    if epi == "gate_resid":
        groups = (M + rpg - 1) // rpg
        gate = gate_of(family, groups, N)
        gm = ((3 * n_idx) % 7).double() - 2.5
        c.gate_mod_parent, c.gate_mod = _tailed(gm, torch.bfloat16)
        c.gate_e0_parent, c.gate_e0 = _window((gate - gm[None, :]).to(torch.bfloat16), 0, 4, 0, 0)
        assert is_bf16(gm) and is_bf16(gate - gm[None, :]) and is_bf16(gate)
        assert torch.equal((c.gate_mod.float()[None, :] + c.gate_e0.float()).to(torch.bfloat16).double(), gate), "the gate is exact"
        c.gate_rows = gate[m_idx // rpg]
        steps.append(steps[-1] * c.gate_rows)
    if epi in ("resid", "gate_resid"):
        r = ((7 * m_idx[:, None] + 5 * n_idx[None, :]) % 17 - 8).double()
        if family == "D" and epi == "gate_resid":
            r = r * c.gate_rows
        assert is_bf16(r)
        c.resid_parent, c.resid = _window(r.to(torch.bfloat16), 3, 4, 1, 0)
        steps.append(steps[-1] + r)
    if epi != "gelu":
        for s in steps:
            assert is_f32(s) and float(s.abs().max()) < 2 ** 24, "every epilogue intermediate is exact in fp32"
    c.ref64 = apply_epilogue(c, y)
    c.ref = c.ref64.float().to(torch.bfloat16)
    assert not bool(c.ref64.isnan().any())
    return c


def small_share(case) -> float:
    """Family D: the share of products with |y| <= 256, which bf16 holds exactly."""
    return float((case.y_raw.abs() <= 256).double().mean())


def unit_sensitivity(case) -> float:
    """The share of elements whose rounded reference changes when the raw product moves by +1 and by -1."""
    scale = case.scale if case.fp8 else torch.ones_like(case.y)
    up = apply_epilogue(case, (case.y_raw + 1) * scale).float().to(torch.bfloat16)
    dn = apply_epilogue(case, (case.y_raw - 1) * scale).float().to(torch.bfloat16)
    return float(((up != case.ref) & (dn != case.ref)).double().mean())


def plain_reference(case) -> Tensor:
    """float64 A W^T with the scales and the epilogue, from the windows: what every closed form must equal."""
    y = case.a.double() @ case.w.double().T
    if case.fp8:
        y = y * case.scale
    return apply_epilogue(case, y)


def gelu_fp32_error(case) -> float:
    """Largest |gelu_fp32 - gelu_fp64| of torch's CPU tanh-GELU over the case's own y + bias."""
    y = case.y + case.bias.double()[None, :]
    gelu = torch.nn.functional.gelu
    return float((gelu(y.float(), approximate="tanh").double() - gelu(y, approximate="tanh")).abs().max())


def out_elements(case) -> int:
    return (case.M + 3) * case.ldo


def new_canary(case, device="cpu", inplace: bool = False) -> Canary:
    """The output buffer of a launch: M + 3 rows of ldo elements.  inplace: the window pre-filled with the residual."""
    can = Canary(out_elements(case), torch.bfloat16, device)
    if inplace:
        can.region[:case.M * case.ldo].view(case.M, case.ldo)[:, :case.N].copy_(case.resid.to(device))
    return can


# ------------------------------------------------------------------------------------------ checkers
@dataclass
class Report:
    what: str
    ok: bool = True
    blamed: Optional[Tuple[int, int]] = None                                # the first (m, n) that is wrong
    rows: List[int] = field(default_factory=list)                           # every row with a wrong element, sorted
    cols: List[int] = field(default_factory=list)                           # every column with a wrong element, sorted
    bad: int = 0
    compared: int = 0
    stray: int = 0                                                          # elements outside the M x N window that were written
    failures: List[str] = field(default_factory=list)

    def figures(self) -> str:
        return (f"{self.what}: {'ok' if self.ok else 'REJECTED'}, {self.compared} elements compared, {self.bad} wrong in "
                f"{len(self.rows)} rows x {len(self.cols)} columns, {self.stray} stray")

    def assert_ok(self):
        assert self.ok, "; ".join(self.failures[:4])


def check(case, can: Canary, structure: str = "", extra: Optional[float] = None) -> Report:
    """Equality of every element of the M x N window with the reference, as values (extra = None), or the GELU bound
    |out - ref| <= 2^-8 |ref| + extra; and everything outside the window, guard bands included, untouched."""
    M, N, ldo = case.M, case.N, case.ldo
    what = f"{case.family}{'/fp8' if case.fp8 else ''}[{structure} {M}x{N}x{case.K} {case.epi}"
    what += (f" rpg={case.rpg}" if case.epi == "gate_resid" else "") + (f" rps={case.rps}" if case.fp8 else "") + "]"
    rep = Report(what, compared=M * N)
    raw = can.raw.cpu()
    fv = fill_value(torch.bfloat16)
    outside = torch.ones(raw.numel(), dtype=torch.bool)
    outside[GUARD:GUARD + can.n] = ~owned_mask(can.n, M, N, ldo)
    rep.stray = int(((raw != fv) & outside).sum())
    if rep.stray:
        first = int(((raw != fv) & outside).nonzero()[0]) - GUARD
        rep.ok = False
        rep.failures.append(f"{what}: {rep.stray} elements outside the product were written, first at offset {first} (row {first // ldo}, column {first % ldo})")
    out = raw[GUARD:GUARD + M * ldo].view(torch.bfloat16).view(M, ldo)[:, :N].double()
    if extra is None:
        bad = ~(out == case.ref.double())
    else:
        bad = ~((out - case.ref64).abs() <= 2.0 ** -8 * case.ref64.abs() + extra)
    rep.bad = int(bad.sum())
    if rep.bad:
        rep.ok = False
        rep.rows, rep.cols = bad.any(1).nonzero().flatten().tolist(), bad.any(0).nonzero().flatten().tolist()
        m, n = (int(v) for v in bad.nonzero()[0])
        rep.blamed = (m, n)
        k = f", k = {int(case.sigma[m])}" if case.sigma is not None else f", k = {int(case.tau[n])}" if case.tau is not None else ""
        rep.failures.append(f"{what}: {rep.bad} of {M * N} elements wrong in {len(rep.rows)} rows x {len(rep.cols)} columns, first at "
                            f"({m}, {n}){k}: out {float(out[m, n])} ref {float(case.ref64[m, n])}")
    return rep


# ------------------------------------------------------------------------------------------ the tiled emulation
DEFECTS = ("skip_ktile", "double_ktile", "stale_slot_a", "stale_slot_w", "k_mispair", "wrong_half", "ragged_row_to_last",
           "drop_last_row", "gate_group_of_block", "scale_segment_of_block", "col_clamp_off", "resid_ld", "tile_twice",
           "epilogue_swizzle")
NAN = float("nan")


def _flat64(parent: Optional[Tensor], extra: int) -> Optional[Tensor]:
    """The parent's memory as float64, followed by `extra` NaN: reads behind a parent give NaN, as poison does."""
    if parent is None:
        return None
    return torch.cat([parent.reshape(-1).double(), torch.full((extra,), NAN, dtype=torch.float64)])


def _fetch(flat: Tensor, idx: Tensor) -> Tensor:
    return flat[idx.clamp(0, flat.numel() - 1)]


def emulate(case, structure: str, defect: Optional[str] = None, arg=None, inplace: bool = False) -> Canary:
    """The product of `case` as `structure` computes it, in float64, stored into a host Canary.
    defect (one of DEFECTS) / arg:
      skip_ktile              arg = k-tile t: never accumulated
      double_ktile            arg = k-tile t: accumulated twice (t128's tail re-request gone wrong)
      stale_slot_a / _w       arg = k-tile t >= ring depth: its slot still holds k-tile t - depth of A / of W
      k_mispair               W's 16-byte chunks kq and 4 + kq swapped inside every k-tile, A's not
      wrong_half              the second row half of every tile reads the A rows of the first
      ragged_row_to_last      rows >= M take their epilogue operands at their own row and are stored onto row M - 1
      drop_last_row           row M - 1 is not stored
      gate_group_of_block     the gate group of a 16-row block's first row serves the whole block
      scale_segment_of_block  the same for a_scale's segment
      col_clamp_off           the column clamp of bias, gate and w_scale is N - 8, not N - 4 (LDS epilogue and fp8 scales)
      resid_ld                the residual is indexed with ldo
      tile_twice              arg = workgroup b >= 1: it takes the tile of workgroup b - 1, its own is never written
      epilogue_swizzle        LDS epilogue: 8-column chunks c and c ^ 1 swapped on odd rows"""
    assert defect is None or defect in DEFECTS
    M, N, K = case.M, case.N, case.K
    st = resolve_structure(structure, M, N, K, case.fp8)
    bm, bn, group_m, depth = TILING[st]
    kt = kt_elems(case.fp8)
    nk = K // kt
    tiles_m, tiles_n = (M + bm - 1) // bm, (N + bn - 1) // bn
    nwg = tiles_m * tiles_n
    a, w = case.a.double(), case.w.double()
    ldo, ldr = case.ldo, case.ldr
    can = new_canary(case, "cpu", inplace)
    out = can.region.view(torch.int16)
    big = 256 * max(ldo, 16) + 4096
    bias = _flat64(case.bias_parent, big)
    gmod = _flat64(case.gate_mod_parent, big)
    ge0 = _flat64(case.gate_e0_parent, big)
    ge0_stride = N + 4
    if inplace:      # the residual is the output window itself: row stride ldo, read before it is overwritten
        resid, r_off, r_ld = torch.cat([can.region.double(), torch.full((big,), NAN, dtype=torch.float64)]), 0, ldo
    else:
        resid, r_off, r_ld = _flat64(case.resid_parent, big), ldr, ldr
    sa = _flat64(case.a_scale_parent, big)
    sw = _flat64(case.w_scale_parent, big)
    seq = list(range(nk))
    if defect == "skip_ktile":
        seq.remove(arg)
    elif defect == "double_ktile":
        seq.insert(arg, arg)
    if defect in ("stale_slot_a", "stale_slot_w"):
        assert depth <= arg < nk
    for bid in range(nwg):
        tm, tn = tile_of(bid - 1 if defect == "tile_twice" and bid == arg else bid, nwg, tiles_m, tiles_n, group_m)
        m0, n0 = tm * bm, tn * bn
        rows, cols = m0 + torch.arange(bm), n0 + torch.arange(bn)
        a_tile, w_tile = a[rows.clamp(max=M - 1)], w[cols.clamp(max=N - 1)]          # the loads' row clamps
        acc = torch.zeros(bm, bn, dtype=torch.float64)
        ring_a: List[Optional[Tensor]] = [None] * depth
        ring_w: List[Optional[Tensor]] = [None] * depth
        for t in seq:
            slot = t % depth
            if not (defect == "stale_slot_a" and t == arg):
                ring_a[slot] = a_tile[:, t * kt:(t + 1) * kt]
            if not (defect == "stale_slot_w" and t == arg):
                ring_w[slot] = w_tile[:, t * kt:(t + 1) * kt]
            at, wt = ring_a[slot], ring_w[slot]
            if defect == "k_mispair":
                wt = torch.cat([wt[:, kt // 2:], wt[:, :kt // 2]], 1)
            for h in range(2):
                half = slice(h * bm // 2, (h + 1) * bm // 2)
                src = slice(0, bm // 2) if defect == "wrong_half" else half
                acc[half] += at[src] @ wt.T
        # operand indices: the kernels' clamps, per 16-row block and 4-column piece
        r_op = rows if defect == "ragged_row_to_last" else rows.clamp(max=M - 1)
        first = (m0 + (rows - m0) // 16 * 16).clamp(max=M - 1)
        piece = cols - cols % 4
        c_clamped = piece.clamp(max=N - (8 if defect == "col_clamp_off" else 4)) + cols % 4
        c_op = c_clamped if case.lds_epilogue else cols
        z = acc
        if case.fp8:
            seg = (first if defect == "scale_segment_of_block" else rows.clamp(max=M - 1)) // case.rps
            z = z * (_fetch(sa, seg)[:, None] * _fetch(sw, c_clamped)[None, :])
        if case.bias is not None:
            z = z + _fetch(bias, c_op)[None, :]
        if case.epi == "gelu":
            z = torch.nn.functional.gelu(z, approximate="tanh")
        if case.epi == "gate_resid":
            grp = (first if defect == "gate_group_of_block" else r_op) // case.rpg
            gate = _fetch(gmod, c_op)[None, :] + _fetch(ge0, grp[:, None] * ge0_stride + c_op[None, :])
            z = z * gate.float().to(torch.bfloat16).double()
        if case.epi in ("resid", "gate_resid"):
            ld = ldo if defect == "resid_ld" else r_ld
            z = z + _fetch(resid, r_off + r_op[:, None] * ld + c_op[None, :])
        z = z.float().to(torch.bfloat16)
        if defect == "epilogue_swizzle" and case.lds_epilogue:
            odd = ((rows - m0) % 2 == 1)
            z[odd] = z[odd][:, torch.arange(bn) ^ 8]
        # the stores: rows < M; under ragged_row_to_last the rows >= M then land on row M - 1 one by one, the last one wins
        keep_r = rows < (M - 1 if defect == "drop_last_row" else M)
        keep_c = cols < N
        idx = (rows[keep_r][:, None] * ldo + cols[keep_c][None, :]).reshape(-1)
        out[idx] = z[keep_r][:, keep_c].reshape(-1).view(torch.int16)
        if defect == "ragged_row_to_last":
            for r in (rows >= M).nonzero().flatten().tolist():
                out[(M - 1) * ldo + cols[keep_c]] = z[r, keep_c].view(torch.int16)
    return can


# ------------------------------------------------------------------------------------------ what each GPU test launches
def k_of(tiles: int, fp8: bool) -> int:
    return tiles * kt_elems(fp8)


def every_k_cases(fp8: bool):
    for tiles in EVERY_K_TILES:
        K = k_of(tiles, fp8)
        yield build("S", K + 70, EVERY_K_N, K, fp8=fp8, rps=(K + 71) // 2 if fp8 else None)
        yield build("T", EVERY_K_M_T, EVERY_K_N, K, fp8=fp8, rps=37 if fp8 else None)


def row_edge_cases(fp8: bool):
    for M in ROW_EDGE_M:
        for epi in ("resid", "gate_resid"):
            yield build("S", M, ROW_EDGE_N, k_of(ROW_EDGE_KT, fp8), epi, 1, fp8, 1 if fp8 else None)


def column_edge_cases(fp8: bool, form: str):
    for N in COL_EDGE_N_LDS if form == "lds" else COL_EDGE_N_DIRECT:
        for epi in ("bias", "gate_resid"):
            yield build("T", COL_EDGE_M, N, k_of(COL_EDGE_KT, fp8), epi, 37, fp8, 37 if fp8 else None)


def group_cases(fp8: bool, gelu: bool = False):
    """gelu=False: the exact ones (bias, resid, gate_resid with every rows_per_group); gelu=True: the two bounded ones."""
    M, N, tiles = GROUP_M_N_KT
    K = k_of(tiles, fp8)
    for rps in rows_per_segment_list(M) if fp8 else (None,):
        if gelu:
            for family in "ST":
                yield build(family, M, N, K, "gelu", 1, fp8, rps)
            continue
        for epi in ("bias", "resid"):
            yield build("S", M, N, K, epi, 1, fp8, rps)
        for rpg in rows_per_group_list(M):
            yield build("S", M, N, K, "gate_resid", rpg, fp8, rps)


def sum_cases(fp8: bool):
    for M, N, tiles in SUM_SHAPES:
        for epi in ("none", "bias", "resid", "gate_resid"):
            yield build("D", M, N, k_of(tiles, fp8), epi, 37, fp8, (M + 1) // 2 if fp8 else None)


def map_cases(fp8: bool):
    for M, N in MAP_SHAPES:
        yield build("S", M, N, k_of(MAP_KT, fp8), fp8=fp8, rps=37 if fp8 else None)


def auto_cases(fp8: bool):
    M, N, tiles = AUTO_SHAPE
    for family in "SD":
        yield build(family, M, N, k_of(tiles, fp8), "resid", 1, fp8, 37 if fp8 else None)


def inplace_cases(fp8: bool):
    M, N, tiles = INPLACE_M_N_KT
    for epi, rpg in (("resid", 1), ("gate_resid", 37)):
        yield build("S", M, N, k_of(tiles, fp8), epi, rpg, fp8, 37 if fp8 else None)
