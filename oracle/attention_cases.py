"""Closed-form inputs, checkers and a tiled float64 emulation for the three attention kernels of csrc/attention.hip
(w4: 128 query rows per workgroup, w8: 256 rows in anti-phase, r64: the hand-scheduled stream), their folded-key path
(`keys` / `log2w`) and the accumulate epilogue.  Host-only, plain torch; tests/test_gpu_attention_exact.py runs the kernels
on these inputs, tests/test_attention_cases_host.py validates everything here without a GPU.

Every input is exactly representable in bf16 and every answer is known in closed form, so no tolerance is measured on
random data.  c = log2(e) / sqrt(128) ~ 0.1275 is the log2-domain score per unit of q.k; tensors are [B, L, H, 128].

Family A, "selector" (selector_case): which key, which V row.
    Per (batch, head) seeded codes s_j in {+-1}^128, resampled until max_{j != j'} s_j.s_j' <= 64 (asserted);
    k_j = 8 s_j, q_i = 8 s_pi(i), pi a seeded map onto [0, Lk) that hits every key when Lq >= Lk; V Gaussian bf16 (or
    integers in [-8, 8] for the accumulate test), different per (batch, head).
    The winner scores 8192 c ~ 1044 and leads every other key by >= 64 * 64 * c ~ 522 log2 units, so every other
    probability is exactly 0 in fp32 (exp2(-522) underflows; 2^-149 is the smallest fp32), also under r64's lazy reference
    that lags the maximum by at most 8: when the winner arrives the earlier partial sums are rescaled by exp2(-522) = 0.
    Closed form: out[i] = V[pi(i)].
    Bounds:  w4 / w8  bit equality.  p = exp2(residual), the residual being the fp32 rounding of m c (<= 2^-24 * 1044
                      < 2^-13; exactly 0 when s c - m c is one fma, 8192 being a power of two), rounds to bf16 1, and
                      l = p; V / l perturbs V by < 2^-12 relative, less than half a bf16 step (2^-9): it rounds back to V.
             r64      |out - V| <= 2^-7 |V|.  Its P = exp2(delta), delta in [0, 8], is rounded to bf16 (2^-8 relative)
                      before P.V; that moves V by less than one bf16 step before the final rounding.
             auto     the r64 bound (whichever kernel the launch picks meets it).
    The accumulate form (integer V, integer R in `out`): bit equal to bf16(R + V[pi]); |R + V| <= 16 is exact in bf16.

Family B, "classes" (classes_case): exact ties across tiles.
    h_r = rows of the 128 x 128 Sylvester Hadamard matrix, k_j = 8 h_{j mod P}, q_r = 8 h_r for r < P.  Members
    (j = r mod P) score 8192 c ~ 1044, everything else exactly 0 (orthogonal rows), weight exp2(-1044) = 0.  A query averages
    exactly its class: the same slot of every tile for P = 64, alternating tiles for P = 128, a walking slot for P = 100.
    A query whose class is empty (r >= Lk) ties on ALL keys at score 0 and averages all of them: its class is [0, Lk).
    Closed form: out[r] = mean of V over the class, in float64.
    Bounds, n = class size, A = sum |V| over the class:
             w4 / w8  2^-8 |ref| + n 2^-22 A   one bf16 rounding (at most 2^-8 / (1 + 2^-8) of the value; what it leaves
                      covers the reciprocal and the fp32 sum of l) plus an fp32 accumulation of exact products in any
                      order, (n - 1) 2^-24 each way, x 4 for the MFMA's undocumented rounding mode, / n for the mean --
                      the form of tests/test_gpu_gemm_batched.py.
             r64, auto  2^-7 |ref| + n 2^-22 A   (bf16 P: 2^-8 more).

Family C, "uniform" (uniform_case): mask, counts, fold, rows that must not be read.
    Every k_j = -2 h_0 (h_0 = all ones), q_i = 2 t_i h_0 with t_i in {1, 2, 4}: all keys tie at -512 t_i c ~ -65 t_i.
    V[j, d] = g [d = j mod 128], g a power of two that differs per (batch, head).
    Closed form: out[i, d] = g n_d / Lk, n_d = #{j < Lk : j = d mod 128}; EXACTLY 0 where n_d = 0.
    With a fold (keys[b] = n + 1, log2w[b] = log2(same)): out[d] = g (n_d(n) + same [d = n mod 128]) / (n + same).
    Bound: 2^-6 relative, every structure: bf16 P (2^-8), one reciprocal, the final rounding (2^-8), Lk 2^-24 for the
    sum of l; a zero reference admits only 0.  An unmasked tail key scores 0, outweighs the real keys by >= 2^65 and
    zeroes the row; a dropped key changes one class by >= 1/9 relative at Lk <= 1100.
    Windowed (window): the slab is rows [lo, lo + Lk) of a larger tensor whose other rows -- and rows [keys[b], Lk) of the
    window under a fold -- hold poison: "dominant" (K = +16 h_0, V = 1024: such a row would take all the weight) or "nan"
    (reading it at all shows).  include/sf_hip.h: sample b attends rows [0, keys[b]) only.

emulate(): float64 attention that walks 64-key tiles with a running reference (optionally r64's lazy one: moved only when
a row's maximum exceeds it by more than 8) and optionally rounds P to bf16, with injectable DEFECTS.  It is not the code
under test; it shows that correct tiled arithmetic passes every checker and that each defect is rejected."""
import functools
import math
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import List, Optional, Tuple

import torch
from torch import Tensor

D = 128
KT = 64
C_LOG2 = math.log2(math.e) / math.sqrt(D)
GAP = 64                                        # family A: largest allowed s_j . s_j' between different keys
STRUCTURES = ("r64", "w8", "w4")
REL = {"w4": 2.0 ** -8, "w8": 2.0 ** -8, "r64": 2.0 ** -7, "auto": 2.0 ** -7}
UNIFORM_REL = 2.0 ** -6
POISONS = ("dominant", "nan")

# ------------------------------------------------------------------------------------------ the GPU tests' configurations
EVERY_KEY_LK = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 449, 832, 1024, 1025, 1100)
QUERY_EDGE_LQ = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 513)
QUERY_EDGE_LK = 129
TIE_LK, TIE_P = (65, 193, 1100), (64, 100, 128)
UNIFORM_LK, UNIFORM_LQ = (1, 63, 64, 65, 127, 129, 257, 1100), 70
FOLD_N, FOLD_SLABS, FOLD_SAME = (0, 1, 62, 63, 64, 127, 200), (128, 512), (2, 4, 64)
MAP_LK = 65
# (B, H, Lq): workgroups of w4 (128 rows) / w8 and r64 (256 rows), and the branch of attention_r64_kernel's map it reaches
# (q8 = nwg >> 3 slots per XCD, Q = query tiles per pair, f = q8 / Q whole pairs per XCD)
MAP_CASES = (
    (1, 1, 257),     # w4   3 (3 mod 8) | w8, r64   2 (2): q8 = 0, f = 0, every workgroup a leftover, only XCDs 0 and 1 used
    (1, 3, 513),     # w4  15 (7)       | w8, r64   9 (1): q8 = 1 < Q = 3, f = 0, leftovers span three pairs
    (3, 7, 70),      # w4  21 (5)       | w8, r64  21 (5): Q = 1, q8 = 2, f = 2, 16 whole pairs + 5 leftover pairs, batch > 1
    (1, 9, 1030),    # w4  81 (1)       | w8, r64  45 (5): Q = 5, q8 = 5, f = 1, one pair per XCD + 1 pair over 5 XCDs
    (1, 17, 520),    # w4  85 (5)       | w8, r64  51 (3): Q = 3, q8 = 6 = f Q, f = 2, the 3 extra slots hold one pair over XCDs 0, 1, 2
    (2, 12, 257),    # w4  72 (0)       | w8, r64  48 (0): Q = 2, q8 = 6, f = 3, no leftovers at all (nwg = 8 f Q)
    (1, 13, 1800),   # w4 195 (3)       | w8, r64 104 (0): Q = 8, q8 = 13, f = 1, Q does not divide q8: 5 slots per XCD left over
    (1, 7, 300),     # w4  21 (5)       | w8, r64  14 (6): Q = 2, q8 = 1, f = 0 with leftovers on every XCD
    (1, 5, 700),     # w4  30 (6)       | w8, r64  15 (7): Q = 3, q8 = 1, f = 0
    (1, 4, 150),     # w4   8 (0)       | w8, r64   4 (4): fewer workgroups than XCDs
    (1, 5, 200),     # w4  10 (2)       | w8, r64   5 (5)
    (1, 3, 500),     # w4  12 (4)       | w8, r64   6 (6)
)
STORE_LQ, STORE_LK = (1, 65, 257, 300), 129
ACCUM_LK, ACCUM_LQ = (1, 64, 257), 300
# auto picks r64 from 192 workgroups of 256 rows and 512 keys on, w8 from 192 workgroups on, else w4: (B, H, Lq, Lk)
THRESHOLD_CASES = ((4, 48, 1, 512), (4, 47, 1, 512), (4, 48, 1, 511), (4, 47, 1, 511))


def workgroups(B: int, H: int, Lq: int, rows: int) -> int:
    return B * H * ((Lq + rows - 1) // rows)


def fold_pairs(slab: int) -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
    """((n of sample 0, n of sample 1), (same of sample 0, same of sample 1)) for a slab: every n < slab - 1 of FOLD_N
    meets sample 0 and sample 1, the two samples of a launch always differ in n and in same."""
    ns = [n for n in FOLD_N if n < slab - 1]
    return [((ns[i], ns[(i + 3) % len(ns)]), (FOLD_SAME[i % 3], FOLD_SAME[(i + 1) % 3])) for i in range(len(ns))]


# ------------------------------------------------------------------------------------------ helpers
def is_bf16(x: Tensor) -> bool:
    """Every element survives the round trip through bf16 (NaN excluded)."""
    return bool((x.double().to(torch.bfloat16).double() == x.double()).all())


@functools.lru_cache(maxsize=None)
def hadamard() -> Tensor:
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < D:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert bool((h @ h.T == D * torch.eye(D, dtype=torch.float64)).all())
    return h


def softmax_reference(q: Tensor, k: Tensor, v: Tensor, keys=None, log2w=None) -> Tensor:
    """Plain float64 softmax(q k^T / sqrt(128)) v over the attended rows [0, keys[b]), log2w[b] on the last of them."""
    B, Lq, H, _ = q.shape
    out = torch.empty(B, Lq, H, D, dtype=torch.float64)
    for b in range(B):
        lk = k.shape[1] if keys is None else int(keys[b])
        s = torch.einsum("qhd,khd->hqk", q[b].double(), k[b, :lk].double()) * C_LOG2
        if log2w is not None:
            s[:, :, lk - 1] += float(log2w[b])
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
        out[b] = torch.einsum("hqk,khd->qhd", p / p.sum(-1, keepdim=True), v[b, :lk].double())
    return out


# ------------------------------------------------------------------------------------------ family A
def _codes(Lk: int, g: torch.Generator) -> Tensor:
    for _ in range(64):
        s = (torch.randint(0, 2, (Lk, D), generator=g) * 2 - 1).float()
        gram = s @ s.T
        gram.fill_diagonal_(-D)
        if float(gram.max()) <= GAP:
            return s
    raise AssertionError(f"no codes with max correlation <= {GAP} at Lk = {Lk}")


@functools.lru_cache(maxsize=None)
def selector_case(B: int, H: int, Lq: int, Lk: int, integer_v: bool = False, seed: int = 0):
    g = torch.Generator().manual_seed(1_000_003 * seed + 7919 * Lk + 31 * Lq + 5 * H + B)
    q, k = torch.empty(B, Lq, H, D), torch.empty(B, Lk, H, D)
    pi = torch.empty(B, H, Lq, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            s = _codes(Lk, g)
            gram = s @ s.T
            gram.fill_diagonal_(-D)
            assert float(gram.max()) <= GAP, "family A: two keys closer than the gap"
            reps = (Lq + Lk - 1) // Lk
            every = torch.cat([torch.randperm(Lk, generator=g) for _ in range(reps)])[:Lq]     # hits every key when Lq >= Lk
            pi[b, h] = every[torch.randperm(Lq, generator=g)]
            k[b, :, h], q[b, :, h] = 8 * s, 8 * s[pi[b, h]]
            if Lq >= Lk:
                assert len(set(pi[b, h].tolist())) == Lk
    if integer_v:
        v = torch.randint(-8, 9, (B, Lk, H, D), generator=g).float()
    else:
        v = torch.randn(B, Lk, H, D, generator=g)
    q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
    assert is_bf16(8 * torch.ones(1)) and bool((q.abs() == 8).all()) and bool((k.abs() == 8).all())
    # the winner's lead in log2 units: (128 - 64) * 64 * c
    lead = (D - GAP) * 64 * C_LOG2
    assert lead > 149 + 8 + 10 + math.log2(Lk), "family A: the losers must underflow fp32 even under a reference lagging by 8"
    ref = torch.stack([torch.stack([v[b, pi[b, h], h] for h in range(H)], 1) for b in range(B)])      # [B, Lq, H, D]
    return SimpleNamespace(family="selector", q=q, k=k, v=v, pi=pi, ref=ref, keys=None, log2w=None, B=B, H=H, Lq=Lq, Lk=Lk)


# ------------------------------------------------------------------------------------------ family B
@functools.lru_cache(maxsize=None)
def classes_case(B: int, H: int, Lk: int, P: int, seed: int = 0):
    assert 1 <= P <= D
    g = torch.Generator().manual_seed(1_000_003 * seed + 7919 * Lk + 31 * P + 5 * H + B)
    had = hadamard()
    j = torch.arange(Lk)
    k = (8 * had[j % P])[None, :, None, :].expand(B, Lk, H, D).to(torch.bfloat16).contiguous()
    q = (8 * had[:P])[None, :, None, :].expand(B, P, H, D).to(torch.bfloat16).contiguous()
    v = torch.randn(B, Lk, H, D, generator=g).to(torch.bfloat16)
    assert is_bf16(8 * had)
    member = (j[None, :] % P) == torch.arange(P)[:, None]                    # [P, Lk]
    member[~member.any(1)] = True                                           # an empty class ties on every key
    n = member.sum(1)
    want = torch.tensor([len(range(r, Lk, P)) if r < Lk else Lk for r in range(P)])
    assert torch.equal(n, want) and int(n.min()) >= 1, "family B: class sizes"
    w = member.double()
    ref = torch.einsum("rk,bkhd->brhd", w, v.double()) / n.double()[None, :, None, None]
    absacc = torch.einsum("rk,bkhd->brhd", w, v.double().abs())
    return SimpleNamespace(family="classes", q=q, k=k, v=v, ref=ref, n=n, absacc=absacc, keys=None, log2w=None, B=B, H=H, Lq=P, Lk=Lk,
                           P=P)


# ------------------------------------------------------------------------------------------ family C
def _counts(n: int) -> Tensor:
    """n_d = #{j < n : j = d mod 128}"""
    return torch.tensor([len(range(d, n, D)) for d in range(D)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def uniform_case(B: int, H: int, Lq: int, Lk: int, n: Optional[Tuple[int, ...]] = None, same: Optional[Tuple[int, ...]] = None):
    """Without a fold: n, same = None.  With one: per sample b, rows [0, n[b]) are real and row n[b] stands for same[b] rows."""
    t = torch.tensor([1.0, 2.0, 4.0])[torch.arange(Lq) % 3]
    q = (2 * t)[None, :, None, None].expand(B, Lq, H, D).to(torch.bfloat16).contiguous()
    k = torch.full((B, Lk, H, D), -2.0).to(torch.bfloat16)
    gains = torch.tensor([[2.0 ** (1 + b * H + h) for h in range(H)] for b in range(B)], dtype=torch.float64)
    assert gains.unique().numel() == B * H
    v = torch.zeros(B, Lk, H, D, dtype=torch.float64)
    j = torch.arange(Lk)
    for b in range(B):
        for h in range(H):
            v[b, j, h, j % D] = gains[b, h]
    assert is_bf16(q) and is_bf16(k) and is_bf16(v)
    keys = log2w = None
    ref = torch.empty(B, Lq, H, D, dtype=torch.float64)
    for b in range(B):
        if n is None:
            w = _counts(Lk) / Lk
        else:
            assert 0 <= n[b] < Lk - 1 and same[b] >= 2 and len(set(n)) == len(n), "fold: n + 1 rows inside the slab, samples differ"
            w = _counts(n[b])
            w[n[b] % D] += same[b]
            w = w / (n[b] + same[b])
        ref[b] = gains[b][None, :, None] * w[None, None, :]
    if n is not None:
        keys = torch.tensor([x + 1 for x in n], dtype=torch.int32)
        log2w = torch.tensor([math.log2(s) for s in same], dtype=torch.float32)
    return SimpleNamespace(family="uniform", q=q, k=k, v=v.to(torch.bfloat16), ref=ref, keys=keys, log2w=log2w, B=B, H=H, Lq=Lq, Lk=Lk)


def fold_case(slab: int, i: int, Lq: int = UNIFORM_LQ):
    n, same = fold_pairs(slab)[i]
    return uniform_case(2, 2, Lq, slab, n, same)


FRONT, BEHIND = 3, 70          # poisoned rows in front of the window and behind it (more than a whole key tile)


def window(case, poison: str):
    """(k, v): views [B, Lk, H, 128] of rows [FRONT, FRONT + Lk) of larger tensors.  Every other row of those, and rows
    [keys[b], Lk) of the window under a fold, hold the poison."""
    assert poison in POISONS
    B, Lk, H = case.B, case.Lk, case.H
    pk, pv = (16.0, 1024.0) if poison == "dominant" else (float("nan"), float("nan"))
    big_k = torch.full((B, FRONT + Lk + BEHIND, H, D), pk, dtype=torch.bfloat16)
    big_v = torch.full((B, FRONT + Lk + BEHIND, H, D), pv, dtype=torch.bfloat16)
    k, v = big_k[:, FRONT:FRONT + Lk], big_v[:, FRONT:FRONT + Lk]
    for b in range(B):
        lk = Lk if case.keys is None else int(case.keys[b])
        k[b, :lk], v[b, :lk] = case.k[b, :lk], case.v[b, :lk]
    return big_k, big_v


def window_views(big_k: Tensor, big_v: Tensor, Lk: int):
    return big_k[:, FRONT:FRONT + Lk], big_v[:, FRONT:FRONT + Lk]


# ------------------------------------------------------------------------------------------ checkers
@dataclass
class Report:
    what: str
    ok: bool = True
    blamed: List[Tuple[int, int, int]] = field(default_factory=list)       # (batch, head, query row), sorted
    differing: int = 0                                                     # elements that differ from bf16(ref) at all
    worst: float = 0.0                                                     # largest err / tol (inf: outside a zero tolerance)
    failures: List[str] = field(default_factory=list)

    def rows(self, b: int, h: int) -> List[int]:
        return [r for bb, hh, r in self.blamed if (bb, hh) == (b, h)]

    def figures(self) -> str:
        return f"{self.what}: {'ok' if self.ok else 'REJECTED'}, worst err / tol {self.worst:.3f}, {self.differing} elements differ"

    def assert_ok(self):
        assert self.ok, "; ".join(self.failures[:4])


def _report(what: str, out: Tensor, ref: Tensor, tol: Tensor) -> Report:
    """out, ref, tol [B, Lq, H, 128]; an element is bad unless |out - ref| <= tol (a NaN is bad)."""
    o = out.double()
    err = (o - ref.double()).abs()
    bad = ~(err <= tol)
    rep = Report(what)
    rep.differing = int((o != ref.double().to(torch.bfloat16).double()).sum())
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    rep.worst = float(ratio.max())
    if bool(bad.any()):
        rep.ok = False
        rows = bad.any(-1).permute(0, 2, 1).nonzero()                       # (b, h, row)
        rep.blamed = sorted(tuple(int(x) for x in r) for r in rows)
        b, i, h, d = (int(x) for x in bad.nonzero()[0])
        rep.failures.append(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound in {len(rep.blamed)} rows, first at batch {b} "
                            f"head {h} row {i} d {d}: out {float(o[b, i, h, d])} ref {float(ref[b, i, h, d])} tol {float(tol[b, i, h, d])}")
    return rep


def check_selector(out: Tensor, case, structure: str, ref: Optional[Tensor] = None) -> Report:
    """Family A.  w4 / w8: bit equality with V[pi]; r64 / auto: |out - V| <= 2^-7 |V| (module docstring)."""
    ref = case.ref if ref is None else ref
    tol = torch.zeros(ref.shape, dtype=torch.float64) if structure in ("w4", "w8") else 2.0 ** -7 * ref.double().abs()
    rep = _report(f"selector[{structure} B={case.B} H={case.H} Lq={case.Lq} Lk={case.Lk}]", out, ref, tol)
    if structure in ("w4", "w8") and rep.ok and not torch.equal(out.view(torch.int16), ref.view(torch.int16)):      # -0 against +0
        rep.ok = False
        rep.failures.append(rep.what + ": equal values, different bits")
    return rep


def check_classes(out: Tensor, case, structure: str) -> Report:
    """Family B.  REL[structure] |ref| + n 2^-22 A (module docstring)."""
    tol = REL[structure] * case.ref.abs() + case.n.double()[None, :, None, None] * 2.0 ** -22 * case.absacc
    return _report(f"classes[{structure} Lk={case.Lk} P={case.P}]", out, case.ref, tol)


def check_uniform(out: Tensor, case, structure: str = "") -> Report:
    """Family C.  2^-6 relative for every structure; where the reference is 0 only 0 passes; a NaN or inf never does."""
    what = f"uniform[{structure} Lk={case.Lk}" + ("" if case.keys is None else f" keys={case.keys.tolist()}") + "]"
    return _report(what, out, case.ref, UNIFORM_REL * case.ref.abs())


# ------------------------------------------------------------------------------------------ the tiled emulation
DEFECTS = ("drop_last_key", "unmasked_pad", "swap_v", "skip_tile", "double_tile", "stale_v", "wrong_head", "read_row_lk",
           "fold_on_next", "ragged_to_last")
NEG = -1e30


def _bf16_round(x: Tensor) -> Tensor:
    return x.float().to(torch.bfloat16).double()


def _f32_underflow(x: Tensor) -> Tensor:
    """The kernels' probabilities are fp32: below half of the smallest subnormal, 2^-149, they are exactly 0."""
    return torch.where(x < 2.0 ** -150, torch.zeros_like(x), x)


def _emulate_head(q, k, v, lk, wl, bf16_p, lazy, defect, arg, behind):
    """q [Lq, 128], k / v [>= lk, 128] float64 -> O / l [Lq, 128] float64."""
    Lq = q.shape[0]
    nt = (lk + KT - 1) // KT
    kk, vv = torch.zeros(nt * KT, D, dtype=torch.float64), torch.zeros(nt * KT, D, dtype=torch.float64)
    kk[:lk], vv[:lk] = k[:lk], v[:lk]
    valid = torch.arange(nt * KT) < lk
    wrow = lk - 1
    if defect == "drop_last_key":
        valid[lk - 1] = False
    elif defect == "unmasked_pad" and lk < nt * KT:          # the zero K / V row at index lk counts as a key
        valid[lk] = True
    elif defect == "read_row_lk" and lk < nt * KT:           # ... and it is not zero: the row behind the window
        valid[lk] = True
        kk[lk], vv[lk] = behind[0], behind[1]
    elif defect == "swap_v":
        t, a, b = arg
        vv[[KT * t + a, KT * t + b]] = vv[[KT * t + b, KT * t + a]]
    elif defect == "fold_on_next":
        wrow = lk                                            # a masked row, or the first of the next tile that is never walked
    order = list(range(nt))
    if defect == "skip_tile":
        order.remove(arg)
    elif defect == "double_tile":
        order.insert(arg, arg)
    m = torch.full((Lq,), NEG, dtype=torch.float64)
    l = torch.zeros(Lq, dtype=torch.float64)
    o = torch.zeros(Lq, D, dtype=torch.float64)
    for t in order:
        sl = slice(KT * t, KT * t + KT)
        vt = vv[KT * (t - 3):KT * (t - 2)] if defect == "stale_v" and t == arg else vv[sl]
        s = (q @ kk[sl].T) * C_LOG2
        if wl != 0.0 and sl.start <= wrow < sl.stop:
            s[:, wrow - sl.start] += wl
        s[:, ~valid[sl]] = NEG
        mx = s.max(1).values
        m_new = torch.where(mx > m + 8, mx, m) if lazy else torch.maximum(m, mx)
        alpha = _f32_underflow(torch.exp2(m - m_new))
        l, o, m = l * alpha, o * alpha[:, None], m_new
        p = _f32_underflow(torch.exp2(s - m[:, None]))
        l = l + p.sum(1)
        o = o + (_bf16_round(p) if bf16_p else p) @ vt
    return o / l[:, None]


def emulate(q: Tensor, k: Tensor, v: Tensor, keys=None, log2w=None, bf16_p: bool = False, lazy: bool = False,
            defect: Optional[str] = None, arg=None, behind=None, accum: Optional[Tensor] = None, rows: int = 128) -> Tensor:
    """Tiled float64 attention of bf16 [B, L, H, 128] tensors -> bf16 [B, Lq, H, 128].
    bf16_p: P rounded to bf16 before P.V (l sums the unrounded p, as the kernels do).  lazy: r64's reference.
    accum: bf16 [B, Lq, H, 128], out = bf16(accum + O / l).  rows: query rows per workgroup (ragged_to_last only).
    defect (one of DEFECTS) / arg:
      drop_last_key    key lk - 1 masked
      unmasked_pad     the zero K / V row at index lk of the last tile attended (nothing when lk fills its tile)
      swap_v           arg = (tile, a, b): V rows a and b of that tile exchanged, K left alone
      skip_tile        arg = tile
      double_tile      arg = tile
      stale_v          arg = tile t >= 3: that tile reads the V rows of tile t - 3 (a V ring of 3, one slot late)
      wrong_head       K and V of head (h + 1) % H
      read_row_lk      behind = (k_row, v_row) [B, H, 128]: the row behind the window attended as key lk
      fold_on_next     log2w lands on row keys[b] (masked, or never walked) instead of keys[b] - 1
      ragged_to_last   a workgroup's rows past Lq (their Q read as zero) are stored to row Lq - 1"""
    assert defect is None or defect in DEFECTS
    B, Lq, H, _ = q.shape
    out = torch.empty(B, Lq, H, D, dtype=torch.float64)
    for b in range(B):
        lk = k.shape[1] if keys is None else min(max(int(keys[b]), 1), k.shape[1])
        wl = 0.0 if log2w is None else float(log2w[b])
        for h in range(H):
            hs = (h + 1) % H if defect == "wrong_head" else h
            bh = None if behind is None else (behind[0][b, hs].double(), behind[1][b, hs].double())
            qh = q[b, :, h].double()
            if defect == "ragged_to_last" and Lq % rows:
                qh = torch.cat([qh, torch.zeros(1, D, dtype=torch.float64)])
            o = _emulate_head(qh, k[b, :, hs].double(), v[b, :, hs].double(), lk, wl, bf16_p, lazy, defect, arg, bh)
            if o.shape[0] > Lq:
                o = torch.cat([o[:Lq - 1], o[Lq:]])
            out[b, :, h] = o
    if accum is not None:
        out = accum.double() + out
    return out.to(torch.bfloat16)


EMULATED = {"w4": dict(bf16_p=True, lazy=False), "w8": dict(bf16_p=True, lazy=False), "r64": dict(bf16_p=True, lazy=True),
            "auto": dict(bf16_p=True, lazy=True)}
