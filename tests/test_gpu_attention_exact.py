"""GPU tests of the three attention kernels (w4, w8, r64; csrc/attention.hip), the folded-key path and the accumulate
epilogue on inputs whose exact answer is known in closed form (oracle/attention_cases.py).  Run with `-m gpu`.

Every comparison is elementwise, no element is exempt, and no bound is taken from what the kernels give.  The three input
families, their closed forms and the derivation of each bound are in the oracle's docstring; in short, with c =
log2(e) / sqrt(128):

  A selector  k_j = 8 s_j, q_i = 8 s_pi(i), codes s in {+-1}^128 at most 64 apart: the winner leads by >= 64 * 64 * c ~ 522
              log2 units, every other probability is exactly 0 in fp32.  out[i] = V[pi(i)].
              w4 / w8: BIT EQUALITY (p = exp2(residual <= 2^-13) rounds to bf16 1, l = p, V / l moves V by < 2^-12
              relative and rounds back).  r64, auto: |out - V| <= 2^-7 |V| (P = exp2(delta), delta in [0, 8], rounded to
              bf16 before P.V: less than one bf16 step before the final rounding).
  B classes   k_j = 8 h_{j mod P}, q_r = 8 h_r, Hadamard rows: members tie at 8192 c, the rest weigh exp2(-1044) = 0.
              out[r] = the float64 mean of V over the class (n rows, A = sum |V|).
              w4 / w8: 2^-8 |ref| + n 2^-22 A (one bf16 rounding + order-free fp32 accumulation, as
              tests/test_gpu_gemm_batched.py); r64, auto: 2^-7 |ref| + n 2^-22 A (bf16 P).
  C uniform   k_j = -2 h_0, q_i = 2 t_i h_0: all keys tie.  V[j, d] = g [d = j mod 128]: out[i, d] = g n_d / Lk, exactly 0
              where no key has that residue; with a fold, g (n_d(n) + same [d = n]) / (n + same).  2^-6 relative for every
              structure (bf16 P, one reciprocal, the final rounding, Lk 2^-24 for l).  Windowed: every row around the
              attended ones holds poison that would take all the weight ("dominant") or show if read at all ("nan").

tests/test_attention_cases_host.py shows on the CPU that a kernel which drops the last key, leaves a padded key unmasked,
swaps two V rows, skips or repeats a tile, reads a stale ring slot, the wrong head's slab or the row behind the window,
misplaces the fold weight or stores a ragged row to row Lq - 1 fails these tests, and which rows they would blame.

The number of r64 elements that differ from V at all in family A is printed (`-s`) by test_every_key_position."""
import pytest
import torch

from oracle import attention_cases as ac
from self_forcing_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512                                    # bf16 elements in front of and behind a canaried output (keeps 16-byte alignment)
FILL = 0x7FA5                                  # a quiet bf16 NaN with a payload, as int16
FORCED = ac.STRUCTURES
R64_DIFFERING = {"elements": 0, "of": 0}


@pytest.fixture(scope="module", autouse=True)
def r64_differing_total():
    yield
    print(f"\nfamily A, whole file: {R64_DIFFERING['elements']} of {R64_DIFFERING['of']} r64 elements differ from V")


def dev(case):
    """The case's q, k, v on the device, moved once."""
    if not hasattr(case, "dev"):
        case.dev = tuple(t.to(DEV) for t in (case.q, case.k, case.v))
        case.dev_fold = (None, None) if case.keys is None else (case.keys.to(DEV), case.log2w.to(DEV))
    return case.dev


def attend(case, structure, k=None, v=None):
    q, ck, cv = dev(case)
    out = ops.attention(q, ck if k is None else k, cv if v is None else v, structure=structure, keys=case.dev_fold[0], log2w=case.dev_fold[1])
    return out.cpu()


def run_selector(case, structures=FORCED):
    for structure in structures:
        rep = ac.check_selector(attend(case, structure), case, structure)
        if structure == "r64":
            R64_DIFFERING["elements"] += rep.differing
            R64_DIFFERING["of"] += case.ref.numel()
        rep.assert_ok()


# ------------------------------------------------------------------------------------------ 1, 2: every key, every query edge
@pytest.mark.parametrize("Lk", ac.EVERY_KEY_LK)
def test_every_key_position(Lk):
    """Family A, Lq = Lk + 70: every key is some query's only target, in every slot of full and ragged tiles; 1025 and 1100
    take the `Lk > 1024` kernel symbols; 832 and above wrap r64's K ring of 4 and V ring of 3 through all 12 phase pairs."""
    run_selector(ac.selector_case(2, 2, Lk + 70, Lk))
    print(f"\nr64 elements that differ from V so far: {R64_DIFFERING['elements']} of {R64_DIFFERING['of']}")


@pytest.mark.parametrize("Lq", ac.QUERY_EDGE_LQ)
def test_every_query_edge(Lq):
    """Family A, Lk = 129: every row has its own target, so a ragged row stored through a clamped address shows as a wrong
    last row, and a wave or workgroup that takes another's rows shows in those rows."""
    run_selector(ac.selector_case(2, 2, Lq, ac.QUERY_EDGE_LK))


# ------------------------------------------------------------------------------------------ 3: ties across tiles
@pytest.mark.parametrize("P", ac.TIE_P)
@pytest.mark.parametrize("Lk", ac.TIE_LK)
def test_ties_across_tiles(Lk, P):
    """Family B: a query's keys tie exactly, one or none per tile; a dropped, doubled or stale member moves the mean by
    O(1 / n) of a Gaussian row, n <= 18 (65 for the queries without a member at Lk = 65: they average every key)."""
    case = ac.classes_case(2, 2, Lk, P)
    for structure in FORCED:
        rep = ac.check_classes(attend(case, structure), case, structure)
        print("\n" + rep.figures())
        rep.assert_ok()


# ------------------------------------------------------------------------------------------ 4: mask, counts, fold, poison
@pytest.mark.parametrize("poison", ac.POISONS)
@pytest.mark.parametrize("Lk", ac.UNIFORM_LK)
def test_mask_and_counts_inside_a_poisoned_window(Lk, poison):
    """Family C, the slab a window of a larger tensor of the test's own whose other rows are poison."""
    case = ac.uniform_case(2, 2, ac.UNIFORM_LQ, Lk)
    big_k, big_v = (t.to(DEV) for t in ac.window(case, poison))
    k, v = ac.window_views(big_k, big_v, Lk)
    for structure in FORCED + ("auto",):
        ac.check_uniform(attend(case, structure, k, v), case, structure).assert_ok()


@pytest.mark.parametrize("poison", ac.POISONS)
@pytest.mark.parametrize("slab", ac.FOLD_SLABS)
def test_fold_inside_a_poisoned_window(slab, poison):
    """Family C with keys[b] = n + 1 and log2w[b] = log2(same): n in {0, 1, 62, 63, 64, 127, 200} below slab - 1, the two
    samples always with different n and different same; rows [keys[b], slab) and the rows around the window are poison."""
    for i in range(len(ac.fold_pairs(slab))):
        case = ac.fold_case(slab, i)
        big_k, big_v = (t.to(DEV) for t in ac.window(case, poison))
        k, v = ac.window_views(big_k, big_v, slab)
        for structure in FORCED + ("auto",):
            ac.check_uniform(attend(case, structure, k, v), case, structure).assert_ok()


# ------------------------------------------------------------------------------------------ 5: workgroup maps
@pytest.mark.parametrize("B,H,Lq", ac.MAP_CASES)
def test_workgroup_maps(B, H, Lq):
    """Family A, Lk = 65, every (batch, head) with its own codes, values and targets: a workgroup that works on another's
    (batch, head, query tile), or a tile nobody works on, shows in those rows.  The grids take every residue mod 8 for w4
    (sf_xcd_remap) and for w8 / r64; the branches of attention_r64_kernel's map each case reaches are listed at
    oracle.attention_cases.MAP_CASES and asserted in tests/test_attention_cases_host.py."""
    run_selector(ac.selector_case(B, H, Lq, ac.MAP_LK))


# ------------------------------------------------------------------------------------------ 6: stores
class Canary:
    """`n` bf16 output elements between two guard bands, all pre-filled with the NaN pattern."""

    def __init__(self, n):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int16, device=DEV)
        self.region = self.raw[GUARD:GUARD + n].view(torch.bfloat16)

    def assert_untouched_outside(self, owned):
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == FILL).all()), "guard band in front of the output was written"
        assert bool((raw[GUARD + self.n:] == FILL).all()), "guard band behind the output was written"
        stray = (raw[GUARD:GUARD + self.n] != FILL) & ~owned
        assert not bool(stray.any()), f"{int(stray.sum())} elements outside the output were written, first at {int(stray.nonzero()[0])}"


def launch_into_canary(case, structure, pitch):
    """sf_attention through the C ABI into rows of `pitch` elements, batches two spare rows apart -> (rc, out, canary, owned)."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    q, k, v = dev(case)
    o_bs = (Lq + 2) * pitch
    can = Canary(B * o_bs)
    a = _lib.AttentionArgs(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), out=can.region.data_ptr(), B=B, H=H, Lq=Lq, Lk=Lk,
                           q_stride=H * 128, q_bstride=Lq * H * 128, kv_stride=H * 128, kv_bstride=Lk * H * 128, o_stride=pitch,
                           o_bstride=o_bs, structure=_lib.ATTN_STRUCTURES[structure])
    rc = _lib.lib().sf_attention(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    owned = torch.zeros(B * o_bs, dtype=torch.bool)
    torch.as_strided(owned, (B, Lq, H * 128), (o_bs, pitch, 1)).fill_(True)
    out = torch.as_strided(can.region.cpu(), (B, Lq, H, 128), (o_bs, pitch, 128, 1)).contiguous()
    return rc, out, can, owned


@pytest.mark.parametrize("Lq", ac.STORE_LQ)
def test_stores_stay_inside_their_rows(Lq):
    """Family A into a canaried buffer: row pitch H * 128 + 8, batch stride with two spare rows.  Owned elements meet A's
    bounds; the 8 spare columns of every row, the spare rows, and the guard bands keep the fill bit for bit."""
    case = ac.selector_case(2, 2, Lq, ac.STORE_LK)
    for structure in FORCED + ("auto",):
        rc, out, can, owned = launch_into_canary(case, structure, 2 * 128 + 8)
        assert rc == 0, (_lib.lib().sf_last_error() or b"").decode()
        can.assert_untouched_outside(owned)
        ac.check_selector(out, case, structure).assert_ok()


@pytest.mark.parametrize("Lq", ac.STORE_LQ)
def test_stores_into_rows_that_are_only_8_byte_aligned(Lq):
    """Row pitch H * 128 + 4: w4, w8 and auto take the narrow 8-byte stores; forced r64 refuses and writes nothing."""
    case = ac.selector_case(2, 2, Lq, ac.STORE_LK)
    for structure in ("w4", "w8", "auto"):
        rc, out, can, owned = launch_into_canary(case, structure, 2 * 128 + 4)
        assert rc == 0, (_lib.lib().sf_last_error() or b"").decode()
        can.assert_untouched_outside(owned)
        ac.check_selector(out, case, structure).assert_ok()
    rc, _, can, owned = launch_into_canary(case, "r64", 2 * 128 + 4)
    assert rc != 0 and "16-byte aligned output rows" in (_lib.lib().sf_last_error() or b"").decode()
    can.assert_untouched_outside(torch.zeros_like(owned))


# ------------------------------------------------------------------------------------------ 7: accumulate
@pytest.mark.parametrize("Lk", ac.ACCUM_LK)
def test_accumulate_is_exact_on_integers(Lk):
    """Family A with integer V in [-8, 8], `out` pre-filled with integers R in [-8, 8] between two sentinel rows per sample:
    the result is bit equal to bf16(R + V[pi]) (p = 1, l = 1, an integer sum of magnitude <= 16), the sentinels untouched."""
    case = ac.selector_case(2, 2, ac.ACCUM_LQ, Lk, integer_v=True)
    q, k, v = dev(case)
    r = torch.randint(-8, 9, case.ref.shape, generator=torch.Generator().manual_seed(Lk)).to(torch.bfloat16)
    want = (r.double() + case.ref.double()).to(torch.bfloat16)
    for structure in ("w4", "w8", "auto"):
        big = torch.full((2, ac.ACCUM_LQ + 2, 2, 128), FILL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        out = big[:, 1:-1]
        out.copy_(r)
        assert ops.attention_accum(q, k, v, out, structure=structure) is out
        host = big.cpu()
        assert bool((host[:, 0].view(torch.int16) == FILL).all()) and bool((host[:, -1].view(torch.int16) == FILL).all()), "sentinel rows"
        ac.check_selector(host[:, 1:-1], case, "w4", ref=want).assert_ok()


# ------------------------------------------------------------------------------------------ 8: auto at its thresholds
@pytest.mark.parametrize("B,H,Lq,Lk", ac.THRESHOLD_CASES)
def test_auto_on_both_sides_of_its_thresholds(B, H, Lq, Lk):
    """192 workgroups of 256 rows and 512 keys are where auto moves to r64, 192 workgroups where it moves from w4 to w8:
    B * H = 192 against 188, Lk = 512 against 511.  Every side meets the r64 bound of family A."""
    case = ac.selector_case(B, H, Lq, Lk)
    ac.check_selector(attend(case, "auto"), case, "r64").assert_ok()
