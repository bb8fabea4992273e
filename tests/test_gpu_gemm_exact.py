"""GPU tests of the three GEMM kernels and five tilings of csrc/gemm_bf16.hip (t128; pp256 / pp224 / pp192; pp128), both
epilogue forms and the bf16 and fp8 operand paths on inputs whose exact answer is known in closed form
(oracle/gemm_cases.py).  Run with `-m gpu`.

Every comparison is EQUALITY on every element (as values: -0 equals +0, a NaN equals nothing), no element is exempt and no
bound is taken from what the kernels give.  The families, and why each is exact in fp32 in any accumulation order, are in
the oracle's docstring; in short:

  S  A one-hot at sigma(m), W random bf16 (e4m3 for fp8): out[m, n] = W[n, sigma(m)].  Every k, every row.
  T  W one-hot at tau(n), A random: out[m, n] = A[m, tau(n)].  Every k, every column.
  D  integers in {-2 .. 2}: out = A W^T, the sum across all k-tiles; >= 99 % of the products are within the 256 that
     bf16 holds exactly (asserted per shape in tests/test_gemm_cases_host.py).
  Epilogues: integer bias and residual, a gate that is an exact small integer naming its group (powers of two for D),
  fp8 scales that are powers of two per row segment and per column: (y sa sw + bias) gate + resid, rounded once.
  GELU (S and T only) is the one bound: |out - ref| <= 2^-8 |ref| + 4 e, e = the largest |gelu_fp32 - gelu_fp64| of torch's
  CPU tanh-GELU over the case's own y, measured inside the test and printed; 4 stands for the kernel's fast exp2 and rcp.

Every operand is a window of a NaN-filled parent (lda = K + 64, ldw = K + 8, ldr = N + 4, every vector followed by NaN)
and every output lives in a NaN-patterned canary (ldo = N + 8, or N + 4 for the direct epilogue): everything outside the
M x N window must be untouched and a tile nobody wrote fails the equality.  fp8 launches go through sf_gemm_fp8's C ABI so
that their outputs sit in a canary too.

tests/test_gemm_cases_host.py shows on the CPU which defect each test below stands guard against (named in the
docstrings here) and which rows and columns it would blame.  The number of elements compared is printed per test (`-s`)."""
import pytest
import torch

from oracle import gemm_cases as gc
from self_forcing_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI = {"none": _lib.EPI_BIAS, "bias": _lib.EPI_BIAS, "gelu": _lib.EPI_BIAS_GELU, "resid": _lib.EPI_BIAS_RESID,
       "gate_resid": _lib.EPI_BIAS_GATE_RESID}
DTYPES = pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
FORCED = pytest.mark.parametrize("structure", gc.STRUCTURES)
COMPARED = {}


@pytest.fixture(autouse=True)
def compared(request):
    COMPARED[request.node.name] = 0
    yield
    print(f"\n{request.node.name}: {COMPARED[request.node.name]} elements compared")


def dev(case):
    """The case's parents on the device, moved once -> pointers of the windows."""
    if not hasattr(case, "dev"):
        case.dev, case.ptr = {}, {}
        for name in ("a", "w", "bias", "resid", "gate_mod", "gate_e0", "a_scale", "w_scale"):
            parent, view = getattr(case, name + "_parent"), getattr(case, name)
            if parent is not None:
                case.dev[name] = parent.to(DEV)
                case.ptr[name] = case.dev[name].data_ptr() + view.storage_offset() * view.element_size()
    return case.ptr


def launch(case, structure, inplace=False):
    """One launch through the C ABI into a fresh canary -> the canary."""
    ptr = dev(case)
    can = gc.new_canary(case, DEV, inplace)
    g = _lib.GemmArgs()
    g.a, g.w, g.out, g.bias = ptr["a"], ptr["w"], can.ptr(), ptr.get("bias")
    g.resid, g.ldr = (can.ptr(), case.ldo) if inplace else (ptr.get("resid"), case.ldr)
    g.gate_mod, g.gate_e0, g.gate_group_stride, g.rows_per_group = ptr.get("gate_mod"), ptr.get("gate_e0"), case.N + 4, case.rpg
    g.M, g.N, g.K, g.lda, g.ldw, g.ldo = case.M, case.N, case.K, case.lda, case.ldw, case.ldo
    g.epilogue, g.batch, g.structure = EPI[case.epi], 0, _lib.GEMM_STRUCTURES[structure]
    stream = torch.cuda.current_stream().cuda_stream
    if case.fp8:
        rc = _lib.lib().sf_gemm_fp8(g, ptr["a_scale"], case.rps, ptr["w_scale"], stream)
    else:
        rc = _lib.lib().sf_gemm_bf16(g, stream)
    torch.cuda.synchronize()
    assert rc == 0, (_lib.lib().sf_last_error() or b"").decode()
    return can


def run(request, case, structure, inplace=False, extra=None):
    can = launch(case, structure, inplace)
    rep = gc.check(case, can, structure, extra)
    COMPARED[request.node.name] += rep.compared
    rep.assert_ok()
    return can


# ------------------------------------------------------------------------------------------ every k
@DTYPES
@FORCED
def test_every_k(request, structure, fp8):
    """S (M = K + 70) and T (M = 200) at N = 264 and 1 .. 7 and 24 k-tiles: every k is some row's (column's) only source, in
    every lane and chunk of a k-tile and every slot of the double buffer and of the ring of three; 2 and 3 k-tiles take the
    prologue and the more1 / more2 tails.  Guards against skip_ktile, double_ktile, stale_slot_a, stale_slot_w, k_mispair
    and wrong_half.  With one k-tile a forced ping-pong structure falls back to t128: same bits."""
    for case in gc.every_k_cases(fp8):
        can = run(request, case, structure)
        if case.K == gc.kt_elems(fp8):
            assert gc.resolve_structure(structure, case.M, case.N, case.K, fp8) == "t128"
            assert torch.equal(can.raw, launch(case, "t128").raw), f"{structure} with one k-tile is not the 128 x 128 kernel"


# ------------------------------------------------------------------------------------------ every row edge
@DTYPES
@FORCED
def test_every_row_edge(request, structure, fp8):
    """S with resid and gate_resid, rows_per_group = 1 (fp8: rows_per_segment = 1 too), N = 264, two k-tiles, M across each
    tiling's tile height, half height and 16-row block: every row has a residual, a gate and a scale of its own.  Guards
    against ragged_row_to_last, drop_last_row, wrong_half, gate_group_of_block and scale_segment_of_block."""
    for case in gc.row_edge_cases(fp8):
        run(request, case, structure)


# ------------------------------------------------------------------------------------------ every column edge
@DTYPES
@FORCED
@pytest.mark.parametrize("form", ["lds", "direct"])
def test_every_column_edge(request, form, structure, fp8):
    """T with bias and gate_resid (rows_per_group = 37), M = 258, two k-tiles: N % 8 == 0 through the LDS epilogue
    (ldo = N + 8), N % 8 == 4 through the direct one (ldo = N + 4); every column has its own source k, bias, gate and
    w_scale.  Guards against col_clamp_off, epilogue_swizzle, resid_ld and a column tile dropped or written past N."""
    for case in gc.column_edge_cases(fp8, form):
        assert case.lds_epilogue == (form == "lds")
        run(request, case, structure)


# ------------------------------------------------------------------------------------------ groups and segments
@DTYPES
@FORCED
def test_groups_and_segments(request, structure, fp8):
    """S at (300, 264, two k-tiles): bias, resid and gate_resid with every rows_per_group, for fp8 under every
    rows_per_segment; the boundaries fall inside 16-row blocks and the last group is partial.  Guards against
    gate_group_of_block and scale_segment_of_block.  GELU on S and T meets 2^-8 |ref| + 4 e, e measured here from torch's CPU
    tanh-GELU over the case's own y and printed."""
    for case in gc.group_cases(fp8):
        run(request, case, structure)
    for case in gc.group_cases(fp8, gelu=True):
        e = gc.gelu_fp32_error(case)
        if structure == "t128":
            print(f"\ngelu allowance, {case.family}{'/fp8' if fp8 else ''} rps={case.rps}: 4 x {e:.3e}, |y| <= {float((case.y + case.bias.double()).abs().max()):.1f}")
        run(request, case, structure, extra=4 * e)


# ------------------------------------------------------------------------------------------ sums
@DTYPES
@FORCED
def test_sums_across_k_tiles(request, structure, fp8):
    """D at (300, 264, 2 k-tiles), (518, 264, 7) and (1606, 264, 24) without an epilogue and with bias, resid and gate_resid
    (rows_per_group = 37, fp8: rows_per_segment = (M + 1) // 2): every k-tile contributes to every element.  Guards against
    skip_ktile, double_ktile and stale_slot_a / _w in the rows and columns whose selected k lies in another k-tile, where
    S and T cannot see them."""
    for case in gc.sum_cases(fp8):
        run(request, case, structure)


# ------------------------------------------------------------------------------------------ the workgroup-to-tile map
@DTYPES
@FORCED
def test_tile_map(request, structure, fp8):
    """S at two k-tiles with (M, N) in {(1300, 264), (1300, 776), (2100, 520)}: tiles_m is no multiple of GROUP_M, the
    workgroup count no multiple of 8 and the last group partial.  Guards against tile_twice: a tile taken twice leaves
    another one holding the canary's pattern, a tile placed elsewhere shows in its rows and columns."""
    for case in gc.map_cases(fp8):
        run(request, case, structure)


@DTYPES
def test_automatic_dispatch(request, fp8):
    """(1100, 1032, 8 k-tiles) is past auto's threshold: it takes a ping-pong structure.  S and D with a residual."""
    for case in gc.auto_cases(fp8):
        assert gc.resolve_structure("auto", case.M, case.N, case.K, fp8) != "t128"
        run(request, case, "auto")


# ------------------------------------------------------------------------------------------ in place
@DTYPES
@FORCED
def test_residual_aliasing_the_output(request, structure, fp8):
    """S at (300, 264, two k-tiles), resid and gate_resid, the residual read from the output window itself (ldr = ldo): every
    element is read before it is overwritten, by the workgroup that owns it.  The spare columns keep the pattern."""
    for case in gc.inplace_cases(fp8):
        run(request, case, structure, inplace=True)
