"""GPU tests of sf_conv_igemm in every form production launches -- the implicit GEMM of csrc/conv_igemm.hip at every column
tile and both epilogues, the halo-tile kernel of csrc/conv_halo.hip at both widths, with and without its fused
RMS_norm + SiLU output, and the float head -- and of sf_rmsnorm_silu_cl at every lanes-per-row instantiation.
Run with `-m gpu`.

Every comparison is elementwise against float64 computed on the host from the same bf16 inputs (oracle/conv_oracle.py,
which states the data families, the bounds and where they come from; tests/test_conv_kernels_host.py shows that those
checkers pass a correct fp32 implementation and reject ten wrong ones).  Integer family: the bf16 output equals one
round-to-nearest-even of the exact value bit for bit, the float head exactly.  Gaussian family and the norm: the stated
bounds, at every element.  The worst err / tol of every launch is printed (`pytest -s`), never used.

Every launch is built as _lib.ConvArgs by hand, so that ldo > Cout, ldr != ldo, frame offsets, resid aliasing out, a NULL
out and the norm fields are reachable.  Every output lives in a canary buffer (NaN pattern, guard bands, one foreign frame
behind the volume and `out_frame_offset` in front): what a launch does not own must keep the pattern.  Input frames a
launch must not read and the weight columns behind roundup(K, 64) hold NaN.

Measured on an MI355X (worst err / tol; reported, no bound was set from them).  Integer family: every launch bit-equal,
halo = implicit GEMM = AUTO bit for bit.  Gaussian family: 0.753 (halo96_ragged, both structures), 0.512 (halo192_both),
0.711 (ig_cout100), which is the final rounding: the fp32 emulation on the host gives the same three figures; 0.944 on the
13.8 M elements of the Gaussian halo384 launch (the emulation's figure too: a rounding can take 0.996 of the bound); the float head 7.8e-5 (halo) and
5.8e-5 (implicit GEMM).  Fused norm 0.995 - 0.996 and sf_rmsnorm_silu_cl 0.978 - 0.996, again the
final rounding (1 / (1 + 2^-8)); the fused norm and sf_rmsnorm_silu_cl(out) agree in every bit of every case.  No launch
wrote outside what it owns."""
import dataclasses
import functools

import pytest
import torch

from oracle import conv_oracle as co
from self_forcing_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
EPI = {"bias": _lib.CONV_BIAS, "resid": _lib.CONV_BIAS_RESID, "clamp": _lib.CONV_BIAS_CLAMP_F32}


def stream():
    return torch.cuda.current_stream().cuda_stream


def last_error():
    return (_lib.lib().sf_last_error() or b"").decode()


@functools.lru_cache(maxsize=4)
def device_data(c):
    d = co.make_data(c)
    return d, {k: (None if v is None else v.to(DEV)) for k, v in vars(d).items()}


@functools.lru_cache(maxsize=4)
def reference(c):
    """Shared by the launches of one case (the structure is not part of the reference)."""
    return co.conv_reference(c, device_data(c)[0], absacc=c.family == "gauss")


def make_buffers(c, dd):
    bufs = {}
    if c.epilogue == "clamp":
        bufs["out_f32"] = co.Canary(c.out_shape, torch.float32, DEV)
    elif not c.out_null:
        bufs["out"] = co.Canary(c.out_shape, BF16, DEV)
        if c.resid_alias:
            f0 = c.out_frame_offset
            bufs["out"].region[f0:f0 + c.T, :, :, :c.Cout] = dd["resid"][f0:f0 + c.T, :, :, :c.Cout]
    if c.norm:
        bufs["norm_out"] = co.Canary(c.norm_shape, BF16, DEV)
    return bufs


def conv_args(c, dd, bufs, structure):
    a = _lib.ConvArgs()
    a.x, a.w, a.bias = dd["x"].data_ptr(), dd["w"].data_ptr(), dd["bias"].data_ptr()
    a.out = bufs["out"].ptr() if "out" in bufs else None
    a.out_f32 = bufs["out_f32"].ptr() if "out_f32" in bufs else None
    if c.epilogue == "resid":
        a.resid, a.ldr = (bufs["out"].ptr() if c.resid_alias else dd["resid"].data_ptr()), c.ldr_
    a.Tout, a.H, a.W, a.Hin, a.Win, a.Cin, a.Cout = c.T, c.H, c.W, c.Hin, c.Win, c.Cin, c.Cout
    a.kt, a.kh, a.kw, a.upsample, a.t_in_offset = c.kt, c.ks, c.ks, int(c.upsample), c.t_in_offset
    a.ldw, a.ldo, a.out_frame_offset = c.ldw, (0 if c.epilogue == "clamp" else c.ldo_), c.out_frame_offset
    a.interleave_c = c.Cout // 2 if c.interleave else 0
    a.epilogue, a.structure = EPI[c.epilogue], _lib.CONV_STRUCTURES[structure]
    if "norm_out" in bufs:
        a.norm_out, a.norm_gamma, a.norm_ld, a.norm_frame_offset = bufs["norm_out"].ptr(), dd["gamma"].data_ptr(), c.norm_ld_, c.norm_frame_offset
    a.stride_hw, a.stride_t = c.stride_hw, c.stride_t
    return a


def launch(c, dd, bufs, structure):
    rc = _lib.lib().sf_conv_igemm(conv_args(c, dd, bufs, structure), stream())
    torch.cuda.synchronize()
    return rc


def owned_of(c, name):
    return co.norm_owned_mask(c) if name == "norm_out" else co.owned_mask(c)


@functools.lru_cache(maxsize=None)
def run(c, structure):
    """Launch case c through `structure`, check every canary, return the host copies {"out" | "out_f32", "norm_out"}."""
    _, dd = device_data(c)
    bufs = make_buffers(c, dd)
    assert launch(c, dd, bufs, structure) == 0, last_error()
    for name, can in bufs.items():
        can.assert_untouched_outside(owned_of(c, name), f"{c.name} via {structure}: {name}")
    return {name: can.host() for name, can in bufs.items()}


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(co.INT[a.dtype]), b.view(co.INT[b.dtype]))


def rmsnorm_launch(x_ptr, gamma, out_ptr, rows, C, silu):
    rc = _lib.lib().sf_rmsnorm_silu_cl(x_ptr, gamma.data_ptr(), out_ptr, rows, C, int(silu), stream())
    torch.cuda.synchronize()
    return rc


def check_against_auto(c, res):
    """AUTO reaches the structure the dispatch mirror predicts: the same bits as forcing it."""
    predicted = "igemm" if co.dispatch(c, "auto")[0] == "igemm" else "halo"
    auto, forced = run(c, "auto"), (res if predicted == c.structure else run(c, predicted))
    for name in forced:
        assert same_bits(auto[name], forced[name]), f"{c.name}: AUTO differs from {predicted} in {name}"


def igemm_twin(c):
    """The case of IGEMM_CASES that is halo case c without the norm."""
    want = dataclasses.replace(c, name="", structure="igemm", norm=False, norm_ld=0, norm_frame_offset=0, out_null=False)
    return next(t for t in co.IGEMM_CASES if dataclasses.replace(t, name="") == want)


# ------------------------------------------------------------------------------------------ the halo structure
@pytest.mark.parametrize("c", co.HALO_CASES, ids=lambda c: c.name)
def test_halo_structure(c):
    """Forced halo launch against the float64 reference; where out and norm_out both exist, norm_out against
    norm_reference(out) and sf_rmsnorm_silu_cl(out) against the same reference; AUTO picks the halo kernel (same bits);
    the implicit GEMM without the norm gives the same bits (integer family: both are exact)."""
    d, dd = device_data(c)
    res = run(c, "halo")
    worst = co.check_case(c, d, reference(c), res, f"{c.name} via halo")
    print(f"{c.name} {co.dispatch(c)}: worst err / tol {worst}")
    if "out" in res and "norm_out" in res:
        f0 = c.out_frame_offset
        raw = res["out"][f0:f0 + c.T, :, :, :c.Cout].contiguous()
        sep = co.Canary((c.T, c.H, c.W, c.Cout), BF16, DEV)
        raw_d = raw.to(DEV)
        assert rmsnorm_launch(raw_d.data_ptr(), dd["gamma"], sep.ptr(), c.T * c.H * c.W, c.Cout, True) == 0, last_error()
        sep.assert_untouched_outside(torch.ones(sep.shape, dtype=torch.bool), "sf_rmsnorm_silu_cl")
        w2 = co.check_norm(sep.host(), raw, d.gamma, c.Cout, True, what=f"{c.name}: sf_rmsnorm_silu_cl(out)")
        n0 = c.norm_frame_offset
        differ = int((sep.host().view(torch.int16) != res["norm_out"][n0:n0 + c.T, :, :, :c.Cout].contiguous().view(torch.int16)).sum())
        print(f"{c.name}: sf_rmsnorm_silu_cl(out) worst err / tol {w2:.3f}; {differ} of {raw.numel()} elements differ from the fused norm")
    check_against_auto(c, res)
    if c.family == "int" and not c.out_null:
        ig = run(igemm_twin(c), "igemm")
        name = "out" if "out" in res else "out_f32"
        assert same_bits(ig[name], res[name]), f"{c.name}: the implicit GEMM differs from the halo kernel"


def test_halo_three_launch_forms_agree():
    """Cout 192 at 2 x 2 x 2 patches: out + norm (the 192-column tile), norm only (out = NULL), out only (below 160 tiles
    without a norm: the 96-column tile).  Same norm_out bits, same out bits: the two widths compute the same thing."""
    by = {c.name: c for c in co.HALO_CASES}
    both, norm_only, out_only = run(by["halo192_both"], "halo"), run(by["halo192_norm_only"], "halo"), run(by["halo192_out_only"], "halo")
    assert co.dispatch(by["halo192_both"]) == ("halo", 6, 1) and co.dispatch(by["halo192_out_only"]) == ("halo", 3, 2)
    assert set(norm_only) == {"norm_out"} and set(out_only) == {"out"}
    assert same_bits(norm_only["norm_out"], both["norm_out"]), "norm only: norm_out differs"
    assert same_bits(out_only["out"], both["out"]), "NT 3 differs from NT 6"
    g = by["halo192_both_gauss"]                           # and with data whose sum depends on its order
    assert same_bits(run(dataclasses.replace(g, norm=False), "halo")["out"], run(g, "halo")["out"]), "NT 3 differs from NT 6 (Gaussian)"


@pytest.mark.parametrize("family", ["int", "gauss"])
def test_halo_two_column_tiles_equal_frame_by_frame(family):
    """Cout 384 at 100 x 90, two frames: 168 tiles, the 192-column tile with tiles_n = 2.  The same frames one per call
    (84 tiles each: the 96-column tile) into one buffer give the same bits, also with Gaussian data, whose sums depend on
    their order; each call leaves the other frame alone."""
    c = next(c for c in co.HALO_CASES if c.name == "halo384_two_column_tiles")
    if family == "gauss":
        c = dataclasses.replace(c, name=c.name + "_gauss", family="gauss")
        assert co.dispatch(c) == ("halo", 6, 2)
        worst = co.check_case(c, device_data(c)[0], reference(c), run(c, "halo"), c.name)
        print(f"{c.name}: worst err / tol {worst}")
    whole = run(c, "halo")["out"]
    _, dd = device_data(c)
    bufs = {"out": co.Canary(c.out_shape, BF16, DEV)}
    owned = torch.zeros(c.out_shape, dtype=torch.bool)
    for f in range(c.T):
        one = dataclasses.replace(c, T=1, t_in_offset=f, out_frame_offset=f)
        assert co.dispatch(one) == ("halo", 3, 4)
        assert launch(one, dd, bufs, "halo") == 0, last_error()
        owned[f, :, :, :c.Cout] = True
        bufs["out"].assert_untouched_outside(owned, f"frame {f}")
    assert same_bits(bufs["out"].host(), whole)


# ------------------------------------------------------------------------------------------ the implicit GEMM
@pytest.mark.parametrize("c", co.IGEMM_CASES, ids=lambda c: c.name)
def test_igemm_structure(c):
    """Forced implicit GEMM (the last case: AUTO outside the halo domain) against the float64 reference, and AUTO against
    the structure it should pick."""
    d, _ = device_data(c)
    res = run(c, c.structure)
    worst = co.check_case(c, d, reference(c), res, f"{c.name} via {c.structure}")
    print(f"{c.name} {co.dispatch(c)}: worst err / tol {worst}")
    if c.structure == "auto":
        assert co.dispatch(c)[0] == "igemm"
        for name, t in run(c, "igemm").items():
            assert same_bits(res[name], t)
    else:
        check_against_auto(c, res)


def test_pick_nt_is_what_the_case_list_assumes():
    assert all(_lib.lib().sf_conv_pick_nt(c.Cout) == co.pick_nt(c.Cout) for c in co.CASES)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    base = next(c for c in co.HALO_CASES if c.name == "halo96_ring_norm")
    R = dataclasses.replace
    wide = R(base, Cout=384)
    refused = [
        (base, "igemm", "fused norm output exists in the halo kernel only"),
        (wide, "halo", "a fused norm output: Cout 96 or 192"),
        (wide, "auto", "a fused norm output: Cout 96 or 192"),
        (R(base, norm_ld=100), "halo", "norm_ld"),
        (R(base, norm_ld=100), "auto", "norm_ld"),
        (R(base, norm=False, ldo=100), "halo", "ldo"),
        (R(base, norm=False, out_null=True), "halo", "needs out (or norm_out)"),
        (R(base, norm=False, out_null=True), "auto", "needs out (or norm_out)"),
    ]
    for c, structure, reason in refused:
        assert co.dispatch(c, structure) == ("refused",), (c, structure)
        _, dd = device_data(c)
        bufs = make_buffers(c, dd)
        assert launch(c, dd, bufs, structure) != 0, (c.name, structure)
        assert reason in last_error(), (reason, last_error())
        for name, can in bufs.items():
            can.assert_untouched_outside(torch.zeros(can.shape, dtype=torch.bool), f"refused {structure} launch: {name}")


# ------------------------------------------------------------------------------------------ sf_rmsnorm_silu_cl
NORM_WIDTHS = [8, 16, 24, 32, 40, 64, 96, 128, 192, 256, 384, 504, 512]


def lanes_per_row(C):
    lpr = 1
    while lpr * 8 < C:
        lpr *= 2
    return lpr


def test_norm_widths_cover_every_instantiation():
    assert {lanes_per_row(C) for C in NORM_WIDTHS} == {1, 2, 4, 8, 16, 32, 64}


def norm_rows(family, rows, C, g):
    if family == "gauss":
        x = torch.randn((rows, C), generator=g) * 2.0
    elif family == "dominant":                              # |u| near sqrt(C) gamma at one element of every row
        x = torch.randn((rows, C), generator=g) * 0.05
        x[torch.arange(rows), torch.randint(0, C, (rows,), generator=g)] = torch.where(torch.rand((rows,), generator=g) < 0.5, -100.0, 100.0)
    elif family == "zero_row":
        x = torch.randn((rows, C), generator=g)
        x[0] = 0
        x[rows // 2] = 0
    else:                                                   # "large"
        x = 1e4 + 100 * torch.randn((rows, C), generator=g)
    return x.to(BF16)


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("C", NORM_WIDTHS)
def test_rmsnorm_silu_cl_every_element(C, silu):
    """Rows 1 and 2 (256 / LPR) + 3 (two full blocks and a ragged one), out of place and in place, four families of rows;
    every element within 2^-8 |ref| of the float64 reference, an all-zero row gives zeros, the rows behind the last one and
    the guard bands keep the canary."""
    g = torch.Generator().manual_seed(7000 + C)
    gamma = (1 + 0.25 * torch.randn((C,), generator=g)).clamp(0.5, 1.5).to(BF16)
    gamma_d = gamma.to(DEV)
    worst = 0.0
    for rows in (1, 2 * (256 // lanes_per_row(C)) + 3):
        owned = torch.zeros((rows + 2, C), dtype=torch.bool)
        owned[:rows] = True
        for family in ("gauss", "dominant", "zero_row", "large"):
            x = norm_rows(family, rows, C, g)
            x_d = x.to(DEV)
            for in_place in (False, True):
                out = co.Canary((rows + 2, C), BF16, DEV)
                if in_place:
                    out.region[:rows] = x_d
                assert rmsnorm_launch(out.ptr() if in_place else x_d.data_ptr(), gamma_d, out.ptr(), rows, C, silu) == 0, last_error()
                out.assert_untouched_outside(owned, f"C {C} rows {rows} {family}")
                got = out.host()[:rows]
                worst = max(worst, co.check_norm(got, x, gamma, C, silu, what=f"C {C} rows {rows} {family} in_place {in_place}"))
                if family == "zero_row":
                    assert bool((got[0] == 0).all()) and bool((got[rows // 2] == 0).all())
                assert bool(torch.isfinite(got.float()).all())
    print(f"sf_rmsnorm_silu_cl C {C} silu {silu}: worst err / tol {worst:.3f}")
