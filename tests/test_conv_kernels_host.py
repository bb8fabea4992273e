"""Host tests of oracle/conv_oracle.py, the yardstick of tests/test_gpu_conv_kernels.py (no GPU):

  * the fp32 emulation of a correct kernel passes every checker on every case of the GPU case list (integer family: bit
    for bit; Gaussian family: within the bound, the worst err / tol printed with `pytest -s`);
  * ten subtly wrong variants of it are each rejected, and the checker blames the element that is wrong;
  * the case list reaches every kernel, tile width and epilogue that sf_conv_igemm dispatches to, by a mirror of the
    code's rules that is itself compared with sf_conv_pick_nt and pinned on known launches;
  * the canary helper notices a stray store."""
import dataclasses

import pytest
import torch

import self_forcing_amd as sfa
from oracle import conv_oracle as co

BY_NAME = {c.name: c for c in co.CASES}


def emulate_and_check(c, bug=None):
    d = co.make_data(c)
    r = co.conv_reference(c, d, absacc=c.family == "gauss")
    res = co.fp32_emulation(c, d, bug)
    if c.out_null:
        res.pop("out")
    return co.check_case(c, d, r, res, c.name), d, r, res


def test_case_names_are_unique():
    assert len(BY_NAME) == len(co.CASES)


@pytest.mark.parametrize("c", co.CASES, ids=lambda c: c.name)
def test_emulation_passes_every_checker(c):
    """Measured here (worst err / tol): integer family 0 everywhere, bit for bit; Gaussian family 0.753 (halo96_ragged),
    0.512 (halo192_both), 0.711 (ig_cout100), all of it the final rounding, and 2.3e-5 (the fp32 head); fused norm
    0.995 - 0.996 = 1 / (1 + 2^-8), the final rounding of a value just above a power of two."""
    worst, d, r, res = emulate_and_check(c)
    print(f"{c.name}: dispatch {co.dispatch(c)}, worst err / tol {worst}")
    assert bool(r.owned.any()) and not bool(r.owned.all())
    for name, buf in res.items():
        owned = co.norm_owned_mask(c) if name == "norm_out" else r.owned
        assert bool(torch.isnan(buf.float()[~owned]).all()) and not bool(torch.isnan(buf.float()[owned]).any())
    if c.family == "gauss":
        assert 0 < worst["conv"] <= 1
        assert c.Cin <= 128
    if c.norm and not c.out_null:
        assert 0 < worst["norm"] <= 1


def test_inputs_hold_nan_where_a_launch_must_not_read():
    half = 0
    for c in co.CASES:
        d = co.make_data(c)
        assert d.x.shape[0] == c.x_frames_used + 1
        nan = torch.isnan(d.x.float()).flatten(1).all(1)
        assert nan.tolist() == [t < c.t_in_offset or t >= c.x_frames_used for t in range(d.x.shape[0])]
        assert bool((d.w[:, c.K:c.kpad] == 0).all()) and bool(torch.isnan(d.w[:, c.kpad:].float()).all())
        assert not bool(torch.isnan(d.w[:, :c.K].float()).any())
        half += c.ldw > c.kpad
        if c.family == "int":
            assert float(d.x[c.t_in_offset:c.x_frames_used].abs().max()) == 4 and c.K <= 3456
        assert 0.5 <= float(d.gamma.min()) and float(d.gamma.max()) <= 1.5
    assert 2 * half >= len(co.CASES)
    assert any(c.t_in_offset > 0 for c in co.HALO_CASES) and any(c.t_in_offset > 0 for c in co.IGEMM_CASES)


def test_integer_head_clamps_a_share_of_its_results():
    c = BY_NAME["halo_head"]
    r = co.conv_reference(c, co.make_data(c), absacc=False)
    frac = float((r.ref[r.owned].abs() == 1).double().mean())
    assert 0.02 < frac < 0.25, frac             # (the nearest power of two to 5 %: a factor of two away is 0.5 %)


def test_round_once_is_round_to_nearest_even():
    v = torch.tensor([256.0, 257.0, 258.0, 259.0, 261.0, 263.0, -257.0, -259.0, 0.0, 3.0, 511.0, 16777215.0], dtype=torch.float64)
    want = torch.tensor([256.0, 256.0, 258.0, 260.0, 260.0, 264.0, -256.0, -260.0, 0.0, 3.0, 512.0, 16777216.0])
    assert torch.equal(co.round_once_to_bf16(v).float(), want)
    g = torch.Generator().manual_seed(0)
    i = torch.randint(-(1 << 24), 1 << 24, (100000,), generator=g).double()
    assert torch.equal(co.round_once_to_bf16(i), i.float().to(torch.bfloat16))       # (int -> fp32 is exact below 2^24)


# ------------------------------------------------------------------------------------------ wrong variants
def blamed(bug, case, part):
    c = BY_NAME[case]
    with pytest.raises(co.Mismatch) as e:
        emulate_and_check(c, bug)
    assert part in str(e.value), str(e.value)
    owned = int(co.owned_mask(c).sum())
    print(f"{bug} on {case}: {e.value}")
    return c, e.value, owned


@pytest.mark.parametrize("case,part", [("halo96_ragged", "bit-equal"), ("halo96_ragged_gauss", "bound")])
def test_rejects_1_a_tap_dropped_at_a_corner_pixel(case, part):
    c, m, _ = blamed("drop_corner_tap", case, part)
    assert m.index[:3] == (c.out_frame_offset, c.H - 1, c.W - 1) and m.count <= c.T * c.Cout


@pytest.mark.parametrize("case,part", [("halo96_ragged", "bit-equal"), ("halo192_both_gauss", "bound"), ("ig_cout96", "bit-equal")])
def test_rejects_2_the_bias_of_the_neighbouring_group(case, part):
    c, m, owned = blamed("bias_neighbour_group", case, part)
    assert m.index[:3] == (c.out_frame_offset, 0, 0) and 16 <= m.index[3] < 32 and m.count <= owned * 16 // c.Cout


@pytest.mark.parametrize("case", ["halo96_ring_resid", "ig_halo96_ring_alias", "ig_cout36_ldo44"])
def test_rejects_3_the_residual_of_the_next_frame(case):
    c, m, owned = blamed("resid_next_frame", case, "bit-equal")
    assert m.index[0] == c.out_frame_offset and m.count > owned // 2


@pytest.mark.parametrize("case,part", [("halo96_ragged", "bit-equal"), ("halo96_ragged_gauss", "bound"), ("halo192_out_only", "bit-equal")])
def test_rejects_4_a_ragged_patch_row_from_the_clamped_neighbour(case, part):
    c, m, _ = blamed("ragged_clamped_neighbour", case, part)
    assert c.H % 16 != 0 and m.index[:3] == (c.out_frame_offset, c.H - 1, 0) and m.count <= c.T * c.W * c.Cout


@pytest.mark.parametrize("case", ["halo192_both", "halo192_both_gauss", "halo96_ring_norm", "halo_up96"])
def test_rejects_5_the_norm_factor_of_the_neighbouring_row(case):
    c, m, _ = blamed("norm_neighbour_row", case, "[norm]")
    assert m.index[0] == 0 and m.count > c.T * c.H * c.W * c.Cout // 4


@pytest.mark.parametrize("case", ["halo192_both", "halo192_both_gauss", "halo96_ring_norm", "halo_border_48x16"])
def test_rejects_6_the_other_tile_widths_sqrt(case):
    c, m, _ = blamed("norm_other_width", case, "[norm]")
    assert m.index[:3] == (0, 0, 0) and m.count > c.T * c.H * c.W * c.Cout * 9 // 10


@pytest.mark.parametrize("case,part", [("halo_head", "fp32-equal"), ("halo_head_gauss", "bound")])
def test_rejects_7_the_clamp_left_out(case, part):
    c, m, owned = blamed("no_clamp", case, part)
    r = co.conv_reference(c, co.make_data(c), absacc=False)
    clamped = int((r.ref[r.owned].abs() == 1).sum())     # (includes what is exactly +-1 or within the bound of it unclamped)
    assert abs(float(r.ref[m.index])) == 1.0 and 0.9 * clamped <= m.count <= clamped


def test_rejects_8_interleave_halves_swapped():
    c, m, owned = blamed("interleave_swapped", "ig_interleave", "bit-equal")
    assert m.index[0] == c.out_frame_offset and m.count > owned * 9 // 10


@pytest.mark.parametrize("case", ["halo_up96", "ig_halo_up192"])
def test_rejects_9_upsample_rounding_up(case):
    c, m, owned = blamed("upsample_round_up", case, "bit-equal")
    assert m.index[:3] == (0, 0, 0) and m.count > owned * 9 // 10


def test_rejects_10_stride_two_padded_on_the_left():
    c, m, owned = blamed("stride_pad_left", "ig_stride_hw", "bit-equal")
    assert m.index[:3] == (0, 0, 0) and m.count > owned * 9 // 10


def test_every_wrong_variant_has_a_test():
    assert len(co.BUGS) == 10
    src = open(__file__).read()
    assert all(f'"{b}"' in src for b in co.BUGS)


# ------------------------------------------------------------------------------------------ dispatch
def test_pick_nt_mirror_matches_the_library():
    lib = sfa._lib.lib()
    for cout in list(range(1, 800)):
        assert co.pick_nt(cout) == lib.sf_conv_pick_nt(cout), cout
    assert [co.pick_nt(c) for c in (3, 32, 36, 40, 64, 96, 100, 128, 160, 192, 384, 768)] == [1, 1, 2, 2, 2, 3, 4, 4, 1, 6, 6, 6]


def test_dispatch_mirror_on_known_launches():
    """The rule's corner stones, written out by hand from conv_halo.hip / conv_igemm.hip; the GPU test also runs AUTO
    against the forced structure the mirror predicts, bit for bit, on every case."""
    C, R = co.ConvCase, dataclasses.replace
    big = C("x", 192, 192, 3, 3, 1, 240, 416, structure="auto")                  # 15 x 26 = 390 patches
    assert co.dispatch(big) == ("halo", 6, 1)
    assert co.dispatch(R(big, Hin=60, Win=104, Cout=384)) == ("halo", 3, 4)      # 28 patches x 2 < 160: the narrow tile
    assert co.dispatch(R(big, Hin=16 * 10, Win=16 * 16)) == ("halo", 6, 1)       # exactly 160
    assert co.dispatch(R(big, Hin=16 * 10, Win=16 * 16 - 16)) == ("halo", 3, 2)  # 150
    assert co.dispatch(R(big, Hin=16 * 10, Win=16 * 16 - 16, norm=True)) == ("halo", 6, 1)     # a norm needs the whole row
    assert co.dispatch(R(big, Cout=96)) == ("halo", 3, 1)
    assert co.dispatch(R(big, Cout=288)) == ("halo", 3, 3)
    assert co.dispatch(R(big, Cout=128)) == ("igemm", 4, "lds", "even")
    assert co.dispatch(R(big, Hin=15)) == ("igemm", 6, "lds", "even")
    assert co.dispatch(R(big, ks=1)) == ("igemm", 6, "lds", "even")
    assert co.dispatch(R(big, ldo=196)) == ("igemm", 6, "direct", "even")
    assert co.dispatch(R(big, Cin=32, ldo=196)) == ("igemm", 6, "direct", "odd")
    assert co.dispatch(R(big, ldo=196), "halo") == ("refused",)
    assert co.dispatch(R(big, norm=True), "igemm") == ("refused",)
    assert co.dispatch(R(big, norm=True, Cout=384)) == ("refused",)
    assert co.dispatch(R(big, norm=True, norm_ld=196)) == ("refused",)
    assert co.dispatch(R(big, out_null=True)) == ("refused",)
    assert co.dispatch(R(big, Cout=3, epilogue="clamp")) == ("halo_head",)
    assert co.dispatch(R(big, Cout=3, epilogue="clamp"), "igemm") == ("igemm", 1, "direct", "even")
    assert co.dispatch(R(big, Hin=480, Win=832, stride_hw=2)) == ("igemm", 6, "lds", "even")
    assert co.dispatch(R(big, Cout=384, kt=3, ks=1, interleave=True)) == ("igemm", 6, "direct", "even")


def test_case_list_covers_the_dispatch():
    table = co.dispatch_table()
    for name, d in table.items():
        print(f"{name:32s} {d}")
    missing = [item for item in co.REQUIRED_DISPATCH if item not in co.dispatch_coverage()]
    assert not missing, missing
    assert ("refused",) not in table.values()
    for c in co.HALO_CASES:
        assert table[c.name][0].startswith("halo") and co.dispatch(c, "auto") == table[c.name], c.name
    for c in co.IGEMM_CASES:
        assert table[c.name][0] == "igemm", c.name
    # the shapes that exist for one path reach it
    assert table["halo192_both"] == ("halo", 6, 1) and table["halo192_norm_only"] == ("halo", 6, 1) and table["halo192_out_only"] == ("halo", 3, 2)
    assert table["halo384_two_column_tiles"] == ("halo", 6, 2)
    assert co.dispatch(dataclasses.replace(BY_NAME["halo384_two_column_tiles"], T=1)) == ("halo", 3, 4)
    assert table["ig_cout160"] == ("igemm", 1, "lds", "odd") and table["ig_cout40"][1:3] == (2, "lds") and table["ig_cout100"][1:3] == (4, "direct")
    assert table["ig_cout36_ldo36"][2] == "direct" and table["ig_cout36_ldo44"][2] == "direct"
    assert table["auto_ldo100_falls_back"] == ("igemm", 3, "direct", "odd")
    assert table["ig_even_slices"][3] == "even"


def test_a_dropped_item_is_noticed():
    assert ("halo", 6, 2) not in co.dispatch_coverage([c for c in co.CASES if c.name != "halo384_two_column_tiles"])
    assert ("igemm", 1) not in co.dispatch_coverage([c for c in co.CASES if c.Cout not in (32, 160, 3)])


# ------------------------------------------------------------------------------------------ canary
def test_canary_notices_a_stray_store():
    c = BY_NAME["halo96_ragged"]
    owned = co.owned_mask(c)
    can = co.Canary(c.out_shape, torch.bfloat16)
    can.region[owned] = 1.0
    can.assert_untouched_outside(owned)
    can.region[c.out_frame_offset, 0, 0, c.Cout] = 1.0                 # column Cout of a row with ldo > Cout
    with pytest.raises(AssertionError, match=r"first at \(1, 0, 0, 96\)"):
        can.assert_untouched_outside(owned)
    can = co.Canary(c.out_shape, torch.bfloat16)
    can.raw[co.GUARD - 1] = 0
    with pytest.raises(AssertionError, match="in front"):
        can.assert_untouched_outside(owned)
    can = co.Canary((4, 8), torch.float32)
    can.raw[-1] = 0
    with pytest.raises(AssertionError, match="behind"):
        can.assert_untouched_outside(torch.zeros((4, 8), dtype=torch.bool))
