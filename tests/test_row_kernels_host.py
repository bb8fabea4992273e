"""Host tests of oracle/row_oracle.py, the yardstick of tests/test_gpu_row_kernels.py (no GPU):

  * the fp32 emulation of the row kernels' arithmetic passes every checker, family by family, and the headroom it leaves
    under the caps is printed (run with -s to see it);
  * nine subtly wrong variants of that emulation are each rejected, with the rows the checker blames asserted -- this is
    what shows that the GPU tests would fail on a kernel with the same mistake.

A one-pass variance (variant 3) is invisible on the first seven families under the LayerNorm caps: in fp32 it costs
0.51 ulp at worst and flips 0.5 - 0.7 % of a mean-100 row's roundings (the emulation: 0.07 %), both inside the caps.  The
eighth family, "offset" (every element 200 or 201, mean / std = 400), is what rejects it: E[x^2] - mean^2 is the difference of two numbers near
40000 with fp32's 2^-24 each, against a variance of 0.25 (2.5 - 5 ulp measured); the two-pass emulation stays at 0.503 ulp."""
import numpy as np
import pytest
import torch

from oracle import row_oracle as ro

EPS = 1e-6
M, RPG = 17, 3                        # odd M; groups change at rows 3, 9, 15 (second row of a wave's pair) and 6, 12 (first)
G = (M + RPG - 1) // RPG
C = 1536


def rows_of(names, *fams):
    return [r for r, n in enumerate(names) if n in fams]


# ------------------------------------------------------------------------------------------ the emulation passes, with headroom
@pytest.fixture(scope="module")
def headroom():
    seen = {}
    yield seen
    print("\nemulation headroom (worst over families):")
    for key in sorted(seen):
        print(f"  {key[0]:<20} C={key[1]:<5} worst {max(w for w, _ in seen[key]):.3f}   differing at most {max(s for _, s in seen[key]) * 100:.4f} %")


@pytest.mark.parametrize("family", ro.FAMILIES)
@pytest.mark.parametrize("width", [512, 2560, 5120])
def test_emulated_layernorm_passes(width, family, headroom):
    x, names = ro.make_rows(32, width, 100 + width, families=(family,))
    ms, mc, e0 = ro.make_params((width,), 1), ro.make_params((width,), 2), ro.make_params((11, 2, width), 3)
    w, b = ro.make_params((width,), 4), ro.make_params((width,), 5)
    for eps in (1e-6, 1e-5):
        ref = ro.ref_layernorm_modulate(x, ms, mc, e0[:, 0], e0[:, 1], RPG, eps)
        rep = ro.check_layernorm("emulated layernorm_modulate", ro.emu_layernorm_modulate(x, ms, mc, e0[:, 0], e0[:, 1], RPG, eps), ref, names)
        print(f"\n{family:<8} eps={eps:g} {rep.figures()}")
        rep.assert_ok()
        headroom.setdefault(("layernorm_modulate", width), []).append((rep.worst, rep.share))
        rep = ro.check_layernorm("emulated layernorm_affine", ro.emu_layernorm_affine(x, w, b, eps), ro.ref_layernorm_affine(x, w, b, eps), names)
        print(f"{family:<8} eps={eps:g} {rep.figures()}")
        rep.assert_ok()
        headroom.setdefault(("layernorm_affine", width), []).append((rep.worst, rep.share))


@pytest.mark.parametrize("family", ro.FAMILIES)
@pytest.mark.parametrize("width", [512, 4096, 5120])
def test_emulated_rmsnorm_passes(width, family, headroom):
    x, names = ro.make_rows(64, width, 200 + width, families=(family,))
    w = ro.make_params((width,), 6)
    for eps in (1e-6, 1e-5):
        rep = ro.check_rmsnorm(ro.emu_rmsnorm(x, w, eps), ro.ref_rmsnorm(x, w, eps), names, "emulated rmsnorm")
        print(f"\n{family:<8} eps={eps:g} {rep.figures()}")
        rep.assert_ok()
        headroom.setdefault(("rmsnorm", width), []).append((rep.worst, rep.share))


@pytest.mark.parametrize("M,rpg,layout", [(257, 257, "cols34"), (96, 32, "cols01"), (45, 15, "head")])
@pytest.mark.parametrize("width", ro.WIDTHS)
def test_emulation_passes_the_gpu_tests_own_launches(width, M, rpg, layout, headroom):
    """The inputs tests/test_gpu_row_kernels.py launches, at every width: the caps leave room for correct fp32 arithmetic on them
    (the thinnest: 0.853 ulp at C = 3072, a mean-100 row's x = 100 next to a mean of 99.9993 under a shift of exactly 0)."""
    c = ro.modulate_case(M, width, rpg, layout)
    es, ec = ro.e0_views(c["e0"], layout)
    out = ro.emu_layernorm_modulate(c["x"], c["mod_shift"], c["mod_scale"], es, ec, rpg, EPS)
    rep = ro.check_layernorm(f"emulated layernorm_modulate[{layout} M={M}]", out,
                             ro.ref_layernorm_modulate(c["x"], c["mod_shift"], c["mod_scale"], es, ec, rpg, EPS), c["names"])
    print("\n" + rep.figures())
    rep.assert_ok()
    headroom.setdefault(("modulate, GPU inputs", width), []).append((rep.worst, rep.share))
    w = ro.make_params((width,), 7 * width)
    rep = ro.check_rmsnorm(ro.emu_rmsnorm(c["x"], w, EPS), ro.ref_rmsnorm(c["x"], w, EPS), c["names"], f"emulated rmsnorm[M={M}]")
    print(rep.figures())
    rep.assert_ok()
    headroom.setdefault(("rmsnorm, GPU inputs", width), []).append((rep.worst, rep.share))


def test_mixed_launch_passes_and_reports_every_row():
    x, names = ro.make_rows(M, C, 7)
    ms, mc, e0 = ro.make_params((C,), 1), ro.make_params((C,), 2), ro.make_params((G, 2, C), 3)
    rep = ro.check_layernorm("emulated layernorm_modulate", ro.emu_layernorm_modulate(x, ms, mc, e0[:, 0], e0[:, 1], RPG, EPS),
                             ro.ref_layernorm_modulate(x, ms, mc, e0[:, 0], e0[:, 1], RPG, EPS), names)
    rep.assert_ok()
    assert [(r.row, r.group, r.family) for r in rep.rows] == [(r, r // RPG, names[r]) for r in range(M)]
    assert set(names) == set(ro.FAMILIES) and rep.blamed == []
    # the cycle is skewed: a family meets both rows of a wave's pair
    long_names = ro.make_rows(64, 512, 7)[1]
    for fam in ro.FAMILIES:
        assert {r % 2 for r in rows_of(long_names, fam)} == {0, 1}, fam


def test_sinusoid_checker():
    t = torch.tensor([0.0, 1000.0, 833.3333, 937.5, 1e-3], dtype=torch.float32)
    ref = ro.ref_sinusoid(t, 256)
    # an independent float64 evaluation (numpy, exp instead of pow) agrees within the caps
    k = np.arange(128, dtype=np.float64)
    ang = t.double().numpy()[:, None] * np.exp(-k / 128 * np.log(10000.0))[None]
    other = torch.from_numpy(np.concatenate([np.cos(ang), np.sin(ang)], 1)).to(torch.bfloat16)
    for rep in ro.check_sinusoid(other, ref, t):
        print("\n" + rep.figures())
        rep.assert_ok()
    # angles in fp32 are not good enough: t = 1000 loses the low bits of the phase
    ang32 = (t[:, None] * torch.from_numpy(np.exp(-k / 128 * np.log(10000.0))).float()[None])
    bad = torch.cat([ang32.cos(), ang32.sin()], 1).to(torch.bfloat16)
    reps = ro.check_sinusoid(bad, ref, t)
    assert not all(r.ok for r in reps)
    assert 1 in reps[0].blamed + reps[1].blamed, "the t = 1000 row is the one fp32 angles get wrong"
    # the halves swapped: every row of both halves
    swapped = torch.cat([ref[:, 128:], ref[:, :128]], 1)
    assert all(r.blamed == [0, 1, 2, 3, 4] for r in ro.check_sinusoid(swapped, ref, t))


# ------------------------------------------------------------------------------------------ wrong variants are rejected
@pytest.fixture(scope="module")
def ln_case():
    x, names = ro.make_rows(M, C, 11)
    ms, mc, e0 = ro.make_params((C,), 12), ro.make_params((C,), 13), ro.make_params((G, 2, C), 14)
    ref = ro.ref_layernorm_modulate(x, ms, mc, e0[:, 0], e0[:, 1], RPG, EPS)
    add, scl = ro.emu_mod_params(ms, mc, e0[:, 0], e0[:, 1])
    mean, rstd = ro.emu_ln_stats(x.float(), EPS)
    grp = ro.row_groups(M, RPG)
    good = ro.emu_ln_apply(x.float(), mean, rstd, 1.0 + scl.float()[grp], add.float()[grp])
    assert torch.equal(good, ro.emu_layernorm_modulate(x, ms, mc, e0[:, 0], e0[:, 1], RPG, EPS))
    return dict(x=x.float(), names=names, ref=ref, add=add.float(), scl=scl.float(), mean=mean, rstd=rstd, grp=grp, good=good)


def ln_blamed(c, out):
    rep = ro.check_layernorm("variant", out, c["ref"], c["names"])
    assert not rep.ok and rep.failures and all("row" in f and "group" in f and "family" in f for f in rep.failures[:1])
    return rep.blamed


def test_rejects_first_rows_modulation_on_the_second_row(ln_case):
    c = ln_case
    grp = c["grp"].clone()
    odd = torch.arange(1, M, 2)
    grp[odd] = grp[odd - 1]                                   # the pair's second row keeps the first row's group
    out = ro.emu_ln_apply(c["x"], c["mean"], c["rstd"], 1.0 + c["scl"][grp], c["add"][grp])
    assert ln_blamed(c, out) == [3, 9, 15]                   # where the group changes inside a pair; 6 and 12 start a pair


def test_rejects_statistics_shared_by_a_pair(ln_case):
    c = ln_case
    mean, rstd = c["mean"].clone(), c["rstd"].clone()
    odd = torch.arange(1, M, 2)
    mean[odd], rstd[odd] = mean[odd - 1], rstd[odd - 1]
    out = ro.emu_ln_apply(c["x"], mean, rstd, 1.0 + c["scl"][c["grp"]], c["add"][c["grp"]])
    assert ln_blamed(c, out) == odd.tolist()


def test_rejects_one_pass_variance(ln_case):
    c = ln_case
    x = c["x"]
    mean = (ro.lane_tree_sum(x) / C)[:, None]
    var = (ro.lane_tree_sum(x * x) / C)[:, None] - mean * mean
    out = ro.emu_ln_apply(x, mean, torch.rsqrt(var + EPS), 1.0 + c["scl"][c["grp"]], c["add"][c["grp"]])
    blamed = ln_blamed(c, out)
    offset = rows_of(c["names"], "offset")
    assert blamed and set(blamed) & set(offset), f"blamed {blamed}, offset rows {offset}"
    assert set(blamed) <= set(rows_of(c["names"], "offset", "mean100")), f"blamed {blamed}: only rows of a large mean can suffer"


def test_rejects_eps_outside_the_root_and_eps_left_out(ln_case):
    c = ln_case
    x = c["x"]
    d = x - c["mean"]
    var = (ro.lane_tree_sum(d * d) / C)[:, None]
    apply = lambda rstd: ro.emu_ln_apply(x, c["mean"], rstd, 1.0 + c["scl"][c["grp"]], c["add"][c["grp"]])  # noqa: E731
    assert ln_blamed(c, apply(1.0 / (var.sqrt() + EPS))) == rows_of(c["names"], "tiny")
    # without eps a constant row is 0 * inf
    assert ln_blamed(c, apply(torch.rsqrt(var))) == rows_of(c["names"], "tiny", "const")


def test_rejects_a_ragged_last_row_that_repeats_its_neighbour(ln_case):
    c = ln_case
    out = c["good"].clone()
    out[M - 1] = out[M - 2]
    assert ln_blamed(c, out) == [M - 1]


def test_rejects_shift_and_scale_swapped(ln_case):
    c = ln_case
    out = ro.emu_ln_apply(c["x"], c["mean"], c["rstd"], 1.0 + c["add"][c["grp"]], c["scl"][c["grp"]])
    assert ln_blamed(c, out) == list(range(M))               # constant rows too: they must equal the shift


def test_rejects_scale_without_the_one(ln_case):
    c = ln_case
    out = ro.emu_ln_apply(c["x"], c["mean"], c["rstd"], c["scl"][c["grp"]], c["add"][c["grp"]])
    assert ln_blamed(c, out) == [r for r in range(M) if c["names"][r] != "const"]    # a constant row is the shift either way


def test_affine_checker_rejects_the_same_mistakes():
    x, names = ro.make_rows(M, C, 21)
    w, b = ro.make_params((C,), 22), ro.make_params((C,), 23)
    ref = ro.ref_layernorm_affine(x, w, b, EPS)
    ro.check_layernorm("emulated layernorm_affine", ro.emu_layernorm_affine(x, w, b, EPS), ref, names).assert_ok()
    mean, rstd = ro.emu_ln_stats(x.float(), EPS)
    odd = torch.arange(1, M, 2)
    mean[odd], rstd[odd] = mean[odd - 1], rstd[odd - 1]
    rep = ro.check_layernorm("variant", ro.emu_ln_apply(x.float(), mean, rstd, w.float()[None], b.float()[None]), ref, names)
    assert rep.blamed == odd.tolist()
    rep = ro.check_layernorm("variant", ro.emu_layernorm_affine(x, b, w, EPS), ref, names)
    assert rep.blamed == list(range(M))


@pytest.fixture(scope="module")
def rms_case():
    x, names = ro.make_rows(M, C, 31)
    w = ro.make_params((C,), 32)
    return dict(x=x.float(), names=names, w=w.float(), ref=ro.ref_rmsnorm(x, w, EPS))


def test_rejects_rmsnorm_with_one_rounding(rms_case):
    c = rms_case
    out = (c["x"] * ro.emu_rms_r(c["x"], EPS) * c["w"][None]).to(torch.bfloat16)
    rep = ro.check_rmsnorm(out, c["ref"], c["names"])
    assert not rep.ok and rep.worst <= ro.RMS_STEP_CAP          # never far off: it is the count of differing elements that tells
    assert rep.blamed == [r for r in range(M) if c["names"][r] != "const"]          # 3.25 r rounds to 1 either way


def test_rejects_rmsnorm_over_c_minus_1(rms_case):
    c = rms_case
    out = ((c["x"] * ro.emu_rms_r(c["x"], EPS, denom=C - 1)).to(torch.bfloat16).float() * c["w"][None]).to(torch.bfloat16)
    rep = ro.check_rmsnorm(out, c["ref"], c["names"])
    assert not rep.ok
    # x r is 1 on a constant row and 0.9975 / 1.0025 on an offset row: r (1 + 1 / 2C) rounds to the same bf16 values there
    assert rep.blamed == [r for r in range(M) if c["names"][r] not in ("const", "offset")]
