"""Host tests of oracle/attention_cases.py, the yardstick of tests/test_gpu_attention_exact.py (no GPU):

  * every builder's precondition holds (the gap of family A, the class sizes of family B, bf16 representability) and
    every closed form equals float64 softmax over the attended rows to 1e-12;
  * the tiled float64 emulation -- exact or lazy reference, P rounded to bf16 or not -- passes every checker at every
    shape the GPU tests launch;
  * ten defects injected into that emulation are each rejected on a named configuration of the GPU tests, with the rows
    the checker blames asserted (run with -s to see which checker caught which).  This is what shows that the GPU tests
    would fail on a kernel with the same mistake.  Where a family cannot see a defect, that is asserted too: a tile
    counted twice or a zero key left unmasked does not move family A (V 2 / 2 = V; score 0 against 1044), which is why
    families B and C exist."""
import math

import pytest
import torch

from oracle import attention_cases as ac

VARIANTS = [("w4", dict(bf16_p=False, lazy=False)), ("w4", ac.EMULATED["w4"]), ("r64", ac.EMULATED["r64"])]
VARIANT_IDS = ["exact", "bf16P", "bf16P-lazy"]


def all_rows(case):
    return [(b, h, i) for b in range(case.B) for h in range(case.H) for i in range(case.Lq)]


def rows_where(case, pred):
    return [(b, h, i) for b in range(case.B) for h in range(case.H) for i in range(case.Lq) if pred(int(case.pi[b, h, i]))]


def emu(case, **kw):
    return ac.emulate(case.q, case.k, case.v, keys=case.keys, log2w=case.log2w, **kw)


def caught(defect, rep, config):
    assert not rep.ok and rep.failures
    print(f"\n{defect:<16} on {config:<34} rejected by {rep.what}: {len(rep.blamed)} rows blamed, worst err / tol {rep.worst:.3g}")
    return rep.blamed


# ------------------------------------------------------------------------------------------ builders and closed forms
@pytest.mark.parametrize("Lk", [1, 65, 257, 1100])
def test_selector_preconditions_and_closed_form(Lk):
    c = ac.selector_case(2, 2, Lk + 70, Lk)
    assert ac.is_bf16(c.q) and ac.is_bf16(c.k) and c.v.dtype == torch.bfloat16
    for b in range(2):
        for h in range(2):
            s = c.k[b, :, h].double() / 8
            assert bool((s.abs() == 1).all())
            gram = s @ s.T
            gram.fill_diagonal_(-128)
            assert float(gram.max()) <= 64
            assert sorted(set(c.pi[b, h].tolist())) == list(range(Lk)), "pi hits every key"
            assert torch.equal(c.q[b, :, h], c.k[b, c.pi[b, h], h])
    if Lk > 1:      # the slabs differ per (batch, head)
        assert not torch.equal(c.k[0, :, 0], c.k[0, :, 1]) and not torch.equal(c.v[0], c.v[1]) and not torch.equal(c.pi[0, 0], c.pi[1, 1])
    assert (128 - 64) * 64 * ac.C_LOG2 > 522
    assert float((ac.softmax_reference(c.q, c.k, c.v) - c.ref.double()).abs().max()) <= 1e-12


def test_selector_builder_refuses_codes_without_the_gap(monkeypatch):
    monkeypatch.setattr(ac, "GAP", 8)
    with pytest.raises(AssertionError, match="no codes"):
        ac._codes(65, torch.Generator().manual_seed(0))


def test_selector_with_fewer_queries_than_keys_and_integer_values():
    c = ac.selector_case(2, 2, 33, ac.QUERY_EDGE_LK)
    assert c.pi.shape == (2, 2, 33) and len(set(c.pi[0, 0].tolist())) == 33
    c = ac.selector_case(2, 2, ac.ACCUM_LQ, 64, integer_v=True)
    assert bool((c.v.double() == c.v.double().round()).all()) and float(c.v.double().abs().max()) == 8


@pytest.mark.parametrize("P", ac.TIE_P)
@pytest.mark.parametrize("Lk", ac.TIE_LK)
def test_classes_preconditions_and_closed_form(Lk, P):
    c = ac.classes_case(2, 2, Lk, P)
    assert ac.is_bf16(c.q) and ac.is_bf16(c.k) and c.Lq == P
    assert int(c.n.max()) <= max(18, Lk if P > Lk else 0) and int(c.n.min()) >= 1
    for r in (0, P - 1):
        want = Lk if r >= Lk else len(range(r, Lk, P))
        assert int(c.n[r]) == want
    scores = torch.einsum("qd,kd->qk", c.q[0, :, 0].double(), c.k[0, :, 0].double())
    assert set(scores.unique().tolist()) <= {0.0, 8192.0}, "members 8192, everything else exactly 0"
    assert float((ac.softmax_reference(c.q, c.k, c.v) - c.ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("Lk", ac.UNIFORM_LK)
def test_uniform_preconditions_and_closed_form(Lk):
    c = ac.uniform_case(2, 2, ac.UNIFORM_LQ, Lk)
    assert ac.is_bf16(c.q) and ac.is_bf16(c.k) and ac.is_bf16(c.v)
    assert {float(x) for x in c.q[0, :, 0, 0]} == ({2.0, 4.0, 8.0} if c.Lq >= 3 else {2.0})
    assert len({float(c.v[b, 0, h, 0]) for b in range(2) for h in range(2)}) == 4, "a gain per (batch, head)"
    assert float((ac.softmax_reference(c.q, c.k, c.v) - c.ref).abs().max()) <= 1e-12
    if Lk < 128:
        assert bool((c.ref[..., Lk:] == 0).all()) and bool((c.ref[..., :Lk] > 0).all())


@pytest.mark.parametrize("slab", ac.FOLD_SLABS)
def test_fold_preconditions_and_closed_form(slab):
    pairs = ac.fold_pairs(slab)
    assert sorted(n for (n, _), _ in pairs) == sorted(n for (_, n), _ in pairs) == [n for n in ac.FOLD_N if n < slab - 1]
    assert {s for _, ss in pairs for s in ss} == set(ac.FOLD_SAME)
    for i, ((n0, n1), (s0, s1)) in enumerate(pairs):
        assert n0 != n1 and s0 != s1
        c = ac.fold_case(slab, i)
        assert c.keys.tolist() == [n0 + 1, n1 + 1] and c.log2w.tolist() == [math.log2(s0), math.log2(s1)]
        # the folded form against float64 softmax over the UNFOLDED slab: n real rows, then `same` copies of row n
        for b, (n, same) in enumerate(((n0, s0), (n1, s1))):
            idx = torch.cat([torch.arange(n), torch.full((same,), n)])
            full = ac.softmax_reference(c.q[b:b + 1], c.k[b:b + 1, idx], c.v[b:b + 1, idx])
            assert float((full - c.ref[b:b + 1]).abs().max()) <= 1e-12
        assert float((ac.softmax_reference(c.q, c.k, c.v, c.keys, c.log2w) - c.ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("poison", ac.POISONS)
def test_window_puts_poison_on_every_row_that_must_not_be_read(poison):
    c = ac.fold_case(128, 2)
    big_k, big_v = ac.window(c, poison)
    k, v = ac.window_views(big_k, big_v, c.Lk)
    assert big_k.shape[1] == ac.FRONT + c.Lk + ac.BEHIND and ac.BEHIND > ac.KT
    bad = (lambda t: bool(t.isnan().all())) if poison == "nan" else (lambda t: bool((t.double() >= 16).all()))
    for b in range(2):
        n = int(c.keys[b])
        assert torch.equal(k[b, :n], c.k[b, :n]) and torch.equal(v[b, :n], c.v[b, :n])
        for t in (big_k, big_v):
            assert bad(t[b, :ac.FRONT]) and bad(t[b, ac.FRONT + n:])
    # the poison would show: attended as one more key it moves every row out of bound
    out = ac.emulate(c.q, k, v, keys=c.keys + 1, log2w=c.log2w)
    assert ac.check_uniform(out, c).blamed == all_rows(c)


def test_map_cases_reach_every_residue_and_every_branch_of_the_r64_map():
    for rows in (128, 256):
        assert {ac.workgroups(B, H, Lq, rows) % 8 for B, H, Lq in ac.MAP_CASES} == set(range(8))
    seen = set()
    for B, H, Lq in ac.MAP_CASES:
        nwg, Q = ac.workgroups(B, H, Lq, 256), (Lq + 255) // 256
        q8, f = nwg >> 3, (nwg >> 3) // Q
        left = nwg - 8 * f * Q
        seen.add("f=0" if f == 0 else "f=1 with leftovers" if f == 1 and left else "f>=2" if f >= 2 else "f=1")
        if q8 % Q:
            seen.add("Q does not divide q8")
        if left == 0:
            seen.add("no leftovers")
        # the map itself, as attention_r64_kernel writes it, is a bijection onto (pair, query tile)
        got = []
        for bid in range(nwg):
            xcd, jx, r8 = bid & 7, bid >> 3, nwg & 7
            if jx < f * Q:
                got.append((xcd * f + jx // Q, jx % Q))
            else:
                g = jx - f * Q
                for i in range(8):
                    px = (i >> 1) + 4 * (i & 1)
                    if ((xcd & 3) * 2 + (xcd >> 2)) > i:
                        g += q8 + (1 if px < r8 else 0) - f * Q
                got.append((8 * f + g // Q, g % Q))
        assert sorted(got) == [(bh, qt) for bh in range(B * H) for qt in range(Q)]
    assert seen >= {"f=0", "f=1 with leftovers", "f>=2", "Q does not divide q8", "no leftovers"}


# ------------------------------------------------------------------------------------------ the emulation passes everywhere
@pytest.mark.parametrize("structure,opts", VARIANTS, ids=VARIANT_IDS)
def test_emulation_passes_every_key_and_every_query_edge(structure, opts):
    for Lk in ac.EVERY_KEY_LK:
        c = ac.selector_case(2, 2, Lk + 70, Lk)
        ac.check_selector(emu(c, **opts), c, structure).assert_ok()
    for Lq in ac.QUERY_EDGE_LQ:
        c = ac.selector_case(2, 2, Lq, ac.QUERY_EDGE_LK)
        ac.check_selector(emu(c, **opts), c, structure).assert_ok()


@pytest.mark.parametrize("structure,opts", VARIANTS, ids=VARIANT_IDS)
def test_emulation_passes_ties(structure, opts):
    for Lk in ac.TIE_LK:
        for P in ac.TIE_P:
            c = ac.classes_case(2, 2, Lk, P)
            rep = ac.check_classes(emu(c, **opts), c, structure)
            print("\n" + rep.figures())
            rep.assert_ok()


@pytest.mark.parametrize("structure,opts", VARIANTS, ids=VARIANT_IDS)
def test_emulation_passes_uniform_fold_and_poison(structure, opts):
    for Lk in ac.UNIFORM_LK:
        c = ac.uniform_case(2, 2, ac.UNIFORM_LQ, Lk)
        for poison in ac.POISONS:
            k, v = ac.window_views(*ac.window(c, poison), Lk)
            ac.check_uniform(ac.emulate(c.q, k, v, **opts), c, structure).assert_ok()
    for slab in ac.FOLD_SLABS:
        for i in range(len(ac.fold_pairs(slab))):
            c = ac.fold_case(slab, i)
            for poison in ac.POISONS:
                k, v = ac.window_views(*ac.window(c, poison), slab)
                rep = ac.check_uniform(ac.emulate(c.q, k, v, keys=c.keys, log2w=c.log2w, **opts), c, structure)
                rep.assert_ok()


@pytest.mark.parametrize("structure,opts", VARIANTS, ids=VARIANT_IDS)
def test_emulation_passes_maps_stores_accumulate_and_thresholds(structure, opts):
    for B, H, Lq in ac.MAP_CASES:
        c = ac.selector_case(B, H, Lq, ac.MAP_LK)
        ac.check_selector(emu(c, **opts), c, structure).assert_ok()
    for Lq in ac.STORE_LQ:
        c = ac.selector_case(2, 2, Lq, ac.STORE_LK)
        ac.check_selector(emu(c, **opts), c, structure).assert_ok()
    for B, H, Lq, Lk in ac.THRESHOLD_CASES:
        c = ac.selector_case(B, H, Lq, Lk)
        ac.check_selector(emu(c, **opts), c, "r64").assert_ok()
    for Lk in ac.ACCUM_LK:
        c = ac.selector_case(2, 2, ac.ACCUM_LQ, Lk, integer_v=True)
        r = torch.randint(-8, 9, c.ref.shape, generator=torch.Generator().manual_seed(Lk)).to(torch.bfloat16)
        want = (r.double() + c.ref.double()).to(torch.bfloat16)
        assert bool((want.double() == r.double() + c.ref.double()).all()), "R + V is exact in bf16"
        ac.check_selector(emu(c, accum=r, **opts), c, "w4", ref=want).assert_ok()


# ------------------------------------------------------------------------------------------ injected defects are rejected
W4 = ac.EMULATED["w4"]


def test_rejects_last_key_dropped():
    c = ac.selector_case(2, 2, 65 + 70, 65)
    rep = ac.check_selector(emu(c, defect="drop_last_key", **W4), c, "w4")
    assert caught("drop_last_key", rep, "every key, Lk = 65") == rows_where(c, lambda j: j == 64)
    rep = ac.check_selector(emu(c, defect="drop_last_key", **ac.EMULATED["r64"]), c, "r64")
    assert caught("drop_last_key", rep, "every key, Lk = 65 (r64 bound)") == rows_where(c, lambda j: j == 64)
    u = ac.uniform_case(2, 2, ac.UNIFORM_LQ, 1100)        # the smallest relative change a dropped key makes: 1 / 9 of one class
    rep = ac.check_uniform(emu(u, defect="drop_last_key", **W4), u)
    assert caught("drop_last_key", rep, "mask and counts, Lk = 1100") == all_rows(u)


def test_rejects_an_unmasked_padded_key():
    u = ac.uniform_case(2, 2, ac.UNIFORM_LQ, 65)
    rep = ac.check_uniform(emu(u, defect="unmasked_pad", **W4), u)
    assert caught("unmasked_pad", rep, "mask and counts, Lk = 65") == all_rows(u)
    c = ac.selector_case(2, 2, 65 + 70, 65)              # score 0 against 1044: family A cannot see it
    assert ac.check_selector(emu(c, defect="unmasked_pad", **W4), c, "w4").ok


def test_rejects_two_keys_swapped_in_v():
    c = ac.selector_case(2, 2, 129 + 70, 129)
    rep = ac.check_selector(emu(c, defect="swap_v", arg=(1, 5, 40), **W4), c, "w4")
    assert caught("swap_v", rep, "every key, Lk = 129") == rows_where(c, lambda j: j in (64 + 5, 64 + 40))


def test_rejects_a_skipped_tile():
    c = ac.selector_case(2, 2, 257 + 70, 257)
    rep = ac.check_selector(emu(c, defect="skip_tile", arg=2, **W4), c, "w4")
    assert caught("skip_tile", rep, "every key, Lk = 257") == rows_where(c, lambda j: 128 <= j < 192)


def test_rejects_a_tile_counted_twice():
    c = ac.classes_case(2, 2, 193, 64)
    rep = ac.check_classes(emu(c, defect="double_tile", arg=1, **W4), c, "r64")
    assert caught("double_tile", rep, "ties, Lk = 193, P = 64") == all_rows(c)
    u = ac.uniform_case(2, 2, ac.UNIFORM_LQ, 129)
    rep = ac.check_uniform(emu(u, defect="double_tile", arg=1, **W4), u)
    assert caught("double_tile", rep, "mask and counts, Lk = 129") == all_rows(u)
    s = ac.selector_case(2, 2, 193 + 70, 193)            # V 2 / 2 = V: family A cannot see it
    assert ac.check_selector(emu(s, defect="double_tile", arg=1, **W4), s, "w4").ok


def test_rejects_a_stale_ring_slot():
    c = ac.selector_case(2, 2, 832 + 70, 832)
    rep = ac.check_selector(emu(c, defect="stale_v", arg=5, **ac.EMULATED["r64"]), c, "r64")
    assert caught("stale_v", rep, "every key, Lk = 832") == rows_where(c, lambda j: 320 <= j < 384)


def test_rejects_the_wrong_heads_slab():
    c = ac.selector_case(2, 2, 65 + 70, 65)
    rep = ac.check_selector(emu(c, defect="wrong_head", **ac.EMULATED["r64"]), c, "r64")
    assert caught("wrong_head", rep, "every key, Lk = 65") == all_rows(c)
    c = ac.selector_case(1, 3, 513, ac.MAP_LK)
    rep = ac.check_selector(emu(c, defect="wrong_head", **W4), c, "w4")
    assert caught("wrong_head", rep, "workgroup maps, (1, 3, 513)") == all_rows(c)


@pytest.mark.parametrize("poison", ac.POISONS)
def test_rejects_row_lk_of_the_window_read(poison):
    u = ac.uniform_case(2, 2, ac.UNIFORM_LQ, 65)
    big_k, big_v = ac.window(u, poison)
    k, v = ac.window_views(big_k, big_v, 65)
    behind = (big_k[:, ac.FRONT + 65], big_v[:, ac.FRONT + 65])
    rep = ac.check_uniform(ac.emulate(u.q, k, v, defect="read_row_lk", behind=behind, **W4), u)
    assert caught("read_row_lk", rep, f"mask and counts, Lk = 65, {poison}") == all_rows(u)


def test_rejects_the_fold_weight_on_the_next_row():
    i = [n for (_, n), _ in ac.fold_pairs(128)].index(62)      # n = (64, 62): the weighted row opens a tile / closes one
    c = ac.fold_case(128, i)
    assert c.keys.tolist() == [65, 63]                          # (a sample with n = 0 has one key and no weight to lose)
    for poison in ac.POISONS:
        k, v = ac.window_views(*ac.window(c, poison), 128)
        rep = ac.check_uniform(ac.emulate(c.q, k, v, keys=c.keys, log2w=c.log2w, defect="fold_on_next", **W4), c)
        assert caught("fold_on_next", rep, f"fold, slab 128, n = {c.keys.tolist()}, {poison}") == all_rows(c)


def test_rejects_a_ragged_row_stored_to_the_last_row():
    for Lq, rows in ((129, 128), (257, 256), (513, 256)):
        c = ac.selector_case(2, 2, Lq, ac.QUERY_EDGE_LK)
        rep = ac.check_selector(emu(c, defect="ragged_to_last", rows=rows, **W4), c, "w4")
        assert caught("ragged_to_last", rep, f"every query edge, Lq = {Lq}") == [(b, h, Lq - 1) for b in range(2) for h in range(2)]
    c = ac.selector_case(2, 2, 256, ac.QUERY_EDGE_LK)     # no ragged row, nothing to misplace
    assert ac.check_selector(emu(c, defect="ragged_to_last", rows=128, **W4), c, "w4").ok
