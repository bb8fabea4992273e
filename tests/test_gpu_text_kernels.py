"""GPU tests, kernel by kernel, of the row kernels around the text encoder and the i2v model type: sf_t5_softmax_bias,
sf_embedding_gather, sf_mul_bf16, sf_zero_masked_rows (t5_encoder.hip), sf_layernorm_rows and sf_patchify_i2v (i2v.hip),
through the C ABI.  Run with `-m gpu`.

Every comparison is elementwise against float64 (or bit for bit, for the kernels that only move data) computed on the
host from the same bf16 / fp32 inputs; no element is exempt.  Every output lies between guard bands pre-filled with a
NaN bit pattern that must survive the launch.

Bounds (from the arithmetic, not from what the kernels give):
  sf_t5_softmax_bias   |p - ref| <= 2^-8 ref + 1e-30.  One rounding to bf16 (8 significant bits) is at most
                       2^-8 / (1 + 2^-8) of the value; the 2^-16 ref = 1.5e-5 ref it leaves over covers the fp32 logit sum,
                       exponential, row sum and reciprocal (logits of magnitude up to 60: under 1e-5).  The floor covers
                       probabilities that underflow in fp32; the logits are built with an unmasked spread of at most 60
                       per row (e^-60 / 512 > 1e-29), so it excuses nothing visible.
                       Masked columns and columns [L, ld) are exactly +0; every row sums to 1 within 2^-7.
  sf_layernorm_rows    |out - ref| <= 2^-8 |ref| + 2^-20 (|w| |xhat| + |b|), xhat the float64 normalised value: the one
                       rounding to bf16, plus the fp32 statistics and the cancellation in xhat w + b (the kernel's
                       statistics and three fp32 operations per element come to about 2^-22 (|w| |xhat| + |b|)).
  sf_mul_bf16          bit-identical to bf16(float(a) * float(b)) wherever the exact product is zero or has a magnitude in
                       [2^-100, 2^100] (nothing near fp32's or bf16's subnormal range is claimed).
  the other three      bit-identical: they copy."""
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512
FILL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC5A5A5}     # quiet NaNs with a payload
INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def stream():
    return torch.cuda.current_stream().cuda_stream


def last_error():
    return (_lib.lib().sf_last_error() or b"").decode()


def random_bits(shape, g):
    """bf16 tensors of uniformly random bit patterns (NaN, inf, subnormals and -0 included): for kernels that only copy."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


class Guarded:
    """`n` elements of `dtype` on the device between two guard bands; bands and elements pre-filled with the NaN pattern."""

    def __init__(self, n, dtype=torch.bfloat16, init=None):
        self.n, self.dtype = n, dtype
        self.raw = torch.full((n + 2 * GUARD,), FILL[dtype], dtype=INT[dtype], device=DEV)
        self.region = self.raw[GUARD:GUARD + n].view(dtype)
        if init is not None:
            self.region.copy_(init.reshape(-1))

    def ptr(self):
        return self.region.data_ptr()

    def host(self):
        """The elements on the host, after checking both guard bands."""
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == FILL[self.dtype]).all()), "guard band in front of the output was written"
        assert bool((raw[GUARD + self.n:] == FILL[self.dtype]).all()), "guard band behind the output was written"
        return raw[GUARD:GUARD + self.n].view(self.dtype)


def bits(t):
    return t.contiguous().view(INT[t.dtype])


# ------------------------------------------------------------------------------------------ sf_t5_softmax_bias
def _mask(kind, L):
    m = torch.ones(L, dtype=torch.long)
    if kind == "first":
        m[1:] = 0
    elif kind == "all_but_last":
        m[L - 1:] = 0
    elif kind == "holes":                  # every third key off, the last key on
        m[1::3] = 0
        m[L - 1] = 1
    return m


def _softmax_case(H, L, ld, kind, spread, seed):
    """Inputs and float64 reference.  The TOTAL logits (s + bias) are drawn first, s is what is left after the bias: row 1
    of every head is a spike (key 0 is `spread - 10` above the rest), row 2 all-equal logits."""
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(32, H, generator=g) * 3).to(torch.bfloat16)
    rb = sfa.relative_position_buckets(L)
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
    bias = emb.double()[rb.long()[idx]].permute(2, 0, 1)                       # [H, L, L]
    total = (torch.rand(H, L, L, generator=g, dtype=torch.float64) - 0.5) * (spread - 1)
    if L > 1:
        total[:, 1] = (torch.rand(H, L, generator=g, dtype=torch.float64) - 0.5) * 8
        total[:, 1, 0] = 4 + (spread - 10)
    if L > 2:
        total[:, 2] = 0
    s = torch.zeros(H, L, ld)
    s[:, :, :L] = (total - bias).float()
    mask = _mask(kind, L)
    logits = s[:, :, :L].double() + bias                                       # what the kernel is asked for, exactly
    on = mask.bool()
    assert float((logits[:, :, on].amax(-1) - logits[:, :, on].amin(-1)).max()) <= spread
    ref = torch.softmax(logits.masked_fill(~on[None, None, :], float("-inf")), -1)
    if kind == "holes":                    # what a real pass leaves there: anything
        off = (~on).nonzero().flatten()
        for n, v in enumerate((1e4, float("inf"), float("nan"))):
            s[:, :, off[n::3]] = v
        s[:, :, L:] = float("nan")
    return s, emb, rb, mask, ref


def _run_softmax(s, emb, rb, mask, H, L, ld):
    p = Guarded(H * L * ld)
    s_d, e_d, r_d, m_d = s.to(DEV), emb.to(DEV), rb.to(DEV), mask.to(DEV)       # alive across the call
    _lib.check(_lib.lib().sf_t5_softmax_bias(s_d.data_ptr(), p.ptr(), e_d.data_ptr(), r_d.data_ptr(), m_d.data_ptr(), H, L, ld, stream()))
    torch.cuda.synchronize()
    return p.host().view(H, L, ld)


def _check_softmax(p, ref, mask, L):
    assert not bool(torch.isnan(p.float()).any())
    assert bool((bits(p[:, :, L:]) == 0).all()), "columns [L, ld) are not +0"
    assert bool((bits(p[:, :, :L][:, :, mask == 0]) == 0).all()), "masked columns are not +0"
    got = p[:, :, :L].double()
    err, tol = (got - ref).abs(), 2.0 ** -8 * ref + 1e-30
    bad = ~(err <= tol)
    if bool(bad.any()):
        h, i, j = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} probabilities out of bound, first at head {h} query {i} key {j}: {float(got[h, i, j])} vs "
                             f"{float(ref[h, i, j])}; worst err / tol {float((err / tol).max()):.2f}")
    assert float((got.sum(-1) - 1).abs().max()) <= 2.0 ** -7


@pytest.mark.parametrize("kind", ["all", "first", "all_but_last", "holes"])
@pytest.mark.parametrize("H,L,ld", [(1, 4, 4), (1, 4, 64), (3, 100, 128), (8, 256, 256), (2, 260, 320), (2, 512, 512)])
def test_t5_softmax_bias_elementwise(H, L, ld, kind):
    """Every probability of every row, the rows at both ends of the bucket table (queries 0 and L - 1; at L = 512 the
    distances beyond 128 saturate) like all others.  emb ~ N(0, 3^2), so a neighbouring bucket moves a probability by far
    more than the bound.  With the hole mask the masked logits hold +1e4, +inf and NaN and the padding columns NaN."""
    s, emb, rb, mask, ref = _softmax_case(H, L, ld, kind, 60, 1000 * H + L + ld)
    _check_softmax(_run_softmax(s, emb, rb, mask, H, L, ld), ref, mask, L)


def test_t5_softmax_bias_wide_spread_still_sums_to_one():
    """A spread of 200 between the unmasked logits of a row: most probabilities underflow, the row still sums to 1
    (checked within 2^-7 like everywhere) and holds no NaN."""
    H, L, ld = 2, 260, 320
    s, emb, rb, mask, ref = _softmax_case(H, L, ld, "holes", 200, 7)
    _check_softmax(_run_softmax(s, emb, rb, mask, H, L, ld), ref, mask, L)


# ------------------------------------------------------------------------------------------ sf_embedding_gather
def _gather(ids, table_d, vocab, dim):
    ids_d = ids.to(DEV)
    out = Guarded(ids.numel() * dim)
    _lib.check(_lib.lib().sf_embedding_gather(ids_d.data_ptr(), table_d.data_ptr(), out.ptr(), ids.numel(), dim, vocab, stream()))
    torch.cuda.synchronize()
    return out.host().view(ids.numel(), dim)


@pytest.mark.parametrize("dim", [8, 512, 2056, 4096])      # 2056: 257 chunks of 8, a second trip for thread 0 only
def test_embedding_gather_small(dim):
    """Rows 0 and vocab - 1, repeats, and the out-of-range ids -1, vocab and 2^40, which the C ABI clamps into the table."""
    vocab = 50
    table = random_bits((vocab, dim), torch.Generator().manual_seed(dim))
    table_d = table.to(DEV)
    for ids in ([0, vocab - 1, 3, 3, -1, vocab, 2 ** 40], [0], [vocab - 1], [-1], [vocab], [2 ** 40], [17]):     # 7 tokens and 1
        ids = torch.tensor(ids, dtype=torch.int64)
        want = table[ids.clamp(0, vocab - 1)]
        assert torch.equal(bits(_gather(ids, table_d, vocab, dim)), bits(want)), ids.tolist()


def test_embedding_gather_at_the_production_table_geometry():
    """umT5-XXL's table: 256384 rows of 4096, 2.1 GB, row offsets beyond 2^30 elements.  Only the gathered rows are
    initialised.  (The table has no row 262143 = 2^18 - 1: as an id it is out of range and clamps to the last row.)"""
    vocab, dim = 256384, 4096
    table_d = torch.empty(vocab, dim, dtype=torch.bfloat16, device=DEV)
    rows = [0, 1, 131072, vocab - 2, vocab - 1]
    vals = random_bits((len(rows), dim), torch.Generator().manual_seed(9))
    table_d[torch.tensor(rows, device=DEV)] = vals.to(DEV)
    ids = torch.tensor([vocab - 1, 131072, 0, 262143, 1, vocab - 2, 131072], dtype=torch.int64)
    pick = [4, 2, 0, 4, 1, 3, 2]
    got = _gather(ids, table_d, vocab, dim)
    del table_d
    torch.cuda.empty_cache()
    assert torch.equal(bits(got), bits(vals[pick]))


# ------------------------------------------------------------------------------------------ sf_mul_bf16
def _mul(a_d, b_d, out_ptr, n):
    rc = _lib.lib().sf_mul_bf16(a_d, b_d, out_ptr, n, stream())
    torch.cuda.synchronize()
    return rc


def _mul_operands(n, seed):
    """One operand walks over every finite bf16 value (a seeded shuffle, repeated or cut to n), the other over ten
    multipliers, so that over 8 x 65537 elements every value meets several of them."""
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    every = every[torch.isfinite(every.float())]
    every = every[torch.randperm(every.numel(), generator=torch.Generator().manual_seed(seed))]
    i = torch.arange(n)
    a = every[i % every.numel()]
    mult = torch.tensor([1, -1, 0.3, -0.3, 3, -3, 2.0 ** -60, -2.0 ** -60, 2.0 ** 60, -2.0 ** 60]).to(torch.bfloat16)
    b = mult[(i + i // every.numel()) % 10]
    return a, b


def _claimed(a, b):
    exact = (a.double() * b.double()).abs()
    return (exact == 0) | ((exact >= 2.0 ** -100) & (exact <= 2.0 ** 100))


@pytest.mark.parametrize("n", [8, 8 * 255, 8 * 256, 8 * 257, 8 * 65537])
def test_mul_bf16_bit_exact(n):
    a, b = _mul_operands(n, n)
    for x, y in ((a, b), (b, a)):
        want = (x.float() * y.float()).to(torch.bfloat16)
        ok = _claimed(x, y)
        x_d, y_d = x.to(DEV), y.to(DEV)
        out = Guarded(n)
        assert _mul(x_d.data_ptr(), y_d.data_ptr(), out.ptr(), n) == 0, last_error()
        assert torch.equal(bits(out.host())[ok], bits(want)[ok])


@pytest.mark.parametrize("alias", ["a", "b"])
def test_mul_bf16_in_place(alias):
    n = 8 * 257
    a, b = _mul_operands(n, 3)
    want = (a.float() * b.float()).to(torch.bfloat16)
    ok = _claimed(a, b)
    out = Guarded(n, init=a if alias == "a" else b)
    other = (b if alias == "a" else a).to(DEV)
    pa, pb = (out.ptr(), other.data_ptr()) if alias == "a" else (other.data_ptr(), out.ptr())
    assert _mul(pa, pb, out.ptr(), n) == 0, last_error()
    assert torch.equal(bits(out.host())[ok], bits(want)[ok])


def test_mul_bf16_inf_nan_and_refusal():
    inf, nan = float("inf"), float("nan")
    a = torch.tensor([inf, -inf, nan, inf, 0.0, 1.0, -2.0, inf, -inf, 3.0e38, -3.0e38, nan, 1.0, -0.0, 5.0, nan]).to(torch.bfloat16)
    b = torch.tensor([2.0, -1.0, 1.0, 0.0, inf, nan, -inf, inf, inf, 3.0e38, 3.0e38, nan, 1.0, 7.0, inf, 0.0]).to(torch.bfloat16)
    want = (a.float() * b.float()).to(torch.bfloat16)
    a_d, b_d = a.to(DEV), b.to(DEV)
    out = Guarded(16)
    assert _mul(a_d.data_ptr(), b_d.data_ptr(), out.ptr(), 16) == 0, last_error()
    got = out.host()
    assert torch.equal(torch.isnan(got.float()), torch.isnan(want.float()))
    fin = ~torch.isnan(want.float())
    assert torch.equal(bits(got)[fin], bits(want)[fin])              # +-inf (also from overflow), 1 and -0 as IEEE has them
    assert _mul(a_d.data_ptr(), b_d.data_ptr(), out.ptr(), 12) != 0 and "multiple of 8" in last_error()
    assert torch.equal(bits(out.host()), bits(got))                  # the refused call launched nothing


# ------------------------------------------------------------------------------------------ sf_zero_masked_rows
@pytest.mark.parametrize("kind", ["zeros", "ones", "holes"])
@pytest.mark.parametrize("dim", [8, 2056, 4096])
@pytest.mark.parametrize("rows", [1, 5, 300])
def test_zero_masked_rows(rows, dim, kind):
    """Rows with mask 0 become +0 in every element, whatever they held (NaN, inf, -0); every other row keeps its bits,
    for any non-zero mask value (the kernel tests != 0)."""
    g = torch.Generator().manual_seed(rows + dim)
    x = random_bits((rows, dim), g)
    x[:, 0], x[:, 1], x[:, 2] = float("nan"), float("inf"), -0.0
    if kind == "zeros":
        mask = torch.zeros(rows, dtype=torch.long)
    elif kind == "ones":
        mask = torch.ones(rows, dtype=torch.long)
    else:
        mask = torch.tensor([0, 1, 2, -1, 0, 1 << 40, 0])[(torch.arange(rows) + rows) % 7]
    want = torch.where((mask != 0)[:, None], bits(x), torch.zeros((), dtype=torch.int16))
    buf = Guarded(rows * dim, init=x)
    m_d = mask.to(DEV)
    assert _lib.lib().sf_zero_masked_rows(buf.ptr(), m_d.data_ptr(), rows, dim, stream()) == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(buf.host()).view(rows, dim), want)


# ------------------------------------------------------------------------------------------ sf_layernorm_rows
LN_KINDS = 4
LN_CONST = 3.140625


def _ln_row(kind, C, g):
    if kind == 0:
        return torch.randn(C, generator=g)
    if kind == 1:                          # a one-pass variance (E[x^2] - mean^2 in fp32) loses this row
        return 1000 + 4 * torch.randn(C, generator=g)
    if kind == 2:                          # variance 0: the output is the bias, exactly
        return torch.full((C,), LN_CONST)
    r = torch.randn(C, generator=g)
    r[int(torch.randint(C, (1,), generator=g))] = 3.0e4
    return r


def _ln_check(x, w, b, kinds, eps):
    M, C = x.shape
    xd, wd, bd = x.double(), w.double(), b.double()
    mean = xd.mean(-1, keepdim=True)
    xhat = (xd - mean) / torch.sqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + eps)
    ref = xhat * wd + bd
    tol = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * (wd.abs() * xhat.abs() + bd.abs())
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), b.to(DEV)
    out = Guarded(M * C)
    assert _lib.lib().sf_layernorm_rows(x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), out.ptr(), M, C, eps, stream()) == 0, last_error()
    torch.cuda.synchronize()
    got = out.host().view(M, C)
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        per_kind = {k: float((err / tol)[[i for i in range(M) if kinds[i] == k]].max()) for k in sorted(set(kinds))}
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements out of bound, first at row {r} (kind {kinds[r]}) column {c}: "
                             f"{float(got[r, c])} vs {float(ref[r, c])}; worst err / tol per row kind {per_kind}")
    for i in range(M):
        if kinds[i] == 2:
            assert torch.equal(bits(got[i]), bits(b)), f"constant row {i} is not the bias"
    inplace = Guarded(M * C, init=x)       # out may alias x
    assert _lib.lib().sf_layernorm_rows(inplace.ptr(), w_d.data_ptr(), b_d.data_ptr(), inplace.ptr(), M, C, eps, stream()) == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(inplace.host()), bits(got).view(-1))


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("M", [1, 4, 5, 257])             # the grid's last block is partly empty at 1, 5 and 257
@pytest.mark.parametrize("C", [8, 320, 512, 520, 1280, 5120])    # 520: a ragged last lane group; 5120: ten trips
def test_layernorm_rows(C, M, eps):
    """Rows of four kinds in turn: N(0, 1); N(1000, 4^2), which a one-pass variance loses; a constant row, whose output
    is the bias exactly; a row with one outlier of 3e4.  With M = 1 each kind is a launch of its own."""
    g = torch.Generator().manual_seed(C * 1000 + M)
    w = (1 + 0.5 * torch.randn(C, generator=g)).to(torch.bfloat16)
    b = (0.5 * torch.randn(C, generator=g)).to(torch.bfloat16)
    if M == 1:
        for kind in range(LN_KINDS):
            _ln_check(_ln_row(kind, C, g).to(torch.bfloat16)[None], w, b, [kind], eps)
        return
    kinds = [i % LN_KINDS for i in range(M)]
    x = torch.stack([_ln_row(k, C, g) for k in kinds]).to(torch.bfloat16)
    _ln_check(x, w, b, kinds, eps)


# ------------------------------------------------------------------------------------------ sf_patchify_i2v
@pytest.mark.parametrize("ymode", ["own", "shared", "window"])
@pytest.mark.parametrize("cx,cy,cpad", [(16, 20, 48), (16, 20, 36)])
@pytest.mark.parametrize("B,F,H,W", [(1, 1, 2, 2), (2, 3, 6, 10), (1, 21, 60, 104)])     # the last: 1.57 M items > 4096 x 256, the grid-stride loop
def test_patchify_i2v_bit_exact(B, F, H, W, cx, cy, cpad, ymode):
    """cat([x, y], channel) -> 2 x 2 patches -> columns c * 4 + p * 2 + q, zero-padded to cpad * 4.  y comes as its own
    [B, cy, F, H, W] tensor, as one image for the whole batch (batch stride 0), or as a frame window of a longer clip
    buffer (channel stride F_total H W), which is how the streaming path passes it."""
    g = torch.Generator().manual_seed(B + F + H + W + cpad)
    x = random_bits((B, F, cx, H, W), g)
    if ymode == "own":
        y_store = random_bits((B, cy, F, H, W), g)
        y, y_bs = y_store, cy * F * H * W
    elif ymode == "shared":
        y_store = random_bits((1, cy, F, H, W), g)
        y, y_bs = y_store.expand(B, cy, F, H, W), 0
    else:
        y_store = random_bits((B, cy, F + 3, H, W), g)
        y, y_bs = y_store[:, :, 1:1 + F], cy * (F + 3) * H * W
    y_cs, y_fs = y_store.stride(1), y_store.stride(2)
    cat = torch.cat([bits(x), bits(y).permute(0, 2, 1, 3, 4)], dim=2)          # [B, F, cx + cy, H, W]
    pat = cat.reshape(B, F, cx + cy, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, (cx + cy) * 4)
    want = torch.cat([pat, torch.zeros(pat.shape[0], (cpad - cx - cy) * 4, dtype=torch.int16)], dim=1)
    x_d, y_d = x.to(DEV), y_store.to(DEV)
    y_ptr = y_d.data_ptr() + (y_fs * 2 if ymode == "window" else 0)            # frame 1 of the clip buffer
    cols = Guarded(want.numel())
    assert _lib.lib().sf_patchify_i2v(x_d.data_ptr(), y_ptr, cols.ptr(), B, F, cx, cy, cpad, H, W, y_bs, y_cs, y_fs, stream()) == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(cols.host()).view(want.shape), want)
