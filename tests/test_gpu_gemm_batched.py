"""GPU tests of sf_gemm_bf16's batched launches (one grid row per batch entry, as the text encoder's per-head products
use them) and of the direct epilogue that serves N % 8 == 4, ldo % 8 == 4 and the raw fp32 output.  Run with `-m gpu`.

Every comparison is elementwise against float64 computed on the host from the same bf16 inputs; no element is exempt.

Bounds (derived from the arithmetic, not from what the kernels give).  ref = the whole epilogue expression in float64,
absacc = |a| @ |w|^T in float64:
    bf16 outputs   |out - ref| <= 2^-8 |ref| + K 2^-22 absacc
    fp32 outputs   |out - ref| <=              K 2^-22 absacc
  * 2^-8 |ref| is the one round-to-nearest-even to bf16 at the end (8 significant bits: at most 2^-8 / (1 + 2^-8) of the
    value); the 2^-16 |ref| it leaves over covers the fp32 roundings of the bias, gate and residual arithmetic (2^-24 each).
  * (K - 1) 2^-24 sum |a_i w_i| bounds an fp32 accumulation of exact bf16 products in any order; x 4 because the MFMA's
    internal rounding mode is not documented as round-to-nearest-even.
  * The gate epilogue's reference applies bf16(gate_mod + gate_e0) as the kernel does: that rounding is specified.
  * The GELU epilogue gets an additive allowance for evaluating tanh-GELU in fp32, see test_direct_epilogue_every_structure.

Canaries.  Every output lives inside a larger buffer pre-filled with a NaN bit pattern.  After the launch everything the
product does not own must hold that pattern bit for bit: columns [N, ldo) of every row, rows >= M, the gaps between
batch entries, and a guard band in front of and behind the buffer."""
import pytest
import torch

from oracle.gemm_cases import INT, Canary, owned_mask          # the NaN-patterned output buffer, shared with test_gpu_gemm_exact.py
from self_forcing_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRUCTURES = ["t128", "pp256", "pp224", "pp192", "pp128"]


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def gemm_args(a_ptr, w_ptr, out_ptr, M, N, K, lda, ldw, ldo, epi=_lib.EPI_BIAS, bias=None, resid_ptr=None, ldr=0, batch=0,
              strides=(0, 0, 0, 0), structure="auto"):
    g = _lib.GemmArgs()
    g.a, g.w, g.out, g.bias, g.resid = a_ptr, w_ptr, out_ptr, None if bias is None else bias.data_ptr(), resid_ptr
    g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.ldr = M, N, K, lda, ldw, ldo, ldr
    g.epilogue, g.batch, g.structure, g.rows_per_group = epi, batch, _lib.GEMM_STRUCTURES[structure], 1
    g.a_bstride, g.w_bstride, g.o_bstride, g.r_bstride = strides
    return g


def launch(g):
    rc = _lib.lib().sf_gemm_bf16(g, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def last_error():
    return (_lib.lib().sf_last_error() or b"").decode()


def products(a, w):
    """float64 a @ w^T and |a| @ |w|^T of host tensors [..., M, K], [..., N, K]."""
    a, w = a.double(), w.double()
    return a @ w.transpose(-1, -2), a.abs() @ w.abs().transpose(-1, -2)


def assert_within(out, ref, absacc, K, bf16_out, extra=0.0, what=""):
    tol = K * 2.0 ** -22 * absacc + extra
    if bf16_out:
        tol = tol + 2.0 ** -8 * ref.abs()
    err = (out.double() - ref).abs()
    bad = ~(err <= tol)                         # (a NaN in `out` is bad too)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        worst = float((err / tol.clamp_min(1e-300))[~torch.isnan(err)].max()) if bool((~torch.isnan(err)).any()) else float("nan")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, first at {i}: out {float(out[i])} "
                             f"ref {float(ref[i])} tol {float(tol[i])}; worst err / tol {worst:.3f}")


# ------------------------------------------------------------------------------------------ the text encoder's three products
@pytest.mark.parametrize("L", [4, 100, 260])
@pytest.mark.parametrize("H", [1, 3])
def test_t5_logits_batched_f32(H, L):
    """q k^T of every head in one launch: q and k are the two halves of one [L, 2 * 64 H] tensor, head h reads columns
    [64 h, 64 h + 64) of each (lda = ldw = 128 H, batch stride 64), K = 64 is a single k-tile, the raw fp32 output's batch
    stride counts floats.  Every head has its own random slice, so a dropped or swapped stride changes the numbers."""
    g = torch.Generator().manual_seed(100 * H + L)
    lpad = (L + 63) // 64 * 64
    qk = bf((L, 128 * H), g)
    q, k = qk[:, :64 * H].reshape(L, H, 64).permute(1, 0, 2), qk[:, 64 * H:].reshape(L, H, 64).permute(1, 0, 2)
    ref, absacc = products(q, k)                                               # [H, L, L]
    qk_d = qk.to(DEV)
    n = H * L * lpad + 2 * lpad
    out = Canary(n, torch.float32)
    ga = gemm_args(qk_d.data_ptr(), qk_d.data_ptr() + 64 * H * 2, out.ptr(), L, L, 64, 128 * H, 128 * H, lpad, epi=_lib.EPI_F32, batch=H,
                   strides=(64, 64, L * lpad, 0))
    assert launch(ga) == 0, last_error()
    out.assert_untouched_outside(owned_mask(n, L, L, lpad, H, L * lpad))
    got = out.host()[:H * L * lpad].view(H, L, lpad)[:, :, :L]
    assert_within(got, ref, absacc, 64, bf16_out=False, what="logits")


@pytest.mark.parametrize("L", [4, 100, 260])
@pytest.mark.parametrize("H", [1, 3])
def test_t5_pv_batched_into_column_slices(H, L):
    """P V of every head in one launch: A = p [H][L][lpad], W = V^T [64 H][lpad] (64 rows per head: N = 64 < the 128-column
    tile, so the row clamp of the W loads acts inside every head), K = lpad in {64, 128, 320}; head h writes columns
    [64 h, 64 h + 64) of the [L, 64 H] output (ldo = 64 H, batch stride 64).  Columns [L, lpad) of p and V^T are zero."""
    g = torch.Generator().manual_seed(200 * H + L)
    lpad = (L + 63) // 64 * 64
    p = torch.rand((H, L, lpad), generator=g).to(torch.bfloat16)
    vt = bf((64 * H, lpad), g)
    p[:, :, L:] = 0
    vt[:, L:] = 0
    ref, absacc = products(p, vt.view(H, 64, lpad))                            # [H, L, 64]
    ref, absacc = ref.permute(1, 0, 2).reshape(L, 64 * H), absacc.permute(1, 0, 2).reshape(L, 64 * H)
    p_d, vt_d = p.to(DEV), vt.to(DEV)
    n = (L + 3) * 64 * H
    out = Canary(n, torch.bfloat16)
    ga = gemm_args(p_d.data_ptr(), vt_d.data_ptr(), out.ptr(), L, 64, lpad, lpad, lpad, 64 * H, batch=H, strides=(L * lpad, 64 * lpad, 64, 0))
    assert launch(ga) == 0, last_error()
    out.assert_untouched_outside(owned_mask(n, L, 64, 64 * H, H, 64))
    assert_within(out.host()[:L * 64 * H].view(L, 64 * H), ref, absacc, lpad, bf16_out=True, what="P V")


@pytest.mark.parametrize("K", [512, 64])
@pytest.mark.parametrize("L", [100, 260, 4])
def test_t5_v_transposed_leaves_padding_columns_alone(L, K):
    """V^T [64 H][L] = Wv xn^T written with ldo = lpad: N = L is 4 (mod 8) at every length here, so the direct epilogue
    stores it.  The encoder zeroes columns [L, lpad) once per pass and relies on every layer leaving them as they are."""
    H = 3
    g = torch.Generator().manual_seed(300 + L + K)
    lpad = (L + 63) // 64 * 64
    wv, xn = bf((64 * H, K), g, 1.0 / K ** 0.5), bf((L, K), g)
    ref, absacc = products(wv, xn)
    wv_d, xn_d = wv.to(DEV), xn.to(DEV)
    n = (64 * H + 3) * lpad
    out = Canary(n, torch.bfloat16)
    assert launch(gemm_args(wv_d.data_ptr(), xn_d.data_ptr(), out.ptr(), 64 * H, L, K, K, K, lpad)) == 0, last_error()
    out.assert_untouched_outside(owned_mask(n, 64 * H, L, lpad))
    assert_within(out.host()[:64 * H * lpad].view(64 * H, lpad)[:, :L], ref, absacc, K, bf16_out=True, what="V^T")


# ------------------------------------------------------------------------------------------ batch strides in general
@pytest.mark.parametrize("N", [72, 68])        # the LDS epilogue and the direct one
def test_batched_residual_with_its_own_stride_and_in_place(N):
    """bias + residual with batch = 3: the bias is shared by the batch, the residual has a row stride and a batch stride
    of its own (r_bstride != o_bstride), the outputs are separated by two unwritten rows.  Then once more with the
    residual aliasing the output.  Forcing a ping-pong structure on a batched product falls back to the 128 x 128
    kernel: same bits."""
    M, K, B = 130, 128, 3
    ldo, ldr = N + 8, N + 12
    o_bs, r_bs = (M + 2) * ldo, (M + 5) * ldr
    g = torch.Generator().manual_seed(400 + N)
    a, w, bias, resid = bf((B, M, K), g), bf((B, N, K), g, 1.0 / K ** 0.5), bf((N,), g, 0.5), bf((B, M + 5, ldr), g)
    y, absacc = products(a, w)
    ref = y + bias.double() + resid[:, :M, :N].double()
    a_d, w_d, bias_d, resid_d = a.to(DEV), w.to(DEV), bias.to(DEV), resid.to(DEV)
    n = B * o_bs
    owned = owned_mask(n, M, N, ldo, B, o_bs)

    def run(out, resid_ptr, ldr_, r_bs_, structure="auto", batch=B):
        ga = gemm_args(a_d.data_ptr(), w_d.data_ptr(), out.ptr(), M, N, K, K, K, ldo, epi=_lib.EPI_BIAS_RESID, bias=bias_d, resid_ptr=resid_ptr,
                       ldr=ldr_, batch=batch, strides=(M * K, N * K, o_bs, r_bs_), structure=structure)
        assert launch(ga) == 0, last_error()
        out.assert_untouched_outside(owned if batch == B else owned_mask(n, M, N, ldo, batch, o_bs))
        return torch.as_strided(out.host(), (batch, M, N), (o_bs, ldo, 1))

    out = Canary(n, torch.bfloat16)
    got = run(out, resid_d.data_ptr(), ldr, r_bs)
    assert_within(got, ref, absacc, K, bf16_out=True, what="batched residual")

    inplace = Canary(n, torch.bfloat16)
    torch.as_strided(inplace.region, (B, M, N), (o_bs, ldo, 1)).copy_(resid_d[:, :M, :N])
    assert torch.equal(run(inplace, inplace.ptr(), ldo, o_bs).view(torch.int16), got.view(torch.int16)), "resid aliasing out"

    two = run(Canary(n, torch.bfloat16), resid_d.data_ptr(), ldr, r_bs, structure="t128", batch=2)
    assert torch.equal(two.view(torch.int16), got[:2].view(torch.int16))
    forced = run(Canary(n, torch.bfloat16), resid_d.data_ptr(), ldr, r_bs, structure="pp256", batch=2)
    assert torch.equal(forced.view(torch.int16), two.view(torch.int16)), "pp256 forced on a batched product"


@pytest.mark.parametrize("epi", [_lib.EPI_F32, _lib.EPI_BIAS])
def test_batch_of_zero_or_one_ignores_the_strides(epi):
    """batch = 0 and batch = 1 are the unbatched product, whatever the stride fields hold."""
    M, N, K = 100, 100, 64
    dtype = torch.float32 if epi == _lib.EPI_F32 else torch.bfloat16
    g = torch.Generator().manual_seed(500)
    a_d, w_d = bf((M, K), g).to(DEV), bf((N, K), g).to(DEV)
    res = []
    for batch, strides in ((0, (0, 0, 0, 0)), (0, (64, 64, 256, 128)), (1, (64, 64, 256, 128))):
        out = Canary((M + 2) * 128, dtype)
        assert launch(gemm_args(a_d.data_ptr(), w_d.data_ptr(), out.ptr(), M, N, K, K, K, 128, epi=epi, batch=batch, strides=strides)) == 0, last_error()
        out.assert_untouched_outside(owned_mask(out.n, M, N, 128))
        res.append(out.host().view(INT[dtype]))
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2])


def test_batch_refusals_launch_nothing():
    M, N, K = 64, 64, 128
    a_d = torch.zeros(4 * M * K, dtype=torch.bfloat16, device=DEV)
    w_d = torch.zeros(4 * N * K, dtype=torch.bfloat16, device=DEV)
    scale = torch.ones(N, dtype=torch.float32, device=DEV)
    out = Canary(4 * M * N, torch.bfloat16)
    for strides in ((M * K + 4, N * K, M * N, 0), (M * K, N * K, M * N + 2, 0)):     # a_bstride % 8 != 0, o_bstride % 4 != 0
        assert launch(gemm_args(a_d.data_ptr(), w_d.data_ptr(), out.ptr(), M, N, K, K, K, N, batch=2, strides=strides)) != 0
        assert "batch strides" in last_error()
    ga = gemm_args(a_d.data_ptr(), w_d.data_ptr(), out.ptr(), M, N, K, K, K, N, batch=2, strides=(M * K, N * K, M * N, 0))
    rc = _lib.lib().sf_gemm_fp8(ga, scale.data_ptr(), M, scale.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and "bf16-only" in last_error()
    out.assert_untouched_outside(torch.zeros(out.n, dtype=torch.bool))


# ------------------------------------------------------------------------------------------ the direct epilogue
def _gelu_fp32_error(y):
    """Largest |gelu_fp32 - gelu_fp64| of torch's CPU tanh-GELU over the fp32 values of y."""
    y32 = y.float()
    gelu = torch.nn.functional.gelu
    return float((gelu(y32, approximate="tanh").double() - gelu(y32.double(), approximate="tanh")).abs().max())


@pytest.mark.parametrize("epi", ["bias", "gelu", "resid", "gate_resid"])
@pytest.mark.parametrize("M,N,K,ldo", [(300, 260, 128, 260), (300, 264, 128, 268), (1, 4, 128, 4)])
def test_direct_epilogue_every_structure(M, N, K, ldo, epi):
    """N % 8 == 4 with a tight ldo, N % 8 == 0 with ldo % 8 == 4, and the smallest product there is: the direct epilogue of
    the 128 x 128 kernel and the fall-back of every ping-pong structure.  The residual is a view of a wider tensor with
    ldr = 4 (mod 8).  The five structures agree bit for bit; the 128 x 128 one meets the elementwise bound.

    GELU allowance: 4 x the largest |gelu_fp32(y) - gelu_fp64(y)| of torch's CPU float32 tanh-GELU over this test's own y
    (measured on the host inside the test: 3.6e-7 at (300, 260, 128), 3.8e-7 at (300, 264, 128), 3.4e-8 at (1, 4, 128), so
    at most 1.5e-6 after the factor 4, which stands for the kernel's fast exponential and reciprocal)."""
    g = torch.Generator().manual_seed(M + N + K + ldo)
    ldr = N + (8 if N % 8 == 4 else 12)
    a, w, bias, resid_full = bf((M, K), g), bf((N, K), g, 1.0 / K ** 0.5), bf((N,), g, 0.5), bf((M, ldr), g)
    groups = 3 if M % 3 == 0 else 1
    gate_mod, e0 = bf((N,), g, 0.5), bf((groups, 6, N), g, 0.5)
    y, absacc = products(a, w)
    y = y + bias.double()
    resid = resid_full[:, :N]
    resid_d = resid_full.to(DEV)[:, :N]
    kw, extra = {}, 0.0
    if epi == "gelu":
        ref = torch.nn.functional.gelu(y, approximate="tanh")
        extra = 4 * _gelu_fp32_error(y)
        print(f"gelu allowance at {(M, N, K)}: 4 x {extra / 4:.3e}")
    elif epi == "resid":
        ref, kw = resid.double() + y, dict(resid=resid_d)
    elif epi == "gate_resid":
        gate = (gate_mod.float()[None] + e0[:, 2].float()).to(torch.bfloat16).double()
        ref = resid.double() + y * gate.repeat_interleave(M // groups, dim=0)
        kw = dict(resid=resid_d, gate_mod=gate_mod.to(DEV), gate_e0=e0.to(DEV)[:, 2], rows_per_group=M // groups)
    else:
        ref = y
    a_d, w_d, bias_d = a.to(DEV), w.to(DEV), bias.to(DEV)
    n = (M + 3) * ldo
    owned = owned_mask(n, M, N, ldo)
    first = None
    for structure in STRUCTURES:
        out = Canary(n, torch.bfloat16)
        view = out.region[:M * ldo].view(M, ldo)[:, :N]
        ops.gemm(a_d, w_d, bias_d, epilogue=epi, out=view, structure=structure, **kw)
        torch.cuda.synchronize()
        out.assert_untouched_outside(owned)
        got = out.host()[:M * ldo].view(M, ldo)[:, :N]
        if first is None:
            first = got
            assert_within(got, ref, absacc, K, bf16_out=True, extra=extra, what=f"{epi} {structure}")
        else:
            assert torch.equal(got.view(torch.int16), first.view(torch.int16)), f"{structure} differs from t128"
