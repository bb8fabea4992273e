"""GPU tests of the DiT row kernels of csrc/elementwise.hip -- layernorm_modulate, layernorm_affine, rmsnorm,
sinusoid_embedding -- at every instantiated width, at ragged tails and at modulation-group edges inside a wave's pair of
rows, in the layouts the forward uses; of the GEMM gate epilogue at the same group edges; and of one whole forward at an odd
group size (a 6 x 10 latent, 15 tokens per frame).  Run with `-m gpu`.

References, acceptance conditions and the per-row checkers are oracle/row_oracle.py's; tests/test_row_kernels_host.py shows
on the host that the same checkers reject a kernel that shares statistics or modulation between a wave's two rows, computes a
one-pass variance, misplaces eps, drops a ragged row, swaps shift and scale, forgets the `1 +`, rounds RMSNorm once or
divides by C - 1.  Every launch's rows cycle through the numeric families; `pytest -s` prints each launch's worst figures."""
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import _lib, ops
from oracle import row_oracle as ro
from oracle import wan_oracle as wo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FA5                      # a quiet NaN with a payload: nothing computes it
EPSES = (1e-6, 1e-5)


def stream():
    return torch.cuda.current_stream().cuda_stream


def last_error():
    return (_lib.lib().sf_last_error() or b"").decode()


def sentinel_rows(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int16, device=DEV)


def untouched(t):
    return bool((t == SENTINEL).all())


@lru_cache(maxsize=None)
def rows(M, width):
    return ro.make_rows(M, width, 1000 * M + width)          # modulate_case's rows


@pytest.fixture(scope="module", autouse=True)
def figures():
    """Collects every launch's (worst, share) per kernel and prints the extremes when the module is done."""
    seen = {}
    yield seen
    print("\nworst figures of the kernels over all launches:")
    for kernel in sorted(seen):
        print(f"  {kernel:<22} worst {max(w for w, _ in seen[kernel]):.3f}   differing at most {max(s for _, s in seen[kernel]) * 100:.4f} % of a launch")


def judge(rep, figures, kernel):
    print(rep.figures())
    figures.setdefault(kernel, []).append((rep.worst, rep.share))
    rep.assert_ok()


# ------------------------------------------------------------------------------------------ layernorm_modulate
MOD_CASES = [(1, 1), (2, 1), (7, 3), (45, 15), (96, 32), (257, 257), (10, 1000)]
LAYOUTS = list(ro.MOD_LAYOUTS)


def mod_inputs(M, width, rpg, layout):
    """Host tensors and their device twins: (x, names, mod_shift, mod_scale, e0_shift, e0_scale), then the same without names."""
    c = ro.modulate_case(M, width, rpg, layout)
    host = (c["x"], c["names"], c["mod_shift"], c["mod_scale"]) + ro.e0_views(c["e0"], layout)
    return host, (c["x"].to(DEV), c["mod_shift"].to(DEV), c["mod_scale"].to(DEV)) + ro.e0_views(c["e0"].to(DEV), layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,rpg", MOD_CASES)
@pytest.mark.parametrize("width", ro.WIDTHS)
def test_layernorm_modulate(width, M, rpg, layout, figures):
    (x, names, ms, mc, es, ec), (x_d, ms_d, mc_d, es_d, ec_d) = mod_inputs(M, width, rpg, layout)
    assert es_d.stride(0) == (width if layout == "head" else 6 * width)
    for eps in EPSES:
        out = ops.layernorm_modulate(x_d, ms_d, mc_d, es_d, ec_d, rpg, eps).cpu()
        ref = ro.ref_layernorm_modulate(x, ms, mc, es, ec, rpg, eps)
        judge(ro.check_layernorm(f"layernorm_modulate[{layout} M={M} rows_per_group={rpg} eps={eps:g}]", out, ref, names), figures,
              "layernorm_modulate")


# ------------------------------------------------------------------------------------------ layernorm_affine
@pytest.mark.parametrize("M", [1, 2, 3, 257])
@pytest.mark.parametrize("width", ro.WIDTHS)
def test_layernorm_affine(width, M, figures):
    x, names = rows(M, width)
    w, b = ro.make_params((width,), 5 * width + 1), ro.make_params((width,), 5 * width + 2)
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), b.to(DEV)
    for eps in EPSES:
        out = ops.layernorm_affine(x_d, w_d, b_d, eps).cpu()
        judge(ro.check_layernorm(f"layernorm_affine[M={M} eps={eps:g}]", out, ro.ref_layernorm_affine(x, w, b, eps), names), figures,
              "layernorm_affine")


# ------------------------------------------------------------------------------------------ no stray writes (C ABI)
@pytest.mark.parametrize("mode", ["modulate", "affine"])
@pytest.mark.parametrize("width", ro.WIDTHS)
def test_layernorm_writes_m_rows_and_no_more(width, mode, figures):
    """Odd M through the C ABI into the head of a larger sentinel-filled buffer: a wave's clamped second row, or a row count
    rounded up to the pair, would show behind row M - 1.  The buffer is larger than anything the kernel could touch."""
    M, rpg, spare = 7, 3, 9
    (x, names, ms, mc, es, ec), (x_d, ms_d, mc_d, es_d, ec_d) = mod_inputs(M, width, rpg, "cols34")
    buf = sentinel_rows(M + spare, width)
    lib = _lib.lib()
    if mode == "modulate":
        rc = lib.sf_layernorm_modulate(x_d.data_ptr(), buf.data_ptr(), M, width, 1e-6, ms_d.data_ptr(), mc_d.data_ptr(), es_d.data_ptr(),
                                       ec_d.data_ptr(), es_d.stride(0), rpg, stream())
        ref = ro.ref_layernorm_modulate(x, ms, mc, es, ec, rpg, 1e-6)
    else:
        rc = lib.sf_layernorm_affine(x_d.data_ptr(), ms_d.data_ptr(), mc_d.data_ptr(), buf.data_ptr(), M, width, 1e-6, stream())
        ref = ro.ref_layernorm_affine(x, ms, mc, 1e-6)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert untouched(buf[M:]), f"layernorm_{mode} C={width} M={M}: rows behind row {M - 1} were written"
    judge(ro.check_layernorm(f"layernorm_{mode}[C ABI M={M}]", buf[:M].view(torch.bfloat16).cpu(), ref, names), figures, f"layernorm_{mode}")


# ------------------------------------------------------------------------------------------ rmsnorm
@pytest.mark.parametrize("call", ["contiguous", "strided_input", "padded_output", "in_place"])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("width", ro.WIDTHS)
def test_rmsnorm(width, M, call, figures):
    x, names = rows(M, width)
    w = ro.make_params((width,), 7 * width)
    x_d, w_d = x.to(DEV), w.to(DEV)
    for eps in EPSES:
        plain = ops.rmsnorm(x_d, w_d, eps)
        if call == "contiguous":
            out = plain
        elif call == "strided_input":                          # the middle C columns of [M, 3C]
            wide = torch.randn(M, 3 * width, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(DEV)
            wide[:, width:2 * width] = x_d
            out = ops.rmsnorm(wide[:, width:2 * width], w_d, eps)
        elif call == "padded_output":                          # ldo = C + 8 inside a sentinel-filled buffer
            buf = sentinel_rows(M + 3, width + 8)
            out = ops.rmsnorm(x_d, w_d, eps, out=buf.view(torch.bfloat16)[:M, :width])
            torch.cuda.synchronize()
            assert untouched(buf[:M, width:]), f"rmsnorm C={width} M={M}: the 8 padding columns were written"
            assert untouched(buf[M:]), f"rmsnorm C={width} M={M}: rows behind row {M - 1} were written"
        else:                                                  # as the forward calls it
            out = x_d.clone()
            assert ops.rmsnorm(out, w_d, eps, out=out) is out
        assert torch.equal(out, plain), f"rmsnorm C={width} M={M} {call}: bits differ from the contiguous out-of-place call"
        judge(ro.check_rmsnorm(out.cpu(), ro.ref_rmsnorm(x, w, eps), names, f"rmsnorm[{call} M={M} eps={eps:g}]"), figures, "rmsnorm")


@pytest.mark.parametrize("why,width,ldx", [("ldx < C", 512, 504), ("ldx % 8 != 0", 512, 516), ("C = 3584", 3584, 3584)])
def test_rmsnorm_refuses(why, width, ldx):
    M = 3
    x_d = torch.zeros(M, max(width, ldx), dtype=torch.bfloat16, device=DEV)
    w_d = torch.ones(width, dtype=torch.bfloat16, device=DEV)
    buf = sentinel_rows(M + 1, width)
    rc = _lib.lib().sf_rmsnorm(x_d.data_ptr(), ldx, w_d.data_ptr(), buf.data_ptr(), width, M, width, 1e-6, stream())
    torch.cuda.synchronize()
    assert rc != 0, f"sf_rmsnorm accepted {why}"
    assert "sf_rmsnorm" in last_error(), last_error()
    assert untouched(buf), f"sf_rmsnorm refused {why} but wrote the output"


# ------------------------------------------------------------------------------------------ sinusoid_embedding
def timesteps(n, kind):
    if kind == "int64":
        return {1: torch.tensor([1000]), 3: torch.tensor([0, 250, 1000])}.get(n, torch.linspace(0, 1000, n).long())
    named = [937.5, 0.0, 1000.0, 833.3333, 1e-3]
    if n <= 3:
        return torch.tensor({1: named[:1], 3: named[2:]}[n], dtype=torch.float32)
    u = torch.linspace(0, 1, n - len(named), dtype=torch.float64)
    return torch.cat([torch.tensor(named, dtype=torch.float64), 1000 * 5 * u / (1 + 4 * u)]).float()     # shift-5 warped steps


@pytest.mark.parametrize("kind", ["float32", "int64"])
@pytest.mark.parametrize("dim", [2, 256, 258, 5120])
@pytest.mark.parametrize("n", [1, 3, 257])
def test_sinusoid_embedding(n, dim, kind, figures):
    t = timesteps(n, kind)
    assert t.numel() == n and t.dtype == getattr(torch, kind)
    out = ops.sinusoid_embedding(t.to(DEV), dim).cpu()
    assert out.shape == (n, dim)
    for rep in ro.check_sinusoid(out, ro.ref_sinusoid(t, dim), t, f"sinusoid_embedding[n={n} dim={dim} {kind}]"):
        judge(rep, figures, "sinusoid_embedding")


# ------------------------------------------------------------------------------------------ GEMM gate epilogue at group edges
@pytest.mark.parametrize("structure", ["t128", "pp256", "pp224", "pp192", "pp128"])
@pytest.mark.parametrize("rpg", [1, 15, 7])
@pytest.mark.parametrize("M,N,K", [(45, 64, 64), (45, 132, 64), (257, 384, 128)])
def test_gemm_gate_at_group_edges(M, N, K, rpg, structure):
    """gate_resid with m / rows_per_group changing inside a 16-row MFMA tile (and a ragged last group with 7): test_gemm's
    reference and its 4e-3 bound, applied to every row on its own, so that one row gated by its neighbour's group fails."""
    g = torch.Generator().manual_seed(M * 7 + N + K + rpg)
    bf = lambda shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)  # noqa: E731
    a, w, bias, resid = bf((M, K)), bf((N, K), 1.0 / K ** 0.5), bf((N,), 0.5), bf((M, N))
    G = (M + rpg - 1) // rpg
    gate_mod, e0 = bf((N,), 0.5), bf((G, 6, N), 0.5)
    gate = (gate_mod.float()[None] + e0[:, 2].float()).to(torch.bfloat16).double()                   # [G, N]
    assert torch.unique(gate, dim=0).shape[0] == G
    grp = ro.row_groups(M, rpg)
    ref = resid.double() + (a.double() @ w.double().t() + bias.double()) * gate[grp]
    out = ops.gemm(a.to(DEV), w.to(DEV), bias.to(DEV), epilogue="gate_resid", resid=resid.to(DEV), gate_mod=gate_mod.to(DEV),
                   gate_e0=e0.to(DEV)[:, 2], rows_per_group=rpg, structure=structure).double().cpu()
    rel = (out - ref).norm(dim=1) / ref.norm(dim=1)
    worst = int(rel.argmax())
    print(f"gemm gate_resid {structure} M={M} N={N} K={K} rows_per_group={rpg}: worst row {worst} (group {int(grp[worst])}) rel {float(rel[worst]):.2e}")
    assert float(rel[worst]) < 4e-3, (f"gemm gate_resid {structure} N={N}: row {worst} of group {int(grp[worst])} (rows_per_group {rpg}) is off by "
                                      f"{float(rel[worst]):.3e} of its norm")


# ------------------------------------------------------------------------------------------ a forward at an odd group size
def test_forward_with_15_tokens_per_frame_vs_oracle():
    """The reduced model on a 6 x 10 latent (15 tokens per frame), 3 frames x 2 samples with six different timesteps: the
    modulation groups of every LayerNorm and gate change at odd rows.  test_14b_layer_shape_vs_oracle's recipe and bound,
    the bound applied to every sample's every frame."""
    shape = sfa.WAN_REDUCED
    sd = sfa.synth_state_dict(shape, seed=3)
    g = torch.Generator().manual_seed(15)
    B, F, H, W = 2, 3, 6, 10
    fs = (H // 2) * (W // 2)
    assert fs == 15
    noisy = torch.randn(B, F, 16, H, W, generator=g).to(torch.bfloat16)
    pe = torch.randn(B, 512, shape.text_dim, generator=g).to(torch.bfloat16)
    pe[0, 90:] = 0
    pe[1, 33:] = 0
    ts = torch.tensor([[1000.0, 937.5, 833.3333], [625.0, 500.0, 250.0]])
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                           num_frame_per_block=1, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=shape, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV)
    pipe = sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe.to(DEV)), vae=sfa.IdentityVAE())
    pipe.frame_seq_length = fs
    pipe._initialize_kv_cache(B, torch.bfloat16, DEV, cache_tokens=F * fs)
    pipe._initialize_crossattn_cache(B, torch.bfloat16, DEV)
    flow, x0 = gen(noisy.to(DEV), {"prompt_embeds": pe.to(DEV)}, ts.to(DEV), pipe.kv_cache1, pipe.crossattn_cache, 0)
    Wf = wo.prepare_weights(sd, torch.float32)
    cfg = wo.OracleConfig(dim=shape.dim, ffn_dim=shape.ffn_dim, num_heads=shape.num_heads, num_layers=shape.num_layers, text_dim=shape.text_dim)
    kv, ca = wo.init_kv_cache(cfg, B, F * fs, torch.float32), wo.init_crossattn_cache(cfg, B, torch.float32)
    rf, rx = wo.wrapper_forward(Wf, cfg, wo.FlowMatchTables(5.0), noisy.float(), pe.float(), ts, kv, ca, 0)
    kgot = pipe.kv_cache1[1]["k"].double().cpu().reshape(B, F, -1)
    kref = kv[1]["k"].double().reshape(B, F, -1)
    for name, got, ref in (("flow", flow, rf), ("x0", x0, rx), ("layer 1 K cache", kgot, kref)):
        got, ref = got.double().cpu().reshape(B, F, -1), ref.double().reshape(B, F, -1)
        rel = (got - ref).norm(dim=2) / ref.norm(dim=2)
        print(f"forward, 15 tokens per frame: {name} rel per sample and frame {[[f'{v:.2e}' for v in r] for r in rel.tolist()]}")
        for b in range(B):
            for f in range(F):
                assert float(rel[b, f]) < 2e-2, f"{name}: sample {b} frame {f} (timestep {float(ts[b, f])}, rows {f * fs}..{f * fs + fs - 1}) is off by {float(rel[b, f]):.3e}"
