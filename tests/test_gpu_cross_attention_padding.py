"""Cross-attention over a prompt's padding: the identical trailing key rows of a K / V slab folded into ONE key whose
exp2-domain score carries log2(their number) (`ops.attention(..., keys, log2w)`, `ops.cross_fold_scan`, and the
wrapper's `fold_cross_padding`).

Tolerances are the existing contracts, nothing new: an attention kernel against fp32 softmax(QK^T)V <= 6e-3 relative
Frobenius (tests/test_gpu_ops.py); the folded form rounds same * p to bf16 once where the unfolded one rounds p and uses it
`same` times -- either way <= 2^-9 relative on the padding term."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import self_forcing_amd as sfa
from oracle import wan_oracle as wo
from self_forcing_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATT_TOL = 6e-3
LAT_H, LAT_W = 8, 12
FS = (LAT_H // 2) * (LAT_W // 2)
LENGTHS = (0, 1, 63, 64, 127, 200, 510, 511, 512)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def length_pairs(Lk):
    """Real lengths of the two samples of one launch, always different: everything folded into one key (0), one real key,
    the padding key closing a tile (63, 127) or opening one (64), same = 2 (Lk - 2), same = 1 (Lk - 1), no padding (Lk)."""
    ls = sorted({n for n in LENGTHS if n <= Lk} | {Lk - 2, Lk - 1, Lk})
    return [(ls[i], ls[(i + 3) % len(ls)]) for i in range(len(ls))]


def fold_of(lengths, Lk):
    same = [Lk - n for n in lengths]
    keys = torch.tensor([Lk if s <= 1 else Lk - s + 1 for s in same], dtype=torch.int32)
    log2w = torch.tensor([0.0 if s <= 1 else math.log2(s) for s in same], dtype=torch.float32)
    return keys.to(DEV), log2w.to(DEV)


@functools.lru_cache(maxsize=None)
def cases(Lk, Lq, family):
    """Inputs and the fp32 reference over ALL Lk keys, once per (slab, queries, family), shared by every structure.
    'random': N(0, 1) everywhere.  'aligned': the queries share a direction u and the padding key is a multiple of u, so
    that s_p (and the more so s_p + log2(same)) is every row's maximum by more than the lazy rescale's 2^8: the rescale
    fires in the last tile, on the key that carries the weight."""
    g = torch.Generator().manual_seed(1000 * Lk + 10 * Lq + len(family))
    B, H = 2, 2
    out = []
    for lens in length_pairs(Lk):
        q, k, v = bf((B, Lq, H, 128), g), bf((B, Lk, H, 128), g), bf((B, Lk, H, 128), g)
        kp, vp = bf((B, 1, H, 128), g), bf((B, 1, H, 128), g)
        if family == "aligned":
            u = torch.nn.functional.normalize(torch.randn(1, 1, H, 128, generator=g), dim=-1)
            q = (q.float() + 6.0 * u).to(torch.bfloat16)
            kp = (16.0 * u).expand(B, 1, H, 128).to(torch.bfloat16)
        for b, n in enumerate(lens):
            k[b, n:], v[b, n:] = kp[b], vp[b]
        ref = wo.sdpa(q.to(DEV).float(), k.to(DEV).float(), v.to(DEV).float())
        out.append((lens, q.to(DEV), k.to(DEV), v.to(DEV), ref))
    return out


@pytest.mark.parametrize("family", ["random", "aligned"])
@pytest.mark.parametrize("Lq", [72, 300])
@pytest.mark.parametrize("structure,Lk", [("r64", 512), ("w8", 512), ("w4", 512), ("auto", 512), ("w8", 128), ("w4", 128), ("auto", 128)])
def test_folded_attention_vs_fp32_over_all_padded_keys(structure, Lk, Lq, family):
    """Every structure, forced and AUTO, on a slab whose rows behind each sample's real length repeat one padding key,
    attending keys = length + 1 rows with log2(Lk - length) on the last one, against fp32 softmax(QK^T)V over all Lk rows.
    A sample without padding (and one with a single padded row) gives the same bits as the call without the counts."""
    for lens, q, k, v, ref in cases(Lk, Lq, family):
        keys, log2w = fold_of(lens, Lk)
        out = ops.attention(q, k, v, structure=structure, keys=keys, log2w=log2w)
        plain = ops.attention(q, k, v, structure=structure)
        err, err_plain = rel(out, ref), rel(plain, ref)
        print(f"{structure} Lk={Lk} Lq={Lq} {family} lengths={lens}: folded {err:.2e}, all keys {err_plain:.2e}")
        assert err < ATT_TOL, (lens, err)
        for b, n in enumerate(lens):
            assert rel(out[b], ref[b]) < ATT_TOL, (lens, b)
            if n >= Lk - 1:
                assert torch.equal(out[b], plain[b]), (lens, b)
    # no counts at all == the entry point without them
    assert torch.equal(ops.attention(q, k, v, structure=structure, keys=None, log2w=None), plain)


# ------------------------------------------------------------------------------------------ the scan, forwards, rollouts
@pytest.fixture(scope="module")
def sd_reduced():
    return sfa.synth_state_dict(sfa.WAN_REDUCED, seed=0)


def padded_prompts(lengths, g):
    pe = torch.randn(len(lengths), 512, sfa.WAN_REDUCED.text_dim, generator=g).to(torch.bfloat16)
    for b, n in enumerate(lengths):
        pe[b, n:] = 0
    return pe.to(DEV)


def make_pipe(sd, pe, fold=True, nfpb=1):
    args = SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True,
                           independent_first_frame=False, num_frame_per_block=nfpb, context_noise=0)
    gen = sfa.WanDiffusionWrapper(shape=sfa.WAN_REDUCED, state_dict=sd, timestep_shift=5.0, is_causal=True, device=DEV)
    gen.fold_cross_padding = fold
    return sfa.CausalInferencePipeline(args, DEV, generator=gen, text_encoder=sfa.FixedTextEncoder(pe), vae=sfa.IdentityVAE())


def one_forward(sd, pe, x, t, fold=True):
    pipe = make_pipe(sd, pe, fold)
    pipe.frame_seq_length = FS
    B = x.shape[0]
    pipe._initialize_kv_cache(B, torch.bfloat16, DEV, cache_tokens=2 * FS)
    pipe._initialize_crossattn_cache(B, torch.bfloat16, DEV)
    flow, x0 = pipe.generator(x, {"prompt_embeds": pe}, t, pipe.kv_cache1, pipe.crossattn_cache, 0)
    torch.cuda.synchronize()
    return pipe, flow, x0


def test_scan_counts_the_identical_trailing_rows_of_each_layers_cache(sd_reduced):
    g = torch.Generator().manual_seed(7)
    lengths = (37, 150)
    pe = padded_prompts(lengths, g)
    x = bf((2, 2, 16, LAT_H, LAT_W), g).to(DEV)
    t = torch.tensor([[750.0, 750.0], [500.0, 500.0]], device=DEV)
    pipe, _, _ = one_forward(sd_reduced, pe, x, t)
    ck, cv = [c["k"] for c in pipe.crossattn_cache], [c["v"] for c in pipe.crossattn_cache]
    assert len(ck) == 2
    for l in range(2):
        for b, n in enumerate(lengths):   # everything from the embeddings to the caches is row-wise: equal rows stay equal
            assert torch.equal(ck[l][b, n:], ck[l][b, -1:].expand_as(ck[l][b, n:]))
            assert torch.equal(cv[l][b, n:], cv[l][b, -1:].expand_as(cv[l][b, n:]))
    want_keys = torch.tensor([[n + 1 for n in lengths]] * 2, dtype=torch.int32)
    want_w = torch.tensor([[math.log2(512 - n) for n in lengths]] * 2)
    keys, log2w = pipe.generator._cross_fold_buffers(pipe.crossattn_cache, False)    # what the init_cross pass left behind
    assert torch.equal(keys.cpu(), want_keys) and torch.allclose(log2w.cpu(), want_w, rtol=0, atol=1e-6)
    keys, log2w = ops.cross_fold_scan(ck, cv)
    assert torch.equal(keys.cpu(), want_keys) and torch.allclose(log2w.cpu(), want_w, rtol=0, atol=1e-6)
    # one element of one padded V row of layer 1, sample 0: rows 401 .. 511 still repeat, nothing else moves
    cv[1][0, 400, 2, 5] += 1.0
    keys, log2w = ops.cross_fold_scan(ck, cv)
    want_keys[1, 0], want_w[1, 0] = 402, math.log2(111)
    assert torch.equal(keys.cpu(), want_keys) and torch.allclose(log2w.cpu(), want_w, rtol=0, atol=1e-6)
    # ... and in the last row but one of K: same = 1, nothing folded
    ck[0][1, 510, 0, 0] += 1.0
    keys, log2w = ops.cross_fold_scan(ck, cv)
    want_keys[0, 1], want_w[0, 1] = 512, 0.0
    assert torch.equal(keys.cpu(), want_keys) and torch.allclose(log2w.cpu(), want_w, rtol=0, atol=1e-6)
    assert log2w[0, 1].item() == 0.0
    # embeddings that are not padded: every key is attended
    pipe, _, _ = one_forward(sd_reduced, bf((2, 512, sfa.WAN_REDUCED.text_dim), g).to(DEV), x, t)
    keys, log2w = pipe.generator._cross_fold_buffers(pipe.crossattn_cache, False)
    assert torch.equal(keys.cpu(), torch.full((2, 2), 512, dtype=torch.int32)) and not log2w.any()


def test_forward_folded_vs_all_keys_and_batch_vs_alone(sd_reduced):
    g = torch.Generator().manual_seed(11)
    pe = padded_prompts((23, 190), g)
    x = bf((2, 2, 16, LAT_H, LAT_W), g).to(DEV)
    t = torch.tensor([[750.0, 750.0], [500.0, 500.0]], device=DEV)
    _, flow, x0 = one_forward(sd_reduced, pe, x, t)
    _, flow_all, x0_all = one_forward(sd_reduced, pe, x, t, fold=False)
    err = rel(flow, flow_all)
    print(f"forward, folded vs all 512 keys: {err:.2e}")
    assert err < ATT_TOL and rel(x0, x0_all) < ATT_TOL
    for b in range(2):
        _, f1, z1 = one_forward(sd_reduced, pe[b:b + 1], x[b:b + 1], t[b:b + 1])
        assert torch.equal(f1[0], flow[b]) and torch.equal(z1[0], x0[b])


def test_rollout_folded_paired_and_alone(sd_reduced):
    """Two chunks at batch 2, zero-padded prompts of different lengths: folded against all keys within the attention
    contract; the context pass paired with the next chunk's first pass, and each sample alone, give the same bits."""
    g = torch.Generator().manual_seed(13)
    pe = padded_prompts((61, 128), g)
    noise = bf((2, 2, 16, LAT_H, LAT_W), g).to(DEV)
    eps = [bf((2, 16, LAT_H, LAT_W), g) for _ in range(6)]

    def rollout(pe_, noise_, rows, fold=True, paired=True):
        pipe = make_pipe(sd_reduced, pe_, fold)
        pipe.pair_context_with_next = paired
        q = [e[rows] for e in eps]
        pipe.noise_source = lambda t: q.pop(0).reshape(t.shape)
        lat = pipe.inference(noise_, ["p"] * noise_.shape[0], return_latents=True)[1].clone()
        torch.cuda.synchronize()
        return lat

    both = slice(0, 2)
    lat = rollout(pe, noise, both)
    assert torch.equal(lat, rollout(pe, noise, both, paired=False))
    err = rel(lat, rollout(pe, noise, both, fold=False))
    print(f"rollout, folded vs all 512 keys: {err:.2e}")
    assert err < ATT_TOL
    for b in range(2):
        assert torch.equal(rollout(pe[b:b + 1], noise[b:b + 1], slice(b, b + 1))[0], lat[b])
