"""Generate the i2v golden fixture by running the REFERENCE on the CPU (build container only).

TEST INFRASTRUCTURE, like tools/make_golden_clip.py (nothing under oracle/ is touched): imports the reference's
`CausalWanModel` and `WanModel` through `oracle.ref_shim`, builds both with `model_type='i2v', in_dim=36` at the reduced
shape, swaps `img_emb` for `MLPProj(320, dim)` (the reference hard-codes 1280) and loads `synth_state_dict(WAN_I2V_REDUCED)`.

The reference's causal i2v path does not run as written: `CausalWanAttentionBlock` hands `crossattn_cache=` to a
`WanI2VCrossAttention.forward` that does not take it (causal_model.py:324-325, model.py:240).  A FORWARDING SHIM is
installed here: `forward(self, x, context, context_lens, crossattn_cache=None)` calls the original and drops the keyword.
It carries no arithmetic.  The recorded one-chunk causal output is compared with the bidirectional `WanModel` i2v forward
(which runs unmodified) on the same weights and inputs; their distance is stored, and tests/test_i2v_host.py bounds it.

    tests/golden/i2v_reduced.npz
      inputs        x, y, t (stored); clip, pe and the cross-attention case's inputs are regenerated from the seed by
                    `i2v_reference.synthetic_case` and pinned by their stored sums
      img_emb       MLPProj output, rows ROWS of the 257                                   fp32 + the reference's bf16
      cross_attn    WanI2VCrossAttention output of block 0 on the seeded case              fp32 + bf16
      one_chunk     3 frames of 8 x 12 latents from empty caches, t = 500                  fp32 + bf16
      two_chunk     1 frame at t = 0, then 2 frames at t = 700 over the grown KV cache     fp32 + bf16
      bidirectional WanModel(model_type='i2v') on the one-chunk case                       fp32
      k_img / v_img per layer, rows ROWS                                                   fp32 + bf16
      three numbers: the one-chunk causal-vs-bidirectional distance, the bf16-vs-fp32 distance, the clip-swap sensitivity

Weights are regenerated from the seed, not stored.  bf16 tensors are stored as their 16-bit patterns (uint16).

Usage: python tools/make_golden_i2v.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from self_forcing_amd import i2v_reference as ir  # noqa: E402
from self_forcing_amd import weights as wt  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "i2v_reduced.npz")
SEED, INPUT_SEED = 0, 7
FRAMES, H, W = 3, 8, 12
T_ONE, T_TWO = 500.0, (0.0, 700.0)
ROWS = tuple(range(0, 257, 16))              # the stored rows of every 257-row tensor: 0, 16, ..., 256


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def bits(t):
    return t.to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def main():
    from oracle import ref_shim
    ns = ref_shim.load()
    wm, wcm = ns.model_mod, ns.causal_mod
    s = wt.WAN_I2V_REDUCED
    sd = {k: v.float() for k, v in wt.synth_state_dict(s, seed=SEED).items()}
    cfg = dict(model_type="i2v", in_dim=s.in_dim, dim=s.dim, ffn_dim=s.ffn_dim, num_heads=s.num_heads, num_layers=s.num_layers,
               text_dim=s.text_dim, freq_dim=s.freq_dim, out_dim=s.out_dim)

    # the forwarding shim (see the module docstring): no arithmetic
    orig = wm.WanI2VCrossAttention.forward
    wm.WanI2VCrossAttention.forward = lambda self, x, context, context_lens, crossattn_cache=None: orig(self, x, context, context_lens)

    def build(cls):
        m = cls(**cfg).eval().requires_grad_(False)
        m.img_emb = wm.MLPProj(s.clip_dim, s.dim).eval().requires_grad_(False)
        res = m.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys, res.unexpected_keys
        assert all(k.startswith(("pose_proj", "freqs")) for k in res.missing_keys), res.missing_keys
        return m

    causal, bidir = build(wcm.CausalWanModel), build(wm.WanModel)
    case = ir.synthetic_case(s, INPUT_SEED, FRAMES, H, W)
    x, y, clip, pe = case["x"], case["y"], case["clip"], case["pe"]
    fs = (H // 2) * (W // 2)
    n, d = s.num_heads, s.head_dim

    def caches(dtype):
        kv = [{"k": torch.zeros(1, FRAMES * fs, n, d, dtype=dtype), "v": torch.zeros(1, FRAMES * fs, n, d, dtype=dtype),
               "global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])} for _ in range(s.num_layers)]
        cc = [{"k": torch.zeros(1, s.text_len, n, d, dtype=dtype), "v": torch.zeros(1, s.text_len, n, d, dtype=dtype), "is_init": False}
              for _ in range(s.num_layers)]
        return kv, cc

    def run(model, dtype, clip_fea):
        """(one-chunk, two-chunk, img_emb, cross_attn, [k_img], [v_img]) of `model` in `dtype`."""
        c = lambda t: t.to(dtype)  # noqa: E731
        call = lambda kv, cc, xs, ys, ts, start: model(c(xs), t=ts, context=c(pe), seq_len=32760, kv_cache=kv, crossattn_cache=cc,  # noqa: E731
                                                       current_start=start, cache_start=None, clip_fea=c(clip_fea), y=c(ys))
        with torch.no_grad():
            kv, cc = caches(dtype)
            one = call(kv, cc, x, y, torch.full((1, FRAMES), T_ONE), 0)
            kv, cc = caches(dtype)
            a = call(kv, cc, x[:, :, :1], y[:, :, :1], torch.full((1, 1), T_TWO[0]), 0)
            b = call(kv, cc, x[:, :, 1:], y[:, :, 1:], torch.full((1, FRAMES - 1), T_TWO[1]), fs)
            two = torch.cat([a, b], dim=2)
            ctx_img = model.img_emb(c(clip_fea))
            ca = model.blocks[0].cross_attn
            attn = ca(c(case["attn_x"]), torch.cat([c(case["attn_img"]), c(case["attn_ctx"])], dim=1), None)
            kimg = [blk.cross_attn.norm_k_img(blk.cross_attn.k_img(ctx_img)) for blk in model.blocks]
            vimg = [blk.cross_attn.v_img(ctx_img) for blk in model.blocks]
        return one.float(), two.float(), ctx_img.float(), attn.float(), [t.float() for t in kimg], [t.float() for t in vimg]

    ns.set_attention_dtype("input")
    one, two, emb, attn, kimg, vimg = run(causal, torch.float32, clip)
    one_swapped = run(causal, torch.float32, case["clip_other"])[0]
    with torch.no_grad():
        bi = bidir([x[0]], t=torch.tensor([T_ONE]), context=[pe[0]], seq_len=FRAMES * fs, clip_fea=clip, y=[y[0]])
    bi = torch.stack(list(bi)).float()

    ns.set_attention_dtype("bf16")
    causal16 = build(wcm.CausalWanModel).to(torch.bfloat16)
    one16, two16, emb16, attn16, kimg16, vimg16 = run(causal16, torch.bfloat16, clip)

    rows = list(ROWS)
    out = dict(
        seed=SEED, input_seed=INPUT_SEED, frames=FRAMES, H=H, W=W, t_one=T_ONE, t_two=np.array(T_TWO), rows=np.array(rows),
        x=bits(x), y=bits(y),
        input_sums=np.array([case[k].double().abs().sum().item() for k in ("clip", "clip_other", "pe", "attn_x", "attn_ctx", "attn_img")]),
        img_emb=emb[0, rows].numpy(), img_emb_bf16=bits(emb16[0, rows]),
        cross_attn=attn.numpy(), cross_attn_bf16=bits(attn16),
        one_chunk=one.numpy(), one_chunk_bf16=bits(one16), two_chunk=two.numpy(), two_chunk_bf16=bits(two16),
        bidirectional=bi.numpy(),
        k_img=torch.stack(kimg)[:, 0, rows].numpy(), v_img=torch.stack(vimg)[:, 0, rows].numpy(),
        k_img_bf16=bits(torch.stack(kimg16)[:, 0, rows]), v_img_bf16=bits(torch.stack(vimg16)[:, 0, rows]),
        causal_vs_bidirectional=rel(one, bi), bf16_vs_fp32=rel(one16, one), bf16_vs_fp32_two_chunk=rel(two16, two),
        bf16_vs_fp32_kv=max(rel(torch.stack(kimg16), torch.stack(kimg)), rel(torch.stack(vimg16), torch.stack(vimg))),
        clip_swap_sensitivity=rel(one_swapped, one),
    )
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    for k in ("causal_vs_bidirectional", "bf16_vs_fp32", "bf16_vs_fp32_two_chunk", "bf16_vs_fp32_kv", "clip_swap_sensitivity"):
        print(f"  {k} = {out[k]:.3e}")


if __name__ == "__main__":
    main()
