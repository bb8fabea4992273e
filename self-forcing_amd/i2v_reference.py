"""Plain-torch restatement of the generator's i2v model type: `CausalWanModel(model_type='i2v')._forward_inference`
(wan/modules/causal_model.py:725-893) with `MLPProj` (wan/modules/model.py:469-481) and `WanI2VCrossAttention`
(model.py:222-266).  TEST INFRASTRUCTURE like `clip_reference.py`: the portable comparison target of the GPU path, itself
pinned to the reference's recorded outputs by tests/test_i2v_host.py.  Runs on the CPU; the product never calls it.

It composes the functions of `oracle.wan_oracle` (imported, not edited: patch embedding, time and text embeddings, self
attention over the KV cache, the head) with the three i2v pieces, and follows that oracle's two numeric modes, selected by
the dtype of the prepared weights: float32 (bf16-rounded weights, every operation in fp32) and bfloat16 (every torch
operation rounds its result as the reference's op sequence does; the two attention results are added in bf16).

The reference's own causal i2v path does not run as written.  The semantics here are the ones its
bidirectional `WanModel(model_type='i2v')` computes, with the caching of the causal model:
  * the patch embedding reads cat([x, y], channel) with y holding THIS call's frames;
  * the image keys / values are computed with the text keys / values when `is_init` is False and cached beside them
    ("k_img" / "v_img");
  * no mask on either key set.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
IMG_EMB_EPS = 1e-5    # nn.LayerNorm's default (model.py:474-477 pass none)


def _oracle():
    try:
        from oracle import wan_oracle
    except ImportError:   # the repository root is not on sys.path (an installed copy of the package has no oracle)
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import wan_oracle
    return wan_oracle


def oracle_config(shape):
    """The wan_oracle.OracleConfig of a WanShape."""
    wo = _oracle()
    return wo.OracleConfig(dim=shape.dim, ffn_dim=shape.ffn_dim, num_heads=shape.num_heads, num_layers=shape.num_layers, in_dim=shape.in_dim,
                           out_dim=shape.out_dim, freq_dim=shape.freq_dim, text_dim=shape.text_dim, text_len=shape.text_len, eps=shape.eps,
                           local_attn_size=shape.local_attn_size, sink_size=shape.sink_size)


def img_emb(W: Dict[str, Tensor], clip_fea: Tensor) -> Tensor:
    """MLPProj.forward, model.py:469-481: LayerNorm, Linear, GELU (erf), Linear, LayerNorm.  [B, 257, clip_dim] -> [B, 257, dim]."""
    p = "img_emb.proj."
    x = clip_fea.to(W[p + "1.weight"].dtype)
    x = F.layer_norm(x, (x.shape[-1],), W[p + "0.weight"], W[p + "0.bias"], IMG_EMB_EPS)
    x = F.gelu(F.linear(x, W[p + "1.weight"], W[p + "1.bias"]))
    x = F.linear(x, W[p + "3.weight"], W[p + "3.bias"])
    return F.layer_norm(x, (x.shape[-1],), W[p + "4.weight"], W[p + "4.bias"], IMG_EMB_EPS)


def image_kv(W: Dict[str, Tensor], pre: str, cfg, ctx_img: Tensor):
    """k_img = norm_k_img(k_img(ctx_img)), v_img = v_img(ctx_img) (model.py:255-256), each [B, 257, n, d]."""
    wo = _oracle()
    B = ctx_img.shape[0]
    k = wo.rms_norm(F.linear(ctx_img, W[pre + "k_img.weight"], W[pre + "k_img.bias"]), W[pre + "norm_k_img.weight"], cfg.eps)
    v = F.linear(ctx_img, W[pre + "v_img.weight"], W[pre + "v_img.bias"])
    return k.view(B, -1, cfg.num_heads, cfg.head_dim), v.view(B, -1, cfg.num_heads, cfg.head_dim)


def cross_attention(W: Dict[str, Tensor], pre: str, cfg, x: Tensor, context: Tensor, ctx_img: Tensor, cache: Optional[dict]) -> Tensor:
    """WanI2VCrossAttention.forward (model.py:240-266) with the cache of WanT2VCrossAttention (:171-186) extended to the
    image keys: out = o(attn(q, k, v) + attn(q, k_img, v_img)), the same normed q for both, no mask."""
    wo = _oracle()
    B, n, d = x.shape[0], cfg.num_heads, cfg.head_dim
    q = wo.rms_norm(F.linear(x, W[pre + "q.weight"], W[pre + "q.bias"]), W[pre + "norm_q.weight"], cfg.eps).view(B, -1, n, d)
    if cache is not None and cache["is_init"]:
        k, v, k_img, v_img = cache["k"], cache["v"], cache["k_img"], cache["v_img"]
    else:
        k = wo.rms_norm(F.linear(context, W[pre + "k.weight"], W[pre + "k.bias"]), W[pre + "norm_k.weight"], cfg.eps).view(B, -1, n, d)
        v = F.linear(context, W[pre + "v.weight"], W[pre + "v.bias"]).view(B, -1, n, d)
        k_img, v_img = image_kv(W, pre, cfg, ctx_img)
        if cache is not None:
            cache.update(is_init=True, k=k, v=v, k_img=k_img, v_img=v_img)
    o = wo.sdpa(q, k, v).flatten(2) + wo.sdpa(q, k_img, v_img).flatten(2)
    return F.linear(o, W[pre + "o.weight"], W[pre + "o.bias"])


def attention_block(W, i: int, cfg, x: Tensor, e0: Tensor, grid, rope, context: Tensor, ctx_img: Tensor, kv: dict, cross: Optional[dict],
                    current_start: int) -> Tensor:
    """CausalWanAttentionBlock.forward (causal_model.py:284-336) around the i2v cross-attention: wan_oracle.attention_block
    with one line changed."""
    wo = _oracle()
    pre = f"blocks.{i}."
    G = e0.shape[1]
    e = (W[pre + "modulation"].unsqueeze(1) + e0).chunk(6, dim=2)
    h = (wo._per_group(wo.layer_norm(x, cfg.eps), G) * (1 + e[1]) + e[0]).flatten(1, 2)
    y = wo.self_attention(W, pre + "self_attn.", cfg, h, grid, rope, kv, current_start)
    x = x + (wo._per_group(y, G) * e[2]).flatten(1, 2)
    x = x + cross_attention(W, pre + "cross_attn.", cfg, wo.layer_norm(x, cfg.eps, W[pre + "norm3.weight"], W[pre + "norm3.bias"]),
                            context, ctx_img, cross)
    h = (wo._per_group(wo.layer_norm(x, cfg.eps), G) * (1 + e[4]) + e[3]).flatten(1, 2)
    y = F.linear(wo.gelu_tanh(F.linear(h, W[pre + "ffn.0.weight"], W[pre + "ffn.0.bias"])), W[pre + "ffn.2.weight"], W[pre + "ffn.2.bias"])
    return x + (wo._per_group(y, G) * e[5]).flatten(1, 2)


def forward_inference(W: Dict[str, Tensor], cfg, x: Tensor, y: Tensor, t: Tensor, context: Tensor, clip_fea: Tensor, kv_cache: List[dict],
                      crossattn_cache: List[dict], current_start: int, rope=None) -> Tensor:
    """x [B, 16, F, H, W], y [B or 1, 20, F, H, W] (this call's frames), t [B, G], context [B, <= text_len, text_dim],
    clip_fea [B or 1, 257, clip_dim] -> flow [B, 16, F, H, W]."""
    wo = _oracle()
    dtype = W["patch_embedding.weight"].dtype
    if rope is None:
        rope = wo.rope_tables(cfg.head_dim)
    B = x.shape[0]
    assert x.shape[1] + y.shape[1] == W["patch_embedding.weight"].shape[1] and x.shape[2:] == y.shape[2:]
    tok, grid = wo.patch_embed(W, cfg, torch.cat([x.to(dtype), y.to(dtype).expand(B, -1, -1, -1, -1)], dim=1))
    e, e0 = wo.time_embeddings(W, cfg, t, dtype)
    ctx = wo.text_embedding(W, cfg, context.to(dtype))
    ctx_img = img_emb(W, clip_fea.expand(B, -1, -1))
    h = tok
    for i in range(cfg.num_layers):
        h = attention_block(W, i, cfg, h, e0, grid, rope, ctx, ctx_img, kv_cache[i], crossattn_cache[i], current_start)
    return wo.head_unpatchify(W, cfg, h, e.unflatten(0, tuple(t.shape)).unsqueeze(2), grid)


def wrapper_forward(W, cfg, sched, noisy: Tensor, y: Tensor, prompt_embeds: Tensor, clip_fea: Tensor, timestep: Tensor, kv_cache, crossattn_cache,
                    current_start: int, rope=None):
    """WanDiffusionWrapper.forward of an i2v generator (wan_oracle.wrapper_forward with the two image tensors):
    noisy [B, F, 16, H, W], y [B or 1, 20, F, H, W] -> (flow_pred, pred_x0), both [B, F, 16, H, W]."""
    wo = _oracle()
    flow = forward_inference(W, cfg, noisy.permute(0, 2, 1, 3, 4), y, timestep, prompt_embeds, clip_fea, kv_cache, crossattn_cache,
                             current_start, rope).permute(0, 2, 1, 3, 4)
    x0 = wo.flow_to_x0(sched, flow.flatten(0, 1), noisy.flatten(0, 1).to(flow.dtype), timestep.flatten(0, 1)).unflatten(0, flow.shape[:2])
    return flow, x0


# ------------------------------------------------------------------------------------------ the seeded test case
def synthetic_case(shape, seed: int = 0, frames: int = 3, H: int = 8, W: int = 12, prompt_len: int = 40) -> Dict[str, Tensor]:
    """The inputs of tests/golden/i2v_reduced.npz, regenerated from the seed (values rounded to bf16, held in float32):
    x [1, 16, F, H, W], y [1, 20, F, H, W], clip [1, 257, clip_dim], clip_other (an independent draw), pe [1, 512, text_dim]
    (rows from prompt_len on zero), and the inputs of the one-layer cross-attention case: attn_x [1, F h w, dim], attn_ctx
    [1, 512, dim], attn_img [1, 257, dim].  The fixture stores sums of these tensors: a torch whose generator draws other
    numbers is noticed."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()   # noqa: E731
    L = frames * (H // 2) * (W // 2)
    out = {"x": r(1, 16, frames, H, W), "y": r(1, shape.in_dim - 16, frames, H, W), "clip": r(1, shape.clip_len, shape.clip_dim),
           "clip_other": r(1, shape.clip_len, shape.clip_dim), "pe": r(1, shape.text_len, shape.text_dim),
           "attn_x": r(1, L, shape.dim), "attn_ctx": r(1, shape.text_len, shape.dim), "attn_img": r(1, shape.clip_len, shape.dim)}
    out["pe"][:, prompt_len:] = 0
    return out
