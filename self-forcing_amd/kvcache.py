"""KV-cache index arithmetic of the causal self-attention, on host integers, and the cache lists themselves.

Restates wan/modules/causal_model.py:202-236.  The reference keeps
`global_end_index` / `local_end_index` as device tensors and reads them back with `.item()` at
least twice per layer per forward; here the pipeline's integers drive the plan and the device
tensors are only kept up to date for schema compatibility.

The cache lists keep the reference's dict schema (causal_inference.py:278-312).  Lists built here carry three private
keys beside it, which no other module touches: every dict names the one int64 [L, 2] buffer its two index tensors are
views of, and the first layer's dict holds the list of those views and a host mirror of the indices.  Buffer and
mirror are trusted only while the dicts still hold the very tensors recorded with them (the reference's reset REBINDS
the index tensors, causal_inference.py:128-132); a cache built elsewhere has none of the keys and is driven the
reference's way.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch


@dataclass(frozen=True)
class CachePlan:
    evict: int        # tokens dropped from the window before writing (0 = no roll)
    keep: int         # tokens moved from [sink+evict, sink+evict+keep) to [sink, sink+keep)
    sink: int         # sink tokens that never move
    local_end: int    # new local_end_index
    global_end: int   # new global_end_index
    write_start: int  # new K/V rows go to [write_start, local_end)
    attn_start: int   # attention reads rows [attn_start, local_end)


def plan_cache_update(local_end: int, global_end: int, current_start: int, num_new: int, capacity: int,
                      local_attn_size: int, sink_tokens: int, max_attention_size: int) -> CachePlan:
    """One self-attention call's cache update.

    * re-running a chunk (current_end == global_end) overwrites its slots in place;
    * rolling mode (local_attn_size != -1): on overflow the oldest non-sink tokens are evicted;
    * global mode overflow is an error (the reference fails with a slice-shape RuntimeError,
      causal_model.py:228)."""
    current_end = current_start + num_new
    evict = keep = 0
    if local_attn_size != -1 and current_end > global_end and num_new + local_end > capacity:
        evict = num_new + local_end - capacity
        keep = local_end - evict - sink_tokens
        new_local_end = local_end + current_end - global_end - evict
    else:
        new_local_end = local_end + current_end - global_end
    write_start = new_local_end - num_new
    if keep < 0 or write_start < 0 or new_local_end > capacity:
        raise RuntimeError(
            f"KV cache overflow: writing tokens [{write_start}, {new_local_end}) into a cache of {capacity} "
            f"(local_end={local_end}, global_end={global_end}, current_start={current_start}, new={num_new}, "
            f"local_attn_size={local_attn_size})")
    return CachePlan(evict=evict, keep=keep, sink=sink_tokens, local_end=new_local_end, global_end=current_end,
                     write_start=write_start, attn_start=max(0, new_local_end - max_attention_size))


def _set_mirror(d0: dict, global_end: int, local_end: int) -> None:
    d0["_sf_mirror"] = (d0["global_end_index"], d0["local_end_index"], global_end, local_end)


def new_kv_cache(shape, n_layers: int, batch_size: int, cache_tokens: int, dtype, device) -> List[dict]:
    """Per-GPU KV cache, same dict schema as causal_inference.py:278-298.  The 2 x L index tensors are views of one
    [L, 2] buffer so one fill updates them all."""
    index_buffer = torch.zeros(n_layers, 2, dtype=torch.long, device=device)
    kv = []
    for i in range(n_layers):
        kv.append({
            "k": torch.zeros([batch_size, cache_tokens, shape.num_heads, shape.head_dim], dtype=dtype, device=device),
            "v": torch.zeros([batch_size, cache_tokens, shape.num_heads, shape.head_dim], dtype=dtype, device=device),
            "global_end_index": index_buffer[i, 0:1],
            "local_end_index": index_buffer[i, 1:2],
            "_sf_index_buffer": index_buffer,
        })
    _set_mirror(kv[0], 0, 0)
    # the forward call's last kernel writes all 2 x L indices at once while the dicts still hold THESE views
    kv[0]["_sf_index_views"] = [(d["global_end_index"], d["local_end_index"]) for d in kv]
    return kv


def reset_kv_indices(kv: List[dict]) -> None:
    buf = kv[0].get("_sf_index_buffer")
    if buf is not None:
        buf.zero_()
        _set_mirror(kv[0], 0, 0)
    else:  # foreign cache: rebind as the reference does (causal_inference.py:128-132)
        dev = kv[0]["k"].device
        for d in kv:
            d["global_end_index"] = torch.tensor([0], dtype=torch.long, device=dev)
            d["local_end_index"] = torch.tensor([0], dtype=torch.long, device=dev)


def shift_positions(kv_cache: List[dict], delta_tokens: int) -> None:
    """Subtract `delta_tokens` from every layer's `global_end_index` (and the host mirror): the cache's rows now stand
    `delta_tokens` earlier in the timeline.  `local_end_index` -- where they lie in the cache -- does not change.  The
    caller has re-based the cached keys' RoPE by as many frames (`WanDiffusionWrapper.rebase_positions`)."""
    global_end, local_end = read_indices(kv_cache)
    if delta_tokens < 0 or delta_tokens > global_end:
        raise ValueError(f"shift_positions: cannot move global_end={global_end} back by {delta_tokens} tokens")
    if delta_tokens == 0:
        return
    buf = shared_index_buffer(kv_cache)
    if buf is not None:
        buf[:, 0] -= delta_tokens
    else:
        for kv in kv_cache:
            kv["global_end_index"].sub_(delta_tokens)
    _set_mirror(kv_cache[0], global_end - delta_tokens, local_end)


def new_crossattn_cache(shape, n_layers: int, batch_size: int, dtype, device) -> List[dict]:
    """causal_inference.py:300-312.  For an i2v shape every dict also holds the image keys / values "k_img" / "v_img"
    [B, clip_len, H, D], filled with "k" / "v" by the pass that finds is_init False."""
    cache = [{
        "k": torch.zeros([batch_size, shape.text_len, shape.num_heads, shape.head_dim], dtype=dtype, device=device),
        "v": torch.zeros([batch_size, shape.text_len, shape.num_heads, shape.head_dim], dtype=dtype, device=device),
        "is_init": False,
    } for _ in range(n_layers)]
    if getattr(shape, "model_type", "t2v") == "i2v":
        add_image_cache(cache, shape, dtype, device)
    return cache


def add_image_cache(crossattn_cache: List[dict], shape, dtype, device) -> None:
    """Give every dict that lacks them the i2v "k_img" / "v_img" tensors (a cache built elsewhere, reference schema)."""
    batch_size = crossattn_cache[0]["k"].shape[0]
    for d in crossattn_cache:
        for name in ("k_img", "v_img"):
            if name not in d:
                d[name] = torch.zeros([batch_size, shape.clip_len, shape.num_heads, shape.head_dim], dtype=dtype, device=device)


def read_indices(kv_cache: List[dict]):
    """Host values of (global_end, local_end).  The pipeline's integers are mirrored in the
    first layer's dict; a mirror is valid only while the dict still holds the very index
    tensors we last updated (the reference's reset REBINDS them, causal_inference.py:128-132)."""
    d = kv_cache[0]
    mir = d.get("_sf_mirror")
    if mir is not None and mir[0] is d["global_end_index"] and mir[1] is d["local_end_index"]:
        return mir[2], mir[3]
    return int(d["global_end_index"].item()), int(d["local_end_index"].item())


def shared_index_buffer(kv_cache: List[dict]) -> Optional[torch.Tensor]:
    """The int64 [L, 2] buffer all layers' index tensors are views of (caches built by `new_kv_cache`), while the
    dicts still hold those very views; None for foreign or rebound caches."""
    d0 = kv_cache[0]
    buf, views = d0.get("_sf_index_buffer"), d0.get("_sf_index_views")
    if buf is None or views is None or len(views) != len(kv_cache):
        return None
    for kv, (g, l) in zip(kv_cache, views):
        if kv["global_end_index"] is not g or kv["local_end_index"] is not l:
            return None
    return buf


def write_indices(kv_cache: List[dict], global_end: int, local_end: int, done_by_kernel: bool = False) -> None:
    """causal_model.py:235-236.  With the shared buffer the forward call's last kernel has written every row
    (`kv_index_out`); foreign caches get the reference's per-layer fills.  The host mirror is refreshed either way."""
    if not done_by_kernel:
        for kv in kv_cache:
            kv["global_end_index"].fill_(global_end)
            kv["local_end_index"].fill_(local_end)
    _set_mirror(kv_cache[0], global_end, local_end)
