"""Time an open-length session on the MI355X and write one JSON line.

One process, the 1.3B dims with seeded weights, 480 x 832 (60 x 104 latents), chunks of 3 latent frames, a rolling KV cache of
`local_attn_size` 21 frames, no decode (the VAE is the identity: the generator and the session's bookkeeping alone):

* `chunk_ms`: steady-state milliseconds per chunk (the cache full, every chunk evicting) of `open_session` fed the noise chunk by
  chunk against `stream()` of the same build on the same noise, the two taking turns inside every repeat;
* `evict`: `sf_kv_evict` over every layer's K and V with the steady-state plan (one chunk out, the window minus a chunk moved),
  which a chunk pays once, and its share of the session's chunk;
* `rebase_ms`: `WanDiffusionWrapper.rebase_positions` on the full cache (`sf_kv_rope_shift` over every layer's K and the index update);
* `memory`: `torch.cuda.memory_allocated` after chunk 20 and after chunk 400 of one session (1200 latent frames: it re-bases on the
  way), and the re-bases it made.

    python tools/live_session_bench.py [--iters 3] [--chunks 30] [--long_chunks 400] [--out profiles/live_session_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd import ops  # noqa: E402

CHUNK, H, W, WINDOW = 3, 60, 104, 21


def median(v):
    return round(sorted(v)[len(v) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=30, help="chunks per timed run; the first WINDOW / CHUNK + 1 fill the cache and are not counted")
    ap.add_argument("--long_chunks", type=int, default=400)
    ap.add_argument("--sink_size", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_session_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    shape = sfa.WAN_1_3B
    fs = (H // 2) * (W // 2)
    res = {"what": "live_session_bench", "dims": "1.3B", "lat_h": H, "lat_w": W, "frames_per_chunk": CHUNK, "local_attn_size": WINDOW,
           "sink_size": a.sink_size, "iters": a.iters, "chunks": a.chunks}
    gen = sfa.WanDiffusionWrapper(shape=shape, random_init_seed=0, timestep_shift=5.0, is_causal=True, local_attn_size=WINDOW,
                                  sink_size=a.sink_size, device=dev)
    enc = sfa.SyntheticTextEncoder(shape.text_len, shape.text_dim, device=dev)
    args = argparse.Namespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, independent_first_frame=False,
                              num_frame_per_block=CHUNK, context_noise=0)
    pipe = sfa.CausalInferencePipeline(args, dev, generator=gen, text_encoder=enc, vae=sfa.IdentityVAE())
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(1, a.chunks * CHUNK, 16, H, W, generator=g).to(torch.bfloat16).to(dev)
    steady = WINDOW // CHUNK + 1

    def per_chunk(chunks):
        """Wall milliseconds between the chunks of an iterator, each taken when its work has finished on the device."""
        out, t0 = [], time.perf_counter()
        for c in chunks:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out.append((t1 - t0) * 1e3)
            t0 = t1
        return out

    legs = {"stream": lambda: pipe.stream(noise, ["a prompt"], skip_last_context=False),
            "session": lambda: pipe.open_session(["a prompt"], (H, W), noise_feed=noise.split(CHUNK, dim=1))}
    times = {k: [] for k in legs}
    for it in range(1 + a.iters):
        for name, leg in legs.items():
            ms = per_chunk(leg())
            assert len(ms) == a.chunks
            if it:      # the first repeat warms up
                times[name].append(median(ms[steady:-1]))
        print(f"[live_session_bench] repeat {it}: " + ", ".join(f"{k} {v[-1] if v else '-'} ms/chunk" for k, v in times.items()), flush=True)
    res["chunk_ms"] = {k: {"median": median(v), "all": v} for k, v in times.items()}
    res["chunk_ms"]["session_over_stream"] = round(res["chunk_ms"]["session"]["median"] / res["chunk_ms"]["stream"]["median"], 4)

    # ---- eviction: every layer's K and V, the steady-state plan
    kv = pipe.kv_cache1
    sink, evict = a.sink_size * fs, CHUNK * fs
    keep = WINDOW * fs - evict - sink
    scratch = torch.empty(keep * shape.dim * 2, dtype=torch.uint8, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    evict_ms = []
    for it in range(2 + 10):
        e0, e1 = ev(), ev()
        e0.record()
        for d in kv:
            ops.kv_evict(d["k"], sink, evict, keep, scratch)
            ops.kv_evict(d["v"], sink, evict, keep, scratch)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            evict_ms.append(e0.elapsed_time(e1))
    res["evict"] = {"ms_per_chunk": median(evict_ms), "moved_bytes_per_chunk": 2 * 2 * len(kv) * keep * shape.dim * 2,
                    "share_of_session_chunk": round(median(evict_ms) / res["chunk_ms"]["session"]["median"], 4)}

    # ---- one re-base of the full cache
    rebase_ms = []
    for it in range(2 + 10):
        gen._write_indices(kv, 900 * fs, WINDOW * fs)
        e0, e1 = ev(), ev()
        e0.record()
        gen.rebase_positions(kv, 800, fs)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            rebase_ms.append(e0.elapsed_time(e1))
    res["rebase_ms"] = {"median": median(rebase_ms), "rotated_bytes": len(kv) * WINDOW * fs * shape.num_heads * 44 * 2}
    print(f"[live_session_bench] evict {res['evict']}, re-base {res['rebase_ms']}", flush=True)

    # ---- a long session: memory after chunk 20 and after chunk 400
    gd = torch.Generator(device=dev).manual_seed(1)
    session = pipe.open_session(["a prompt"], (H, W), generator=gd)
    memory = {}
    for out in session:
        k = out[0]
        del out
        if k in (20, a.long_chunks):
            torch.cuda.synchronize()
            memory[f"allocated_after_chunk_{k}"] = torch.cuda.memory_allocated()
        if k % 50 == 0:
            print(f"[live_session_bench] long session: chunk {k}, re-bases {session.rebases}", flush=True)
        if k == a.long_chunks:
            session.close()
    res["memory"] = dict(memory, latent_frames=(a.long_chunks + 1) * CHUNK, rebases=session.rebases)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
