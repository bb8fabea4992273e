"""The small kernels around the GEMMs, at the shapes and edges their one-shape tests never reached: the scheduler kernels
(x0 = xt - sigma flow, add_noise, the nearest-timestep lookup), patchify, the fused q/k norm + RoPE + cache append, the
cache eviction, and the small linear in bf16 and FP8.  Every device result is compared with the CPU oracle or with plain
float64 torch on the same inputs.

The tests without the `gpu` mark check the INPUTS of the x0 and lookup tests: that the data would tell a single
fp64 -> bf16 rounding from the reference's double one (fp64 -> fp32 -> bf16, what torch's `.to(bfloat16)` does on a
float64 tensor), and that the lookup's tie timesteps are true ties.  Without them a device test could pass for want of a
hard input."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import self_forcing_amd as sfa
from self_forcing_amd import fp8 as f8
from self_forcing_amd import ops
from oracle import wan_oracle as wo

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SCHED = wo.FlowMatchTables(5.0)
BF16 = torch.bfloat16


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


@functools.lru_cache(maxsize=None)
def opsgold():
    return np.load(os.path.join(GOLD, "ops.npz"))


# ================================================================================== 1. x0, add_noise, the sigma lookup
def head_from_flow(flow):
    """Inverse of the kernel's unpatchify layout: flow [B, F, C, H, W] -> head_out [B*F*(H/2)*(W/2), 4*C] with
    token (f, y//2, x//2) and column ((y&1)*2 + (x&1))*C + c."""
    B, F, C, H, W = flow.shape
    return flow.view(B, F, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 4, 6, 2).reshape(-1, 4 * C).contiguous()


def per_frame(ts, F):
    """timestep [B, groups] -> one per frame [B*F] (frame f belongs to group f // (F / groups))."""
    return ts.repeat_interleave(F // ts.shape[1], dim=1).reshape(-1)


def x0_fp64(flow, xt, ts_frames):
    """xt - sigma flow in float64, unrounded ([N, C, H, W] inputs, one timestep per N); the index as wo.flow_to_x0."""
    idx = torch.argmin((SCHED.timesteps.double()[None] - ts_frames.double()[:, None]).abs(), dim=1)
    return xt.double() - SCHED.sigmas.double()[idx].reshape(-1, 1, 1, 1) * flow.double()


def round_once_to_bf16(d):
    """float64 -> bf16 with ONE round-to-nearest-even, exactly, in integer arithmetic on the float64 bits (bf16 keeps 7
    of the 52 fraction bits; a carry out of the fraction moves into the exponent as it should)."""
    mag = d.abs()
    assert bool(((mag == 0) | ((mag >= 2.0 ** -126) & (mag < 2.0 ** 127))).all()), "outside bf16's normal range"
    b = d.contiguous().view(torch.int64)
    r = ((b + ((1 << 44) - 1) + ((b >> 45) & 1)) >> 45) << 45
    return r.view(torch.float64).to(BF16)      # (exact: the value is a bf16 number already)


def golden_x0():
    z = opsgold()
    return T(z["an_x0"]).to(BF16), T(z["x0_flow"]).to(BF16), T(z["an_t"]), T(z["x0_out_bf16"]).to(BF16)


@functools.lru_cache(maxsize=None)
def frame_480p():
    """One latent frame of the 480p workload (16 x 60 x 104 = 49920 pairs: above the 16384 the x0 kernel's grid covers
    in one pass), N(0, 1) data shared by the generic-sigma tests."""
    g = torch.Generator().manual_seed(60104)
    return bf((1, 1, 16, 60, 104), g), bf((1, 1, 16, 60, 104), g)


def generic_timesteps():
    warped = [float(v) for v in opsgold()["sched5_warped"]]
    return warped + [SCHED.timesteps[i].item() for i in (100, 300, 600, 900)]


# sigma has more than a few significant bits at these (833.33 and the four table entries); 1000, 937.5 and 625 give
# sigma = 1, 15/16 and 5/8, whose products with a bf16 number are exact in float32
GENERIC = [2, 4, 5, 6, 7]


def test_x0_inputs_tell_one_rounding_from_two():
    xt, flow, t, want = golden_x0()
    assert torch.equal(wo.flow_to_x0(SCHED, flow, xt, t), want)          # the oracle reproduces the recorded output
    once = round_once_to_bf16(x0_fp64(flow, xt, t))
    differ = [(once[i] != want[i]).sum().item() for i in range(3)]       # measured: [0, 38, 0] of 1536
    assert differ[0] == 0 and differ[2] == 0 and differ[1] >= 20, differ
    xt, flow = frame_480p()
    for i, ts in enumerate(generic_timesteps()):
        tt = torch.tensor([ts], dtype=torch.float32)
        share = (round_once_to_bf16(x0_fp64(flow[0], xt[0], tt)) != wo.flow_to_x0(SCHED, flow[0], xt[0], tt)).float().mean().item()
        # measured: 2.9 % at 833.33, 0.37 % / 0.44 % / 0.80 % / 1.5 % at table entries 100 / 300 / 600 / 900, 0 elsewhere
        assert (share >= 2e-3) if i in GENERIC else (share == 0), (ts, share)


def tie_timesteps(timesteps):
    """Midpoints of adjacent table entries that are float32 numbers: (midpoints, index of the upper neighbour)."""
    ts = timesteps.double()
    mid = (ts[:-1] + ts[1:]) / 2
    ok = mid.float().double() == mid
    return mid[ok].float(), torch.nonzero(ok).flatten()


def argmin_fp64(timesteps, t):
    return torch.argmin((timesteps.double()[None] - t.double()[:, None]).abs(), dim=1)


def test_lookup_inputs_are_true_ties():
    mid, lo = tie_timesteps(SCHED.timesteps)
    assert mid.numel() >= 500                                            # counted: 515 of 999
    ts = SCHED.timesteps.double()
    assert torch.equal(ts[lo] - mid.double(), mid.double() - ts[lo + 1]) and bool((ts[lo] > ts[lo + 1]).all())
    assert torch.equal(argmin_fp64(SCHED.timesteps, mid), lo)            # torch.argmin: the first of the two
    d = (ts[None] - torch.arange(0, 1001, dtype=torch.float64)[:, None]).abs()
    assert int(((d == d.min(dim=1, keepdim=True).values).sum(dim=1) > 1).sum()) == 0   # no integer timestep ties


def run_x0(flow, xt, ts):
    """flow, xt [B, F, C, H, W] bf16, ts [B, groups] -> the device's (flow, x0) on the host."""
    f, x0 = ops.unpatchify_x0(head_from_flow(flow).to(DEV), xt.to(DEV), ts.to(DEV), SCHED.sigmas.to(DEV), SCHED.timesteps.to(DEV))
    return f.cpu(), x0.cpu()


def assert_x0(flow, xt, ts, want=None):
    B, F = flow.shape[:2]
    got_flow, got = run_x0(flow, xt, ts)
    ref = wo.flow_to_x0(SCHED, flow.flatten(0, 1), xt.flatten(0, 1), per_frame(ts, F)).view_as(flow)
    if want is not None:
        assert torch.equal(ref, want.view_as(flow))
    bad = (got != ref).sum().item()
    print(f"x0 at t={ts.flatten().tolist()}: {bad} of {ref.numel()} elements differ from the reference")
    assert same_bits(got_flow, flow)
    assert torch.equal(got, ref), f"{bad} of {ref.numel()} elements differ"


@gpu
@pytest.mark.parametrize("B,F", [(1, 3), (3, 1)])
def test_unpatchify_x0_recorded_output(B, F):
    """The reference program's own recorded x0 (three frames at t = 937.5, 833.33, 625), as three frames of one sample
    with a timestep each and as three samples of one frame; then int64 timesteps against the oracle."""
    xt, flow, t, want = golden_x0()
    shape = (B, F, 16, 8, 12)
    assert_x0(flow.view(shape), xt.view(shape), t.view(B, F), want)
    assert_x0(flow.view(shape), xt.view(shape), torch.from_numpy(opsgold()["x0_ti"]).view(B, F))


@gpu
@pytest.mark.parametrize("case", range(8))
def test_unpatchify_x0_generic_sigma(case):
    xt, flow = frame_480p()
    assert_x0(flow, xt, torch.tensor([[generic_timesteps()[case]]], dtype=torch.float32))


@gpu
def test_unpatchify_x0_batches_and_groups():
    g = torch.Generator().manual_seed(24)
    xt, flow = bf((2, 4, 16, 8, 12), g), bf((2, 4, 16, 8, 12), g)
    ts = torch.tensor([[833.3333, SCHED.timesteps[300].item()], [SCHED.timesteps[900].item(), 1000.0]], dtype=torch.float32)
    assert_x0(flow, xt, ts)


@gpu
def test_add_noise_rows_longer_than_one_pass():
    """Rows of 16 x 90 x 160 = 230400 elements (720p): above the 131072 a row's workgroups cover in one pass."""
    g = torch.Generator().manual_seed(90160)
    x0, eps = bf((3, 16, 90, 160), g), bf((3, 16, 90, 160), g)
    for t in (torch.tensor([833.3333, SCHED.timesteps[100].item(), SCHED.timesteps[600].item()], dtype=torch.float32),
              torch.tensor([750, 1000, 3], dtype=torch.int64)):
        out = ops.add_noise(x0.to(DEV), eps.to(DEV), t.to(DEV), SCHED.sigmas.to(DEV), SCHED.timesteps.to(DEV))
        assert torch.equal(out.cpu(), SCHED.add_noise(x0, eps, t))


def index_coded_sigmas(n):
    """n distinct float32 values that are bf16 numbers (consecutive bit patterns from 0.125 up), so that add_noise(0, 1)
    returns sigma itself, exactly, and its bits name the table index."""
    return (torch.arange(n, dtype=torch.int32) + 0x3E00).to(torch.int16).view(BF16).float()


def device_lookup(timesteps, t):
    """The table index block_sigma_lookup picks for each timestep, read back through add_noise with rows of 8."""
    n = t.numel()
    out = ops.add_noise(torch.zeros(n, 8, dtype=BF16, device=DEV), torch.ones(n, 8, dtype=BF16, device=DEV), t.to(DEV),
                        index_coded_sigmas(timesteps.numel()).to(DEV), timesteps.to(DEV))
    idx = out.cpu().view(torch.int16).to(torch.int64) - 0x3E00
    assert bool((idx == idx[:, :1]).all())
    return idx[:, 0]


def assert_add_noise_rows(sigmas, timesteps, t, seed):
    """Rows of 8 random elements through add_noise with the table as given, against torch's fp32 formula at the index
    float64 argmin picks."""
    g = torch.Generator().manual_seed(seed)
    x0, eps = bf((t.numel(), 8), g), bf((t.numel(), 8), g)
    s = sigmas[argmin_fp64(timesteps, t)][:, None]
    want = ((1 - s) * x0 + s * eps).to(BF16)
    out = ops.add_noise(x0.to(DEV), eps.to(DEV), t.to(DEV), sigmas.to(DEV), timesteps.to(DEV))
    assert torch.equal(out.cpu(), want)


@gpu
def test_sigma_lookup_ties_and_range_ends():
    mid, lo = tie_timesteps(SCHED.timesteps)
    assert torch.equal(device_lookup(SCHED.timesteps, mid), lo)
    assert_add_noise_rows(SCHED.sigmas, SCHED.timesteps, mid, 1)
    outside = torch.tensor([1000.5, 2000.0, 0.0, -3.0], dtype=torch.float32)
    assert torch.equal(device_lookup(SCHED.timesteps, outside), torch.tensor([0, 0, 999, 999]))
    assert_add_noise_rows(SCHED.sigmas, SCHED.timesteps, outside, 2)
    ends = torch.tensor([1000, 0], dtype=torch.int64)
    assert torch.equal(device_lookup(SCHED.timesteps, ends), torch.tensor([0, 999]))
    assert_add_noise_rows(SCHED.sigmas, SCHED.timesteps, ends, 3)


@gpu
@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_sigma_lookup_custom_tables(n):
    """Tables shorter than, equal to a wave of, and one longer than the 256-thread workgroup: decreasing timesteps on a
    grid of 1/4 with random gaps (every midpoint is a float32 number and a tie), arbitrary sigmas."""
    g = torch.Generator().manual_seed(n)
    gaps = torch.randint(1, 9, (n,), generator=g).double() * 0.5
    timesteps = (gaps.flip(0).cumsum(0).flip(0) + 3.25).float()           # decreasing, last entry > 3.25
    sigmas = torch.rand(n, generator=g)
    mids = (timesteps[:-1] + timesteps[1:]) / 2
    t = torch.cat([timesteps, mids, timesteps + 0.125, timesteps - 0.125,
                   torch.tensor([timesteps[0].item() + 100, 0.0, -50.0])]).float()
    want = argmin_fp64(timesteps, t)
    assert torch.equal(want[n:2 * n - 1], torch.arange(n - 1))              # the ties resolve to the first entry
    assert torch.equal(device_lookup(timesteps, t), want)
    assert_add_noise_rows(sigmas, timesteps, t, n)
    ti = torch.tensor([int(timesteps[0].item()) + 7, int(timesteps[n // 2].item()), 0, -4], dtype=torch.int64)
    assert torch.equal(device_lookup(timesteps, ti), argmin_fp64(timesteps, ti))


# ================================================================================== 2. patchify
@gpu
@pytest.mark.parametrize("shape", [(1, 1, 16, 2, 2), (2, 3, 16, 6, 10), (1, 2, 3, 4, 6), (1, 21, 16, 90, 160)])
def test_patchify_is_a_pure_copy(shape):
    """cols[token (b, f, y//2, x//2)][c*4 + (y&1)*2 + (x&1)] = x[b, f, c, y, x]; the last shape has 1.2 Mi (token,
    channel) elements, more than the grid covers in one pass."""
    B, F, C, H, W = shape
    x = bf(shape, torch.Generator().manual_seed(H * W + C))
    want = x.view(B, F, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, C * 4)
    assert same_bits(ops.patchify(x.to(DEV)), want)


@gpu
def test_patchify_rejects_odd_sizes():
    with pytest.raises(sfa._lib.SfHipError, match="must be even"):
        ops.patchify(torch.zeros(1, 1, 16, 5, 6, dtype=BF16, device=DEV))
    with pytest.raises(sfa._lib.SfHipError, match="must be even"):
        ops.patchify(torch.zeros(1, 1, 16, 4, 7, dtype=BF16, device=DEV))


# ================================================================================== 3. qkv_norm_rope_cache
QKV_CASES = [(1, (1, 30, 52), 12, 20, 1560, 3200),      # the 1.3B model's frame (C = 1536) appended behind one frame
             (1, (3, 6, 10), 40, 1000, 7, 200),         # 14B heads (C = 5120); last time position 1002 of the 1024-entry table
             (2, (1, 7, 9), 8, 0, 0, 63)]               # fills the cache exactly
QKV_CASES += [(2, (2, 3, 5), 4 * n, 3, 11, 50) for n in (1, 2, 3, 4, 5, 6, 8, 10)]   # every channel-count instantiation


@gpu
@pytest.mark.parametrize("B,grid,H,start_frame,write_start,S", QKV_CASES)
def test_qkv_norm_rope_cache_shapes(B, grid, H, start_frame, write_start, S):
    f, h, w = grid
    g = torch.Generator().manual_seed(H * 1000 + h * w)
    C, L = H * 128, f * h * w
    qkv = bf((B * L, 3 * C), g)
    wq, wk = (1 + 0.1 * torch.randn(C, generator=g)).to(BF16), (1 + 0.1 * torch.randn(C, generator=g)).to(BF16)
    k0, v0 = bf((B, S, H, 128), g), bf((B, S, H, 128), g)               # sentinels: random, so a stray row shows
    kc, vc = k0.to(DEV), v0.to(DEV)
    cos, sin = sfa.model.rope_tables(128)
    q = ops.qkv_norm_rope_cache(qkv.to(DEV), wq.to(DEV), wk.to(DEV), kc, vc, cos.to(DEV), sin.to(DEV), grid, write_start, start_frame)
    q, kc, vc = q.view(B, L, H, 128).cpu(), kc.cpu(), vc.cpu()
    rc, rs, split = wo.rope_tables(128)
    x = qkv.view(B, L, 3, C)
    qr = wo.causal_rope_apply(wo.rms_norm(x[:, :, 0], wq, 1e-6).view(B, L, H, 128), grid, rc, rs, split, start_frame)
    kr = wo.causal_rope_apply(wo.rms_norm(x[:, :, 1], wk, 1e-6).view(B, L, H, 128), grid, rc, rs, split, start_frame)
    win = slice(write_start, write_start + L)
    # bounds of test_gpu_ops.test_qkv_norm_rope_cache_vs_oracle (same rounding points as the bf16 oracle; 1-ulp flips from
    # the fp32-vs-fp64 rotation), on K as well as Q and on each batch alone
    for b in range(B):
        for got, ref in ((q[b], qr[b]), (kc[b, win], kr[b])):
            assert rel(got, ref.float()) < 2e-3
            assert (got != ref).float().mean() < 0.02
    # V is a copy; both caches keep every row outside the window (whole tensors compared)
    v_want, k_want = v0.clone(), k0.clone()
    v_want[:, win] = x[:, :, 2].reshape(B, L, H, 128)
    assert same_bits(vc, v_want)
    k_want[:, win] = kc[:, win]
    assert same_bits(kc, k_want)


@gpu
def test_qkv_norm_rope_cache_error_paths():
    cos, sin = (t.to(DEV) for t in sfa.model.rope_tables(128))

    def call(H, grid, start_frame):
        C, L = H * 128, grid[0] * grid[1] * grid[2]
        qkv = torch.zeros(L, 3 * C, dtype=BF16, device=DEV)
        wn = torch.ones(C, dtype=BF16, device=DEV)
        kc = torch.zeros(1, L, H, 128, dtype=BF16, device=DEV)
        ops.qkv_norm_rope_cache(qkv, wn, wn, kc, kc.clone(), cos, sin, grid, 0, start_frame)

    call(4, (2, 2, 2), 1022)                                  # positions 1022, 1023: the table's last entries
    with pytest.raises(sfa._lib.SfHipError, match="table"):
        call(4, (2, 2, 2), 1023)
    with pytest.raises(sfa._lib.SfHipError, match="unsupported shape"):
        call(28, (1, 2, 2), 0)                                # C = 3584: seven chunks of 512, not instantiated


# ================================================================================== 4. kv_evict
@gpu
@pytest.mark.parametrize("S,H,sink,evict,keep", [(40, 4, 0, 6, 20),          # no sink
                                                 (64, 12, 8, 30, 10),        # source and destination disjoint
                                                 (64, 12, 8, 1, 55),         # maximal overlap, the window ends at S
                                                 (37, 40, 3, 5, 29),         # odd S, 14B heads
                                                 (3000, 12, 16, 100, 2800)]) # 8.6 MB per batch: more than one pass (8 MiB)
def test_kv_evict_windows(S, H, sink, evict, keep):
    B = 2
    cache = bf((B, S, H, 128), torch.Generator().manual_seed(S + evict)).to(DEV)
    want = cache.clone()
    want[:, sink:sink + keep] = cache[:, sink + evict:sink + evict + keep].clone()
    scratch = torch.empty(B * keep * H * 128 * 2, dtype=torch.uint8, device=DEV)
    ops.kv_evict(cache, sink, evict, keep, scratch)
    assert same_bits(cache, want)


@gpu
def test_kv_evict_noops_and_error_paths():
    B, S, H = 2, 40, 4
    cache = bf((B, S, H, 128), torch.Generator().manual_seed(9)).to(DEV)
    before = cache.clone()
    byte = torch.empty(1, dtype=torch.uint8, device=DEV)
    ops.kv_evict(cache, 8, 0, 20, byte)
    ops.kv_evict(cache, 8, 6, 0, byte)
    assert same_bits(cache, before)
    need = B * 20 * H * 128 * 2
    with pytest.raises(sfa._lib.SfHipError, match="scratch too small"):
        ops.kv_evict(cache, 8, 6, 20, torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(sfa._lib.SfHipError, match="window out of range"):
        ops.kv_evict(cache, 8, 6, S + 1 - 14, torch.empty(4 * need, dtype=torch.uint8, device=DEV))
    assert same_bits(cache, before)


# ================================================================================== 5. small_linear, bf16 and FP8
def act64(v, name):
    if name == "silu":
        return torch.nn.functional.silu(v)
    if name == "gelu":
        return torch.nn.functional.gelu(v, approximate="tanh")
    return v


def small_linear_inputs(M, K, N):
    g = torch.Generator().manual_seed(M * 100003 + K * 17 + N)
    return bf((M, K), g), bf((N, K), g, 0.05), bf((N,), g, 0.1)


def small_linear_ref(x, w, b, act_in, act_out, dtype=torch.float64):
    """act_out(act_in(x) @ w^T + b) on the bf16 inputs' values; the input activation is rounded to bf16, as the kernel
    stages it."""
    xin = act64(x.double(), act_in).to(BF16).to(dtype) if act_in else x.to(dtype)
    return act64(xin @ w.to(dtype).t() + b.to(dtype), act_out)


def _register_cases():
    """All 32 register-form instantiations (M 1..8 x K-step class x act_in) once, K and N cycling through their lists:
    K = 8, 200, 504 and 1032, 1280 are no multiples of the 512 elements a wave reads per step; N = 1, 3 are fewer
    columns than one wave's four, 130 is no multiple of four."""
    k_lists, n_list, act_out = ([8, 200, 504, 512], [1032, 1280, 1536]), [1, 3, 130, 1536], [None, "silu", "gelu"]
    cases, i, seen = [], 0, [0, 0]
    for M in range(1, 9):
        for cls in (0, 1):
            for act_in in (None, "silu"):
                K = k_lists[cls][seen[cls] % len(k_lists[cls])]
                seen[cls] += 1
                cases.append((M, K, n_list[(i + i // 4) % 4], act_in, act_out[i % 3]))
                i += 1
    return cases


REGISTER_CASES = _register_cases()
# N = 9216 (time_projection of the 1.3B model) needs 2304 waves = 256 workgroups of 9; 9222 columns need 2306 waves, which
# 256 workgroups cover only with ten waves each (sf_small_linear: wpb = min(10, max(4, ceil(waves / 256))))
WIDE_CASES = [(8, 1536, 9216, "silu", None), (8, 1536, 9222, "silu", "silu")]
_ACTS = [None, "silu", "gelu"]
LDS_CASES = [(M, K, N, _ACTS[(i + j) % 3], _ACTS[(i + k) % 3])
             for i, M in enumerate((9, 16, 21, 32)) for j, K in enumerate((64, 1024, 2048)) for k, N in enumerate((2, 130))]
LDS_CASES += [(10, 1024, 3, "silu", None), (2, 2048, 5, None, "gelu"),    # a 2-row pass (after an 8-row one, and alone)
              (3, 256, 130, "gelu", None),                                 # gelu in front is the LDS form's at any M
              (4, 5120, 64, None, None),                                   # 14B time projection: 4 rows x 10 KB of LDS
              (6, 5120, 64, None, None)]                                   # ... and 8 rows x 10 KB = 80 KB, above 64 KB
ALL_SMALL_LINEAR = REGISTER_CASES + WIDE_CASES + LDS_CASES

# Largest element error of a float32 evaluation of the reference formula against the float64 one over ALL_SMALL_LINEAR,
# measured on the CPU: 1.6e-6, at (M, K, N) = (6, 5120, 64) (test_small_linear_fp32_evaluation_error keeps the figure honest).
SL_FP32_ERROR = 2e-6


def bf16_step(v):
    """Spacing of bf16 numbers at magnitude v."""
    return 2.0 ** (math.floor(math.log2(v)) - 7)


def test_small_linear_case_lists_cover_the_dispatch():
    assert len(REGISTER_CASES) == 32
    assert {(M, (K + 511) // 512, a) for M, K, _, a, _ in REGISTER_CASES} == {(M, s, a) for M in range(1, 9) for s in (1, 3) for a in (None, "silu")}
    for pos, values in ((1, {8, 200, 504, 512, 1032, 1280, 1536}), (2, {1, 3, 130, 1536}), (4, {None, "silu", "gelu"})):
        assert {c[pos] for c in REGISTER_CASES} == values
    wpb = [min(10, max(4, ((N + 3) // 4 + 255) // 256)) for _, _, N, _, _ in WIDE_CASES]
    assert wpb == [9, 10]


def test_small_linear_fp32_evaluation_error():
    worst = 0.0
    for M, K, N, act_in, act_out in ALL_SMALL_LINEAR:
        x, w, b = small_linear_inputs(M, K, N)
        worst = max(worst, (small_linear_ref(x, w, b, act_in, act_out, torch.float32).double()
                            - small_linear_ref(x, w, b, act_in, act_out)).abs().max().item())
    assert worst <= SL_FP32_ERROR, worst


@gpu
@pytest.mark.parametrize("M,K,N,act_in,act_out", ALL_SMALL_LINEAR)
def test_small_linear_shapes(M, K, N, act_in, act_out):
    x, w, b = small_linear_inputs(M, K, N)
    ref = small_linear_ref(x, w, b, act_in, act_out)
    out = ops.small_linear(x.to(DEV), w.to(DEV), b.to(DEV), act_in, act_out).cpu()
    assert rel(out, ref) < 4e-3                                   # test_gpu_ops.test_small_linear's bound
    # element-wise: what fp32 arithmetic costs (SL_FP32_ERROR, measured) plus two bf16 steps at the output's largest
    # magnitude: half a step is the output's own rounding, the rest covers a last-bit flip of a staged bf16 activation
    err = (out.double() - ref).abs().max().item()
    assert err <= SL_FP32_ERROR + 2 * bf16_step(ref.abs().max().item()), err


def emulate_fp8(aq, sa, rps, wq, sw, bias):
    """test_gpu_fp8.emulate in float64 on the host: (aq * sa[seg(m)]) @ (wq * sw[n])^T + bias."""
    M = aq.shape[0]
    sa_row = sa.double().repeat_interleave(rps)[:M, None]
    return (aq.double() @ wq.double().t()) * sa_row * sw.double()[None] + bias.double()


@gpu
@pytest.mark.parametrize("M,N,K,rps,act_in", [(7, 130, 256, 3, None),      # ragged last segment (3 + 3 + 1 rows)
                                              (5, 3, 64, 8, None),         # rows_per_segment > M
                                              (32, 64, 8, 5, None),        # M = 32 (four LDS passes), K = 8
                                              (9, 1, 512, 9, "gelu"),      # gelu in front, N = 1
                                              (6, 66, 5120, 2, None)])     # K = 5120
def test_small_linear_fp8_segments(M, N, K, rps, act_in):
    g = torch.Generator().manual_seed(M * N + K)
    x, w, bias = bf((M, K), g, 2.0), bf((N, K), g, 1.0 / K ** 0.5), bf((N,), g, 0.5)
    xa = act64(x.float(), act_in).to(BF16)
    aq, sa = f8.quantize_rows(xa, rps)
    wq, sw = f8.quantize_weight([w])
    ref = emulate_fp8(aq, sa, rps, wq, sw, bias)
    out = ops.small_linear_fp8(x.to(DEV), wq.to(DEV), sw.to(DEV), bias.to(DEV), act_in, None, rows_per_segment=rps)
    assert rel(out, ref) < 4e-3                                   # test_gpu_fp8.test_small_linear_fp8_vs_emulation's bound
