"""First use of the kernels that need more than 64 KiB of dynamic LDS (csrc/sf_launch.h registers a kernel's LDS cap with
the runtime once per device): made from four threads at once, and on a second device.  Each test runs in a fresh child
process (this file as a script), so that the calls really are the process's first.  Run with `-m gpu`.

The shapes are the smallest that reach each kernel, read from the dispatch code:
  gemm forced pp256 / pp224 / pp192 / pp128 at (300, 256, 128): 128 / 112 / 96 / 144 KiB (two k-tiles: the least the ping-pong takes)
  attention forced r64 at (B, H, Lq, Lk) = (1, 2, 100, 200): 112 KiB
  conv_igemm forced halo, [3, 16, 16, 32] -> Cout 96: 146 KiB; forced igemm at Cout 96 takes the 96-column tile (56 KiB, no
  registration), so Cout 192 is here too: the 192-column tile, 80 KiB
  small_linear / small_linear_fp8 at (8, 64, 5120): an 80 KiB activation stage
  clip_attention at L = 480 (CLIP_MAX_L): 157 KiB"""
import os
import subprocess
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
THREADS = 4


def _cases(dev):
    """[(name, call)]: every over-64-KiB kernel family once, on seeded inputs resident on `dev`."""
    from self_forcing_amd import ops
    from self_forcing_amd.vae import repack_conv
    g = torch.Generator().manual_seed(11)

    def bf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)

    cases = []
    a, w, b = bf(300, 128), bf(256, 128, scale=128 ** -0.5), bf(256)
    for st in ("pp256", "pp224", "pp192", "pp128"):
        cases.append((f"gemm {st}", lambda st=st: ops.gemm(a, w, b, structure=st)))
    q, k, v = bf(1, 100, 2, 128), bf(1, 200, 2, 128), bf(1, 200, 2, 128)
    cases.append(("attention r64", lambda: ops.attention(q, k, v, structure="r64")))
    x = bf(3, 16, 16, 32)
    for cout, sts in ((96, ("halo", "igemm")), (192, ("igemm",))):
        cw = repack_conv((torch.randn(cout, 32, 3, 3, 3, generator=g) * (27 * 32) ** -0.5).to(torch.bfloat16)).to(dev)
        cb = bf(cout, scale=0.1)
        for st in sts:
            cases.append((f"conv_igemm {st} cout {cout}", lambda cw=cw, cb=cb, st=st: ops.conv_igemm(x, cw, cb, (3, 3, 3), 1, structure=st)))
    sx, sw, sb = bf(8, 5120), bf(64, 5120, scale=5120 ** -0.5), bf(64)
    cases.append(("small_linear", lambda: ops.small_linear(sx, sw, sb)))
    swq, sws = sw.to(torch.float8_e4m3fn), (torch.rand(64, generator=g) + 0.5).to(dev)
    cases.append(("small_linear_fp8", lambda: ops.small_linear_fp8(sx, swq, sws, sb)))
    qkv = bf(1, 480, 3, 1, 80)
    cases.append(("clip_attention", lambda: ops.clip_attention(qkv)))
    return cases


def _child_concurrent():
    """Four threads, each on its own stream, released together into their first call of every case; then the same calls
    serially.  Every call must succeed and every thread's result equal the serial one bit for bit."""
    dev = torch.device("cuda:0")
    cases = _cases(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(THREADS)]
    torch.cuda.synchronize()
    barrier = threading.Barrier(THREADS)
    results, errors = [None] * THREADS, [None] * THREADS

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                barrier.wait(timeout=60)
                results[i] = [call() for _, call in cases]
            streams[i].synchronize()
        except BaseException as e:   # noqa: BLE001  (reported by the main thread)
            errors[i] = e
            barrier.abort()

    pool = [threading.Thread(target=work, args=(i,)) for i in range(THREADS)]
    for t in pool:
        t.start()
    for t in pool:
        t.join()
    assert errors == [None] * THREADS, errors
    serial = [call() for _, call in cases]
    torch.cuda.synchronize()
    for (name, _), ref, *per_thread in zip(cases, serial, *results):
        assert torch.isfinite(ref.float()).all(), name
        for i, out in enumerate(per_thread):
            assert torch.equal(out, ref), f"{name}: thread {i} differs from the serial call"
    print(f"concurrent first use: {len(cases)} cases x {THREADS} threads bit-equal to serial")


def _child_second_device():
    """The same first calls on device 0, then on device 1, in one process: all succeed, results bit-equal."""
    outs = []
    for d in (0, 1):
        with torch.cuda.device(d):
            outs.append([(name, call().cpu()) for name, call in _cases(torch.device("cuda", d))])
            torch.cuda.synchronize()
    for (name, r0), (_, r1) in zip(*outs):
        assert torch.equal(r0, r1), f"{name}: device 1 differs from device 0"
    print(f"second device: {len(outs[0])} cases bit-equal on devices 0 and 1")


def _run_child(mode):
    res = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=150)
    print(res.stdout)
    assert res.returncode == 0, f"child exited {res.returncode}\n{res.stdout}\n{res.stderr[-4000:]}"
    assert "bit-equal" in res.stdout


def test_concurrent_first_use_of_large_lds_kernels():
    _run_child("concurrent")


def test_first_use_on_a_second_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _run_child("second_device")


if __name__ == "__main__":
    {"concurrent": _child_concurrent, "second_device": _child_second_device}[sys.argv[1]]()
