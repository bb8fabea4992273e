"""The plain-C++ layer of csrc/sf_frame_host.h (what the frame and keypoint entry points share in front of their kernels)
on the host: tests/frame_host_main.cpp is compiled with the host compiler and run.  It shows that `disjoint` names the
first overlapping pair in declaration order for ranges that touch end to start, share one byte, nest, and come in reversed
address order, and that `frame_strides` gives the twelve strides of the three layouts at n=2, h=3, w=5.  (Built with
-fsanitize=address,undefined the same program is that layer's memory check.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_host_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (tried $CXX, c++, g++, clang++)")
    exe = tmp_path / "frame_host"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "self-forcing_amd", "csrc"),
                            os.path.join(ROOT, "tests", "frame_host_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
