"""The registry layer of csrc/sf_launch.h (on which devices a kernel's LDS cap is registered) as plain C++ on the host:
tests/launch_registry_main.cpp is compiled with the host compiler and run.  It shows that concurrent first calls on
several devices all find the cap registered before their launch, that a failed registration is returned and retried,
that device ordinals outside the record are served without indexing it, and that records are per kernel.  (Built with
-fsanitize=thread the same program is the registry's race check.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_registry_host_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (tried $CXX, c++, g++, clang++)")
    exe = tmp_path / "launch_registry"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "self-forcing_amd", "csrc"),
                            os.path.join(ROOT, "tests", "launch_registry_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
