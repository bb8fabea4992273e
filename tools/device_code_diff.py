#!/usr/bin/env python3
"""Do two versions of the kernel sources compile to the same device code?

    tools/device_code_diff.py OLD_CSRC NEW_CSRC [-j N] [--keep DIR]

Compiles every .hip that OLD_CSRC's and NEW_CSRC's Makefiles list, device side only, with each Makefile's own flags
(CXXFLAGS plus the file's FLAGS_<name>) and one fixed -cuid, and compares the code objects byte by byte.  Needs no GPU.
It looks at bytes, not at instructions: "identical" means a host-only change left every kernel exactly as it was; a
file that differs, or that only one side has, is listed and the exit status is 1.

(Without a fixed -cuid hipcc derives a __hip_cuid_<hash> symbol from the whole source text, so any edit would show.)
"""
import argparse
import concurrent.futures
import os
import subprocess
import sys
import tempfile

CUID = "sf-device-code-diff"


def make_vars(csrc, names):
    """The values make gives `names` in csrc's Makefile."""
    rule = "sf-print-vars: ; @printf '%s\\n' " + " ".join(f"'{n}=$({n})'" for n in names)
    out = subprocess.run(["make", "-s", "-C", csrc, "--no-print-directory", f"--eval={rule}", "sf-print-vars"],
                         check=True, capture_output=True, text=True).stdout
    return dict(line.split("=", 1) for line in out.splitlines() if "=" in line)


def compile_device(csrc, src, flags, hipcc, out):
    # run inside csrc on the bare file name, so that no path of the tree gets into the object
    cmd = [hipcc, *flags, "--offload-device-only", f"-cuid={CUID}", "-c", src, "-o", out]
    res = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"{csrc}/{src}: {' '.join(cmd)}\n{res.stderr}")


def build_side(csrc, outdir, pool):
    base = make_vars(csrc, ["HIPCC", "CXXFLAGS", "SRCS"])
    srcs = base["SRCS"].split()
    per_file = make_vars(csrc, [f"FLAGS_{s[:-4]}" for s in srcs])
    jobs = {}
    for s in srcs:
        flags = base["CXXFLAGS"].split() + per_file.get(f"FLAGS_{s[:-4]}", "").split()
        out = os.path.join(outdir, s[:-4] + ".co")
        jobs[s] = (out, pool.submit(compile_device, os.path.abspath(csrc), s, flags, base["HIPCC"], out))
    return jobs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compiles at a time")
    ap.add_argument("--keep", help="keep the code objects under DIR/old and DIR/new")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="sf_device_code_")
    dirs = {k: os.path.join(tmp, k) for k in ("old", "new")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
        old, new = build_side(args.old, dirs["old"], pool), build_side(args.new, dirs["new"], pool)
        for _, fut in list(old.values()) + list(new.values()):
            fut.result()
    bad = 0
    for s in sorted(set(old) | set(new)):
        if s not in old or s not in new:
            verdict = "only in " + ("old" if s in old else "new")
        else:
            a, b = (open(side[s][0], "rb").read() for side in (old, new))
            verdict = "identical" if a == b else f"DIFFERENT ({len(a)} vs {len(b)} bytes)"
        bad += verdict != "identical"
        print(f"{s:28s} {verdict}")
    print(f"{len(set(old) | set(new)) - bad} identical, {bad} not")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
