#!/usr/bin/env python3
"""Do two versions of the kernel sources compile to the same device code?

    tools/device_code_diff.py OLD_CSRC NEW_CSRC [-j N] [--keep DIR] [--by-kernel]

Compiles every .hip that OLD_CSRC's and NEW_CSRC's Makefiles list, device side only, with each Makefile's own flags
(CXXFLAGS plus the file's FLAGS_<name>) and one fixed -cuid, and compares the code objects byte by byte.  Needs no GPU.
It looks at bytes, not at instructions: "identical" means a host-only change left every kernel exactly as it was; a
file that differs, or that only one side has, is listed and the exit status is 1.

--by-kernel: a file that differs is compiled again on both sides with -S, and every kernel symbol is listed as
identical or different (its lines of assembly compared as text), with both sides' instruction counts and whether the
register, LDS and scratch figures of its metadata match.  It still compares and counts only.

(Without a fixed -cuid hipcc derives a __hip_cuid_<hash> symbol from the whole source text, so any edit would show.)
"""
import argparse
import concurrent.futures
import os
import re
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


def compile_device(csrc, src, flags, hipcc, out, mode="-c"):
    # run inside csrc on the bare file name, so that no path of the tree gets into the object
    cmd = [hipcc, *flags, "--offload-device-only", f"-cuid={CUID}", mode, src, "-o", out]
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
        args = (os.path.abspath(csrc), s, flags, base["HIPCC"])
        jobs[s] = (out, pool.submit(compile_device, *args, out), args)
    return jobs


RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels_of(asm):
    """{kernel symbol: (its lines of assembly, its instruction count, its resource lines in the metadata)}."""
    meta = {}
    for entry in re.split(r"\n  - (?=\.)", asm[asm.find("amdhsa.kernels:"):])[1:]:
        fields = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)$", "    " + entry, re.M))
        meta[fields[".name"]] = [fields.get(k) for k in RESOURCES]
    out = {}
    for name, res in meta.items():
        body = re.search(rf"^{re.escape(name)}:.*?^\.Lfunc_end\d+:", asm, re.M | re.S).group(0)
        body = re.sub(r"\.L(BB|func_end)\d+", r".L\1", body).splitlines()   # (labels carry the kernel's position in the file)
        out[name] = (body, sum(1 for line in body if re.match(r"\s+[a-z]", line)), res)
    return out


def by_kernel(name, old, new, tmp):
    sides = []
    for tag, side in (("old", old), ("new", new)):
        out = os.path.join(tmp, tag, name[:-4] + ".s")
        compile_device(*side[name][2], out, mode="-S")
        sides.append(kernels_of(open(out).read()))
    for k in sorted(set(sides[0]) | set(sides[1])):
        if k not in sides[0] or k not in sides[1]:
            print(f"    {k}: only in " + ("old" if k in sides[0] else "new"))
            continue
        (ba, na, ra), (bb, nb, rb) = sides[0][k], sides[1][k]
        print(f"    {k}: {'identical' if ba == bb else 'different'}, {na} vs {nb} instructions, "
              f"resources {'match' if ra == rb else f'DIFFER ({ra} vs {rb})'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compiles at a time")
    ap.add_argument("--keep", help="keep the code objects under DIR/old and DIR/new")
    ap.add_argument("--by-kernel", action="store_true", help="list the kernels of every file that differs")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="sf_device_code_")
    dirs = {k: os.path.join(tmp, k) for k in ("old", "new")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
        old, new = build_side(args.old, dirs["old"], pool), build_side(args.new, dirs["new"], pool)
        for _, fut, _ in list(old.values()) + list(new.values()):
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
        if args.by_kernel and verdict.startswith("DIFFERENT"):
            by_kernel(s, old, new, tmp)
    print(f"{len(set(old) | set(new)) - bad} identical, {bad} not")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
