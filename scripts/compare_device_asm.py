#!/usr/bin/env python3
"""Is the device code of two versions of the HIP sources the same?  (No GPU needed.)

    compare_device_asm.py OLD NEW [--jobs N] [--only norm_act.hip ...] [--rename FROM=TO ...]

OLD and NEW are two assembly files, two directories of `<source>.s` files, or two checkouts of this repository; a
checkout's SOURCES (calm-vit-dte_amd/build.py) are compiled with the build's FLAGS plus `--cuda-device-only -S` into a
temporary directory, at most --jobs compilers at a time.

The comparison is per function symbol, not per file: comments, debug / `.file` directives and blank lines are dropped
and local labels are renumbered in order of appearance, so moving or reordering host code, or code of OTHER kernels,
does not show.  What remains has to match exactly — instructions, registers, and the kernel descriptor
(`.amdhsa_*`: registers, LDS, scratch).  Exit status 0: the same kernels in every file, each with identical text.
A kernel's symbol holds the mangled types of its parameters, so renaming a parameter's struct renames the kernel:
--rename FROM=TO replaces FROM in OLD's text first (--rename NS_7AugNormE=5Norm3), and the kernels pair up again.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DROP = re.compile(r"\s*\.(file|loc|cfi_\w+|ident|addrsig\w*|p2align|section|text|type|size|globl|weak|protected|hidden)\b")
LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def functions(path, rename=()):
    """{symbol: normalised text}, set of kernel symbols."""
    funcs, kernels, cur, name = {}, set(), None, None
    for raw in open(path, errors="replace"):
        for old, new in rename:
            raw = raw.replace(old, new)
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, cur = m.group(1), funcs.setdefault(m.group(1), [])
            kernels.add(name)
        elif re.match(r"\s*\.end_amdhsa_kernel", line):
            cur = None
            continue
        elif re.match(r"\s*\.amdgpu_metadata|\s*\.section\s+\.debug|\s*\.section\s+\.AMDGPU\.csdata", line):
            cur = None
        m = re.match(r"(\w+):$", line)
        if m:
            name = m.group(1)
            cur = None if name.startswith("__hip_cuid_") else funcs.setdefault(name, [])   # (a per-compilation id)
            continue
        if cur is None or DROP.match(line):
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
            continue
        cur.append(line.strip())
    out = {}
    for sym, lines in funcs.items():
        ids = {}
        out[sym] = "\n".join(LOCAL.sub(lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), ln) for ln in lines)
    return out, kernels


def compile_tree(tree, outdir, jobs, only):
    spec = importlib.util.spec_from_file_location("calm_build", os.path.join(tree, "calm-vit-dte_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    sources = [s for s in build.SOURCES if not only or s in only]

    def one(src):
        cmd = [build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o",
                                                 os.path.join(outdir, src.replace(".hip", ".s"))]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(jobs) as pool:
        list(pool.map(one, sources))
    return outdir


def listing(arg, tmp, tag, jobs, only):
    if os.path.isfile(arg):
        return {os.path.basename(arg): arg}
    if os.path.exists(os.path.join(arg, "calm-vit-dte_amd", "build.py")):
        arg = compile_tree(arg, os.path.join(tmp, tag), jobs, only)
    return {f: os.path.join(arg, f) for f in sorted(os.listdir(arg)) if f.endswith(".s")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=[])
    ap.add_argument("--rename", nargs="*", default=[], metavar="FROM=TO")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for tag in ("old", "new"):
            os.makedirs(os.path.join(tmp, tag))
        old, new = (listing(p, tmp, t, min(a.jobs, 16), a.only) for p, t in ((a.old, "old"), (a.new, "new")))
        if os.path.isfile(a.old) and os.path.isfile(a.new):
            pairs = [(os.path.basename(a.new), a.old, a.new)]
        else:
            for f in sorted(set(old) ^ set(new)):
                print(f"{f}: only in {'OLD' if f in old else 'NEW'}")
                bad += 1
            pairs = [(f, old[f], new[f]) for f in sorted(set(old) & set(new))]
        for f, po, pn in pairs:
            (fo, ko), (fn, kn) = functions(po, [r.split("=", 1) for r in a.rename]), functions(pn)
            differ = sorted(s for s in set(fo) & set(fn) if fo[s] != fn[s])
            gone, added = sorted(set(fo) - set(fn)), sorted(set(fn) - set(fo))
            print(f"{f}: {len(kn)} kernels ({len(fn)} symbols); {len(differ)} differ, {len(gone)} gone, {len(added)} new")
            for s in differ + gone + added:
                print("    ", "differs" if s in differ else "gone" if s in gone else "new", s)
            bad += len(differ) + len(gone) + len(added)
    print("device code identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
