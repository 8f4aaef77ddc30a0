#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two csrc directories kernel by kernel (no GPU needed).

    python tools/kernel_asm_diff.py OLD_CSRC NEW_CSRC [--rename OLD=NEW ...] [--glob PATTERN] [--jobs N] [--keep DIR]

Every tdx_*.hip of both directories is compiled with the Makefile's CXXFLAGS plus `--cuda-device-only -S`.  Per kernel
(.amdhsa_kernel name) two pieces of text are compared: the body, from the kernel's label to its .size line, and the
descriptor, .amdhsa_kernel ... .end_amdhsa_kernel.  __hip_cuid_<hex> and the function ordinal in local labels (set to 0) are
normalised; --rename replaces substrings of the
old tree's mangled names (a renamed parameter type) before the comparison.  Exit status 0 only if every kernel is
identical and none is added or lost.
"""
import argparse
import concurrent.futures as cf
import pathlib
import re
import subprocess
import sys
import tempfile


def cxxflags(csrc):
    mk = (csrc / "Makefile").read_text()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    return hipcc, flags.replace("$(ARCH)", arch).split()


def compile_one(hipcc, flags, src, out):
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src.name, "-o", str(out)], cwd=src.parent,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{src}: {r.stderr}")
    return out


def kernels(asm_text, renames):
    """{kernel name: (body, descriptor)} of one assembly file."""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", asm_text)
    # local labels carry the function's ordinal in its file (.LBB<f>_<n>, BB<f>_<n> in comments -- branch targets and loop nests --, .Lfunc_end<f>): it moves when a kernel in front
    # of this one is added, lost or turned into a template, and says nothing about this one
    text = re.sub(r"(\.L|=|Loop )BB\d+_(\d+)", r"\1BB0_\2", text)
    text = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end0", text)
    text = re.sub(r"^(\.LBB0_\d+:)[ \t]+;", r"\1 ;", text, flags=re.M)  # the comment column depends on the ordinal's digits
    for old, new in renames:
        text = text.replace(old, new)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^%s:.*?^\s*\.size\s+%s,[^\n]*\n" % (re.escape(name), re.escape(name)), text, re.M | re.S)
        out[name] = (body.group(0) if body else None, m.group(2))
    return out


def tree_kernels(csrc, outdir, jobs, renames, glob):
    hipcc, flags = cxxflags(csrc)
    srcs = sorted(csrc.glob(glob))
    outdir.mkdir(parents=True, exist_ok=True)
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        outs = list(ex.map(lambda s: compile_one(hipcc, flags, s, outdir / (s.stem + ".s")), srcs))
    found = {}
    for src, o in zip(srcs, outs):
        for name, parts in kernels(o.read_text(), renames).items():
            found[name] = (src.name, *parts)
    return found, len(srcs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old", type=pathlib.Path)
    ap.add_argument("new", type=pathlib.Path)
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--glob", default="tdx_*.hip", help="which sources to compile (default: all of them)")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--keep", type=pathlib.Path, help="keep the .s files in this directory")
    ap.add_argument("-v", "--verbose", action="store_true", help="also list the identical kernels")
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    jobs = max(1, min(a.jobs, 16))
    with tempfile.TemporaryDirectory() as tmp:
        root = a.keep or pathlib.Path(tmp)
        old, nold = tree_kernels(a.old, root / "old", jobs, renames, a.glob)
        new, nnew = tree_kernels(a.new, root / "new", jobs, [], a.glob)
    n = {"identical": 0, "differs": 0, "added": 0, "lost": 0}
    for name in sorted(set(old) | set(new)):
        if name not in new:
            state, where = "lost", old[name][0]
        elif name not in old:
            state, where = "added", new[name][0]
        else:
            (fo, bo, do), (fn, bn, dn) = old[name], new[name]
            what = [w for w, x, y in (("body", bo, bn), ("descriptor", do, dn)) if x is None or x != y]
            state = "differs" if what else "identical"
            where = fn if fo == fn else f"{fo} -> {fn}"
            if what:
                where += " (" + ", ".join(what) + ")"
        n[state] += 1
        if state != "identical" or a.verbose:
            print(f"{state:9s} {name}  [{where}]")
    print(f"old: {len(old)} kernels in {nold} files   new: {len(new)} kernels in {nnew} files   "
          + "   ".join(f"{k}: {v}" for k, v in n.items()))
    return 0 if n["identical"] == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main())
