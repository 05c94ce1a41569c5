#!/usr/bin/env python3
"""dev: per-kernel diff of the gfx950 device assembly of two source trees.

    python tools/kernel_asm_diff.py OLD_TREE NEW_TREE [--map 'PATTERN=REPL' ...] [kernels/file.hip ...]

Compiles each .hip source (default: the halo conv kernels) of both trees to device assembly with
the library's flags (openpose_amd/build.py), cuts the assembly at the kernel symbols and compares
the instruction streams, ignoring comments, directives and the numbering of local labels.  Kernels
are matched by their demangled name without namespace and argument list, so a change that renames
the instantiations (a new template parameter, two kernels made one) can still be compared: each
--map (repeatable, applied in order) is a regex substitution on the NEW tree's names before
matching.  Prints one line per kernel: same / DIFF (with the count of differing lines) / only in
one tree, then the counts per file.  Exit status 1 if any kernel present in both trees differs.
It only compiles and compares.

Example: XHI became a trailing template parameter of conv3_kernel and conv3w8_kernel (default
false), where the hi-only kernels were conv3x_kernel<BM,BN,HR,TAPU,MINB,KS,NW> and
conv3w8x_kernel<BN,NB,MX,BST>:

    python tools/kernel_asm_diff.py OLD NEW \\
        --map 'conv3_kernel<(.*), true, true>=conv3x_kernel<\\1>' \\
        --map 'conv3w8_kernel<(\\d+), (\\d+), false, (\\w+), (\\w+), true, true>=conv3w8x_kernel<\\1, \\2, \\3, \\4>' \\
        --map '(conv3(?:w8)?_kernel<.*), false>=\\1>'
"""
import argparse
import concurrent.futures as cf
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from openpose_amd.build import ARCH, COMMON, DEVICE, HIPCC  # noqa: E402

DEFAULT = ["conv3.hip", "conv3w.hip", "conv3w8.hip", "conv_head.hip"]
KDIR = os.path.join("openpose_amd", "csrc", "kernels")


def device_asm(tree, src, out):
    flags = [f for f in COMMON if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include")]
    cmd = [HIPCC] + flags + ["-x", "hip"] + DEVICE + ["--cuda-device-only", "-S",
                                                     os.path.join(tree, KDIR, src), "-o", out]
    subprocess.run(cmd, check=True)
    with open(out) as f:
        return f.read()


def tidy(symbols):
    """{mangled symbol: demangled name without return type, namespaces and argument list}"""
    symbols = sorted(symbols)
    if not symbols:
        return {}
    names = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    out = {}
    for sym, name in zip(symbols, names):
        name = name.replace("opk::(anonymous namespace)::", "").replace("(opk::ConvArgs)", "")
        out[sym] = re.sub(r"^void\s+", "", name.strip())
    return out


def kernels(asm, maps=()):
    """{tidied name: [normalised instruction lines]} of every .amdhsa_kernel of the assembly text"""
    names = tidy(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)))
    for pat, repl in maps:
        names = {sym: re.sub(pat, repl, name) for sym, name in names.items()}
    if len(set(names.values())) != len(names):
        sys.exit("two kernels of one tree share a name after --map: " +
                 ", ".join(sorted(n for n in names.values() if list(names.values()).count(n) > 1)))
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(names[m.group(1)], [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".LBB")):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("srcs", nargs="*", default=DEFAULT)
    ap.add_argument("--map", action="append", default=[], metavar="PATTERN=REPL",
                    help="regex substitution on the NEW tree's kernel names before matching")
    a = ap.parse_args()
    maps = [tuple(m.split("=", 1)) for m in a.map]
    if any(len(m) != 2 for m in maps):
        ap.error("--map takes PATTERN=REPL")
    bad = 0

    def one(job):
        i, tree, src = job
        if not os.path.exists(os.path.join(tree, KDIR, src)):
            return {}
        return kernels(device_asm(tree, src, os.path.join(tmp, "%d_%s.s" % (i, src))), maps if i else ())

    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        jobs = [(i, tree, src) for src in a.srcs for i, tree in enumerate((a.old, a.new))]
        res = dict(zip([(i, src) for i, _, src in jobs], ex.map(one, jobs)))
    summary = []
    for src in a.srcs:
        ks = [res[(0, src)], res[(1, src)]]
        count = {"same": 0, "DIFF": 0, "only old": 0, "only new": 0}
        for name in sorted(set(ks[0]) | set(ks[1])):
            if name not in ks[0] or name not in ks[1]:
                what = "only old" if name in ks[0] else "only new"
                print("%-12s %s (%d instructions)" % (what, name, len(ks[0].get(name) or ks[1].get(name))))
            elif ks[0][name] == ks[1][name]:
                what = "same"
                print("%-12s %s (%d instructions)" % (what, name, len(ks[0][name])))
            else:
                what = "DIFF"
                d = [x for x in difflib.unified_diff(ks[0][name], ks[1][name], lineterm="", n=0)
                     if x[:1] in "+-" and x[:3] not in ("+++", "---")]
                print("%-12s %s (%d differing lines)" % (what, name, len(d)))
                bad += 1
            count[what] += 1
        summary.append("%-14s %3d kernels: %d same, %d DIFF, %d only old, %d only new" % (
            src, sum(count.values()), count["same"], count["DIFF"], count["only old"], count["only new"]))
    print("\n".join(summary))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
